// Host side of the SIREN Jacobian adjoint (K15): launches, workspace and the C entry
// points cfd_siren_jtape_*.  The kernels are in siren_jtape.hpp (shared with K16,
// siren_jdense.hip).
#include "siren_jtape.hpp"

namespace {

template <int NB, int RS>
void launch_jtape_nb(const cfd::SirenJTapeArgs& a, bool bwd, hipStream_t st) {
    // 8 waves (2 per SIMD, 256 registers each) share one weight stream; NB = 32 holds
    // 256 registers of operands and accumulators alone and runs 4 waves (1 per SIMD,
    // 512 registers, the overflow in AGPRs, no scratch), as K13
    constexpr int WAVES = NB <= 24 ? 8 : 4, TILE = (16 / RS) * WAVES;
    const size_t lds = sizeof(float) * (2 * NB * 256 + (bwd ? 0 : 4 * NB * 16));
    const void* fn = bwd ? (const void*)cfd::siren_jtape_bwd<NB, RS, WAVES>
                         : (const void*)cfd::siren_jtape_fwd<NB, RS, WAVES>;
    CFD_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t tiles = cfd::ceil_div(a.P, TILE);
    CFD_REQUIRE(tiles <= 0x7fffffff, CFD_EARG, "too many (row, sensor) pairs for one call");
    if (bwd)
        hipLaunchKernelGGL((cfd::siren_jtape_bwd<NB, RS, WAVES>), dim3((unsigned)tiles), dim3(64 * WAVES), lds, st, a);
    else
        hipLaunchKernelGGL((cfd::siren_jtape_fwd<NB, RS, WAVES>), dim3((unsigned)tiles), dim3(64 * WAVES), lds, st, a);
    cfd::check_launch(bwd ? "siren_jtape_bwd" : "siren_jtape_fwd");
}

template <int RS>
void launch_jtape(const cfd_siren* h, const cfd::SirenJTapeArgs& a, bool bwd, hipStream_t st) {
    cfd::dispatch_nb(h->NB, [&](auto nbc) { launch_jtape_nb<decltype(nbc)::value, RS>(a, bwd, st); });
}

// every shape check of the pair, before any launch
void jtape_shape_check(const cfd_siren* h, int64_t Ns, int R) {
    CFD_REQUIRE(Ns >= 1 && Ns <= (1 << 20) && R >= 1, CFD_EARG, "bad sensor / row count");
    CFD_REQUIRE(h->cfg.in_coord_features <= 3, CFD_EARG,
                "cfd_siren_jtape: in_coord_features must be 1..3 (the 1 + d chains of a pair share 4 MFMA columns)");
}

struct JTapeWs {
    float *film, *tape, *delta, *D;
    size_t floats;
};

JTapeWs jtape_ws(const cfd_siren* h, int64_t Ns, int R, void* ws) {
    const size_t nf = (size_t)(h->cfg.num_hidden_layers + 1) * h->cfg.hidden_features;
    const size_t P = (size_t)R * Ns, nr = 1 + h->cfg.in_coord_features, L = h->cfg.in_latent_features;
    JTapeWs w;
    w.film = (float*)ws;
    w.tape = w.film + (size_t)R * nf;
    w.delta = w.tape + P * nr * nf;
    w.D = w.delta + P * nf;
    w.floats = 2 * (size_t)R * nf + (nr + 1) * P * nf + (size_t)cfd::gemm_splits((int)nf) * R * L;
    return w;
}

void jtape_args(const cfd_siren* h, cfd::SirenJTapeArgs& a, const JTapeWs& w, int64_t Ns, int R) {
    cfd::handle_args(a, h);
    a.wimg_t = h->wimg_t;
    a.film = w.film;
    a.tape = w.tape;
    a.delta = w.delta;
    a.P = (int64_t)R * Ns;
    a.Ns = (int)Ns;
}

}  // namespace

extern "C" int cfd_siren_jtape_workspace_bytes(const cfd_siren* h, int64_t Ns, int R, size_t* bytes) {
    return cfd::guard([&] {
        CFD_REQUIRE(h && bytes && Ns >= 0 && R >= 0, CFD_EARG, "bad argument");
        *bytes = sizeof(float) * jtape_ws(h, Ns, R, nullptr).floats;
    });
}

extern "C" int cfd_siren_jtape_forward(cfd_siren* h, const float* coords, int64_t Ns, const float* latents, int R,
                                       const float* xmax, const float* xmin, const float* ymax, const float* ymin,
                                       int64_t y_stride, float* out, float* jac, void* ws, size_t ws_bytes,
                                       void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(h && coords && latents && out && jac && ws, CFD_EARG, "null argument");
        jtape_shape_check(h, Ns, R);
        CFD_REQUIRE((xmax == nullptr) == (xmin == nullptr) && (ymax == nullptr) == (ymin == nullptr), CFD_EARG,
                    "normaliser bounds must be set in pairs");
        CFD_REQUIRE(((uintptr_t)ws & 15) == 0, CFD_EARG, "workspace must be 16-byte aligned");
        const JTapeWs w = jtape_ws(h, Ns, R, ws);
        CFD_REQUIRE(ws_bytes >= sizeof(float) * w.floats, CFD_EARG, "workspace too small");
        auto st = (hipStream_t)stream;
        cfd::SirenJTapeArgs a{};
        jtape_args(h, a, w, Ns, R);
        a.coords = coords;
        a.xmax = xmax;
        a.xmin = xmin;
        a.ymax = ymax;
        a.ymin = ymin;
        a.ystride = y_stride;
        a.out = out;
        a.jac = jac;
        cfd::film_vectors(h, latents, R, w.film, st);
        if (a.d == 1)
            launch_jtape<2>(h, a, false, st);
        else
            launch_jtape<4>(h, a, false, st);
    });
}

extern "C" int cfd_siren_jtape_vjp(cfd_siren* h, const float* g_out, const float* g_jac, int64_t Ns, int R,
                                   const float* ymax, const float* ymin, int64_t y_stride, float* g_latents, void* ws,
                                   size_t ws_bytes, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(h && g_latents && ws, CFD_EARG, "null argument");
        jtape_shape_check(h, Ns, R);
        CFD_REQUIRE((ymax == nullptr) == (ymin == nullptr), CFD_EARG, "ymax/ymin must both be set or both NULL");
        CFD_REQUIRE(((uintptr_t)ws & 15) == 0, CFD_EARG, "workspace must be 16-byte aligned");
        const JTapeWs w = jtape_ws(h, Ns, R, ws);
        CFD_REQUIRE(ws_bytes >= sizeof(float) * w.floats, CFD_EARG, "workspace too small");
        auto st = (hipStream_t)stream;
        cfd::SirenJTapeArgs a{};
        jtape_args(h, a, w, Ns, R);
        a.ymax = ymax;
        a.ymin = ymin;
        a.ystride = y_stride;
        a.gout = g_out;
        a.gjac = g_jac;
        if (a.d == 1)
            launch_jtape<2>(h, a, true, st);
        else
            launch_jtape<4>(h, a, true, st);
        cfd::latent_grad_from_delta(h, w.delta, w.D, Ns, R, g_latents, st);
    });
}
