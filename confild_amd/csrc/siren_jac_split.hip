// Fused SIREN/FiLM decode with its coordinate Jacobian on f16 MFMA with fp32-level
// accuracy (K13s): K13's layer algebra (siren_jac.hip) on K7s's arithmetic
// (siren_fused_split, siren_split.hip).
//
// Columns as K13: column j16 = RS * point + role, role 0 the value, roles 1..d the
// tangents (RS = 4, or 2 at d = 1); a lane owns column lane % 16 in the 16x16x32 MFMA
// as in the 16x16x4 one, so the role logic is K13's: the DPP group_value move fetches
// the value column's pre-activation, each lane runs one sine or cosine, accumulators
// start at the FiLM row in value lanes and at 0 in tangent lanes.  Products as K7s:
// the image wimg16 (W s_i = Wh + Wl, s_i a power of two), the FiLM rows pre-scaled by
// s_i, Wl xh + Wh xl + Wh xh on three v_mfma_f32_16x16x32_f16 per 32 features, the
// accumulator blocks 2q, 2q + 1 being the next layer's B fragment q.  The hidden
// weights stream once per tile for all 1 + d chains through a 2-slot LDS-DMA ring.
//
// Range ("hold and normalise"): X = sin(u) lies in [-1, 1], the
// tangents T_k = w0 cos(u) (W T_k) have no bound.  A layer's fp32 outputs stay in
// their accumulator registers until its last block (the kernel holds acc[NB] and one
// operand set, K13's register budget: the epilogue overwrites the operand set in
// place, there is no second set as in K7s).  Then each tangent column takes its exact
// largest magnitude (in-lane over its NB * 4 features, two __shfl_xor over the four
// lanes that share the column), is multiplied by the power of two that brings it to
// [2^12, 2^13) (column_exponent / scale_split8, siren_jac.hpp) and split.  The column's
// exponents add up in an integer and are undone at the head with one ldexpf: exact,
// and a function of the column's own values alone, so the bits of a (row, point) pair
// depend on neither b, N, the point's index nor its neighbours, and scaling the
// coordinates by a power of two scales the Jacobian by exactly its inverse.  Value
// columns take exponent 0 (K7s's split).  An all-zero column (the idle column at
// d = 2, a tangent that is identically 0) takes exponent 0 and stays 0.
#include "siren_jac.hpp"

namespace cfd {

template <int NB, int RS, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 2) void siren_jac_split(SirenJacSplitArgs p) {
    static_assert(NB % 2 == 0, "split-f16 chain needs H % 32 == 0");
    constexpr int NQ = NB / 2;
    constexpr int PPW = 16 / RS;       // points per wave
    constexpr int TILE = PPW * WAVES;  // points per workgroup
    constexpr int H = NB * 16;
    constexpr int BLK = NB * 256;      // floats per output block: NQ x (hi, lo) x 512 halves
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wbuf = smem;            // 2 ring slots
    float* film = smem + 2 * BLK;  // (nh+1) x H (hidden layers' rows pre-scaled by s_i), then w0 as (H, 4)

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int j16 = lane & 15;
    const int role = j16 & (RS - 1);   // 0: value, k: d/dx_{k-1}
    const bool value = role == 0;
    const int64_t b = p.b0 + blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * TILE + wave * PPW + j16 / RS;
    const int64_t nc = n < p.N ? n : p.N - 1;
    const int nh = p.nh;
    const float w0f = p.w0f;
    CFD_DASSERT(p.d >= 1 && p.d < RS && p.c >= 1 && p.c <= 4 && b < p.b && nc >= 0 && nh >= 1);

    {
        const float* fsrc = p.film + b * (int64_t)(nh + 1) * H;
        const int nf = (nh + 1) * H;
        for (int i = threadIdx.x * 4; i < nf; i += 64 * WAVES * 4) {
            const int layer = i / H;
            const float sc = layer == 0 ? 1.0f : p.wscale[layer - 1];
            *(f4*)(film + i) = *(const f4*)(fsrc + i) * sc;  // power of two: exact
        }
    }
    float* w0s = film + (nh + 1) * H;
    for (int f = threadIdx.x; f < H; f += 64 * WAVES) {
        f4 w = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < p.d; ++k) w[k] = p.w0[f * p.d + k];
        *(f4*)(w0s + 4 * f) = w;
    }
    // normalised coordinates; tsc = w0 * s_{role-1} for a live tangent column, else 0
    float cn[3] = {0.f, 0.f, 0.f};
    float tsc = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k < p.d) {
            float v = p.coords[nc * p.d + k];
            float sk = 1.0f;
            if (p.xmax) {
                const float hi = p.xmax[k], lo = p.xmin[k];
                v = (v - lo) / (hi - lo) * 2.0f - 1.0f;
                sk = 2.0f / (hi - lo);
            }
            cn[k] = v;
            if (role == k + 1) tsc = w0f * sk;
        }
    }

    __syncthreads();
    siren_issue_block<NB, WAVES>(p.wimg, 0, wbuf, wave, lane);

    f4 acc[NB];          // a layer's fp32 outputs, held until its column maxima are known
    JFrag BH[NQ], BL[NQ]; // the layer's B operands (hi, lo)
    int E = 0;           // the column's accumulated exponent: tangent = 2^E * (what the chain carries)
    // acc (fp32 X / T of a whole layer) -> BH, BL at the column's own power-of-two scale
    auto normalise_split = [&]() __attribute__((always_inline)) {
        float m = 0.f;
        static_for<NB>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
#pragma unroll
            for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(acc[q][r]));
        });
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const int e = value ? 0 : column_exponent(m);
        E += e;
        static_for<NQ>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            scale_split8(acc[2 * q], acc[2 * q + 1], e, BH[q], BL[q]);
        });
    };

    // ---- layer 0 (d -> H, fp32 VALU) ----
    static_for<NB>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const f4 fv = *(const f4*)(film + 16 * q + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f4 w = *(const f4*)(w0s + 4 * (16 * q + 4 * g + r));
            const float sc = sincos_role(w0f * layer0_preact(cn, w, p.d, fv[r]), value);
            const float wk = role == 1 ? w[0] : role == 2 ? w[1] : w[2];
            acc[q][r] = value ? sc : sc * (tsc * wk);
        }
    });

    // ---- hidden layers: one split-f16 MFMA chain carries the value and the tangents ----
    const int nblocks = nh * NB;
    int J = 0;
    // block 0 landed (this wave's pieces) and is published by every wave
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int layer = 1; layer <= nh; ++layer) {
        normalise_split();
        const float m = w0f / p.wscale[layer - 1];  // power-of-two scale: exact
        static_for<NB>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            acc[j] = ring_step_split<NB, WAVES>(p.wimg, wbuf, J, nblocks, BH, BL, [&] {
                f4 a = *(const f4*)(film + layer * H + 16 * j + 4 * g);
                if (!value) a = f4{0.f, 0.f, 0.f, 0.f};
                return a;
            }, wave, lane);
        });
        // acc = s_i (F_i + W_i X) in value lanes, s_i W_i T 2^-E in tangent lanes
        static_for<NB>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float av = acc[q][r];
                const float sc = sincos_role(m * group_value<RS>(av), value);
                acc[q][r] = value ? sc : (m * sc) * av;
            }
        });
    }

    // ---- last layer (H -> c) per column; value: bias + de-normalisation, tangent: its slope ----
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int oc = 0; oc < 4; ++oc) {
        if (oc < p.c) {
            const float* wr = p.wout + oc * H + 4 * g;
            float s = 0.f;
            static_for<NB>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                const f4 w = *(const f4*)(wr + 16 * q);
                s = fmaf(w.x, acc[q][0], s);
                s = fmaf(w.y, acc[q][1], s);
                s = fmaf(w.z, acc[q][2], s);
                s = fmaf(w.w, acc[q][3], s);
            });
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            o[oc] = value ? s + p.bout[oc] : ldexpf(s, E);   // the column's exponent, undone exactly
        }
    }
    if (n < p.N && g < p.c && role <= p.d) {
        float v = g == 0 ? o[0] : g == 1 ? o[1] : g == 2 ? o[2] : o[3];
        float hi = 1.0f, lo = -1.0f;
        if (p.ymax) {
            const int64_t yi = n * p.ystride + g;
            hi = p.ymax[yi];
            lo = p.ymin[yi];
        }
        const int64_t oi = (b * p.N + n) * p.c + g;
        CFD_DASSERT(oi >= 0 && oi < (int64_t)p.b * p.N * p.c);
        if (value) {
            if (p.ymax) v = (v + 1.0f) / 2.0f * (hi - lo) + lo;
            if (p.out) p.out[oi] = v;
        } else {
            if (p.ymax) v = v * ((hi - lo) / 2.0f);
            const int64_t ji = oi * p.d + (role - 1);
            CFD_DASSERT(ji >= 0 && ji < (int64_t)p.b * p.N * p.c * p.d);
            p.jac[ji] = v;
        }
    }
}

}  // namespace cfd

namespace {

constexpr int JS_WAVES = 8;   // 2 per SIMD, 256 registers each, sharing one weight stream

template <int RS>
void launch_jac_split(int nb, const cfd::SirenJacSplitArgs& a, hipStream_t st) {
    cfd::dispatch_nb_split(nb, "internal: split Jacobian width not checked", [&](auto nbc) {
        constexpr int NB = decltype(nbc)::value;
        cfd::launch_decode(cfd::siren_jac_split<NB, RS, JS_WAVES>, "siren_jac_split", a, NB, (16 / RS) * JS_WAVES,
                           JS_WAVES, st);
    });
}

}  // namespace

extern "C" int cfd_siren_forward_jacobian_split(cfd_siren* h, const float* coords, int64_t N, const float* latents,
                                                int b, const float* xmax, const float* xmin, const float* ymax,
                                                const float* ymin, int64_t y_stride, float* out, float* jac, void* ws,
                                                size_t ws_bytes, void* stream) {
    return cfd::guard([&] {
        const char* fn = "cfd_siren_forward_jacobian_split";
        cfd::decode_check(fn, "the 1 + d chains of a point share 4 MFMA columns", h, coords, N, latents, b, xmax, xmin,
                          ymax, ymin, jac);
        cfd::split_refusal(fn, h);
        auto st = (hipStream_t)stream;
        auto a = cfd::decode_args<cfd::SirenJacSplitArgs>(h, coords, N, latents, b, xmax, xmin, ymax, ymin, y_stride,
                                                          out, jac, ws, ws_bytes, st);
        a.wimg = h->wimg16;
        a.wscale = h->wscale;
        if (a.d == 1)
            launch_jac_split<2>(h->NB, a, st);
        else
            launch_jac_split<4>(h->NB, a, st);
    });
}
