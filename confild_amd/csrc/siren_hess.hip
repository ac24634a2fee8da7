// Fused SIREN/FiLM decode with its coordinate Jacobian and Hessian for gfx950 (K14).
//
// For each (latent row, query point): the value of the FiLM/SIREN chain, its d
// forward-mode tangents and its second-order (Taylor-mode) chains with respect to the
// physical coordinates, in one launch.  With a_k = W0[:, k] s_k:
//   layer 0  : u = w0 (W0 cn + F0);  X = sin u;  T_k = w0 cos u * a_k
//              S_kl = -w0^2 sin u * a_k a_l
//   hidden i : u = w0 (W_i X + F_i); A_k = W_i T_k;  H_kl = W_i S_kl   (one MFMA chain)
//              X = sin u;  T_k = w0 cos u * A_k
//              S_kl = w0 cos u * H_kl - w0^2 sin u * A_k A_l
//   last     : out = W_L X + b_L;  J_k = W_L T_k;  G_kl = W_L S_kl
//   physical : out, jac as K13;  hess[b, n, o, k, l] = (ymax - ymin)[o] / 2 * G_kl[o]
// with cn = norm(x) and s_k = 2 / (xmax_k - xmin_k) (1 without a coordinate normaliser).
//
// Design (DESIGN.md "K14"): K13's chain (siren_jac.hip) with more roles per point.
// Column j16 = RS * point + role: role 0 the value, roles 1..d the tangents, then the
// nsec second-order roles (the d diagonal ones xx, yy, zz first, then xy, xz, yz);
// the remaining columns of a group carry zeros.  RS = 4 at d = 1 (4 points per wave),
// 8 at d = 2 and for the diagonal at d = 3 (2 points), 16 for the full Hessian at
// d = 3 (1 point).  Every chain is linear through W_i, so all of them come out of the
// same MFMAs on one stream of the weights.  A second-order column needs three values
// of other columns of its group per element and layer: the value column's
// pre-activation and the pre-activations A_k, A_l of two tangent columns; its sine it
// computes itself, and the cosine is the one a tangent column of the group has just
// computed for the same argument.  A group lies inside a 16-lane row, and the four
// arrive by ds_bpermute_b32 (the LDS crossbar, no LDS memory).  Value and tangent columns evaluate K13's expressions;
// the second-order update is one fixed fmaf sequence, the same in every instantiation.
#include "siren_hess.hpp"

namespace cfd {

template <int NB, int RS, int WAVES>
__global__ __launch_bounds__(64 * WAVES, NB <= 24 ? 2 : 1) void siren_hess_fused(SirenHessArgs p) {
    constexpr int PPW = 16 / RS;       // points per wave
    constexpr int TILE = PPW * WAVES;  // points per workgroup
    constexpr int H = NB * 16;
    constexpr int BLK = NB * 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wbuf = smem;            // 2 ring slots
    float* film = smem + 2 * BLK;  // (nh+1) x H, then w0 as (H, 4)

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int j16 = lane & 15;
    const int role = j16 & (RS - 1);
    const int d = p.d;
    const HessRole R = hess_role(lane, role, d, p.nsec);
    const bool value = R.value, tangent = R.tangent, second = R.second;
    const int ck = R.ck, cl = R.cl;
    const int src_v = R.src_v, src_k = R.src_k, src_l = R.src_l, src_c = R.src_c;
    const int64_t b = p.b0 + blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * TILE + wave * PPW + j16 / RS;
    const int64_t nc = n < p.N ? n : p.N - 1;
    const int nh = p.nh;
    const float w0f = p.w0f;
    const float w0sq = w0f * w0f;
    CFD_DASSERT(d >= 1 && d <= 3 && 1 + d + p.nsec <= RS && p.c >= 1 && p.c <= 4 && b < p.b && nc >= 0);
    CFD_DASSERT(ck <= cl && cl < d && src_v >= 0 && src_k >= 0 && src_k < 256 && src_l >= 0 && src_l < 256);

    {
        const float* fsrc = p.film + b * (int64_t)(nh + 1) * H;
        const int nf = (nh + 1) * H;
        for (int i = threadIdx.x * 4; i < nf; i += 64 * WAVES * 4) *(f4*)(film + i) = *(const f4*)(fsrc + i);
    }
    float* w0s = film + (nh + 1) * H;
    for (int f = threadIdx.x; f < H; f += 64 * WAVES) {
        f4 w = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < d; ++k) w[k] = p.w0[f * d + k];
        *(f4*)(w0s + 4 * f) = w;
    }
    // normalised coordinates; tsc = w0 * s_k for a tangent column (K13's), sk / sl the
    // coordinate scales of a second-order column
    float cn[3] = {0.f, 0.f, 0.f};
    float tsc = 0.f, sk = 0.f, sl = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k < d) {
            float v = p.coords[nc * d + k];
            float s = 1.0f;
            if (p.xmax) {
                const float hi = p.xmax[k], lo = p.xmin[k];
                v = (v - lo) / (hi - lo) * 2.0f - 1.0f;
                s = 2.0f / (hi - lo);
            }
            cn[k] = v;
            if (tangent && ck == k) tsc = w0f * s;
            if (second && ck == k) sk = s;
            if (second && cl == k) sl = s;
        }
    }

    __syncthreads();
    if (nh > 0) siren_issue_block<NB, WAVES>(p.wimg, 0, wbuf, wave, lane);

    // ---- layer 0 ----
    float X[NB][4];
    static_for<NB>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const f4 fv = *(const f4*)(film + 16 * q + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f4 w = *(const f4*)(w0s + 4 * (16 * q + 4 * g + r));
            // sine in the value and second-order columns, cosine in the tangent columns
            const float sc = sincos_role(w0f * layer0_preact(cn, w, d, fv[r]), !tangent);
            const float wk = ck == 0 ? w[0] : ck == 1 ? w[1] : w[2];
            const float wl = cl == 0 ? w[0] : cl == 1 ? w[1] : w[2];
            const float sv = second_order(w0f, w0sq, sc, 0.0f, 0.0f, wk * sk, wl * sl);
            X[q][r] = value ? sc : tangent ? sc * (tsc * wk) : second ? sv : 0.0f;
        }
    });

    // ---- hidden layers: one fp32 MFMA chain carries every role ----
    const int nblocks = nh * NB;
    int J = 0;
    for (int layer = 1; layer <= nh; ++layer) {
        f4 acc[NB];
        static_for<NB>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (J + 1 < nblocks) siren_issue_block<NB, WAVES>(p.wimg, J + 1, wbuf + ((J + 1) & 1) * BLK, wave, lane);
            const float* wb = wbuf + (J & 1) * BLK;
            f4 a = *(const f4*)(film + layer * H + 16 * j + 4 * g);
            if (!value) a = f4{0.f, 0.f, 0.f, 0.f};
            static_for<NB>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                const f4 w = *(const f4*)(wb + (q * 64 + lane) * 4);
                a = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, X[q][0], a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, X[q][1], a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, X[q][2], a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, X[q][3], a, 0, 0, 0);
            });
            acc[j] = a;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            ++J;
        });
        static_for<NB>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float av = acc[q][r];
                const float x = w0f * lane_value(src_v, av);
                const float ak = lane_value(src_k, av);
                const float al = lane_value(src_l, av);
                // one reduction and one polynomial per lane: the sine in the value and
                // second-order columns, the cosine in the tangent columns, from where the
                // second-order columns fetch it (tangent 0 of the group has it for the same x)
                const float sc = sincos_role(x, !tangent);
                const float cu = lane_value(src_c, sc);
                const float sv = second_order(w0f, w0sq, sc, cu, av, ak, al);
                X[q][r] = value ? sc : tangent ? (w0f * sc) * av : second ? sv : 0.0f;
            }
        });
    }

    // ---- last layer (H -> c) per column; value: bias + de-normalisation, others: their slope ----
    float o[4];
    hess_head<NB>(p, X, g, value, o);
    hess_store(p, R, o, n, b, g);
}

}  // namespace cfd

namespace {

template <int RS>
void launch_hess(const cfd_siren* h, const cfd::SirenHessArgs& a, hipStream_t st) {
    cfd::dispatch_nb(h->NB, [&](auto nbc) {
        // K13's workgroup shapes: 8 waves (2 per SIMD) share one weight stream; NB = 32
        // runs 4 waves (1 per SIMD, the overflow in AGPRs)
        constexpr int NB = decltype(nbc)::value, WAVES = NB <= 24 ? 8 : 4;
        cfd::launch_decode(cfd::siren_hess_fused<NB, RS, WAVES>, "siren_hess_fused", a, NB, (16 / RS) * WAVES, WAVES,
                           st);
    });
}

}  // namespace

extern "C" int cfd_siren_hessian_workspace_bytes(const cfd_siren* h, int b, size_t* bytes) {
    return cfd_siren_workspace_bytes(h, b, bytes);   // the FiLM vectors (b, nh+1, H)
}

extern "C" int cfd_siren_forward_hessian(cfd_siren* h, const float* coords, int64_t N, const float* latents, int b,
                                         const float* xmax, const float* xmin, const float* ymax, const float* ymin,
                                         int64_t y_stride, float* out, float* jac, float* hess, int diag_only, void* ws,
                                         size_t ws_bytes, void* stream) {
    return cfd::guard([&] {
        cfd::decode_check("cfd_siren_forward_hessian",
                          "the value, tangent and second-order chains of a point share 16 MFMA columns", h, coords, N,
                          latents, b, xmax, xmin, ymax, ymin, hess);
        auto st = (hipStream_t)stream;
        auto a = cfd::decode_args<cfd::SirenHessArgs>(h, coords, N, latents, b, xmax, xmin, ymax, ymin, y_stride, out,
                                                      jac, ws, ws_bytes, st);
        a.hess = hess;
        a.diag = diag_only != 0;
        // always the exact fp32 chain, whatever the handle's compute mode.  d <= 2 runs
        // the full form for both outputs; d = 3 has a diagonal form of 8 columns per point
        const int d = a.d;
        const bool full = d < 3 || !a.diag;
        a.nsec = full ? d * (d + 1) / 2 : d;
        if (d == 1)
            launch_hess<4>(h, a, st);
        else if (d == 2 || !full)
            launch_hess<8>(h, a, st);
        else
            launch_hess<16>(h, a, st);
    });
}
