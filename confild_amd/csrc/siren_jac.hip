// Fused SIREN/FiLM decode with its coordinate Jacobian for gfx950 (K13).
//
// For each (latent row, query point): the value of the FiLM/SIREN chain
// (N/cnf/nf_networks.py:480-495) and its forward-mode derivative with respect to
// the physical coordinates, in one launch:
//   layer 0  : u = w0 (W0 cn + F0);  X = sin(u);  T_k = w0 cos(u) * W0[:, k] s_k
//   hidden i : u = w0 (W_i X + F_i); A_k = W_i T_k;  X = sin(u);  T_k = w0 cos(u) * A_k
//   last     : out = W_L X + b_L;    J_k = W_L T_k
//   physical : out_phys = denorm(out);  jac[b, n, o, k] = (ymax - ymin)[o] / 2 * J_k[o]
// with cn = norm(x) and s_k = 2 / (xmax_k - xmin_k) (1 without a coordinate normaliser).
//
// Design (DESIGN.md "K13"): siren_fused's exact fp32 MFMA chain (siren.hip) with the
// 1 + d chains of a point laid into the MFMA's 16 columns: column j16 = RS * point +
// role, role 0 the value, roles 1..d the tangents (RS = 4: 4 points per wave, one
// idle column per point at d = 2; RS = 2 at d = 1: 8 points x 2 roles).  The MFMA
// treats its columns independently and the A operand (the weight block from the LDS
// ring, streamed once per tile) is shared by all of them, so W_i X and every
// W_i T_k come out of the same instructions.  Accumulators start at the FiLM vector
// in the value column and at 0 in the tangent columns.  The only cross-column
// traffic is the value column's pre-activation, which the tangent columns of its
// group read with one DPP quad-permute move (no LDS); each lane then runs one range
// reduction and one polynomial: the sine in the value column, the cosine in the
// tangent columns (sincos_role, siren_jac.hpp: bit for bit sin_cw / cos_cw of common.hpp).
// Activations and tangents never leave registers; X[NB][4] / acc[NB] are
// siren_fused's, so is the register budget.
#include "siren_jac.hpp"

namespace cfd {

template <int NB, int RS, int WAVES>
__global__ __launch_bounds__(64 * WAVES, NB <= 24 ? 2 : 1) void siren_jac_fused(SirenJacArgs p) {
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
    const int role = j16 & (RS - 1);   // 0: value, k: d/dx_{k-1}
    const bool value = role == 0;
    const int64_t b = p.b0 + blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * TILE + wave * PPW + j16 / RS;
    const int64_t nc = n < p.N ? n : p.N - 1;
    const int nh = p.nh;
    const float w0f = p.w0f;
    CFD_DASSERT(p.d >= 1 && p.d < RS && p.c >= 1 && p.c <= 4 && b < p.b && nc >= 0);

    {
        const float* fsrc = p.film + b * (int64_t)(nh + 1) * H;
        const int nf = (nh + 1) * H;
        for (int i = threadIdx.x * 4; i < nf; i += 64 * WAVES * 4) *(f4*)(film + i) = *(const f4*)(fsrc + i);
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
    if (nh > 0) siren_issue_block<NB, WAVES>(p.wimg, 0, wbuf, wave, lane);

    // ---- layer 0 ----
    float X[NB][4];
    static_for<NB>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const f4 fv = *(const f4*)(film + 16 * q + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f4 w = *(const f4*)(w0s + 4 * (16 * q + 4 * g + r));
            const float sc = sincos_role(w0f * layer0_preact(cn, w, p.d, fv[r]), value);
            const float wk = role == 1 ? w[0] : role == 2 ? w[1] : w[2];
            X[q][r] = value ? sc : sc * (tsc * wk);
        }
    });

    // ---- hidden layers: one fp32 MFMA chain carries the value and the tangents ----
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
                const float sc = sincos_role(w0f * group_value<RS>(av), value);
                X[q][r] = value ? sc : (w0f * sc) * av;
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
                s = fmaf(w.x, X[q][0], s);
                s = fmaf(w.y, X[q][1], s);
                s = fmaf(w.z, X[q][2], s);
                s = fmaf(w.w, X[q][3], s);
            });
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            o[oc] = value ? s + p.bout[oc] : s;
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

template <int RS>
void launch_jac(const cfd_siren* h, const cfd::SirenJacArgs& a, hipStream_t st) {
    cfd::dispatch_nb(h->NB, [&](auto nbc) {
        // 8 waves (2 per SIMD, 256 VGPRs each) share one weight stream; NB = 32 holds
        // 128 + 128 registers of activations and accumulators alone, so it runs 4
        // waves (1 per SIMD: 512 registers, the overflow in AGPRs, no scratch)
        constexpr int NB = decltype(nbc)::value, WAVES = NB <= 24 ? 8 : 4;
        cfd::launch_decode(cfd::siren_jac_fused<NB, RS, WAVES>, "siren_jac_fused", a, NB, (16 / RS) * WAVES, WAVES, st);
    });
}

}  // namespace

extern "C" int cfd_siren_jacobian_workspace_bytes(const cfd_siren* h, int b, size_t* bytes) {
    return cfd_siren_workspace_bytes(h, b, bytes);   // the FiLM vectors (b, nh+1, H)
}

extern "C" int cfd_siren_forward_jacobian(cfd_siren* h, const float* coords, int64_t N, const float* latents, int b,
                                          const float* xmax, const float* xmin, const float* ymax, const float* ymin,
                                          int64_t y_stride, float* out, float* jac, void* ws, size_t ws_bytes,
                                          void* stream) {
    return cfd::guard([&] {
        cfd::decode_check("cfd_siren_forward_jacobian", "the 1 + d chains of a point share 4 MFMA columns", h, coords, N,
                          latents, b, xmax, xmin, ymax, ymin, jac);
        auto st = (hipStream_t)stream;
        const auto a = cfd::decode_args<cfd::SirenJacArgs>(h, coords, N, latents, b, xmax, xmin, ymax, ymin, y_stride,
                                                           out, jac, ws, ws_bytes, st);
        // always the exact fp32 chain, whatever the handle's compute mode
        if (a.d == 1)
            launch_jac<2>(h, a, st);
        else
            launch_jac<4>(h, a, st);
    });
}
