// Latent gradient of a linear functional of the SIREN's value and coordinate
// Jacobian at a few points (K15): g_z = d/dz ( <G0, out(z)> + <G1, jac(z)> ), with out
// (R, Ns, c) and jac (R, Ns, c, d) as cfd_siren_forward_jacobian defines them.  Reverse
// mode over K13's forward mode (siren_jac.hip), for the DPS sampler's derivative
// sensors (vorticity, divergence, wall shear).
//
// Forward (siren_jtape_fwd): K13's fp32 MFMA chain and column layout (column =
// RS * pair + role, role 0 the value, roles 1..d the tangents) over the P = R x Ns
// (latent row, sensor) pairs of siren_tape_fwd, each pair reading its own row's FiLM
// vectors.  Per layer i it also writes every live column's accumulator to the tape
// (P, nh+1, 1+d, H): u_i = W_i X_{i-1} + F_i from the value column, A_{i,k} =
// W_i T_{i-1,k} from tangent column k (layer 0: A_{0,k} = W_0[:, k] s_k).
//   X_i = sin(w0 u_i),  T_{i,k} = w0 cos(w0 u_i) A_{i,k}
//
// Backward (siren_jtape_bwd): the same columns on the transposed image in reverse
// layer order (siren_tape_bwd's stream).  The value column carries u-bar, tangent
// column k carries A-bar_k, so every W_i^T product of the 1 + d chains comes out of
// one weight stream:
//   u-bar_i   = w0 cos(w0 u_i) X-bar - w0^2 sin(w0 u_i) sum_k A_{i,k} T-bar_k
//   A-bar_i,k = w0 cos(w0 u_i) T-bar_k
//   X-bar <- W_i^T u-bar_i,  T-bar_k <- W_i^T A-bar_i,k
// Per element each lane reads its pair's u from the tape and runs one sincos_role
// (sine in the value lane, cosine in the tangent lanes); the value lane takes the
// cosine from tangent 1 of its group and the T-bar_k from the group's tangent
// accumulators with DPP quad-permute moves (no LDS), and reads its d taped A_k.
// u-bar is written as delta (P, nh+1, H), the layout sensor_sum_kernel /
// siren_latent_grad consume; only u-bar feeds g_z because A_k does not depend on F.
//
// Always the exact fp32 chain, whatever cfd_siren_set_compute chose.  A pair's
// columns never mix with another pair's, so its bits do not depend on R, on the
// other rows or on the samples sharing the call.
//
// DENSE (K16, siren_jdense.hip: whole-field derivative measurements in bounded
// memory): the same two chains on row-aligned tiles -- grid (point tile, row of the
// block), p.Ns the points of the chunk, p.P = rows x p.Ns -- points past the chunk's
// end clamped for loads and dead for stores.  The backward stores no u-bar: per layer
// the tile's u-bar is added over its pairs on chip (the value lanes of a wave by DPP
// row rotates, the waves in wave order through WAVES x H floats of LDS) and one
// (nh+1) H partial is stored per tile at p.part.  The DENSE = false instantiations
// are K15's kernels unchanged.
#pragma once
#include <type_traits>

#include "siren_jac.hpp"

namespace cfd {

struct SirenJTapeArgs {
    const float* w0;      // (H, d)
    const float* wimg;    // forward weight image
    const float* wimg_t;  // transposed image, layers nh..1
    const float* wout;    // (c, H)
    const float* bout;    // (c)
    const float* film;    // (R, nh+1, H)
    const float* coords;  // (Ns, d)
    const float* xmax;
    const float* xmin;
    const float* ymax;
    const float* ymin;
    float* tape;          // (P, nh+1, 1+d, H)
    float* delta;         // (P, nh+1, H)
    float* out;           // (P, c)
    float* jac;           // (P, c, d)
    const float* gout;    // (P, c) or null (zero)
    const float* gjac;    // (P, c, d) or null (zero)
    int64_t P;
    int64_t ystride;
    int Ns, d, c, nh;
    float w0f;
};
// DENSE: film / tape / out / jac / gout / gjac are the row block's and the chunk's
struct SirenJDenseArgs : SirenJTapeArgs {
    float* part;          // (rows, tiles of the chunk, (nh+1) H) tile sums of u-bar
};
template <bool DENSE>
using JTapeArgsOf = std::conditional_t<DENSE, SirenJDenseArgs, SirenJTapeArgs>;

// lane `k` of each group of RS columns (RS = 2: k = 1 only): DPP quad_perm, no LDS
template <int RS, int K>
__device__ __forceinline__ float group_lane(float v) {
    static_assert(K >= 1 && K < RS, "a tangent column of the group");
    constexpr int ctrl = RS == 4 ? K * 0x55 /* quad_perm [K,K,K,K] */ : 0xF5 /* quad_perm [1,1,3,3] */;
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false));
}

template <int NB, int RS, int WAVES, bool DENSE = false>
__global__ __launch_bounds__(64 * WAVES, NB <= 24 ? 2 : 1) void siren_jtape_fwd(JTapeArgsOf<DENSE> p) {
    constexpr int PPW = 16 / RS;       // pairs per wave
    constexpr int TILE = PPW * WAVES;  // pairs per workgroup
    constexpr int H = NB * 16;
    constexpr int BLK = NB * 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wbuf = smem;            // 2 ring slots
    float* w0s = smem + 2 * BLK;   // (H, 4)

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int j16 = lane & 15;
    const int role = j16 & (RS - 1);   // 0: value, k: d/dx_{k-1}
    const bool value = role == 0;
    // the pair n of the P, clamped to nc for loads.  DENSE: point pn of row blockIdx.y,
    // n = P marks a dead one (past the chunk's end), clamped to the row's last point
    const int64_t pn = (int64_t)blockIdx.x * TILE + wave * PPW + j16 / RS;
    const int64_t n = !DENSE ? pn : pn < p.Ns ? (int64_t)blockIdx.y * p.Ns + pn : p.P;
    const int64_t nc = n < p.P ? n : !DENSE ? p.P - 1 : (int64_t)blockIdx.y * p.Ns + p.Ns - 1;
    const int64_t row = !DENSE ? nc / p.Ns : (int64_t)blockIdx.y;
    const int sensor = (int)(nc - row * p.Ns);
    const int nh = p.nh, nl = nh + 1, nr = 1 + p.d;
    const float w0f = p.w0f;
    const float* film = p.film + row * nl * H;
    const bool store = n < p.P && role <= p.d;
    float* tp = p.tape + (nc * nl * nr + (role <= p.d ? role : 0)) * H;   // this column's slot of layer 0
    CFD_DASSERT(p.d >= 1 && p.d < RS && p.c >= 1 && p.c <= 4 && nc >= 0 && nc < p.P && sensor >= 0 && sensor < p.Ns);

    for (int f = threadIdx.x; f < H; f += 64 * WAVES) {
        f4 w = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < p.d; ++k) w[k] = p.w0[f * p.d + k];
        *(f4*)(w0s + 4 * f) = w;
    }
    // normalised coordinates; ssc = s_{role-1} for a live tangent column, else 0
    float cn[3] = {0.f, 0.f, 0.f};
    float ssc = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k < p.d) {
            float v = p.coords[(int64_t)sensor * p.d + k];
            float sk = 1.0f;
            if (p.xmax) {
                const float hi = p.xmax[k], lo = p.xmin[k];
                v = (v - lo) / (hi - lo) * 2.0f - 1.0f;
                sk = 2.0f / (hi - lo);
            }
            cn[k] = v;
            if (role == k + 1) ssc = sk;
        }
    }
    const float tsc = w0f * ssc;

    __syncthreads();
    if (nh > 0) siren_issue_block<NB, WAVES>(p.wimg, 0, wbuf, wave, lane);

    // ---- layer 0 ----
    float X[NB][4];
    static_for<NB>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const f4 fv = *(const f4*)(film + 16 * q + 4 * g);
        f4 tv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f4 w = *(const f4*)(w0s + 4 * (16 * q + 4 * g + r));
            float a = cn[0] * w[0];
#pragma unroll
            for (int k = 1; k < 3; ++k)
                if (k < p.d) a = fmaf(cn[k], w[k], a);
            const float u = a + fv[r];
            const float sc = sincos_role(w0f * u, value);
            const float wk = role == 1 ? w[0] : role == 2 ? w[1] : w[2];
            X[q][r] = value ? sc : sc * (tsc * wk);
            tv[r] = value ? u : ssc * wk;
        }
        if (store) {
            CFD_DASSERT((tp - p.tape) + 16 * q + 4 * g + 4 <= p.P * nl * nr * H);
            *(f4*)(tp + 16 * q + 4 * g) = tv;
        }
    });

    if constexpr (DENSE) {
        // block 0 landed in every wave's pieces before any wave reads it
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // ---- hidden layers: one fp32 MFMA chain carries the value and the tangents ----
    const int nblocks = nh * NB;
    int J = 0;
    for (int layer = 1; layer <= nh; ++layer) {
        f4 acc[NB];
        static_for<NB>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (J + 1 < nblocks) siren_issue_block<NB, WAVES>(p.wimg, J + 1, wbuf + ((J + 1) & 1) * BLK, wave, lane);
            const float* wb = wbuf + (J & 1) * BLK;
            f4 a = {0.f, 0.f, 0.f, 0.f};
            if (value) a = *(const f4*)(film + layer * H + 16 * j + 4 * g);
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
        float* tl = tp + (int64_t)layer * nr * H;
        static_for<NB>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            if (store) {
                CFD_DASSERT((tl - p.tape) + 16 * q + 4 * g + 4 <= p.P * nl * nr * H);
                *(f4*)(tl + 16 * q + 4 * g) = acc[q];
            }
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
    if (store && g < p.c) {
        float v = g == 0 ? o[0] : g == 1 ? o[1] : g == 2 ? o[2] : o[3];
        float hi = 1.0f, lo = -1.0f;
        if (p.ymax) {
            const int64_t yi = (int64_t)sensor * p.ystride + g;
            hi = p.ymax[yi];
            lo = p.ymin[yi];
        }
        const int64_t oi = n * p.c + g;
        CFD_DASSERT(oi >= 0 && oi < p.P * p.c);
        if (value) {
            if (p.ymax) v = (v + 1.0f) / 2.0f * (hi - lo) + lo;
            p.out[oi] = v;
        } else {
            if (p.ymax) v = v * ((hi - lo) / 2.0f);
            const int64_t ji = oi * p.d + (role - 1);
            CFD_DASSERT(ji >= 0 && ji < p.P * p.c * p.d);
            p.jac[ji] = v;
        }
    }
}

template <int NB, int RS, int WAVES, bool DENSE = false>
__global__ __launch_bounds__(64 * WAVES, NB <= 24 ? 2 : 1) void siren_jtape_bwd(JTapeArgsOf<DENSE> p) {
    constexpr int PPW = 16 / RS;
    constexpr int TILE = PPW * WAVES;
    constexpr int H = NB * 16;
    constexpr int BLK = NB * 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wbuf = smem;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int j16 = lane & 15;
    const int role = j16 & (RS - 1);
    const bool value = role == 0;
    const int64_t pn = (int64_t)blockIdx.x * TILE + wave * PPW + j16 / RS;   // n, nc: as the forward
    const int64_t n = !DENSE ? pn : pn < p.Ns ? (int64_t)blockIdx.y * p.Ns + pn : p.P;
    const int64_t nc = n < p.P ? n : !DENSE ? p.P - 1 : (int64_t)blockIdx.y * p.Ns + p.Ns - 1;
    const int sensor = (int)(nc % p.Ns);
    const int nh = p.nh, nl = nh + 1, d = p.d, nr = 1 + d;
    const float w0f = p.w0f;
    const bool live = n < p.P;
    const float* tp = p.tape + nc * nl * nr * H;   // the pair's tape: (nh+1, 1+d, H)
    float* dt = DENSE ? nullptr : p.delta + nc * nl * H;
    float* red = smem + 2 * BLK;                   // DENSE: (WAVES, H) sums of one layer's u-bar
    CFD_DASSERT(d >= 1 && d < RS && p.c >= 1 && p.c <= 4 && nc >= 0 && nc < p.P);

    if (nh > 0) siren_issue_block<NB, WAVES>(p.wimg_t, 0, wbuf, wave, lane);

    // this column's gradient w.r.t. the raw head output: G0 (value) or G1[.., role-1]
    // (tangent) times (ymax - ymin) / 2; zero in an idle column and past the last pair
    float dy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int oc = 0; oc < 4; ++oc) {
        if (oc < p.c) {
            float v = 0.f;
            if (live && value && p.gout) v = p.gout[nc * p.c + oc];
            if (live && !value && role <= d && p.gjac) {
                const int64_t ji = (nc * p.c + oc) * d + (role - 1);
                CFD_DASSERT(ji >= 0 && ji < p.P * p.c * d);
                v = p.gjac[ji];
            }
            if (p.ymax) {
                const int64_t yi = (int64_t)sensor * p.ystride + oc;
                v = v * ((p.ymax[yi] - p.ymin[yi]) / 2.0f);
            }
            dy[oc] = v;
        }
    }

    // a: X-bar (value column) / T-bar_k (tangent column k) of layer li, features
    // 16 q + 4 g + r -> u-bar_li (value) / A-bar_li,k (tangent), the next B operand
    auto epilogue = [&](int li, int q, const f4 a) -> f4 {
        const float* us = tp + (int64_t)li * nr * H + 16 * q + 4 * g;
        CFD_DASSERT((us - p.tape) + (int64_t)d * H + 4 <= p.P * nl * nr * H);
        const f4 uu = *(const f4*)us;
        f4 A1 = {0.f, 0.f, 0.f, 0.f}, A2 = A1, A3 = A1;
        if (value) {
            A1 = *(const f4*)(us + H);
            if (d > 1) A2 = *(const f4*)(us + 2 * H);
            if (d > 2) A3 = *(const f4*)(us + 3 * H);
        }
        f4 res;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sc = sincos_role(w0f * uu[r], value);
            const float cs = group_lane<RS, 1>(sc);     // the cosine, for the value lane
            float tb = A1[r] * group_lane<RS, 1>(a[r]);
            if constexpr (RS == 4) {
                tb = fmaf(A2[r], group_lane<RS, 2>(a[r]), tb);
                tb = fmaf(A3[r], group_lane<RS, 3>(a[r]), tb);
            }
            const float ub = (w0f * cs) * a[r] - ((w0f * w0f) * sc) * tb;
            res[r] = value ? ub : (w0f * sc) * a[r];
        }
        if constexpr (DENSE) {
            // the wave's pairs in fixed lane order: value lanes sit RS apart in the lane
            // row, so row rotates by 8, 4 (and 2 at RS = 2) add them, as K9t's sum mode.
            // A dead lane's dy is zero, so its u-bar is an exact zero.
            f4 s = res;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = s[r];
                v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false));
                v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xF, 0xF, false));
                if constexpr (RS == 2)
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xF, 0xF, false));
                s[r] = v;
            }
            if (j16 == 0) {
                CFD_DASSERT(wave * H + 16 * q + 4 * g + 4 <= WAVES * H);
                *(f4*)(red + wave * H + 16 * q + 4 * g) = s;
            }
        } else {
            if (live && value) {
                CFD_DASSERT((dt - p.delta) + (int64_t)li * H + 16 * q + 4 * g + 4 <= p.P * nl * H);
                *(f4*)(dt + (int64_t)li * H + 16 * q + 4 * g) = res;
            }
        }
        return res;
    };
    // DENSE: layer li's wave sums added in wave order, one store per feature.  The
    // barrier also orders weight block 0 (every wave's pieces) before the first MFMA;
    // the next write of `red` comes after the weight stream's barriers of a layer.
    auto tile_sum = [&](int li) {
        if constexpr (DENSE) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            float* dst = p.part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nl * H + (int64_t)li * H;
            for (int f = threadIdx.x; f < H; f += 64 * WAVES) {
                float s = red[f];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) s += red[w * H + f];
                CFD_DASSERT((dst - p.part) + f < (int64_t)gridDim.y * gridDim.x * nl * H);
                dst[f] = s;
            }
        }
    };

    // ---- head: X-bar = W_L^T g-bar_o, T-bar_k = W_L^T g-bar_J,k ----
    float X[NB][4];
    static_for<NB>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        f4 gx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * q + 4 * g + r;
            float s = 0.f;
#pragma unroll
            for (int oc = 0; oc < 4; ++oc)
                if (oc < p.c) s = fmaf(p.wout[oc * H + f], dy[oc], s);
            gx[r] = s;
        }
        const f4 res = epilogue(nh, q, gx);
#pragma unroll
        for (int r = 0; r < 4; ++r) X[q][r] = res[r];
    });
    tile_sum(nh);

    const int nblocks = nh * NB;
    int J = 0;
    for (int layer = nh; layer >= 1; --layer) {
        f4 acc[NB];
        static_for<NB>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (J + 1 < nblocks)
                siren_issue_block<NB, WAVES>(p.wimg_t, J + 1, wbuf + ((J + 1) & 1) * BLK, wave, lane);
            const float* wb = wbuf + (J & 1) * BLK;
            f4 a = {0.f, 0.f, 0.f, 0.f};
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
        const int li = layer - 1;
        static_for<NB>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const f4 res = epilogue(li, q, acc[q]);
#pragma unroll
            for (int r = 0; r < 4; ++r) X[q][r] = res[r];
        });
        tile_sum(li);
    }
}

}  // namespace cfd
