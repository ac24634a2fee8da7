// Dense masked DPS adjoint (K12): the residual norm ||y - m (.) A(z)||_2 of a whole
// measured field and its gradient w.r.t. the latent rows, in bounded memory.
//
// The Case4 adjoint (siren.hip: cfd_siren_tape_forward / cfd_siren_tape_vjp) keeps
// every layer's pre-activation and delta of every (row, point) pair in HBM:
// 2 R N (nh+1) H floats, 22.5 KB per pair at the Case2 widths (H = 256, nh = 10),
// 94 GB for one sample of 256 rows x 16384 points.  Here the N points are walked
// in chunks of whole 64-point slabs; per chunk
//   dense_tape_fwd      the fp32 MFMA chain of siren_tape_fwd, its pair tiles
//                       aligned to rows: grid (point tile, row), 4 waves x 16 points;
//   dense_residual      g = -m (y - m A) over (row, point, channel), written over A,
//                       and the slab's sum of squares as one double per (row, slab);
//   dense_tape_bwd      the chain of siren_tape_bwd on the same tiles.  SUM form: the
//                       tile's deltas are added on chip (16 points by a lane butterfly,
//                       the 4 waves in wave order through LDS) and one (nh+1) H partial
//                       is stored per tile; DELTA form: every delta is stored and
//                       dense_slab_sum adds each slab's 64 points after;
//   dense_accum         D[row] += the chunk's slab partials in slab order, and the
//                       row's sum of squares likewise.
// In split compute (the default) the chain is K9t instead (siren_split.hip): the
// K-split split-f16 tape forward over the chunk's pairs and the sum-mode K9t
// backward on row-aligned 16-point tiles, one partial per tile, four tiles added per
// slab by dense_slab_sum; or K9t's delta tape and the same column sums.
// The norm is one scalar per sample and the VJP is linear in its seed, so the
// backward is seeded with the unnormalised g and g_z = (D . V) / norm at the end.
// A slab is 64 consecutive points counted from point 0 (one fp32 tile, four K9t
// tiles), a chunk is a whole number of slabs and rows never mix: the reduction tree is a function of N
// alone, so the bits of g_z and of the norm depend neither on the budget nor on
// how many samples share the call.
#include <algorithm>
#include <cmath>

#include "siren.hpp"

namespace cfd {

constexpr int kSlab = CFD_DENSE_SLAB;   // 4 waves x 16 points

struct DenseArgs {
    const float* w0;
    const float* wimg;
    const float* wimg_t;
    const float* wout;
    const float* bout;
    const float* film;    // (rows of this block, nh+1, H)
    const float* coords;  // this chunk's first point
    const float* xmax;
    const float* xmin;
    const float* ymax;    // this chunk's first point (ystride > 0) or the (c) table
    const float* ymin;
    float* u;             // (rows, nc, nh+1, H)
    float* delta;         // (rows, nc, nh+1, H), DELTA form
    float* part;          // (rows, slabs, (nh+1) H) tile partials
    float* out;           // (rows, nc, c): A, then g in place
    int64_t ystride;
    int nc;               // points in this chunk
    int d, c, nh;
    float w0f;
};

template <int NB>
__global__ __launch_bounds__(256) void dense_tape_fwd(DenseArgs p) {
    constexpr int WAVES = 4, H = NB * 16, BLK = NB * 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wbuf = smem;
    float* w0s = smem + 2 * BLK;  // (H, 4)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, j16 = lane & 15;
    const int n = (int)blockIdx.x * kSlab + wave * 16 + j16;
    const bool live = n < p.nc;
    const int pt = live ? n : p.nc - 1;
    const int64_t row = blockIdx.y;
    const int nh = p.nh, nl = nh + 1;
    const float* film = p.film + row * nl * H;
    const int64_t pair = row * p.nc + pt;
    float* ut = p.u + pair * nl * H;
    CFD_DASSERT(pt >= 0 && pt < p.nc);

    for (int f = threadIdx.x; f < H; f += 64 * WAVES) {
        f4 w = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < p.d; ++k) w[k] = p.w0[f * p.d + k];
        *(f4*)(w0s + 4 * f) = w;
    }
    float cn[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < p.d) {
            float v = p.coords[(int64_t)pt * p.d + k];
            if (p.xmax) v = (v - p.xmin[k]) / (p.xmax[k] - p.xmin[k]) * 2.0f - 1.0f;
            cn[k] = v;
        }
    }
    __syncthreads();
    if (nh > 0) siren_issue_block<NB, WAVES>(p.wimg, 0, wbuf, wave, lane);

    float X[NB][4];
    static_for<NB>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const f4 fv = *(const f4*)(film + 16 * q + 4 * g);
        f4 uu;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f4 w = *(const f4*)(w0s + 4 * (16 * q + 4 * g + r));
            float a = cn[0] * w[0];
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (k < p.d) a = fmaf(cn[k], w[k], a);
            uu[r] = a + fv[r];
            X[q][r] = sin_cw(p.w0f * uu[r]);
        }
        if (live) *(f4*)(ut + 16 * q + 4 * g) = uu;
    });

    // block 0 landed in every wave's pieces before any wave reads it
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nblocks = nh * NB;
    int J = 0;
    for (int layer = 1; layer <= nh; ++layer) {
        f4 acc[NB];
        static_for<NB>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (J + 1 < nblocks) siren_issue_block<NB, WAVES>(p.wimg, J + 1, wbuf + ((J + 1) & 1) * BLK, wave, lane);
            const float* wb = wbuf + (J & 1) * BLK;
            // four interleaved accumulation chains (k-steps 0..3 of every 16), added
            // pairwise: no MFMA waits on the one before it, and the rounding error of
            // the K-long sum is that of the K-split tape kernels (four chains of K / 4)
            f4 a0 = *(const f4*)(film + layer * H + 16 * j + 4 * g);
            f4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
            static_for<NB>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                const f4 w = *(const f4*)(wb + (q * 64 + lane) * 4);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, X[q][0], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, X[q][1], a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, X[q][2], a2, 0, 0, 0);
                a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, X[q][3], a3, 0, 0, 0);
            });
            acc[j] = (a0 + a1) + (a2 + a3);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            ++J;
        });
        static_for<NB>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            if (live) *(f4*)(ut + layer * H + 16 * q + 4 * g) = acc[q];
#pragma unroll
            for (int r = 0; r < 4; ++r) X[q][r] = sin_cw(p.w0f * acc[q][r]);
        });
    }

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
            o[oc] = s + p.bout[oc];
        }
    }
    if (live && g < p.c) {
        float v = g == 0 ? o[0] : g == 1 ? o[1] : g == 2 ? o[2] : o[3];
        if (p.ymax) {
            const int64_t yi = (int64_t)pt * p.ystride + g;
            const float hi = p.ymax[yi], lo = p.ymin[yi];
            v = (v + 1.0f) / 2.0f * (hi - lo) + lo;
        }
        p.out[pair * p.c + g] = v;
    }
}

// SUM: store one (nh+1) H partial per tile; else every delta (siren_tape_bwd)
template <int NB, bool SUM>
__global__ __launch_bounds__(256) void dense_tape_bwd(DenseArgs p) {
    constexpr int WAVES = 4, H = NB * 16, BLK = NB * 256;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wbuf = smem;
    float* red = smem + 2 * BLK;   // SUM: WAVES x (nh+1) H sums over each wave's 16 points
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, j16 = lane & 15;
    const int n = (int)blockIdx.x * kSlab + wave * 16 + j16;
    const bool live = n < p.nc;
    const int pt = live ? n : p.nc - 1;
    const int64_t row = blockIdx.y;
    const int nh = p.nh, nl = nh + 1, nf = nl * H;
    const int64_t pair = row * p.nc + pt;
    const float* ut = p.u + pair * nl * H;
    float* dt = SUM ? nullptr : p.delta + pair * nl * H;
    const float w0f = p.w0f;
    CFD_DASSERT(pt >= 0 && pt < p.nc);

    if (nh > 0) siren_issue_block<NB, WAVES>(p.wimg_t, 0, wbuf, wave, lane);
    float dy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int oc = 0; oc < 4; ++oc) {
        if (oc < p.c) {
            float v = live ? p.out[pair * p.c + oc] : 0.f;
            if (p.ymax) {
                const int64_t yi = (int64_t)pt * p.ystride + oc;
                v = v * ((p.ymax[yi] - p.ymin[yi]) / 2.0f);
            }
            dy[oc] = v;
        }
    }
    // a dead lane's dy is zero, so every delta of it is an exact zero: it adds
    // nothing to the tile's sums
    auto emit = [&](int li, int q, f4 dd) {
        if constexpr (SUM) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1)
#pragma unroll
                for (int r = 0; r < 4; ++r) dd[r] += __shfl_xor(dd[r], m);
            if (j16 == 0) *(f4*)(red + wave * nf + li * H + 16 * q + 4 * g) = dd;
        } else {
            if (live) *(f4*)(dt + li * H + 16 * q + 4 * g) = dd;
        }
    };
    float X[NB][4];
    static_for<NB>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const f4 uu = *(const f4*)(ut + nh * H + 16 * q + 4 * g);
        f4 dd;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * q + 4 * g + r;
            float gx = 0.f;
#pragma unroll
            for (int oc = 0; oc < 4; ++oc)
                if (oc < p.c) gx = fmaf(p.wout[oc * H + f], dy[oc], gx);
            dd[r] = gx * (w0f * cos_cw(w0f * uu[r]));
            X[q][r] = dd[r];
        }
        emit(nh, q, dd);
    });

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // block 0: every wave's pieces
    __syncthreads();
    const int nblocks = nh * NB;
    int J = 0;
    for (int layer = nh; layer >= 1; --layer) {
        f4 acc[NB];
        static_for<NB>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (J + 1 < nblocks)
                siren_issue_block<NB, WAVES>(p.wimg_t, J + 1, wbuf + ((J + 1) & 1) * BLK, wave, lane);
            const float* wb = wbuf + (J & 1) * BLK;
            f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;   // four chains, as the forward
            static_for<NB>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                const f4 w = *(const f4*)(wb + (q * 64 + lane) * 4);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, X[q][0], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, X[q][1], a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, X[q][2], a2, 0, 0, 0);
                a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, X[q][3], a3, 0, 0, 0);
            });
            acc[j] = (a0 + a1) + (a2 + a3);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            ++J;
        });
        const int li = layer - 1;
        static_for<NB>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const f4 uu = *(const f4*)(ut + li * H + 16 * q + 4 * g);
            f4 dd;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dd[r] = acc[q][r] * (w0f * cos_cw(w0f * uu[r]));
                X[q][r] = dd[r];
            }
            emit(li, q, dd);
        });
    }
    if constexpr (SUM) {
        __syncthreads();
        float* dst = p.part + (row * gridDim.x + blockIdx.x) * nf;
        for (int i = threadIdx.x * 4; i < nf; i += 64 * WAVES * 4) {
            f4 s = *(const f4*)(red + i);
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s += *(const f4*)(red + w * nf + i);
            *(f4*)(dst + i) = s;
        }
    }
}

// g = -m (y - m A) written over A; the slab's sum of (y - m A)^2 in double.
// grid (slab of the chunk, row of the block); one value per thread (64 points x c <= 256).
__global__ __launch_bounds__(256) void dense_residual_kernel(float* __restrict__ Ag, const float* __restrict__ y,
                                                             int y_rows, const float* __restrict__ mask,
                                                             int mask_rows, int64_t N, int64_t n0, int nc, int c,
                                                             int64_t r0, double* __restrict__ sspart) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int s = blockIdx.x;
    const int64_t r = blockIdx.y;
    const int npts = min(kSlab, nc - s * kSlab);
    const int i = threadIdx.x;
    double sq = 0.0;
    if (i < npts * c) {
        const int pl = s * kSlab + i / c, k = i % c;
        CFD_DASSERT(pl < nc && n0 + pl < N);
        const int64_t ia = (r * nc + pl) * c + k;
        const int64_t it = (n0 + pl) * c + k;
        const float yv = y[((r0 + r) % y_rows) * N * c + it];
        const float m = mask ? mask[((r0 + r) % mask_rows) * N * c + it] : 1.0f;
        const float res = yv - m * Ag[ia];
        Ag[ia] = -(m * res);
        sq = (double)res * res;
    }
    red[i] = sq;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (i < w) red[i] += red[i + w];
        __syncthreads();
    }
    if (i == 0) sspart[r * gridDim.x + s] = red[0];
}

// part[row][slab] = sum of the slab's items, in item order (four in flight, as
// colsum_part_kernel): the 64 per-point deltas of the delta forms (per = 64), or the
// four 16-point tile sums of the sum-mode K9t backward (per = 4: (t0 + t1) + (t2 + t3))
__global__ __launch_bounds__(256) void dense_slab_sum(const float* __restrict__ items, float* __restrict__ part,
                                                      int n_items, int per, int64_t nf) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = blockIdx.y;
    const int s = blockIdx.z;
    if (f >= nf) return;
    const int p0 = s * per, p1 = min(n_items, p0 + per);
    CFD_DASSERT(p0 < n_items);
    const float* src = items + (r * n_items) * nf + f;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int q = p0;
    for (; q + 3 < p1; q += 4) {
        const float v0 = src[q * nf], v1 = src[(q + 1) * nf], v2 = src[(q + 2) * nf], v3 = src[(q + 3) * nf];
        a0 += v0;
        a1 += v1;
        a2 += v2;
        a3 += v3;
    }
    for (; q < p1; ++q) a0 += src[q * nf];
    part[(r * gridDim.z + s) * nf + f] = (a0 + a1) + (a2 + a3);
}

// D[row] += the chunk's slab partials, slab by slab; the rows' sums of squares likewise
__global__ __launch_bounds__(256) void dense_accum_kernel(const float* __restrict__ part,
                                                          const double* __restrict__ sspart, float* __restrict__ D,
                                                          double* __restrict__ rowss, int rows, int slabs,
                                                          int64_t nf) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows * nf) {
        const int64_t r = i / nf, f = i - r * nf;
        float s = D[i];
        for (int k = 0; k < slabs; ++k) s += part[(r * slabs + k) * nf + f];
        D[i] = s;
    }
    if (i < rows) {
        double s = rowss[i];
        for (int k = 0; k < slabs; ++k) s += sspart[i * slabs + k];
        rowss[i] = s;
    }
}

// norm[b] = sqrt(sum of the sample's row sums, in row order)
__global__ void dense_norm_kernel(const double* __restrict__ rowss, float* __restrict__ norm, int B, int T) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += rowss[(int64_t)b * T + t];
    norm[b] = (float)sqrt(s);
}

// g_z[r] /= norm of r's sample (zero where the norm is zero: cfd_dps_residual)
__global__ void dense_scale_kernel(float* __restrict__ gz, const float* __restrict__ norm, int64_t total, int64_t per) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float nb = norm[i / per];
    gz[i] = nb > 0.f ? gz[i] / nb : 0.f;
}

namespace {

size_t up64(size_t n) { return (n + 63) / 64 * 64; }

struct DensePlan {
    int rb = 0;           // rows per block
    int64_t ks = 0;       // slabs per chunk
    size_t floats = 0;    // workspace
    // offsets (floats)
    size_t film, D, gpart, rowss, u, delta, part, out, sspart;
};

// the layout for rb rows per block and ks slabs per chunk
// items: floats per (row, slab) of the per-item buffer: 64 nf (delta tape), 4 nf (K9t tile sums), 0
DensePlan dense_layout(const cfd_siren_cfg& cfg, int R, int rb, int64_t ks, size_t items) {
    const size_t nf = (size_t)(cfg.num_hidden_layers + 1) * cfg.hidden_features, L = cfg.in_latent_features;
    const size_t c = cfg.out_features, nc = (size_t)ks * kSlab;
    DensePlan p;
    p.rb = rb;
    p.ks = ks;
    size_t off = 0;
    auto take = [&](size_t n) {
        const size_t o = off;
        off += up64(n);
        return o;
    };
    p.film = take((size_t)R * nf);
    p.D = take((size_t)R * nf);
    p.gpart = take((size_t)gemm_splits((int)nf) * R * L);
    p.rowss = take(2 * (size_t)R);
    p.u = take((size_t)rb * nc * nf);
    p.delta = take((size_t)rb * ks * items);
    p.part = take((size_t)rb * ks * nf);
    p.out = take((size_t)rb * nc * c);
    p.sspart = take(2 * (size_t)rb * ks);
    p.floats = off;
    return p;
}

// the largest chunk within the budget: all R rows and as many slabs as fit, or,
// where one slab of all rows does not fit, one slab of as many rows as fit.
// A function of (configuration, R, budget, form) and of N only through the cap
// at N's own slab count.
DensePlan dense_plan(const cfd_siren_cfg& cfg, int64_t N, int R, size_t budget, size_t items) {
    CFD_REQUIRE(N >= 1 && R >= 1, CFD_EARG, "dense adjoint: empty problem");
    if (budget == 0) budget = CFD_DENSE_DEFAULT_BUDGET;
    const size_t bfl = budget / sizeof(float);
    const int64_t nslab = ceil_div(N, kSlab);
    const int rmax = std::min(R, 65535);
    const size_t fixed = dense_layout(cfg, R, 0, 0, items).floats;
    const size_t one = dense_layout(cfg, R, 1, 1, items).floats - fixed + 4 * 64;   // per (row, slab), with padding
    CFD_REQUIRE(bfl >= fixed + one, CFD_EARG, "dense adjoint: the budget is too small for one 64-point slab of one row");
    int rb = rmax;
    int64_t ks = (int64_t)((bfl - fixed) / (one * (size_t)rmax));
    if (ks < 1) {
        ks = 1;
        rb = (int)std::min<size_t>((size_t)rmax, (bfl - fixed) / one);
    }
    ks = std::min<int64_t>(std::min(ks, nslab), 65535);   // a grid dimension of the slab kernels
    DensePlan p = dense_layout(cfg, R, rb, ks, items);
    while (p.floats > bfl && (p.ks > 1 || p.rb > 1)) p = dense_layout(cfg, R, p.ks > 1 ? p.rb : p.rb - 1, p.ks > 1 ? p.ks - 1 : 1, items);
    CFD_REQUIRE(p.floats <= bfl, CFD_EARG, "dense adjoint: the budget is too small for one 64-point slab of one row");
    return p;
}

size_t bwd_sum_lds(const cfd_siren_cfg& cfg) {
    const size_t H = cfg.hidden_features, NB = H / 16;
    return sizeof(float) * (2 * NB * 256 + 4 * (size_t)(cfg.num_hidden_layers + 1) * H);
}

// the forms a call runs.  Compute: the K9t split-f16 tape kernels for a handle in
// split compute whose width K9t has a form for (measured faster at the Case2
// widths, profiles/dense_dps.json) unless the fp32 chain is asked for; a handle in
// CFD_SIREN_F32 always runs the exact fp32 chain.  Backward: the sum form unless
// the delta form is asked for, or, in the fp32 chain, the WAVES x (nh+1) H sums do
// not fit in LDS beside the weight ring.
bool split_width(const cfd_siren_cfg& cfg) {
    return cfg.num_hidden_layers >= 1 && cfg.hidden_features % 16 == 0 && tape_split_supported(cfg.hidden_features / 16);
}
void dense_forms_of(const cfd_siren_cfg& cfg, bool split_compute, int bwd_form, int compute_form, bool& split,
                    bool& delta) {
    split = split_compute && split_width(cfg) && compute_form != CFD_DENSE_COMPUTE_F32;
    delta = bwd_form == CFD_DENSE_BWD_DELTA || (!split && bwd_sum_lds(cfg) > 160 * 1024);
}
void dense_forms(const cfd_siren* h, bool& split, bool& delta) {
    dense_forms_of(h->cfg, h->compute == CFD_SIREN_SPLIT_F16, h->dense_bwd, h->dense_compute, split, delta);
}
// floats per (row, slab) of the per-item buffer
size_t dense_items(const cfd_siren_cfg& cfg, bool split, bool delta) {
    const size_t nf = (size_t)(cfg.num_hidden_layers + 1) * cfg.hidden_features;
    return delta ? (size_t)kSlab * nf : split ? (size_t)(kSlab / 16) * nf : 0;
}

template <int NB>
void launch_dense_nb(const DenseArgs& a, int rows, int mode, hipStream_t st) {
    const int H = NB * 16;
    const dim3 grid((unsigned)ceil_div(a.nc, kSlab), (unsigned)rows);
    if (mode == 0) {
        const size_t lds = sizeof(float) * (2 * NB * 256 + 4 * H);
        CFD_HIP(hipFuncSetAttribute((const void*)dense_tape_fwd<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((dense_tape_fwd<NB>), grid, dim3(256), lds, st, a);
        check_launch("dense_tape_fwd");
    } else if (mode == 1) {
        const size_t lds = sizeof(float) * (2 * NB * 256 + 4 * (size_t)(a.nh + 1) * H);
        CFD_HIP(hipFuncSetAttribute((const void*)dense_tape_bwd<NB, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
        hipLaunchKernelGGL((dense_tape_bwd<NB, true>), grid, dim3(256), lds, st, a);
        check_launch("dense_tape_bwd(sum)");
    } else {
        const size_t lds = sizeof(float) * (2 * NB * 256);
        CFD_HIP(hipFuncSetAttribute((const void*)dense_tape_bwd<NB, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
        hipLaunchKernelGGL((dense_tape_bwd<NB, false>), grid, dim3(256), lds, st, a);
        check_launch("dense_tape_bwd(delta)");
    }
}

// mode 0: forward; 1: sum backward; 2: delta backward
void launch_dense(int NB, const DenseArgs& a, int rows, int mode, hipStream_t st) {
    switch (NB) {
        case 1: return launch_dense_nb<1>(a, rows, mode, st);
        case 2: return launch_dense_nb<2>(a, rows, mode, st);
        case 3: return launch_dense_nb<3>(a, rows, mode, st);
        case 4: return launch_dense_nb<4>(a, rows, mode, st);
        case 6: return launch_dense_nb<6>(a, rows, mode, st);
        case 8: return launch_dense_nb<8>(a, rows, mode, st);
        case 12: return launch_dense_nb<12>(a, rows, mode, st);
        case 16: return launch_dense_nb<16>(a, rows, mode, st);
        case 24: return launch_dense_nb<24>(a, rows, mode, st);
        case 32: return launch_dense_nb<32>(a, rows, mode, st);
        default: throw Error{CFD_EARG, "hidden_features must be 16*{1,2,3,4,6,8,12,16,24,32}"};
    }
}

}  // namespace

// the chunk and tail steps shared with the dense Jacobian adjoint (K16, siren_jdense.hip)
void launch_dense_slab_sum(const float* items, float* part, int n_items, int per, int64_t nf, int rows, int slabs,
                           hipStream_t st) {
    hipLaunchKernelGGL(dense_slab_sum, dim3((unsigned)ceil_div(nf, 256), rows, slabs), dim3(256), 0, st, items, part,
                       n_items, per, nf);
    check_launch("dense_slab_sum");
}

void launch_dense_accum(const float* part, const double* sspart, float* D, double* rowss, int rows, int slabs,
                        int64_t nf, hipStream_t st) {
    hipLaunchKernelGGL(dense_accum_kernel, dim3((unsigned)ceil_div((int64_t)rows * nf, 256)), dim3(256), 0, st, part,
                       sspart, D, rowss, rows, slabs, nf);
    check_launch("dense_accum_kernel");
}

void dense_tail(const cfd_siren* h, const float* D, const double* rowss, float* norm, float* g_latents, float* gpart,
                int R, int T, hipStream_t st) {
    const int L = h->cfg.in_latent_features, B = R / T;
    const int nf = (h->cfg.num_hidden_layers + 1) * h->cfg.hidden_features;
    hipLaunchKernelGGL(dense_norm_kernel, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, st, rowss, norm, B, T);
    check_launch("dense_norm_kernel");
    launch_gemm_f32(false, D, nf, h->V, L, nullptr, g_latents, L, R, L, nf, st, gpart);
    hipLaunchKernelGGL(dense_scale_kernel, dim3((unsigned)ceil_div((int64_t)R * L, 256)), dim3(256), 0, st, g_latents,
                       norm, (int64_t)R * L, (int64_t)T * L);
    check_launch("dense_scale_kernel");
}

}  // namespace cfd

extern "C" int cfd_siren_dense_plan(const cfd_siren_cfg* cfg, int64_t N, int R, size_t budget, int bwd_form,
                                    int compute_form, size_t* bytes, int64_t* chunk_points, int* block_rows) {
    return cfd::guard([&] {
        CFD_REQUIRE(cfg && bytes, CFD_EARG, "null argument");
        CFD_REQUIRE(cfg->hidden_features >= 16 && cfg->hidden_features % 16 == 0 && cfg->num_hidden_layers >= 0 &&
                        cfg->in_latent_features >= 1 && cfg->out_features >= 1 && cfg->out_features <= 4,
                    CFD_EARG, "bad SIREN configuration");
        bool split, delta;
        cfd::dense_forms_of(*cfg, true, bwd_form, compute_form, split, delta);
        const cfd::DensePlan p = cfd::dense_plan(*cfg, N, R, budget, cfd::dense_items(*cfg, split, delta));
        *bytes = sizeof(float) * p.floats;
        if (chunk_points) *chunk_points = p.ks * cfd::kSlab;
        if (block_rows) *block_rows = p.rb;
    });
}

extern "C" int cfd_siren_dense_workspace_bytes(const cfd_siren* h, int64_t N, int R, size_t budget, size_t* bytes) {
    return cfd::guard([&] {
        CFD_REQUIRE(h && bytes, CFD_EARG, "null argument");
        bool split, delta;
        cfd::dense_forms(h, split, delta);
        *bytes = sizeof(float) * cfd::dense_plan(h->cfg, N, R, budget, cfd::dense_items(h->cfg, split, delta)).floats;
    });
}

extern "C" int cfd_siren_dense_set_form(cfd_siren* h, int bwd_form, int compute_form) {
    return cfd::guard([&] {
        CFD_REQUIRE(h, CFD_EARG, "null handle");
        CFD_REQUIRE(bwd_form == CFD_DENSE_BWD_SUM || bwd_form == CFD_DENSE_BWD_DELTA, CFD_EARG,
                    "unknown dense backward form");
        CFD_REQUIRE(compute_form == CFD_DENSE_COMPUTE_AUTO || compute_form == CFD_DENSE_COMPUTE_F32, CFD_EARG,
                    "unknown dense compute form");
        h->dense_bwd = bwd_form;
        h->dense_compute = compute_form;
    });
}

extern "C" int cfd_siren_dense_grad(cfd_siren* h, const float* coords, int64_t N, const float* latents, int R,
                                    int rows_per_sample, const float* xmax, const float* xmin, const float* ymax,
                                    const float* ymin, int64_t y_stride, const float* y, int y_rows,
                                    const float* mask, int mask_rows, float* g_latents, float* norm, void* ws,
                                    size_t ws_bytes, size_t budget, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(h && coords && latents && y && g_latents && norm && ws, CFD_EARG, "null argument");
        CFD_REQUIRE(N >= 1 && N <= ((int64_t)1 << 30) && R >= 1, CFD_EARG, "bad point / row count");
        const int T = rows_per_sample;
        CFD_REQUIRE(T >= 1 && R % T == 0, CFD_EARG, "rows_per_sample must divide the row count");
        CFD_REQUIRE(y_rows == T || y_rows == R, CFD_EARG, "y_rows must be rows_per_sample or R");
        CFD_REQUIRE(!mask || mask_rows == 1 || mask_rows == T || mask_rows == R, CFD_EARG,
                    "mask_rows must be 1, rows_per_sample or R");
        CFD_REQUIRE((xmax == nullptr) == (xmin == nullptr) && (ymax == nullptr) == (ymin == nullptr), CFD_EARG,
                    "normaliser bounds must be set in pairs");
        CFD_REQUIRE(((uintptr_t)ws & 15) == 0, CFD_EARG, "workspace must be 16-byte aligned");
        for (const auto& p : h->params) CFD_REQUIRE(p.set, CFD_ESTATE, "SIREN parameter not set: " + p.key);
        const int nh = h->cfg.num_hidden_layers, H = h->cfg.hidden_features, L = h->cfg.in_latent_features;
        const int c = h->cfg.out_features, d = h->cfg.in_coord_features;
        const int64_t nf = (int64_t)(nh + 1) * H;
        CFD_REQUIRE(L % 4 == 0 && nf % 16 == 0, CFD_ESHAPE,
                    "dense adjoint needs in_latent_features % 4 == 0 and (nh+1)*H % 16 == 0");
        bool split, delta;
        cfd::dense_forms(h, split, delta);
        const cfd::DensePlan pl = cfd::dense_plan(h->cfg, N, R, budget, cfd::dense_items(h->cfg, split, delta));
        CFD_REQUIRE(ws_bytes >= sizeof(float) * pl.floats, CFD_EARG, "workspace too small");
        cfd::DeviceGuard dg(h->device);
        auto st = (hipStream_t)stream;
        float* base = (float*)ws;
        float* film = base + pl.film;
        float* D = base + pl.D;
        double* rowss = (double*)(base + pl.rowss);
        double* sspart = (double*)(base + pl.sspart);
        cfd::film_vectors(h, latents, R, film, st);
        CFD_HIP(hipMemsetAsync(D, 0, sizeof(float) * (size_t)R * nf, st));
        CFD_HIP(hipMemsetAsync(rowss, 0, sizeof(double) * (size_t)R, st));
        const int64_t chunk = pl.ks * cfd::kSlab;
        for (int r0 = 0; r0 < R; r0 += pl.rb) {
            const int rows = std::min(pl.rb, R - r0);
            for (int64_t n0 = 0; n0 < N; n0 += chunk) {
                const int nc = (int)std::min<int64_t>(chunk, N - n0);
                const int slabs = (int)cfd::ceil_div(nc, cfd::kSlab);
                const float* cchunk = coords + n0 * d;
                const float* ymx = ymax ? ymax + n0 * y_stride : nullptr;
                const float* ymn = ymin ? ymin + n0 * y_stride : nullptr;
                if (split) {   // K9t: the K-split split-f16 tape kernels over the chunk's pairs
                    cfd::SirenTapeArgs a{};
                    a.w0 = h->w0;
                    a.wimg = h->wimg;
                    a.wimg_t = h->wimg_t;
                    a.wout = h->wout;
                    a.bout = h->bout;
                    a.film = film + (int64_t)r0 * nf;
                    a.coords = cchunk;
                    a.xmax = xmax;
                    a.xmin = xmin;
                    a.ymax = ymx;
                    a.ymin = ymn;
                    a.ystride = y_stride;
                    a.u = base + pl.u;
                    a.delta = base + pl.delta;
                    a.out = base + pl.out;
                    a.gout = base + pl.out;
                    a.wimg16 = h->wimg16;
                    a.wimg16t = h->wimg16t;
                    a.wscale = h->wscale;
                    a.P = (int64_t)rows * nc;
                    a.Ns = nc;
                    a.d = d;
                    a.c = c;
                    a.nh = nh;
                    a.w0f = h->cfg.w0;
                    cfd::launch_tape_split(h->NB, a, false, st);
                    hipLaunchKernelGGL(cfd::dense_residual_kernel, dim3(slabs, rows), dim3(256), 0, st, base + pl.out,
                                       y, y_rows, mask, mask ? mask_rows : 1, N, n0, nc, c, (int64_t)r0, sspart);
                    cfd::check_launch("dense_residual_kernel");
                    if (delta) cfd::launch_tape_split(h->NB, a, true, st);
                    else cfd::launch_tape_split_sum(h->NB, a, rows, st);   // a.delta: 16-point tile sums
                } else {
                    cfd::DenseArgs a{};
                    a.w0 = h->w0;
                    a.wimg = h->wimg;
                    a.wimg_t = h->wimg_t;
                    a.wout = h->wout;
                    a.bout = h->bout;
                    a.film = film + (int64_t)r0 * nf;
                    a.coords = cchunk;
                    a.xmax = xmax;
                    a.xmin = xmin;
                    a.ymax = ymx;
                    a.ymin = ymn;
                    a.ystride = y_stride;
                    a.u = base + pl.u;
                    a.delta = base + pl.delta;
                    a.part = base + pl.part;
                    a.out = base + pl.out;
                    a.nc = nc;
                    a.d = d;
                    a.c = c;
                    a.nh = nh;
                    a.w0f = h->cfg.w0;
                    cfd::launch_dense(h->NB, a, rows, 0, st);
                    hipLaunchKernelGGL(cfd::dense_residual_kernel, dim3(slabs, rows), dim3(256), 0, st, base + pl.out,
                                       y, y_rows, mask, mask ? mask_rows : 1, N, n0, nc, c, (int64_t)r0, sspart);
                    cfd::check_launch("dense_residual_kernel");
                    cfd::launch_dense(h->NB, a, rows, delta ? 2 : 1, st);
                }
                if (delta || split) {
                    const int n_items = delta ? nc : (int)cfd::ceil_div(nc, 16), per = delta ? cfd::kSlab : cfd::kSlab / 16;
                    cfd::launch_dense_slab_sum(base + pl.delta, base + pl.part, n_items, per, nf, rows, slabs, st);
                }
                cfd::launch_dense_accum(base + pl.part, sspart, D + (int64_t)r0 * nf, rowss + r0, rows, slabs, nf, st);
            }
        }
        cfd::dense_tail(h, D, rowss, norm, g_latents, base + pl.gpart, R, T, st);
    });
}
