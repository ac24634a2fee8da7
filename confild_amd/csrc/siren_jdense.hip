// Dense derivative measurements for DPS in bounded memory (K16): the residual norm
//   || y - m (.) A(z) ||_2,  A[r, n, m] = sum_o wv[n, m, o] out[r, n, o] + sum_{o,k} wj[n, m, o, k] jac[r, n, o, k]
// of linear stencils on the decoded value and its exact coordinate Jacobian at every
// point of a field (vorticity, divergence, wall shear; value readings too), and its
// gradient w.r.t. the latent rows.
//
// The Jacobian adjoint K15 (siren_jtape.hip) keeps (2 + d) (nh+1) H floats of tape
// and deltas per (row, point) pair in HBM: 45 KB at the Case2 widths, 189 GB for one
// sample of 256 rows x 16384 points.  Here K12's driver (dps_dense.hip) walks the N
// points in chunks of whole 64-point slabs around the DENSE forms of K15's kernels
// (siren_jtape.hpp); per chunk
//   siren_jtape_fwd<DENSE>   K15's chain on row-aligned tiles, grid (point tile, row):
//                            the chunk's tape (rows, nc, nh+1, 1+d, H), out and jac;
//   jdense_residual          per (row, point): A, r = y - m A, g = -m r contracted to
//                            g_out = wv^T g and g_jac = wj^T g over out / jac in place,
//                            and the slab's sum of r^2 as one double per (row, slab);
//   siren_jtape_bwd<DENSE>   K15's reverse chain seeded with g_out / g_jac; u-bar is
//                            summed over the tile on chip, one (nh+1) H partial per tile;
//   dense_slab_sum           a slab's tiles (64 / TILE of them) added in tile order
//                            (not launched where the tile is the slab, d = 1 at NB <= 24);
//   dense_accum              D[row] += the chunk's slabs in slab order, sums of squares too.
// Then norm[b] = sqrt(the sample's row sums) and g_z = (D . V) / norm (dense_tail).
// The backward is seeded with the unnormalised g because the norm is known only
// after the last chunk and the VJP is linear in its seed.  No delta tape: the chunk
// holds (1 + d) rows nc (nh+1) H floats of tape, out, jac, the tile and slab partials.
// No atomics: tile, slab, chunk and row sums all run in index order, slabs count from
// point 0 of the call and a chunk is a whole number of slabs, so the reduction tree is
// a function of N alone and the bits of g_z and of the norms depend neither on the
// budget, nor on the row blocking, nor on the samples sharing the call.
// Always the exact fp32 chain, whatever cfd_siren_set_compute chose.
#include <algorithm>

#include "siren_jtape.hpp"

namespace cfd {

constexpr int kJSlab = CFD_DENSE_SLAB;

// One thread per point of the slab, readings in reading order; grid (slab of the
// chunk, row of the block).  y / mask: tables of (N, M), row r0 + r reads table
// (r0 + r) % rows; wv (M, c) or (N, M, c), wj (M, c, d) or (N, M, c, d).
__global__ __launch_bounds__(kJSlab) void jdense_residual_kernel(
    float* __restrict__ out, float* __restrict__ jac, const float* __restrict__ wv, int wv_pp,
    const float* __restrict__ wj, int wj_pp, const float* __restrict__ y, int y_rows, const float* __restrict__ mask,
    int mask_rows, int64_t N, int64_t n0, int nc, int M, int c, int d, int64_t r0, double* __restrict__ sspart) {
#pragma clang fp contract(off)
    __shared__ double red[kJSlab];
    const int s = blockIdx.x;
    const int64_t r = blockIdx.y;
    const int npts = min(kJSlab, nc - s * kJSlab);
    const int i = threadIdx.x;
    double sq = 0.0;
    if (i < npts) {
        const int pl = s * kJSlab + i;
        const int64_t pg = n0 + pl;            // the point of the call
        const int64_t pair = r * nc + pl;      // the pair of the chunk
        CFD_DASSERT(pl < nc && pg < N && c >= 1 && c <= 4 && d >= 1 && d <= 3 && (wv || wj));
        CFD_DASSERT(pair >= 0 && pair < (int64_t)gridDim.y * nc);
        float o[4] = {0.f, 0.f, 0.f, 0.f}, J[12];
        float go[4] = {0.f, 0.f, 0.f, 0.f}, gj[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) J[k] = gj[k] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < c) o[k] = out[pair * c + k];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < c * d) J[k] = jac[pair * c * d + k];
        const float* yt = y ? y + ((r0 + r) % y_rows) * N * M + pg * M : nullptr;
        const float* mt = mask ? mask + ((r0 + r) % mask_rows) * N * M + pg * M : nullptr;
        const float* wvp = wv ? wv + (wv_pp ? pg * M * c : 0) : nullptr;
        const float* wjp = wj ? wj + (wj_pp ? pg * M * c * d : 0) : nullptr;
        for (int m = 0; m < M; ++m) {
            CFD_DASSERT(!wv_pp || (pg * M + m + 1) * c <= N * M * c);
            CFD_DASSERT(!wj_pp || (pg * M + m + 1) * c * d <= N * M * c * d);
            CFD_DASSERT(pg * M + m < N * M);
            float A = 0.f;
            if (wvp) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < c) A += wvp[m * c + k] * o[k];
            }
            if (wjp) {
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    if (k < c * d) A += wjp[m * c * d + k] * J[k];
            }
            const float mm = mt ? mt[m] : 1.0f;
            const float res = (yt ? yt[m] : 0.0f) - mm * A;
            const float g = -(mm * res);
            sq += (double)res * res;
            if (wvp) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < c) go[k] += wvp[m * c + k] * g;
            }
            if (wjp) {
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    if (k < c * d) gj[k] += wjp[m * c * d + k] * g;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < c) out[pair * c + k] = go[k];
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < c * d) jac[pair * c * d + k] = gj[k];
    }
    red[i] = sq;
    __syncthreads();
    if (i == 0) {
        double t = 0.0;
        for (int k = 0; k < npts; ++k) t += red[k];   // point order
        CFD_DASSERT(s < (int)gridDim.x);
        sspart[r * gridDim.x + s] = t;
    }
}

namespace {

size_t jup64(size_t n) { return (n + 63) / 64 * 64; }

// K15's tile: 16 / RS pairs per wave, 8 waves at NB <= 24 and 4 at NB = 32
int jdense_tile(const cfd_siren_cfg& cfg) {
    const int RS = cfg.in_coord_features == 1 ? 2 : 4, NB = cfg.hidden_features / 16;
    return (16 / RS) * (NB <= 24 ? 8 : 4);
}

struct JDensePlan {
    int rb = 0;           // rows per block
    int64_t ks = 0;       // slabs per chunk
    size_t floats = 0;    // workspace
    // offsets (floats)
    size_t film, D, gpart, rowss, tape, tiles, part, out, jac, sspart;
};

JDensePlan jdense_layout(const cfd_siren_cfg& cfg, int R, int rb, int64_t ks) {
    const size_t nf = (size_t)(cfg.num_hidden_layers + 1) * cfg.hidden_features, L = cfg.in_latent_features;
    const size_t c = cfg.out_features, d = cfg.in_coord_features, nc = (size_t)ks * kJSlab;
    JDensePlan p;
    p.rb = rb;
    p.ks = ks;
    size_t off = 0;
    auto take = [&](size_t n) {
        const size_t o = off;
        off += jup64(n);
        return o;
    };
    p.film = take((size_t)R * nf);
    p.D = take((size_t)R * nf);
    p.gpart = take((size_t)gemm_splits((int)nf) * R * L);
    p.rowss = take(2 * (size_t)R);
    p.tape = take((size_t)rb * nc * (1 + d) * nf);
    const size_t per = kJSlab / jdense_tile(cfg);   // tiles per slab; 1: the tile partials are the slab partials
    p.tiles = take((size_t)rb * ks * per * nf);
    p.part = per > 1 ? take((size_t)rb * ks * nf) : p.tiles;
    p.out = take((size_t)rb * nc * c);
    p.jac = take((size_t)rb * nc * c * d);
    p.sspart = take(2 * (size_t)rb * ks);
    p.floats = off;
    return p;
}

void jdense_cfg_check(const cfd_siren_cfg& cfg) {
    CFD_REQUIRE(cfg.hidden_features >= 16 && cfg.hidden_features % 16 == 0 && cfg.num_hidden_layers >= 0 &&
                    cfg.in_latent_features >= 1 && cfg.out_features >= 1 && cfg.out_features <= 4 &&
                    cfg.in_coord_features >= 1,
                CFD_EARG, "bad SIREN configuration");
    CFD_REQUIRE(cfg.in_coord_features <= 3, CFD_EARG,
                "cfd_siren_jdense: in_coord_features must be 1..3 (the 1 + d chains of a pair share 4 MFMA columns)");
}

// dense_plan's rule (dps_dense.hip): all R rows and as many slabs as fit, or, where one
// slab of all rows does not fit, one slab of as many rows as fit
JDensePlan jdense_plan(const cfd_siren_cfg& cfg, int64_t N, int R, int M, size_t budget) {
    jdense_cfg_check(cfg);
    CFD_REQUIRE(N >= 1 && N <= ((int64_t)1 << 30) && R >= 1, CFD_EARG, "dense Jacobian adjoint: bad point / row count");
    CFD_REQUIRE(M >= 1, CFD_EARG, "dense Jacobian adjoint: at least one reading per point");
    if (budget == 0) budget = CFD_DENSE_DEFAULT_BUDGET;
    const size_t bfl = budget / sizeof(float);
    const int64_t nslab = ceil_div(N, kJSlab);
    const int rmax = std::min(R, 65535);
    const size_t fixed = jdense_layout(cfg, R, 0, 0).floats;
    const size_t one = jdense_layout(cfg, R, 1, 1).floats - fixed + 6 * 64;   // per (row, slab), with padding
    const char* small = "dense Jacobian adjoint: the budget is too small for one 64-point slab of one row";
    CFD_REQUIRE(bfl >= fixed + one, CFD_EARG, small);
    int rb = rmax;
    int64_t ks = (int64_t)((bfl - fixed) / (one * (size_t)rmax));
    if (ks < 1) {
        ks = 1;
        rb = (int)std::min<size_t>((size_t)rmax, (bfl - fixed) / one);
    }
    ks = std::min<int64_t>(std::min(ks, nslab), 65535);   // a grid dimension of the slab kernels
    JDensePlan p = jdense_layout(cfg, R, rb, ks);
    while (p.floats > bfl && (p.ks > 1 || p.rb > 1))
        p = jdense_layout(cfg, R, p.ks > 1 ? p.rb : p.rb - 1, p.ks > 1 ? p.ks - 1 : 1);
    CFD_REQUIRE(p.floats <= bfl, CFD_EARG, small);
    return p;
}

template <int NB, int RS>
void launch_jdense_nb(const SirenJDenseArgs& a, int rows, bool bwd, hipStream_t st) {
    constexpr int WAVES = NB <= 24 ? 8 : 4, TILE = (16 / RS) * WAVES, H = NB * 16;
    static_assert(kJSlab % TILE == 0, "a slab is a whole number of tiles");
    const size_t lds = sizeof(float) * (2 * NB * 256 + (bwd ? WAVES * H : 4 * H));
    const void* fn = bwd ? (const void*)siren_jtape_bwd<NB, RS, WAVES, true>
                         : (const void*)siren_jtape_fwd<NB, RS, WAVES, true>;
    CFD_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)ceil_div(a.Ns, TILE), (unsigned)rows);
    if (bwd)
        hipLaunchKernelGGL((siren_jtape_bwd<NB, RS, WAVES, true>), grid, dim3(64 * WAVES), lds, st, a);
    else
        hipLaunchKernelGGL((siren_jtape_fwd<NB, RS, WAVES, true>), grid, dim3(64 * WAVES), lds, st, a);
    check_launch(bwd ? "siren_jtape_bwd(dense)" : "siren_jtape_fwd(dense)");
}

template <int RS>
void launch_jdense(int nb, const SirenJDenseArgs& a, int rows, bool bwd, hipStream_t st) {
    dispatch_nb(nb, [&](auto nbc) { launch_jdense_nb<decltype(nbc)::value, RS>(a, rows, bwd, st); });
}

}  // namespace
}  // namespace cfd

extern "C" int cfd_siren_jdense_plan(const cfd_siren_cfg* cfg, int64_t N, int R, int M, size_t budget, size_t* bytes,
                                     int64_t* chunk_points, int* block_rows) {
    return cfd::guard([&] {
        CFD_REQUIRE(cfg && bytes, CFD_EARG, "null argument");
        const cfd::JDensePlan p = cfd::jdense_plan(*cfg, N, R, M, budget);
        *bytes = sizeof(float) * p.floats;
        if (chunk_points) *chunk_points = p.ks * cfd::kJSlab;
        if (block_rows) *block_rows = p.rb;
    });
}

extern "C" int cfd_siren_jdense_workspace_bytes(const cfd_siren* h, int64_t N, int R, int M, size_t budget,
                                                size_t* bytes) {
    return cfd::guard([&] {
        CFD_REQUIRE(h && bytes, CFD_EARG, "null argument");
        *bytes = sizeof(float) * cfd::jdense_plan(h->cfg, N, R, M, budget).floats;
    });
}

extern "C" int cfd_siren_jdense_grad(cfd_siren* h, const float* coords, int64_t N, const float* latents, int R,
                                     int rows_per_sample, const float* xmax, const float* xmin, const float* ymax,
                                     const float* ymin, int64_t y_stride, const float* wv, int wv_per_point,
                                     const float* wj, int wj_per_point, int M, const float* y, int y_rows,
                                     const float* mask, int mask_rows, float* g_latents, float* norm, void* ws,
                                     size_t ws_bytes, size_t budget, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(h && coords && latents && g_latents && norm && ws, CFD_EARG, "null argument");
        CFD_REQUIRE(wv || wj, CFD_EARG, "value weights, Jacobian weights or both must be set");
        CFD_REQUIRE(M >= 1, CFD_EARG, "at least one reading per point");
        CFD_REQUIRE(N >= 1 && N <= ((int64_t)1 << 30) && R >= 1, CFD_EARG, "bad point / row count");
        const int T = rows_per_sample;
        CFD_REQUIRE(T >= 1 && R % T == 0, CFD_EARG, "rows_per_sample must divide the row count");
        CFD_REQUIRE(!y || y_rows == T || y_rows == R, CFD_EARG, "y_rows must be rows_per_sample or R");
        CFD_REQUIRE(!mask || mask_rows == 1 || mask_rows == T || mask_rows == R, CFD_EARG,
                    "mask_rows must be 1, rows_per_sample or R");
        CFD_REQUIRE((xmax == nullptr) == (xmin == nullptr) && (ymax == nullptr) == (ymin == nullptr), CFD_EARG,
                    "normaliser bounds must be set in pairs");
        CFD_REQUIRE(((uintptr_t)ws & 15) == 0, CFD_EARG, "workspace must be 16-byte aligned");
        for (const auto& p : h->params) CFD_REQUIRE(p.set, CFD_ESTATE, "SIREN parameter not set: " + p.key);
        const int nh = h->cfg.num_hidden_layers, H = h->cfg.hidden_features, L = h->cfg.in_latent_features;
        const int c = h->cfg.out_features, d = h->cfg.in_coord_features;
        const int64_t nf = (int64_t)(nh + 1) * H;
        const cfd::JDensePlan pl = cfd::jdense_plan(h->cfg, N, R, M, budget);   // d <= 3 and the budget
        CFD_REQUIRE(L % 4 == 0 && nf % 16 == 0, CFD_ESHAPE,
                    "dense Jacobian adjoint needs in_latent_features % 4 == 0 and (nh+1)*H % 16 == 0");
        CFD_REQUIRE(ws_bytes >= sizeof(float) * pl.floats, CFD_EARG, "workspace too small");
        cfd::DeviceGuard dg(h->device);
        auto st = (hipStream_t)stream;
        float* base = (float*)ws;
        float* film = base + pl.film;
        float* D = base + pl.D;
        double* rowss = (double*)(base + pl.rowss);
        double* sspart = (double*)(base + pl.sspart);
        const int tile = cfd::jdense_tile(h->cfg), per = cfd::kJSlab / tile;
        cfd::film_vectors(h, latents, R, film, st);
        CFD_HIP(hipMemsetAsync(D, 0, sizeof(float) * (size_t)R * nf, st));
        CFD_HIP(hipMemsetAsync(rowss, 0, sizeof(double) * (size_t)R, st));
        const int64_t chunk = pl.ks * cfd::kJSlab;
        for (int r0 = 0; r0 < R; r0 += pl.rb) {
            const int rows = std::min(pl.rb, R - r0);
            for (int64_t n0 = 0; n0 < N; n0 += chunk) {
                const int nc = (int)std::min<int64_t>(chunk, N - n0);
                const int slabs = (int)cfd::ceil_div(nc, cfd::kJSlab);
                const int tiles = (int)cfd::ceil_div(nc, tile);
                cfd::SirenJDenseArgs a{};
                cfd::handle_args(a, h);
                a.wimg_t = h->wimg_t;
                a.film = film + (int64_t)r0 * nf;
                a.coords = coords + n0 * d;
                a.xmax = xmax;
                a.xmin = xmin;
                a.ymax = ymax ? ymax + n0 * y_stride : nullptr;
                a.ymin = ymin ? ymin + n0 * y_stride : nullptr;
                a.ystride = y_stride;
                a.tape = base + pl.tape;
                a.out = base + pl.out;
                a.jac = base + pl.jac;
                a.gout = wv ? base + pl.out : nullptr;
                a.gjac = wj ? base + pl.jac : nullptr;
                a.part = base + pl.tiles;
                a.P = (int64_t)rows * nc;
                a.Ns = nc;
                if (d == 1) cfd::launch_jdense<2>(h->NB, a, rows, false, st);
                else cfd::launch_jdense<4>(h->NB, a, rows, false, st);
                hipLaunchKernelGGL(cfd::jdense_residual_kernel, dim3(slabs, rows), dim3(cfd::kJSlab), 0, st,
                                   base + pl.out, base + pl.jac, wv, wv_per_point, wj, wj_per_point, y, y ? y_rows : 1,
                                   mask, mask ? mask_rows : 1, N, n0, nc, M, c, d, (int64_t)r0, sspart);
                cfd::check_launch("jdense_residual_kernel");
                if (d == 1) cfd::launch_jdense<2>(h->NB, a, rows, true, st);
                else cfd::launch_jdense<4>(h->NB, a, rows, true, st);
                if (per > 1) cfd::launch_dense_slab_sum(base + pl.tiles, base + pl.part, tiles, per, nf, rows, slabs, st);
                cfd::launch_dense_accum(base + pl.part, sspart, D + (int64_t)r0 * nf, rowss + r0, rows, slabs, nf, st);
            }
        }
        cfd::dense_tail(h, D, rowss, norm, g_latents, base + pl.gpart, R, T, st);
    });
}
