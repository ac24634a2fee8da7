// Diffusion sampler epilogue (K6), Philox normals and latent de-normalisation.
//
// cfd_sched_step replaces, for ModelMeanType.EPSILON + ModelVarType.FIXED_LARGE,
//   _predict_xstart_from_eps -> clamp(-1,1) -> q_posterior_mean_variance
//   -> sample = mean + nonzero_mask * exp(0.5*logvar) * noise
// (U/src/gaussian_diffusion.py:300-314,328-333,208-230,395-439) and the DDIM
// update (:537-585).  Coefficients are the reference's float64 tables cast to
// fp32 per timestep (cast done once on the host, _extract_into_tensor :899-912);
// the elementwise maths is evaluated in the reference's operation order with
// fp contraction disabled, so for identical (x, eps, noise) the result is the
// reference's bit for bit.
#include <cmath>
#include <string>

#include "common.hpp"
#include "sampler.hpp"

namespace cfd {

struct Philox {
    static __device__ __forceinline__ uint4 round(uint4 c, uint2 k) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
        return make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k.x, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k.y,
                          (uint32_t)p0);
    }
    static __device__ __forceinline__ uint4 gen(uint64_t seed, uint64_t ctr_lo, uint64_t ctr_hi) {
        uint4 c = make_uint4((uint32_t)ctr_lo, (uint32_t)(ctr_lo >> 32), (uint32_t)ctr_hi, (uint32_t)(ctr_hi >> 32));
        uint2 k = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            c = round(c, k);
            k.x += 0x9E3779B9u;
            k.y += 0xBB67AE85u;
        }
        return c;
    }
    // Four N(0,1) floats for group `grp` of stream (seed, counter).
    static __device__ __forceinline__ void normal4(uint64_t seed, uint64_t counter, uint64_t grp, float z[4]) {
        const uint4 r = gen(seed, grp, counter);
        const float u1 = ((float)r.x + 1.0f) * 2.3283064365386963e-10f;  // (0, 1]
        const float u2 = (float)r.y * 2.3283064365386963e-10f;
        const float u3 = ((float)r.z + 1.0f) * 2.3283064365386963e-10f;
        const float u4 = (float)r.w * 2.3283064365386963e-10f;
        const float r1 = sqrtf(-2.0f * logf(fminf(u1, 1.0f)));
        const float r2 = sqrtf(-2.0f * logf(fminf(u3, 1.0f)));
        float s1, c1, s2, c2;
        sincospif(2.0f * u2, &s1, &c1);
        sincospif(2.0f * u4, &s2, &c2);
        z[0] = r1 * c1;
        z[1] = r1 * s1;
        z[2] = r2 * c2;
        z[3] = r2 * s2;
    }
};

__global__ void randn_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t counter, uint64_t goff) {
    const int64_t grp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t base = grp * 4;
    if (base >= n) return;
    float z[4];
    Philox::normal4(seed, counter, goff + (uint64_t)grp, z);
    if (base + 3 < n) {
        *(f4*)(out + base) = f4{z[0], z[1], z[2], z[3]};  // out 16-B aligned when n % 4 == 0 (checked by caller)
    } else {
        for (int j = 0; j < 4 && base + j < n; ++j) out[base + j] = z[j];
    }
}

struct StepArgs {
    const float* coefs;  // (n_t, CFD_NCOEF)
    const float* x;
    const float* eps;
    const int64_t* t;
    const float* noise;  // may be null -> Philox
    float* x_out;
    float* xs_out;       // may be null
    int64_t n;           // elements per sample
    int64_t total;       // B * n
    uint64_t seed, counter, goff;  // goff: Philox group offset (= element offset / 4)
    int kind, clip;
    const SamplerCtl* ctl;         // native loop: (seed, counter, goff) from device memory, or null
};

// Known-row replacement (step_kernel<true, *>): after the step's sample s,
//   q = a_i * known + b_i * n2,  out = m * q + (1 - m) * s
// with (a_i, b_i) = (sqrt(abar_prev[i]), sqrt(1 - abar_prev[i])) from `tab`.
struct KnownArgs {
    const float* known;   // (1 | B, n)
    const float* mask;    // (1 | B, n), values in [0, 1]
    int64_t known_bstride, mask_bstride;   // 0 (shared) or n
    const float* tab;     // (n_t, 2)
    const float* noise2;  // may be null -> Philox(seed, counter2)
    uint64_t counter2;    // read from ctl->counter2 in the native loop
};

// Resampling jump (step_kernel<true, true>): after the known-row step's out,
//   out = ja * out + jb * z3
// the merged forward step from the level the step produced up to level `to`,
// (ja, jb) = (sqrt(rho), sqrt(1 - rho)), rho = abar[to] / abar[i - 1].  jb == 0
// (a step of the schedule that does not jump) leaves the known-row step's bits.
struct JumpArgs {
    float ja, jb;
    const float* noise3;  // may be null -> Philox(seed, counter3)
    uint64_t counter3;    // read from ctl->counter3 in the native loop
    const float* jtab;    // native loop: (n_steps, 2) rows (ja, jb) indexed by the step number, or null
    int64_t n_steps;      // rows of jtab
};

template <bool KNOWN, bool JUMP>
__global__ void step_kernel(StepArgs a, KnownArgs kn, JumpArgs jp) {
#pragma clang fp contract(off)
    const int64_t grp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t base = grp * 4;
    if (base >= a.total) return;
    float z[4];
    if (a.noise) {
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = (base + j < a.total) ? a.noise[base + j] : 0.f;
    } else if (a.ctl) {
        Philox::normal4(a.ctl->seed, a.ctl->counter, a.ctl->goff + (uint64_t)grp, z);
    } else {
        Philox::normal4(a.seed, a.counter, a.goff + (uint64_t)grp, z);
    }
    float z2[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (KNOWN) {
        if (kn.noise2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) z2[j] = (base + j < a.total) ? kn.noise2[base + j] : 0.f;
        } else if (a.ctl) {
            Philox::normal4(a.ctl->seed, a.ctl->counter2, a.ctl->goff + (uint64_t)grp, z2);
        } else {
            Philox::normal4(a.seed, kn.counter2, a.goff + (uint64_t)grp, z2);
        }
    }
    float ja = 1.0f, jb = 0.0f;
    float z3[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (JUMP) {
        ja = jp.ja;
        jb = jp.jb;
        if (jp.jtab) {
            // the step number is the same for the whole launch: a uniform load
            const uint64_t k = a.ctl->counter;
            CFD_DASSERT(k < (uint64_t)jp.n_steps);
            ja = jp.jtab[k * 2];
            jb = jp.jtab[k * 2 + 1];
        }
        if (jb != 0.0f) {
            if (jp.noise3) {
#pragma unroll
                for (int j = 0; j < 4; ++j) z3[j] = (base + j < a.total) ? jp.noise3[base + j] : 0.f;
            } else if (a.ctl) {
                Philox::normal4(a.ctl->seed, a.ctl->counter3, a.ctl->goff + (uint64_t)grp, z3);
            } else {
                Philox::normal4(a.seed, jp.counter3, a.goff + (uint64_t)grp, z3);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = base + j;
        if (i >= a.total) break;
        const int64_t b = i / a.n;
        const int64_t t = a.t[b];
        const float* c = a.coefs + t * CFD_NCOEF;
        const float x = a.x[i], e = a.eps[i];
        // pred_xstart = sqrt_recip_ac * x - sqrt_recipm1_ac * eps   (:328-333)
        float xs = c[CFD_COEF_SRA] * x - c[CFD_COEF_SRM1] * e;
        if (a.clip) xs = fminf(fmaxf(xs, -1.0f), 1.0f);
        const float mask = t != 0 ? 1.0f : 0.0f;
        float out;
        if (a.kind == CFD_STEP_DDPM) {
            // mean = coef1 * x0 + coef2 * x_t   (:217-220); sample (:431-438)
            const float mean = c[CFD_COEF_M1] * xs + c[CFD_COEF_M2] * x;
            out = mean + mask * c[CFD_COEF_SIGMA] * z[j];
        } else {
            // eps' = (sra * x - x0) / srm1 (:345-349); mean_pred (:566-570)
            const float e2 = (c[CFD_COEF_SRA] * x - xs) / c[CFD_COEF_SRM1];
            const float mean = xs * c[CFD_COEF_SQRT_ABP] + c[CFD_COEF_DIR] * e2;
            out = mean + mask * c[CFD_COEF_SIGMA_DDIM] * z[j];
        }
        if constexpr (KNOWN) {
            const int64_t e = i - b * a.n;
            const float m = kn.mask[b * kn.mask_bstride + e];
            const float q = kn.tab[t * 2] * kn.known[b * kn.known_bstride + e] + kn.tab[t * 2 + 1] * z2[j];
            out = m * q + (1.0f - m) * out;
        }
        if constexpr (JUMP) {
            if (jb != 0.0f) out = ja * out + jb * z3[j];
        }
        a.x_out[i] = out;
        if (a.xs_out) a.xs_out[i] = xs;
    }
}

__global__ void latent_denorm_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n,
                                     const float* __restrict__ vmax, const float* __restrict__ vmin, int64_t period) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t k = i % period;
    // (gen + 1) * (max - min) / 2. + min   (scripts/inference.py:61)
    y[i] = (x[i] + 1.0f) * (vmax[k] - vmin[k]) / 2.0f + vmin[k];
}

// ---------------------------------------------------------------------------
// DPS glue: the elementwise links of
// d||y - A(x0_hat)|| / d x_t that are not the U-Net or SIREN adjoints.
// ---------------------------------------------------------------------------
// per sample b: r = y - A, norm_b = ||r||_2 (float64 sum), g_A = -r / norm_b
// (torch.linalg.norm backward; zero gradient where the norm is 0), condition_methods.py:33-35
__global__ __launch_bounds__(256) void dps_residual_kernel(const float* __restrict__ y, int64_t y_bstride,
                                                           const float* __restrict__ A, float* __restrict__ gA,
                                                           float* __restrict__ norm, int64_t n) {
    const int64_t b = blockIdx.x;
    const float* yb = y + b * y_bstride;
    const float* Ab = A + b * n;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float r = yb[i] - Ab[i];
        s += (double)r * r;
    }
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float nb = (float)sqrt(red[0]);
    if (threadIdx.x == 0) norm[b] = nb;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float r = yb[i] - Ab[i];
        gA[b * n + i] = nb > 0.f ? -(r / nb) : 0.f;
    }
}

// Linear sensor stencils on the value and the coordinate Jacobian (K15's residual):
//   A[r, s, m] = sum_o wv[s, m, o] out[r, s, o] + sum_{o,k} wj[s, m, o, k] jac[r, s, o, k]
// per sample b (rows_per_sample rows): norm_b = ||y - A||_2 (float64 sum, the order of
// dps_residual_kernel), g_out = wv^T (-(y - A) / norm_b), g_jac = wj^T (-(y - A) / norm_b);
// zero gradients where the norm is 0.  One thread per (row, sensor); A is formed by
// the same code in both passes, so the gradient uses the residual the norm summed.
struct DpsLinearArgs {
    const float* y;       // (rows_per_sample | R, Ns, M)
    const float* out;     // (R, Ns, c)
    const float* jac;     // (R, Ns, c, d) or null
    const float* wv;      // (1 | Ns, M, c) or null
    const float* wj;      // (1 | Ns, M, c, d) or null
    float* g_out;         // (R, Ns, c) or null
    float* g_jac;         // (R, Ns, c, d) or null
    float* norm;          // (B)
    float* A;             // (R, Ns, M) or null
    int64_t wv_stride, wj_stride;   // per sensor: 0 (shared) or M c / M c d
    int y_per_sample, Ns, M, c, d, rows;
};

__device__ __forceinline__ float dps_linear_A(const DpsLinearArgs& p, const float* o, const float* j, int s, int m) {
    float a = 0.f;
    if (p.wv) {
        const float* w = p.wv + s * p.wv_stride + (int64_t)m * p.c;
        for (int q = 0; q < p.c; ++q) a = fmaf(w[q], o[q], a);
    }
    if (p.wj) {
        const float* w = p.wj + s * p.wj_stride + (int64_t)m * p.c * p.d;
        for (int q = 0; q < p.c * p.d; ++q) a = fmaf(w[q], j[q], a);
    }
    return a;
}

__global__ __launch_bounds__(256) void dps_residual_linear(DpsLinearArgs p) {
    const int64_t b = blockIdx.x;
    const int np = p.rows * p.Ns;   // (row, sensor) pairs of the sample
    const int cd = p.c * p.d;
    double sum = 0.0;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        const int64_t pr = b * np + i;
        const int s = i % p.Ns;
        const float* yb = p.y + (p.y_per_sample ? pr : (int64_t)i) * p.M;
        const float* o = p.out + pr * p.c;
        const float* j = p.jac ? p.jac + pr * cd : nullptr;
        for (int m = 0; m < p.M; ++m) {
            const float a = dps_linear_A(p, o, j, s, m);
            if (p.A) p.A[pr * p.M + m] = a;
            const float r = yb[m] - a;
            sum += (double)r * r;
        }
    }
    __shared__ double red[256];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float nb = (float)sqrt(red[0]);
    if (threadIdx.x == 0) p.norm[b] = nb;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        const int64_t pr = b * np + i;
        const int s = i % p.Ns;
        const float* yb = p.y + (p.y_per_sample ? pr : (int64_t)i) * p.M;
        const float* o = p.out + pr * p.c;
        const float* j = p.jac ? p.jac + pr * cd : nullptr;
        float go[4] = {0.f, 0.f, 0.f, 0.f};
        float gj[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int m = 0; m < p.M; ++m) {
            const float r = yb[m] - dps_linear_A(p, o, j, s, m);
            const float gm = nb > 0.f ? -(r / nb) : 0.f;
            if (p.wv) {
                const float* w = p.wv + s * p.wv_stride + (int64_t)m * p.c;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < p.c) go[q] = fmaf(w[q], gm, go[q]);
            }
            if (p.wj) {
                const float* w = p.wj + s * p.wj_stride + (int64_t)m * cd;
#pragma unroll
                for (int q = 0; q < 12; ++q)
                    if (q < cd) gj[q] = fmaf(w[q], gm, gj[q]);
            }
        }
        if (p.g_out) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < p.c) p.g_out[pr * p.c + q] = go[q];
        }
        if (p.g_jac) {
#pragma unroll
            for (int q = 0; q < 12; ++q)
                if (q < cd) p.g_jac[pr * cd + q] = gj[q];
        }
    }
}

// g_z -> (d_eps, g_direct) through Case4Operator._unnorm (measurements.py:219-220),
// clamp(-1, 1) (posterior_mean_variance.py:40-45; gradient passes on the closed
// interval) and x0 = sra * x - srm1 * eps (:120-123)
__global__ void dps_latent_grad_kernel(const float* __restrict__ coefs, int clip, const float* __restrict__ x,
                                       const float* __restrict__ eps, const int64_t* __restrict__ t,
                                       const float* __restrict__ gz, const float* __restrict__ vmax,
                                       const float* __restrict__ vmin, int64_t period, float* __restrict__ d_eps,
                                       float* __restrict__ g_direct, int64_t n, int64_t total) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / n, k = i % period;
    const float* c = coefs + t[b] * CFD_NCOEF;
    const float x0u = c[CFD_COEF_SRA] * x[i] - c[CFD_COEF_SRM1] * eps[i];
    const bool pass = !clip || (x0u >= -1.0f && x0u <= 1.0f);
    const float gx0 = (gz[i] / 2.0f) * (vmax[k] - vmin[k]);
    const float g = pass ? gx0 : 0.0f;
    d_eps[i] = -g * c[CFD_COEF_SRM1];
    g_direct[i] = g * c[CFD_COEF_SRA];
}

// ---------------------------------------------------------------------------
// 'inpainting' under 'ps' (measurements.py:40-56, A(x0) = mask * x0 on the latent
// image): residual norm and the two latent-gradient links in one call, no SIREN.
// Per sample: x0 as step_kernel's xs (the same expression), r = y - m * x0,
// norm = ||r||_2 in float64.  The sum runs over fixed chunks of LR_CHUNK elements:
// thread t of chunk c adds elements c * LR_CHUNK + t + 256 j (j ascending), the
// 256 thread sums fold by halves, and the chunk partials add in chunk order -- a
// function of n_per_sample alone, whatever B or the grid.  No atomics.
// ---------------------------------------------------------------------------
constexpr int LR_CHUNK = 4096;

struct LatentResArgs {
    const float* coefs;
    const float* x;
    const float* eps;
    const int64_t* t;
    const float* y;
    const float* mask;
    int64_t y_bstride, mask_bstride;
    int64_t n;       // elements per sample
    int clip;
};

__device__ __forceinline__ float latent_x0(const LatentResArgs& a, const float* c, int64_t i, bool* pass) {
#pragma clang fp contract(off)
    float xs = c[CFD_COEF_SRA] * a.x[i] - c[CFD_COEF_SRM1] * a.eps[i];
    *pass = !a.clip || (xs >= -1.0f && xs <= 1.0f);
    if (a.clip) xs = fminf(fmaxf(xs, -1.0f), 1.0f);
    return xs;
}

// grid (chunks, B): partial[b * chunks + c] = sum of r^2 over chunk c of sample b
__global__ __launch_bounds__(256) void dps_latent_partial_kernel(LatentResArgs a, double* __restrict__ partial) {
#pragma clang fp contract(off)
    const int64_t b = blockIdx.y;
    const float* c = a.coefs + a.t[b] * CFD_NCOEF;
    const int64_t lo = (int64_t)blockIdx.x * LR_CHUNK;
    const int64_t hi = lo + LR_CHUNK < a.n ? lo + LR_CHUNK : a.n;
    double s = 0.0;
    for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
        bool pass;
        const float x0 = latent_x0(a, c, b * a.n + e, &pass);
        const float r = a.y[b * a.y_bstride + e] - a.mask[b * a.mask_bstride + e] * x0;
        s += (double)r * r;
    }
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[b * gridDim.x + blockIdx.x] = red[0];
}

// grid (chunks, B): norm_b from the partials in chunk order, then
// g = -m * (r / norm_b) (zero where the norm is 0, or where the clamp cut x0),
// d_eps = -g * srm1, g_direct = g * sra   (as dps_latent_grad_kernel)
__global__ __launch_bounds__(256) void dps_latent_residual_kernel(LatentResArgs a, const double* __restrict__ partial,
                                                                  float* __restrict__ norm, float* __restrict__ d_eps,
                                                                  float* __restrict__ g_direct) {
#pragma clang fp contract(off)
    const int64_t b = blockIdx.y;
    const float* c = a.coefs + a.t[b] * CFD_NCOEF;
    double s = 0.0;
    for (unsigned k = 0; k < gridDim.x; ++k) s += partial[b * gridDim.x + k];
    const float nb = (float)sqrt(s);
    if (blockIdx.x == 0 && threadIdx.x == 0) norm[b] = nb;
    const int64_t lo = (int64_t)blockIdx.x * LR_CHUNK;
    const int64_t hi = lo + LR_CHUNK < a.n ? lo + LR_CHUNK : a.n;
    for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
        const int64_t i = b * a.n + e;
        bool pass;
        const float x0 = latent_x0(a, c, i, &pass);
        const float m = a.mask[b * a.mask_bstride + e];
        const float r = a.y[b * a.y_bstride + e] - m * x0;
        const float g = (pass && nb > 0.f) ? -(m * (r / nb)) : 0.0f;
        d_eps[i] = -g * c[CFD_COEF_SRM1];
        g_direct[i] = g * c[CFD_COEF_SRA];
    }
}

// x_t -= (d/dx_prev) * scale   (condition_methods.py:88)
__global__ void dps_update_kernel(const float* __restrict__ sample, const float* __restrict__ g_direct,
                                  const float* __restrict__ g_unet, float scale, float* __restrict__ x_out,
                                  int64_t n) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    x_out[i] = sample[i] - (g_direct[i] + g_unet[i]) * scale;
}

// cfd_dps_update followed by known-row replacement (the guided sampler with known rows):
//   img = sample - (g_direct + g_unet) * scale     (dps_update_kernel's expression, the same bits)
//   q   = a_i * known + b_i * n2,  out = m * q + (1 - m) * img     (step_kernel<true, *>'s, the same bits)
// Four elements per thread and step_kernel's Philox group offset, so n2 is the
// normal step_kernel<true, false> draws for the same (seed, counter2, offset).
struct DpsKnownArgs {
    const float* sample;
    const float* g_direct;
    const float* g_unet;
    float scale;
    float* x_out;
    const int64_t* t;     // (B) table indices
    int64_t n;            // elements per sample
    int64_t total;        // B * n
    uint64_t seed, goff;  // goff: Philox group offset (= element offset / 4)
    int vec;              // every array 16-byte aligned and n % 4 == 0: a group is one f4 of one sample
};

__device__ __forceinline__ float dps_known_elem(float s, float gd, float gu, float scale, float a, float b, float kv,
                                                float m, float z2) {
#pragma clang fp contract(off)
    const float img = s - (gd + gu) * scale;
    const float q = a * kv + b * z2;
    return m * q + (1.0f - m) * img;
}

__global__ void dps_update_known_kernel(DpsKnownArgs a, KnownArgs kn) {
#pragma clang fp contract(off)
    const int64_t grp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t base = grp * 4;
    if (base >= a.total) return;
    float z2[4];
    if (kn.noise2) {
        if (a.vec) {
            const f4 v = *(const f4*)(kn.noise2 + base);
            z2[0] = v.x, z2[1] = v.y, z2[2] = v.z, z2[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) z2[j] = (base + j < a.total) ? kn.noise2[base + j] : 0.f;
        }
    } else {
        Philox::normal4(a.seed, kn.counter2, a.goff + (uint64_t)grp, z2);
    }
    if (a.vec) {
        // n % 4 == 0: the group's four elements belong to one sample
        const int64_t b = base / a.n;
        const int64_t e = base - b * a.n;
        CFD_DASSERT(base + 3 < a.total && e + 3 < a.n);
        const int64_t t = a.t[b];
        const float ta = kn.tab[t * 2], tb = kn.tab[t * 2 + 1];
        const f4 s = *(const f4*)(a.sample + base);
        const f4 gd = *(const f4*)(a.g_direct + base);
        const f4 gu = *(const f4*)(a.g_unet + base);
        const f4 kv = *(const f4*)(kn.known + b * kn.known_bstride + e);
        const f4 m = *(const f4*)(kn.mask + b * kn.mask_bstride + e);
        f4 o;
        o.x = dps_known_elem(s.x, gd.x, gu.x, a.scale, ta, tb, kv.x, m.x, z2[0]);
        o.y = dps_known_elem(s.y, gd.y, gu.y, a.scale, ta, tb, kv.y, m.y, z2[1]);
        o.z = dps_known_elem(s.z, gd.z, gu.z, a.scale, ta, tb, kv.z, m.z, z2[2]);
        o.w = dps_known_elem(s.w, gd.w, gu.w, a.scale, ta, tb, kv.w, m.w, z2[3]);
        *(f4*)(a.x_out + base) = o;
        return;
    }
    // unaligned arrays or n % 4 != 0 (a group may straddle samples, the last one may be short)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = base + j;
        if (i >= a.total) break;
        const int64_t b = i / a.n;
        const int64_t e = i - b * a.n;
        const int64_t t = a.t[b];
        a.x_out[i] = dps_known_elem(a.sample[i], a.g_direct[i], a.g_unet[i], a.scale, kn.tab[t * 2], kn.tab[t * 2 + 1],
                                    kn.known[b * kn.known_bstride + e], kn.mask[b * kn.mask_bstride + e], z2[j]);
    }
}

// native loop bookkeeping (one workgroup): the step's timesteps from the
// host-built sequences, and the step counter for the Philox stream
__global__ void sampler_advance_kernel(SamplerCtl* ctl, const int64_t* __restrict__ tidx_seq,
                                       const int64_t* __restrict__ tmodel_seq, int64_t* __restrict__ t_idx,
                                       int64_t* __restrict__ t_model, int B) {
    const uint64_t k = ctl->k;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        t_idx[b] = tidx_seq[k];
        t_model[b] = tmodel_seq[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ctl->counter = k;
        ctl->counter2 = CFD_KNOWN_COUNTER + k;
        ctl->counter3 = CFD_JUMP_COUNTER + k;
        ctl->k = k + 1;
    }
}

__global__ void sampler_set_kernel(SamplerCtl* ctl, uint64_t k, uint64_t seed, uint64_t goff) {
    if (threadIdx.x == 0) {
        ctl->k = k;
        ctl->counter = k;
        ctl->counter2 = CFD_KNOWN_COUNTER + k;
        ctl->counter3 = CFD_JUMP_COUNTER + k;
        ctl->seed = seed;
        ctl->goff = goff;
    }
}

}  // namespace cfd

struct cfd_sched {
    float* coefs = nullptr;
    int n_t = 0;
    int device = 0;
};

namespace cfd {
const float* sched_coefs(const cfd_sched* s) { return s->coefs; }
int sched_nt(const cfd_sched* s) { return s->n_t; }

void launch_sampler_advance(SamplerCtl* ctl, const int64_t* tidx_seq, const int64_t* tmodel_seq, int64_t* t_idx,
                            int64_t* t_model, int B, hipStream_t st) {
    hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(64), 0, st, ctl, tidx_seq, tmodel_seq, t_idx, t_model, B);
    check_launch("sampler_advance_kernel");
}

void launch_sampler_set(SamplerCtl* ctl, uint64_t k, uint64_t seed, uint64_t goff, hipStream_t st) {
    hipLaunchKernelGGL(sampler_set_kernel, dim3(1), dim3(64), 0, st, ctl, k, seed, goff);
    check_launch("sampler_set_kernel");
}

void launch_sched_step_ctl(const cfd_sched* s, int kind, int clip, float* x, const float* eps, const int64_t* t,
                           const SamplerCtl* ctl, int64_t n_per_sample, int B, hipStream_t st) {
    StepArgs a{s->coefs, x, eps, t, nullptr, x, nullptr, n_per_sample, n_per_sample * B, 0, 0, 0, kind, clip, ctl};
    const int64_t groups = ceil_div(a.total, 4);
    hipLaunchKernelGGL((step_kernel<false, false>), dim3((unsigned)ceil_div(groups, 256)), dim3(256), 0, st, a, KnownArgs{},
                       JumpArgs{});
    check_launch("step_kernel");
}

void launch_sched_step_known_ctl(const cfd_sched* s, int kind, int clip, float* x, const float* eps, const int64_t* t,
                                 const SamplerCtl* ctl, const float* known, const float* mask, const float* table,
                                 int64_t n_per_sample, int B, hipStream_t st) {
    StepArgs a{s->coefs, x, eps, t, nullptr, x, nullptr, n_per_sample, n_per_sample * B, 0, 0, 0, kind, clip, ctl};
    KnownArgs kn{known, mask, n_per_sample, n_per_sample, table, nullptr, 0};
    const int64_t groups = ceil_div(a.total, 4);
    hipLaunchKernelGGL((step_kernel<true, false>), dim3((unsigned)ceil_div(groups, 256)), dim3(256), 0, st, a, kn,
                       JumpArgs{});
    check_launch("step_kernel<known>");
}

void launch_sched_step_jump_ctl(const cfd_sched* s, int kind, int clip, float* x, const float* eps, const int64_t* t,
                                const SamplerCtl* ctl, const float* known, const float* mask, const float* table,
                                const float* jtab, int n_steps, int64_t n_per_sample, int B, hipStream_t st) {
    StepArgs a{s->coefs, x, eps, t, nullptr, x, nullptr, n_per_sample, n_per_sample * B, 0, 0, 0, kind, clip, ctl};
    KnownArgs kn{known, mask, n_per_sample, n_per_sample, table, nullptr, 0};
    JumpArgs jp{1.0f, 0.0f, nullptr, 0, jtab, n_steps};
    const int64_t groups = ceil_div(a.total, 4);
    hipLaunchKernelGGL((step_kernel<true, true>), dim3((unsigned)ceil_div(groups, 256)), dim3(256), 0, st, a, kn, jp);
    check_launch("step_kernel<known, jump>");
}
}  // namespace cfd

extern "C" int cfd_sched_create(const float* host_coefs, int n_t, int device, cfd_sched** out) {
    return cfd::guard([&] {
        CFD_REQUIRE(host_coefs && out && n_t > 0, CFD_EARG, "bad argument");
        cfd::DeviceGuard dg(device);
        auto* s = new cfd_sched();
        s->n_t = n_t;
        s->device = device;
        CFD_HIP(hipMalloc(&s->coefs, sizeof(float) * n_t * CFD_NCOEF));
        CFD_HIP(hipMemcpy(s->coefs, host_coefs, sizeof(float) * n_t * CFD_NCOEF, hipMemcpyHostToDevice));
        *out = s;
    });
}

extern "C" void cfd_sched_destroy(cfd_sched* s) {
    if (!s) return;
    (void)hipFree(s->coefs);
    delete s;
}

extern "C" int cfd_sched_step(const cfd_sched* s, int kind, int clip, const float* x, const float* eps,
                              const int64_t* t, const float* noise, uint64_t seed, uint64_t counter, uint64_t offset,
                              float* x_out, float* xstart_out, int64_t n_per_sample, int B, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(s && x && eps && t && x_out, CFD_EARG, "null argument");
        CFD_REQUIRE(offset % 4 == 0, CFD_EARG, "noise offset must be a multiple of 4");
        CFD_REQUIRE(kind == CFD_STEP_DDPM || kind == CFD_STEP_DDIM, CFD_EARG, "unknown step kind");
        CFD_REQUIRE(n_per_sample > 0 && B > 0, CFD_EARG, "empty step");
        cfd::StepArgs a{s->coefs, x, eps, t, noise, x_out, xstart_out, n_per_sample, n_per_sample * B,
                        seed, counter, offset / 4, kind, clip, nullptr};
        const int64_t groups = cfd::ceil_div(a.total, 4);
        hipLaunchKernelGGL((cfd::step_kernel<false, false>), dim3((unsigned)cfd::ceil_div(groups, 256)), dim3(256), 0,
                           (hipStream_t)stream, a, cfd::KnownArgs{}, cfd::JumpArgs{});
        cfd::check_launch("step_kernel");
    });
}

extern "C" int cfd_sched_step_known(const cfd_sched* s, int kind, int clip, const float* x, const float* eps,
                                    const int64_t* t, const float* noise, uint64_t seed, uint64_t counter,
                                    uint64_t offset, float* x_out, float* xstart_out, int64_t n_per_sample, int B,
                                    const float* known, int64_t known_bstride, const float* mask,
                                    int64_t mask_bstride, const float* table, const float* noise2, uint64_t counter2,
                                    void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(s && x && eps && t && x_out && known && mask && table, CFD_EARG, "null argument");
        CFD_REQUIRE(offset % 4 == 0, CFD_EARG, "noise offset must be a multiple of 4");
        CFD_REQUIRE(kind == CFD_STEP_DDPM || kind == CFD_STEP_DDIM, CFD_EARG, "unknown step kind");
        CFD_REQUIRE(n_per_sample > 0 && B > 0, CFD_EARG, "empty step");
        CFD_REQUIRE((known_bstride == 0 || known_bstride == n_per_sample) &&
                        (mask_bstride == 0 || mask_bstride == n_per_sample),
                    CFD_EARG, "known rows and mask must be shared (stride 0) or per sample (stride n)");
        cfd::StepArgs a{s->coefs, x, eps, t, noise, x_out, xstart_out, n_per_sample, n_per_sample * B,
                        seed, counter, offset / 4, kind, clip, nullptr};
        cfd::KnownArgs kn{known, mask, known_bstride, mask_bstride, table, noise2, counter2};
        const int64_t groups = cfd::ceil_div(a.total, 4);
        hipLaunchKernelGGL((cfd::step_kernel<true, false>), dim3((unsigned)cfd::ceil_div(groups, 256)), dim3(256), 0,
                           (hipStream_t)stream, a, kn, cfd::JumpArgs{});
        cfd::check_launch("step_kernel<known>");
    });
}

extern "C" int cfd_sched_step_jump(const cfd_sched* s, int kind, int clip, const float* x, const float* eps,
                                   const int64_t* t, const float* noise, uint64_t seed, uint64_t counter,
                                   uint64_t offset, float* x_out, float* xstart_out, int64_t n_per_sample, int B,
                                   const float* known, int64_t known_bstride, const float* mask,
                                   int64_t mask_bstride, const float* table, const float* noise2, uint64_t counter2,
                                   float ja, float jb, const float* noise3, uint64_t counter3, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(s && x && eps && t && x_out && known && mask && table, CFD_EARG, "null argument");
        CFD_REQUIRE(offset % 4 == 0, CFD_EARG, "noise offset must be a multiple of 4");
        CFD_REQUIRE(kind == CFD_STEP_DDPM || kind == CFD_STEP_DDIM, CFD_EARG, "unknown step kind");
        CFD_REQUIRE(n_per_sample > 0 && B > 0, CFD_EARG, "empty step");
        CFD_REQUIRE((known_bstride == 0 || known_bstride == n_per_sample) &&
                        (mask_bstride == 0 || mask_bstride == n_per_sample),
                    CFD_EARG, "known rows and mask must be shared (stride 0) or per sample (stride n)");
        cfd::StepArgs a{s->coefs, x, eps, t, noise, x_out, xstart_out, n_per_sample, n_per_sample * B,
                        seed, counter, offset / 4, kind, clip, nullptr};
        cfd::KnownArgs kn{known, mask, known_bstride, mask_bstride, table, noise2, counter2};
        cfd::JumpArgs jp{ja, jb, noise3, counter3, nullptr, 0};
        const int64_t groups = cfd::ceil_div(a.total, 4);
        hipLaunchKernelGGL((cfd::step_kernel<true, true>), dim3((unsigned)cfd::ceil_div(groups, 256)), dim3(256), 0,
                           (hipStream_t)stream, a, kn, jp);
        cfd::check_launch("step_kernel<known, jump>");
    });
}

extern "C" int cfd_randn(float* out, int64_t n, uint64_t seed, uint64_t counter, uint64_t offset, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(out && n > 0, CFD_EARG, "bad argument");
        CFD_REQUIRE(offset % 4 == 0, CFD_EARG, "noise offset must be a multiple of 4");
        CFD_REQUIRE(((uintptr_t)out & 15) == 0, CFD_EARG, "randn output must be 16-byte aligned");
        const int64_t groups = cfd::ceil_div(n, 4);
        hipLaunchKernelGGL(cfd::randn_kernel, dim3((unsigned)cfd::ceil_div(groups, 256)), dim3(256), 0,
                           (hipStream_t)stream, out, n, seed, counter, offset / 4);
        cfd::check_launch("randn_kernel");
    });
}

extern "C" int cfd_latent_denorm(const float* x, float* y, int64_t n, const float* vmax, const float* vmin,
                                 int64_t period, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(x && y && vmax && vmin && n > 0 && period > 0, CFD_EARG, "bad argument");
        hipLaunchKernelGGL(cfd::latent_denorm_kernel, dim3((unsigned)cfd::ceil_div(n, 256)), dim3(256), 0,
                           (hipStream_t)stream, x, y, n, vmax, vmin, period);
        cfd::check_launch("latent_denorm_kernel");
    });
}

extern "C" int cfd_dps_residual(const float* y, int64_t y_batch_stride, const float* A, float* g_A, float* norm,
                                int64_t n_per_sample, int B, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(y && A && g_A && norm && n_per_sample > 0 && B > 0, CFD_EARG, "bad argument");
        CFD_REQUIRE(y_batch_stride == 0 || y_batch_stride == n_per_sample, CFD_EARG,
                    "measurement must be shared (stride 0) or per sample (stride n)");
        hipLaunchKernelGGL(cfd::dps_residual_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, y, y_batch_stride, A,
                           g_A, norm, n_per_sample);
        cfd::check_launch("dps_residual_kernel");
    });
}

extern "C" int cfd_dps_residual_linear(const float* y, int y_per_sample, const float* out, const float* jac,
                                       const float* wv, int wv_per_sensor, const float* wj, int wj_per_sensor,
                                       float* g_out, float* g_jac, float* norm, float* A, int64_t Ns, int M, int c,
                                       int d, int rows_per_sample, int B, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(y && out && norm && (wv || wj), CFD_EARG, "null argument (at least one weight set is required)");
        CFD_REQUIRE((wv == nullptr) == (g_out == nullptr), CFD_EARG, "wv and g_out must both be set or both NULL");
        CFD_REQUIRE((wj == nullptr) == (g_jac == nullptr) && (!wj || jac), CFD_EARG,
                    "wj, jac and g_jac must all be set or wj and g_jac both NULL");
        CFD_REQUIRE(Ns >= 1 && Ns <= (1 << 20) && M >= 1 && c >= 1 && c <= 4 && d >= 1 && d <= 3 &&
                        rows_per_sample >= 1 && B >= 1,
                    CFD_EARG, "bad shape (c <= 4, d <= 3)");
        CFD_REQUIRE((int64_t)rows_per_sample * Ns <= 0x7fffffff, CFD_EARG, "too many (row, sensor) pairs per sample");
        cfd::DpsLinearArgs p{};
        p.y = y;
        p.out = out;
        p.jac = jac;
        p.wv = wv;
        p.wj = wj;
        p.g_out = g_out;
        p.g_jac = g_jac;
        p.norm = norm;
        p.A = A;
        p.wv_stride = wv_per_sensor ? (int64_t)M * c : 0;
        p.wj_stride = wj_per_sensor ? (int64_t)M * c * d : 0;
        p.y_per_sample = y_per_sample;
        p.Ns = (int)Ns;
        p.M = M;
        p.c = c;
        p.d = d;
        p.rows = rows_per_sample;
        hipLaunchKernelGGL(cfd::dps_residual_linear, dim3(B), dim3(256), 0, (hipStream_t)stream, p);
        cfd::check_launch("dps_residual_linear");
    });
}

extern "C" int cfd_dps_latent_grad(const cfd_sched* s, int clip, const float* x, const float* eps, const int64_t* t,
                                   const float* g_z, const float* vmax, const float* vmin, int64_t period,
                                   float* d_eps, float* g_direct, int64_t n_per_sample, int B, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(s && x && eps && t && g_z && vmax && vmin && d_eps && g_direct, CFD_EARG, "null argument");
        CFD_REQUIRE(n_per_sample > 0 && B > 0 && period > 0 && n_per_sample % period == 0, CFD_EARG,
                    "latent bounds must tile the latent");
        const int64_t total = n_per_sample * B;
        hipLaunchKernelGGL(cfd::dps_latent_grad_kernel, dim3((unsigned)cfd::ceil_div(total, 256)), dim3(256), 0,
                           (hipStream_t)stream, s->coefs, clip, x, eps, t, g_z, vmax, vmin, period, d_eps, g_direct,
                           n_per_sample, total);
        cfd::check_launch("dps_latent_grad_kernel");
    });
}

extern "C" int cfd_dps_latent_residual_workspace_bytes(int64_t n_per_sample, int B, size_t* bytes) {
    return cfd::guard([&] {
        CFD_REQUIRE(bytes && n_per_sample > 0 && B > 0, CFD_EARG, "bad argument");
        *bytes = sizeof(double) * (size_t)cfd::ceil_div(n_per_sample, (int64_t)cfd::LR_CHUNK) * (size_t)B;
    });
}

extern "C" int cfd_dps_latent_residual(const cfd_sched* s, int clip, const float* x, const float* eps,
                                       const int64_t* t, const float* y, int64_t y_bstride, const float* mask,
                                       int64_t mask_bstride, float* norm, float* d_eps, float* g_direct,
                                       int64_t n_per_sample, int B, void* workspace, size_t ws_bytes, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(s && x && eps && t && y && mask && norm && d_eps && g_direct && workspace, CFD_EARG,
                    "null argument");
        CFD_REQUIRE(n_per_sample > 0 && B > 0 && B <= 65535, CFD_EARG, "batch outside 1..65535");
        CFD_REQUIRE((y_bstride == 0 || y_bstride == n_per_sample) && (mask_bstride == 0 || mask_bstride == n_per_sample),
                    CFD_EARG, "measurement and mask must be shared (stride 0) or per sample (stride n)");
        const int64_t chunks = cfd::ceil_div(n_per_sample, (int64_t)cfd::LR_CHUNK);
        CFD_REQUIRE(ws_bytes >= sizeof(double) * (size_t)chunks * (size_t)B, CFD_EARG, "workspace too small");
        CFD_REQUIRE(((uintptr_t)workspace & 7) == 0, CFD_EARG, "workspace must be 8-byte aligned");
        cfd::LatentResArgs a{s->coefs, x, eps, t, y, mask, y_bstride, mask_bstride, n_per_sample, clip};
        const dim3 grid((unsigned)chunks, (unsigned)B);
        hipLaunchKernelGGL(cfd::dps_latent_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, a,
                           (double*)workspace);
        cfd::check_launch("dps_latent_partial_kernel");
        hipLaunchKernelGGL(cfd::dps_latent_residual_kernel, grid, dim3(256), 0, (hipStream_t)stream, a,
                           (const double*)workspace, norm, d_eps, g_direct);
        cfd::check_launch("dps_latent_residual_kernel");
    });
}

extern "C" int cfd_dps_update(const float* sample, const float* g_direct, const float* g_unet, float scale,
                              float* x_out, int64_t n, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(sample && g_direct && g_unet && x_out && n > 0, CFD_EARG, "bad argument");
        hipLaunchKernelGGL(cfd::dps_update_kernel, dim3((unsigned)cfd::ceil_div(n, 256)), dim3(256), 0,
                           (hipStream_t)stream, sample, g_direct, g_unet, scale, x_out, n);
        cfd::check_launch("dps_update_kernel");
    });
}

extern "C" int cfd_dps_update_known(const float* sample, const float* g_direct, const float* g_unet, float scale,
                                    float* x_out, const int64_t* t, int64_t n_per_sample, int B, const float* known,
                                    int64_t known_bstride, const float* mask, int64_t mask_bstride, const float* table,
                                    const float* noise2, uint64_t seed, uint64_t counter2, uint64_t offset,
                                    void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(sample && g_direct && g_unet && x_out && t && known && mask && table, CFD_EARG, "null argument");
        CFD_REQUIRE(offset % 4 == 0, CFD_EARG, "noise offset must be a multiple of 4");
        CFD_REQUIRE(n_per_sample > 0 && B > 0, CFD_EARG, "empty step");
        CFD_REQUIRE((known_bstride == 0 || known_bstride == n_per_sample) &&
                        (mask_bstride == 0 || mask_bstride == n_per_sample),
                    CFD_EARG, "known rows and mask must be shared (stride 0) or per sample (stride n)");
        const uintptr_t bits = (uintptr_t)sample | (uintptr_t)g_direct | (uintptr_t)g_unet | (uintptr_t)x_out |
                               (uintptr_t)known | (uintptr_t)mask | (uintptr_t)noise2;
        const int vec = (bits & 15) == 0 && n_per_sample % 4 == 0;
        cfd::DpsKnownArgs a{sample, g_direct, g_unet, scale, x_out, t, n_per_sample, n_per_sample * B,
                            seed, offset / 4, vec};
        cfd::KnownArgs kn{known, mask, known_bstride, mask_bstride, table, noise2, counter2};
        const int64_t groups = cfd::ceil_div(a.total, 4);
        hipLaunchKernelGGL(cfd::dps_update_known_kernel, dim3((unsigned)cfd::ceil_div(groups, 256)), dim3(256), 0,
                           (hipStream_t)stream, a, kn);
        cfd::check_launch("dps_update_known_kernel");
    });
}

// ---------------------------------------------------------------------------
// Adam / AdamW (torch.optim.Adam / AdamW, fp32, amsgrad off; weight_decay > 0 is
// AdamW's decoupled decay, param *= 1 - lr wd, first): the optimisers of the CNF
// training loop (N/scripts/train.py:385-416) and of the diffusion TrainLoop (AdamW,
// U/src/train_util.py:78-80).  The reference steps them on its GPU, where torch's
// default is the multi-tensor (foreach) path of torch/optim/adam.py; per element,
// in that path's operation order and with the fused multiply-adds its device
// kernels execute (pinned bit for bit against torch.optim.AdamW on the MI355X by
// tests/test_gpu_optim.py; the probe is tools/dev/optim_probe.py):
//   exp_avg.lerp_(grad, 1 - beta1)          w < 0.5: fma(w, g - m, m)
//                                           else:    fma(-(g - m), 1 - w, g)
//   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//                                           fma(1 - beta2, g * g, v * beta2)
//   denom = exp_avg_sq.sqrt() / sqrt(1 - beta2^step) + eps   (IEEE sqrt, division)
//   param.addcdiv_(exp_avg, denom, value=-lr / (1 - beta1^step))
//                                           fma(-step_size, m / denom, p)
// The step-dependent scalars are formed in double on the host as torch does.
// torch's CPU kernels differ in two places (addcmul as fma(value * g, g, v),
// addcdiv as p + (value * m) / denom, and a vectorised sqrt that is not always
// correctly rounded): within an ulp of this on the same inputs.
// ---------------------------------------------------------------------------
namespace cfd {
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, int64_t n, float w1, float beta2, float w2, float bc2s, float eps,
                            float neg_step, float decay) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float pi = p[i];
    if (decay != 1.0f) pi = pi * decay;   // AdamW: param.mul_(1 - lr * weight_decay) first
    const float gi = g[i];
    float mi = m[i];
    mi = w1 < 0.5f ? __builtin_fmaf(w1, gi - mi, mi) : __builtin_fmaf(-(gi - mi), 1.0f - w1, gi);
    const float vi = __builtin_fmaf(w2, gi * gi, v[i] * beta2);
    const float denom = sqrtf(vi) / bc2s + eps;
    p[i] = __builtin_fmaf(neg_step, mi / denom, pi);
    m[i] = mi;
    v[i] = vi;
}
}  // namespace cfd

extern "C" int cfd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                             double beta1, double beta2, double eps, double weight_decay, int64_t step, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(param && grad && exp_avg && exp_avg_sq && n >= 0 && step >= 1, CFD_EARG, "bad argument");
        CFD_REQUIRE(lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0 && weight_decay >= 0,
                    CFD_EARG, "Adam hyper-parameters out of range");
        if (n == 0) return;
        const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
        const double step_size = lr / bc1, bc2s = std::sqrt(bc2);
        hipLaunchKernelGGL(cfd::adam_kernel, dim3((unsigned)cfd::ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                           param, grad, exp_avg, exp_avg_sq, n, (float)(1.0 - beta1), (float)beta2,
                           (float)(1.0 - beta2), (float)bc2s, (float)eps, (float)(-step_size),
                           (float)(1.0 - lr * weight_decay));
        cfd::check_launch("adam_kernel");
    });
}
