// Shared pieces of the fused value-and-Jacobian decodes: K13 (siren_jac.hip, exact
// fp32 MFMA chain) and K13s (siren_jac_split.hip, split-f16 MFMA chain).
#pragma once
#include "siren.hpp"

namespace cfd {

struct SirenJacArgs {
    const float* w0;      // (H, d)
    const float* wimg;    // hidden weight image (as SirenArgs)
    const float* wout;    // (c, H)
    const float* bout;    // (c)
    const float* film;    // (b, nh+1, H)
    const float* coords;  // (N, d)
    const float* xmax;
    const float* xmin;
    const float* ymax;
    const float* ymin;
    float* out;           // (b, N, c) or null
    float* jac;           // (b, N, c, d)
    int64_t N;
    int64_t ystride;
    int64_t b0;
    int b;                // latent rows of the call (index assertions)
    int d, c, nh;
    float w0f;
};
// K13s: wimg is the split-f16 image (pack_split_f16), wscale its (nh) power-of-two scales
struct SirenJacSplitArgs : SirenJacArgs {
    const float* wscale;
};

// sin(x) where value is set, cos(x) elsewhere, from one reduction: sin_cw reduces by
// q pi and cos_cw by an odd q' pi/2 with a split of pi/2 whose every term is exactly
// half of sin_cw's, so fmaf(2q, c/2, x) == fmaf(q, c, x) bit for bit and both are
// "x - qq * (pi/2 split)" with qq = 2q (sine) or q' (cosine); the polynomial is
// shared.  sin: negate for odd q (qq & 2); cos: negate unless qq & 2.
__device__ __forceinline__ float sincos_role(float x, bool value) {
    const float t = fmaf(x, 0.318309886183790671538f, value ? 0.0f : -0.5f);
    const float qq = fmaf(2.0f, rintf(t), value ? 0.0f : 1.0f);
    float r = fmaf(qq, -1.5703125f, x);
    r = fmaf(qq, -0.00048351287841796875f, r);
    r = fmaf(qq, -3.13855707645416259765625e-07f, r);
    r = fmaf(qq, -6.077100628276710381e-11f, r);
    const float s = r * r;
    float u = 2.6083159809786593541503e-06f;
    u = fmaf(u, s, -0.0001981069071916863322258f);
    u = fmaf(u, s, 0.00833307858556509017944336f);
    u = fmaf(u, s, -0.166666597127914428710938f);
    const float y = fmaf(s, u * r, r);
    const bool neg = (((unsigned)(int)qq & 2u) != 0u) == value;
    const float v = __uint_as_float(__float_as_uint(y) ^ (neg ? (1u << 31) : 0u));
    const float xr = x * 0.159154943091895335768f;
    const float hw = value ? __builtin_amdgcn_sinf(xr) : __builtin_amdgcn_cosf(xr);
    return fabsf(x) < 39000.0f ? v : hw;
}

// the value column's copy of v within each group of RS columns (lanes of a group
// are adjacent and groups never straddle a quad): DPP quad_perm, no LDS
template <int RS>
__device__ __forceinline__ float group_value(float v) {
    constexpr int ctrl = RS == 4 ? 0x00 /* quad_perm [0,0,0,0] */ : 0xA0 /* quad_perm [0,0,2,2] */;
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false));
}

// ---- range handling of the split-f16 derivative chains (K13s) ----
// An MFMA column of tangents has no bound, so before its f16 split it is brought to
// a power-of-two scale of its own.  column_exponent: from the largest magnitude m of
// one column (the same in every lane that holds a part of it), the e with
// m 2^-e in [2^12, 2^13) -- the hi half stays below 2^13 (no overflow for any finite
// m) and the lo half keeps 11 bits of everything down to 2^-13 of the largest
// element (the split's absolute floor is 2^-25).  An all-zero column takes e = 0.
// The scale depends on the column's own values only, so a column's bits do not
// depend on its neighbours.  The chain is linear in the tangents: the caller sums
// the exponents and undoes them once at the head with ldexpf, exactly.
__device__ __forceinline__ int column_exponent(float m) {
    return m > 0.0f ? __builtin_amdgcn_frexp_expf(m) - 13 : 0;
}

typedef _Float16 jh8 __attribute__((ext_vector_type(8)));
typedef _Float16 jh2 __attribute__((ext_vector_type(2)));
typedef float jf2 __attribute__((ext_vector_type(2)));
typedef unsigned ju4 __attribute__((ext_vector_type(4)));

// One B operand of v_mfma_f32_16x16x32_f16 (8 x f16) as 4 packed words, written whole
struct JFrag {
    ju4 v;
    __device__ __forceinline__ jh8 h() const { return __builtin_bit_cast(jh8, v); }
};

// scale_split8: the 8 values of K-chunk q (x0: output block 2q, x1: block 2q + 1; the
// accumulator-as-B order of pack_split_f16) times 2^-e (exact), then hi = f16(x),
// lo = f16(x - hi), both RNE (siren_split.hip's split8 on the scaled values).
__device__ __forceinline__ void scale_split8(const f4& x0, const f4& x1, int e, JFrag& hi, JFrag& lo) {
    unsigned hw[4], lw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float a = ldexpf(w < 2 ? x0[2 * w] : x1[2 * w - 4], -e);
        const float b = ldexpf(w < 2 ? x0[2 * w + 1] : x1[2 * w - 3], -e);
        hw[w] = __builtin_bit_cast(unsigned, __builtin_convertvector((jf2){a, b}, jh2));
        const jf2 hf = __builtin_convertvector(__builtin_bit_cast(jh2, hw[w]), jf2);
        lw[w] = __builtin_bit_cast(unsigned, __builtin_convertvector((jf2){a - hf.x, b - hf.y}, jh2));
    }
    hi.v = (ju4){hw[0], hw[1], hw[2], hw[3]};
    lo.v = (ju4){lw[0], lw[1], lw[2], lw[3]};
    asm volatile("" : "+v"(hi.v), "+v"(lo.v));
}

}  // namespace cfd
