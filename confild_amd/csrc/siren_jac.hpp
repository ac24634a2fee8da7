// Shared pieces of the SIREN derivative kernels: the fused value-and-Jacobian decodes
// K13 (siren_jac.hip, exact fp32 MFMA chain) and K13s (siren_jac_split.hip, split-f16
// MFMA chain), the Hessian decodes K14 / K14s (siren_hess.hpp) and the Jacobian
// adjoints K15 / K16 (siren_jtape.hpp): device pieces first, then the host side of
// the launches and entry points.  A device stage is here only where every kernel
// that uses it compiles to the instructions it had with the stage written out
// (DESIGN.md "Shared stages of the derivative kernels").
#pragma once
#include <algorithm>

#include "siren.hpp"

namespace cfd {

// What the decodes K13 / K13s / K14 / K14s read and write, grid (point tile, latent
// row).  The kernels' argument layouts are as they were when each was tuned (moving a
// field moves the scalar loads and with them the register allocation), so the
// scalars that follow stay with each struct.
struct SirenDecodeArgs {
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
    float* jac;           // (b, N, c, d); K14 / K14s: or null
};
struct SirenJacArgs : SirenDecodeArgs {
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

// layer 0's pre-activation of one feature: cn . w + F0, w the feature's row of w0
__device__ __forceinline__ float layer0_preact(const float (&cn)[3], const f4& w, int d, float f0) {
    float a = cn[0] * w[0];
#pragma unroll
    for (int k = 1; k < 3; ++k)
        if (k < d) a = fmaf(cn[k], w[k], a);
    return a + f0;
}

// ---- range handling of the split-f16 derivative chains (K13s, K14s) ----
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

// One step of the 2-slot LDS-DMA weight ring on the split-f16 chain: issue block
// J + 1, multiply block J (in slot J & 1) into the accumulator -- Wl xh + Wh xl + Wh xh
// on three 16x16x32 MFMAs per K-chunk of 32 features, a block being NB / 2 chunks of
// (hi, lo) x 512 halves -- then wait for block J + 1 (this wave's pieces); the barrier
// publishes every wave's and retires all reads of the slot before its refill.
// start() is the accumulator's initial value, read after the issue as the kernels
// always did.  Chunk q + 1's A fragments are read under chunk q's MFMAs (the
// scheduling barrier keeps the read there: left alone, the compiler reads each
// fragment right before its use and every MFMA waits for the LDS).  Returns the
// block's accumulator.
template <int NB, int WAVES, class Start>
__device__ __forceinline__ f4 ring_step_split(const float* wimg, float* wbuf, int& J, int nblocks,
                                              const JFrag (&BH)[NB / 2], const JFrag (&BL)[NB / 2], Start&& start,
                                              int wave, int lane) {
    constexpr int NQ = NB / 2;
    constexpr int BLK = NB * 256;
    if (J + 1 < nblocks) siren_issue_block<NB, WAVES>(wimg, J + 1, wbuf + ((J + 1) & 1) * BLK, wave, lane);
    const float* wb = wbuf + (J & 1) * BLK;
    f4 a = start();
    jh8 FH = *(const jh8*)(wb + lane * 4);
    jh8 FL = *(const jh8*)(wb + 256 + lane * 4);
    static_for<NQ>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        jh8 FH1 = FH, FL1 = FL;
        if constexpr (q + 1 < NQ) {
            FH1 = *(const jh8*)(wb + (q + 1) * 512 + lane * 4);
            FL1 = *(const jh8*)(wb + (q + 1) * 512 + 256 + lane * 4);
        }
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(FL, BH[q].h(), a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(FH, BL[q].h(), a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(FH, BH[q].h(), a, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        FH = FH1;
        FL = FL1;
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ++J;
    return a;
}

// ---- host side ----

// f(std::integral_constant<int, NB>) for the widths H = 16 NB of the fp32 chain
template <class F>
void dispatch_nb(int NB, F&& f) {
    switch (NB) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 12: return f(std::integral_constant<int, 12>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 24: return f(std::integral_constant<int, 24>{});
        case 32: return f(std::integral_constant<int, 32>{});
        default: throw Error{CFD_EARG, "hidden_features must be 16*{1,2,3,4,6,8,12,16,24,32}"};
    }
}

// the same for the widths of the split-f16 image; split_refusal has refused the
// others, `unchecked` is the internal error of a caller that did not ask it
template <class F>
void dispatch_nb_split(int NB, const char* unchecked, F&& f) {
    switch (NB) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 12: return f(std::integral_constant<int, 12>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 24: return f(std::integral_constant<int, 24>{});
        default: throw Error{CFD_ESTATE, unchecked};
    }
}

// LDS of a decode: 2 ring slots, the FiLM rows (nh+1, H), w0 as (H, 4)
inline size_t deriv_lds(int NB, int nh) {
    const int H = NB * 16;
    return (size_t)(2 * NB * 256 + (nh + 1) * H + 4 * H) * sizeof(float);
}

// A decode kernel of width H = 16 NB on its grid (tile of `tile` points, latent row),
// the rows in slabs of 65535
template <class Args>
void launch_decode(void (*kernel)(Args), const char* name, Args a, int NB, int tile, int waves, hipStream_t st) {
    const size_t lds = deriv_lds(NB, a.nh);
    CFD_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t tiles = ceil_div(a.N, tile);
    CFD_REQUIRE(tiles <= 0x7fffffff, CFD_EARG, "too many query points for one call");
    for (int64_t b0 = 0; b0 < a.b; b0 += 65535) {
        a.b0 = b0;
        const int nb = (int)std::min<int64_t>(65535, a.b - b0);
        hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, nb), dim3(64 * waves), lds, st, a);
        check_launch(name);
    }
}

// the fields every kernel of the family takes from the handle
template <class Args>
void handle_args(Args& a, const cfd_siren* h) {
    a.w0 = h->w0;
    a.wimg = h->wimg;
    a.wout = h->wout;
    a.bout = h->bout;
    a.d = h->cfg.in_coord_features;
    a.c = h->cfg.out_features;
    a.nh = h->cfg.num_hidden_layers;
    a.w0f = h->cfg.w0;
}

// What the four decode entry points (`fn`) check first; `result` is the output that
// must not be null, `columns` why d is bounded.
inline void decode_check(const char* fn, const char* columns, const cfd_siren* h, const float* coords, int64_t N,
                         const float* latents, int b, const float* xmax, const float* xmin, const float* ymax,
                         const float* ymin, const float* result) {
    CFD_REQUIRE(h && coords && latents && result, CFD_EARG, "null argument");
    CFD_REQUIRE(N >= 1 && b >= 1, CFD_EARG, "empty decode");
    CFD_REQUIRE((xmax == nullptr) == (xmin == nullptr), CFD_EARG, "xmax/xmin must both be set or both NULL");
    CFD_REQUIRE((ymax == nullptr) == (ymin == nullptr), CFD_EARG, "ymax/ymin must both be set or both NULL");
    CFD_REQUIRE(h->cfg.in_coord_features <= 3, CFD_EARG,
                std::string(fn) + ": in_coord_features must be 1..3 (" + columns + ")");
}

// What the split-f16 entry point `fn` ("..._split") refuses, after decode_check
inline void split_refusal(const std::string& fn, const cfd_siren* h) {
    const int nh = h->cfg.num_hidden_layers;
    CFD_REQUIRE(nh >= 1, CFD_EARG,
                fn + ": num_hidden_layers must be >= 1 (no hidden product to run on f16 MFMA; use " +
                    fn.substr(0, fn.size() - 6) + ")");
    CFD_REQUIRE(h->cfg.hidden_features % 32 == 0, CFD_EARG,
                fn + ": hidden_features must be a multiple of 32 (32-feature K-chunks of the f16 MFMA)");
    CFD_REQUIRE(siren_split_supported(h->NB), CFD_EARG,
                fn + ": hidden_features must be 32*{1,2,3,4,6,8,12} (512 has no split-f16 image: its register file "
                     "holds one wave per SIMD)");
    CFD_REQUIRE(deriv_lds(h->NB, nh) <= 160 * 1024, CFD_EARG, fn + ": SIREN too deep for the LDS staging (160 KiB)");
}

// The rest of a decode entry point: the workspace check, the FiLM vectors (b, nh+1, H)
// into the workspace, and the launch arguments (out may be null).
template <class Args>
Args decode_args(const cfd_siren* h, const float* coords, int64_t N, const float* latents, int b, const float* xmax,
                 const float* xmin, const float* ymax, const float* ymin, int64_t y_stride, float* out, float* jac,
                 void* ws, size_t ws_bytes, hipStream_t st) {
    size_t need = 0;
    cfd_siren_workspace_bytes(h, b, &need);
    CFD_REQUIRE(ws && ws_bytes >= need, CFD_EARG, "workspace too small");
    cfd::film_vectors(h, latents, b, (float*)ws, st);
    Args a{};
    handle_args(a, h);
    a.film = (const float*)ws;
    a.coords = coords;
    a.xmax = xmax;
    a.xmin = xmin;
    a.ymax = ymax;
    a.ymin = ymin;
    a.out = out;
    a.jac = jac;
    a.N = N;
    a.ystride = y_stride;
    a.b = b;
    return a;
}

}  // namespace cfd
