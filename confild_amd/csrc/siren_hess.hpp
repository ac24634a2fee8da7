// Shared pieces of the fused value-Jacobian-Hessian decodes: K14 (siren_hess.hip,
// exact fp32 MFMA chain) and K14s (siren_hess_split.hip, split-f16 MFMA chain).
#pragma once
#include "siren_jac.hpp"

namespace cfd {

struct SirenHessArgs : SirenDecodeArgs {
    float* hess;          // (b, N, c, d, d), or (b, N, c, d) with diag
    int64_t N;
    int64_t ystride;
    int64_t b0;
    int b;                // latent rows of the call (index assertions)
    int d, c, nh;
    int nsec;             // second-order roles: d (diagonal only) or d (d + 1) / 2
    int diag;             // hess holds the diagonal only
    float w0f;
};
// K14s: wimg is the split-f16 image (pack_split_f16), wscale its (nh) power-of-two scales
struct SirenHessSplitArgs : SirenHessArgs {
    const float* wscale;
};

// v of the lane whose byte address (4 * lane) is addr: ds_bpermute_b32, no LDS memory
__device__ __forceinline__ float lane_value(int addr, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
}

// the second-order update of one element, one fixed order for every form:
// w0 cos u * h - ((w0^2 sin u) * ak) * al
__device__ __forceinline__ float second_order(float w0f, float w0sq, float su, float cu, float h, float ak,
                                              float al) {
    const float t = ((w0sq * su) * ak) * al;
    return fmaf(w0f * cu, h, -t);
}

// The role of a lane's MFMA column (column j16 = RS * point + role): role 0 the value,
// roles 1..d the tangents, then the nsec second-order roles (xx, yy, zz first, then
// xy, xz, yz); the rest of a group carries zeros.
struct HessRole {
    bool value, tangent, second;
    int ck, cl;                       // the coordinates (k, l), k <= l, of this column
    // byte addresses (ds_bpermute) of the group's value column, of tangents k and l and
    // of the column whose cosine this one reads
    int src_v, src_k, src_l, src_c;
};

__device__ __forceinline__ HessRole hess_role(int lane, int role, int d, int nsec) {
    HessRole R;
    const int sidx = role - 1 - d;     // index among the second-order roles
    R.value = role == 0;
    R.tangent = role >= 1 && role <= d;
    R.second = sidx >= 0 && sidx < nsec;
    // tangent k = l = role - 1; second order xx, yy, zz, then xy, xz, yz
    int ck = 0, cl = 0;
    if (R.tangent) ck = cl = role - 1;
    if (R.second) {
        const int pr = sidx - d;
        ck = pr < 0 ? sidx : pr == 2 ? 1 : 0;
        cl = pr < 0 ? sidx : pr == 0 ? 1 : 2;
    }
    R.ck = ck;
    R.cl = cl;
    const int base = lane - role;
    R.src_v = 4 * base;
    R.src_k = R.second ? 4 * (base + 1 + ck) : 4 * lane;
    R.src_l = R.second ? 4 * (base + 1 + cl) : 4 * lane;
    R.src_c = 4 * (base + 1);  // the first tangent column: cos u
    return R;
}

// The stores of lane group g (output channel g) of point n, row b: o holds the head's
// sums of this column for the c channels (the value with its bias).  Value:
// de-normalisation; the others: their slope.
__device__ __forceinline__ void hess_store(const SirenHessArgs& p, const HessRole& R, const float (&o)[4], int64_t n,
                                           int64_t b, int g) {
    const int d = p.d;
    if (n < p.N && g < p.c && (R.value || R.tangent || R.second)) {
        float v = g == 0 ? o[0] : g == 1 ? o[1] : g == 2 ? o[2] : o[3];
        float hi = 1.0f, lo = -1.0f;
        if (p.ymax) {
            const int64_t yi = n * p.ystride + g;
            hi = p.ymax[yi];
            lo = p.ymin[yi];
        }
        const int64_t oi = (b * p.N + n) * p.c + g;
        [[maybe_unused]] const int64_t no = (int64_t)p.b * p.N * p.c;
        CFD_DASSERT(oi >= 0 && oi < no);
        if (R.value) {
            if (p.ymax) v = (v + 1.0f) / 2.0f * (hi - lo) + lo;
            if (p.out) p.out[oi] = v;
        } else {
            if (p.ymax) v = v * ((hi - lo) / 2.0f);
            if (R.tangent) {
                const int64_t ji = oi * d + R.ck;
                CFD_DASSERT(ji >= 0 && ji < no * d);
                if (p.jac) p.jac[ji] = v;
            } else if (p.diag) {
                const int64_t di = oi * d + R.ck;
                CFD_DASSERT(di >= 0 && di < no * d);
                if (R.ck == R.cl) p.hess[di] = v;
            } else {
                // both halves from the same lane: symmetric to the bit
                const int64_t h0 = (oi * d + R.ck) * d + R.cl, h1 = (oi * d + R.cl) * d + R.ck;
                CFD_DASSERT(h0 >= 0 && h0 < no * d * d && h1 >= 0 && h1 < no * d * d);
                p.hess[h0] = v;
                if (R.ck != R.cl) p.hess[h1] = v;
            }
        }
    }
}

// The last layer (H -> c) of one column: the sums over the H features, X[q][r] the
// column's element 16 q + 4 g + r (the lane's share, then the four lane groups); a
// value column adds the bias.
template <int NB, class XT>
__device__ __forceinline__ void hess_head(const SirenHessArgs& p, const XT& X, int g, bool value, float (&o)[4]) {
    constexpr int H = NB * 16;
#pragma unroll
    for (int oc = 0; oc < 4; ++oc) {
        o[oc] = 0.f;
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
}

}  // namespace cfd
