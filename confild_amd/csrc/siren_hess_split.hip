// Fused SIREN/FiLM decode with its coordinate Jacobian and Hessian on f16 MFMA with
// fp32-level accuracy (K14s): K14's layer algebra (siren_hess.hip) on K13s's arithmetic
// (siren_jac_split.hip).
//
// Columns as K14: column j16 = RS * point + role, role 0 the value, roles 1..d the
// tangents, then the nsec second-order roles; RS = 4 at d = 1, 8 at d = 2 and for the
// diagonal at d = 3, 16 for the full Hessian at d = 3.  The role count is a launch
// argument, and the ds_bpermute fetches are K14's: the value column's pre-activation,
// A_k, A_l, and the cosine of tangent 0 of the group; each lane runs one reduction and
// one polynomial.  Products as K13s: the image wimg16 (W s_i = Wh + Wl, s_i a power of
// two), the FiLM rows pre-scaled by s_i, Wl xh + Wh xl + Wh xh on three
// v_mfma_f32_16x16x32_f16 per 32 features, accumulator blocks 2q, 2q + 1 being the
// next layer's B fragment q; the hidden weights stream once per tile for all roles
// through a 2-slot LDS-DMA ring, chunk q + 1's A fragments read under chunk q's MFMAs.
//
// Range ("hold and normalise" with frames): every tangent and every
// second-order column carries an integer exponent E, true = carried * 2^E, and is
// brought to [2^12, 2^13) by column_exponent / scale_split8 before its split, as in
// K13s; value columns take exponent 0.  After a hidden layer's MFMAs a second-order
// lane holds H'_kl in frame E_kl and fetches A'_k, A'_l in the frames E_k, E_l of
// their columns (two more crossbar moves per layer for the exponents).  The update
//   w0 cos u * H_kl - (w0^2 sin u * A_k) * A_l
// is formed in the common frame F = max(E_kl, E_k + E_l): the operand of the term whose
// frame is smaller (H_kl, or A_k) is multiplied by 2^(its frame - F) with ldexpf, which
// only ever scales down, so it cannot overflow, and a flush to zero there is below
// 2^-100 of the other term.  The column goes on in frame F, the next normalisation
// adds its e, and the head undoes E with one ldexpf, exactly.  F depends on the point's
// own columns only, so the bits of a (row, point) pair depend on neither b, N, the
// point's index nor its neighbours; scaling coordinate k by a power of two moves the
// exponents by integers and no carried bit.  The op sequence is the same in every
// instantiation: the diagonal form is the full form's diagonal to the bit.
#include "siren_hess.hpp"

namespace cfd {

template <int NB, int RS, int WAVES>
__global__ __launch_bounds__(64 * WAVES, WAVES == 8 ? 2 : 1) void siren_hess_split(SirenHessSplitArgs p) {
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
    const int role = j16 & (RS - 1);
    const int d = p.d;
    const HessRole R = hess_role(lane, role, d, p.nsec);
    const bool value = R.value, tangent = R.tangent, second = R.second;
    const int ck = R.ck, cl = R.cl;
    const int64_t b = p.b0 + blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * TILE + wave * PPW + j16 / RS;
    const int64_t nc = n < p.N ? n : p.N - 1;
    const int nh = p.nh;
    const float w0f = p.w0f;
    const float w0sq = w0f * w0f;
    CFD_DASSERT(d >= 1 && d <= 3 && 1 + d + p.nsec <= RS && p.c >= 1 && p.c <= 4 && b < p.b && nc >= 0 && nh >= 1);
    CFD_DASSERT(ck <= cl && cl < d && R.src_v >= 0 && R.src_k >= 0 && R.src_k < 256 && R.src_l >= 0 &&
                R.src_l < 256 && R.src_c >= 0 && R.src_c < 256);

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
    siren_issue_block<NB, WAVES>(p.wimg, 0, wbuf, wave, lane);

    f4 acc[NB];           // a layer's fp32 outputs, held until its column maxima are known
    JFrag BH[NQ], BL[NQ]; // the layer's B operands (hi, lo)
    int E = 0;            // the column's frame: true = 2^E * (what the chain carries)
    // acc (fp32 X / T / S of a whole layer) -> BH, BL at the column's own power-of-two scale
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

    // ---- layer 0 (d -> H, fp32 VALU), K14's expressions ----
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
            acc[q][r] = value ? sc : tangent ? sc * (tsc * wk) : second ? sv : 0.0f;
        }
    });

    // ---- hidden layers: one split-f16 MFMA chain carries every role ----
    const int nblocks = nh * NB;
    int J = 0;
    // block 0 landed (this wave's pieces) and is published by every wave
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int layer = 1; layer <= nh; ++layer) {
        normalise_split();
        // frames of this layer's accumulators: a second-order lane takes E_k, E_l of its
        // group's tangent columns and moves to F = max(E_kl, E_k + E_l); dh, dt <= 0 are
        // what its H_kl and its A_k are scaled down by.  Every other lane keeps its frame.
        const int Ek = __builtin_amdgcn_ds_bpermute(R.src_k, E);
        const int El = __builtin_amdgcn_ds_bpermute(R.src_l, E);
        const int F = second ? max(E, Ek + El) : E;
        const float ws = p.wscale[layer - 1];
        const float m = w0f / ws;                                 // power-of-two scale: exact
        const int ie = 1 - __builtin_amdgcn_frexp_expf(ws);       // 2^ie = 1 / s_i
        const int dh = ie + (E - F), dt = second ? ie + (Ek + El - F) : ie;
        E = F;
        static_for<NB>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            acc[j] = ring_step_split<NB, WAVES>(p.wimg, wbuf, J, nblocks, BH, BL, [&] {
                f4 a = *(const f4*)(film + layer * H + 16 * j + 4 * g);
                if (!value) a = f4{0.f, 0.f, 0.f, 0.f};
                return a;
            }, wave, lane);
        });
        // acc = s_i (F_i + W_i X) in value lanes, s_i W_i T_k 2^-E_k in tangent lanes,
        // s_i W_i S_kl 2^-E_kl in second-order lanes
        static_for<NB>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float av = acc[q][r];
                const float x = m * lane_value(R.src_v, av);
                const float ak = ldexpf(lane_value(R.src_k, av), dt);
                const float al = ldexpf(lane_value(R.src_l, av), ie);
                const float sc = sincos_role(x, !tangent);
                const float cu = lane_value(R.src_c, sc);
                const float sv = second_order(w0f, w0sq, sc, cu, ldexpf(av, dh), ak, al);
                acc[q][r] = value ? sc : tangent ? (m * sc) * av : second ? sv : 0.0f;
            }
        });
    }

    // ---- last layer (H -> c) per column; the column's frame undone exactly ----
    float o[4];
    hess_head<NB>(p, acc, g, value, o);
#pragma unroll
    for (int oc = 0; oc < 4; ++oc)
        if (!value) o[oc] = ldexpf(o[oc], E);
    hess_store(p, R, o, n, b, g);
}

}  // namespace cfd

namespace {

template <int RS>
void launch_hess_split(int nb, const cfd::SirenHessSplitArgs& a, hipStream_t st) {
    cfd::dispatch_nb_split(nb, "internal: split Hessian width not checked", [&](auto nbc) {
        // K13s's workgroup: 8 waves (2 per SIMD, 256 registers each) share one weight stream
        constexpr int NB = decltype(nbc)::value, WAVES = 8;
        cfd::launch_decode(cfd::siren_hess_split<NB, RS, WAVES>, "siren_hess_split", a, NB, (16 / RS) * WAVES, WAVES,
                           st);
    });
}

}  // namespace

extern "C" int cfd_siren_forward_hessian_split(cfd_siren* h, const float* coords, int64_t N, const float* latents,
                                               int b, const float* xmax, const float* xmin, const float* ymax,
                                               const float* ymin, int64_t y_stride, float* out, float* jac,
                                               float* hess, int diag_only, void* ws, size_t ws_bytes, void* stream) {
    return cfd::guard([&] {
        const char* fn = "cfd_siren_forward_hessian_split";
        cfd::decode_check(fn, "the value, tangent and second-order chains of a point share 16 MFMA columns", h, coords,
                          N, latents, b, xmax, xmin, ymax, ymin, hess);
        cfd::split_refusal(fn, h);
        auto st = (hipStream_t)stream;
        auto a = cfd::decode_args<cfd::SirenHessSplitArgs>(h, coords, N, latents, b, xmax, xmin, ymax, ymin, y_stride,
                                                           out, jac, ws, ws_bytes, st);
        a.wimg = h->wimg16;
        a.wscale = h->wscale;
        a.hess = hess;
        a.diag = diag_only != 0;
        // not selected by cfd_siren_set_compute: always the split-f16 chain.  d <= 2 runs
        // the full form for both outputs; d = 3 has a diagonal form of 8 columns per point
        const int d = a.d;
        const bool full = d < 3 || !a.diag;
        a.nsec = full ? d * (d + 1) / 2 : d;
        if (d == 1)
            launch_hess_split<4>(h->NB, a, st);
        else if (d == 2 || !full)
            launch_hess_split<8>(h->NB, a, st);
        else
            launch_hess_split<16>(h->NB, a, st);
    });
}
