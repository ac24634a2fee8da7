// K1p: the pointwise (1x1, stride 1) split-f16 forward convolutions -- qkv,
// proj_out and skip_connection -- as a plain GEMM over channels-last rows
// (gfx950).
//
// Same operands and numerics as conv_gemm_kernel<..., MODE=2> (K1s,
// unet_kernels.hip): activations split x = xh + xl (f16 RNE) as they are staged,
// weights pre-split (s w) = wh + wl, each product as wl.xh + wh.xl + wh.xh on
// v_mfma_f32_16x16x32_f16 with fp32 accumulation, K tiles in ascending order --
// fp32-level error against fp64.
//
// What a 1x1 does not need is gone: row m of A is pixel m (no pixel table, no
// division, no (tap, channel) position), a 32-channel K tile comes wholly from
// src1 or from src2 (C1 % 32 == 0), and every operand load is a bounds-checked
// buffer load whose offset is one multiply-add.  K is short (128-1024), so the
// tiles are small enough that the chip is filled without split-K (no partial
// slab, no reduction launch, and a qkv always packs K / V in its epilogue) and
// PF K tiles per thread are in flight through a register ring, not one per
// barrier.  Never split over K: an output's order of summation is the K tile
// order, whatever the batch or the plan.
#include <algorithm>

#include "unet_kernels.hpp"

namespace cfd {

// the K1s LDS layout of a 32-deep f16 row (unet_kernels.hip, lds_swz_bf):
// conflict-free ds_read_b128 fragment reads and ds_write_b64 staging
__device__ __forceinline__ int pswz(int row, int chunk) { return row * 64 + ((chunk + 2 * ((row >> 2) & 1)) & 3) * 16; }

// hi = f16(x) (RNE, packed convert), lo = f16(x - hi) by v_fma_mix, 4 values
__device__ __forceinline__ void split4_mix_p(const f4& x, uint2& hi, uint2& lo) {
    typedef _Float16 h2_ __attribute__((ext_vector_type(2)));
    typedef float f2_ __attribute__((ext_vector_type(2)));
    hi.x = __builtin_bit_cast(unsigned, __builtin_convertvector((f2_){x[0], x[1]}, h2_));
    hi.y = __builtin_bit_cast(unsigned, __builtin_convertvector((f2_){x[2], x[3]}, h2_));
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=&v"(lo.x) : "v"(x[0]), "v"(hi.x));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo.x) : "v"(x[1]), "v"(hi.x));
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=&v"(lo.y) : "v"(x[2]), "v"(hi.y));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo.y) : "v"(x[3]), "v"(hi.y));
}

// Workgroup tile BM x BN x 32, NW waves as (NW / 2) x 2, each wave
// (BM / (NW / 2)) x (BN / 2) of 16x16 accumulator tiles.  One LDS stage holds
// the A hi, A lo, B hi, B lo planes of a K tile; two stages.
template <int BM, int BN, int NW, int PF>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void conv_p_kernel(ConvArgs a) {
    constexpr int NT = 64 * NW;
    constexpr int WM = BM / (NW / 2), WN = BN / 2;
    constexpr int TM = WM / 16, TN = WN / 16;
    constexpr int RPP = NT / 8;                    // staged rows per pass (8 threads per 32-deep row)
    constexpr int AIT = BM / RPP, BIT = BN / RPP;
    static_assert(TM >= 1 && TN >= 1 && AIT >= 1 && BIT >= 1 && BM % RPP == 0 && BN % RPP == 0, "tile");
    constexpr int APL = BM * 64, BPL = BN * 64;    // bytes of one f16 plane of a stage
    constexpr int STAGE = 2 * APL + 2 * BPL;
    // the epilogue reuses both stages as the BM x BN fp32 tile
    static_assert(BM * BN * 4 <= 2 * STAGE && BM % 32 == 0 && BM * BN / 4 % NT == 0, "epilogue tile");
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    CFD_STAMP(a.stamps, 3, a.seq, 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx, by, bz;
    xcd_tile(a.xcd, bx, by, bz);
    const int m0 = bx * BM, n0 = by * BN;
    const int kq = tid & 7, rsub = tid >> 3;

    // bounds-checked operands: a row past M (or a weight row past Cout) gets an
    // offset beyond the descriptor's range and reads zero
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.src1, 0, a.M * a.C1 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.src2 ? a.src2 : a.src1), 0, a.src2 ? a.M * a.C2 * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rwh = __builtin_amdgcn_make_buffer_rsrc((void*)a.wbf, 0, a.Cout * a.K * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rwl = __builtin_amdgcn_make_buffer_rsrc((void*)a.wlo, 0, a.Cout * a.K * 2, 0x00020000);
    unsigned a_off1[AIT], a_off2[AIT], b_off[BIT];
#pragma unroll
    for (int it = 0; it < AIT; ++it) {
        const int m = m0 + rsub + it * RPP;
        a_off1[it] = m < a.M ? (unsigned)(m * a.C1 + 4 * kq) * 4u : 0x80000000u;
        a_off2[it] = m < a.M ? (unsigned)(m * a.C2 + 4 * kq) * 4u : 0x80000000u;
    }
#pragma unroll
    for (int it = 0; it < BIT; ++it) {
        const int n = n0 + rsub + it * RPP;
        b_off[it] = n < a.Cout ? (unsigned)(n * a.K + 4 * kq) * 2u : 0x80000000u;
    }
    const int nkt = a.K / 32;

    f4 ra[PF][AIT];
    uint2 rbh[PF][BIT], rbl[PF][BIT];
    auto load_tile = [&](int kt, int sl) {
        const int cb = __builtin_amdgcn_readfirstlane(kt * 32);
        const bool second = cb >= a.C1;
        const __amdgpu_buffer_rsrc_t rsa = second ? rs2 : rs1;
        const int sa = (second ? cb - a.C1 : cb) * 4;
        CFD_DASSERT(cb + 32 <= a.K && (second ? cb - a.C1 + 32 <= a.C2 : cb + 32 <= a.C1));
#pragma unroll
        for (int it = 0; it < AIT; ++it) {
            CFD_DASSERT(m0 + rsub + it * RPP >= a.M || (second ? a_off2[it] : a_off1[it]) + sa + 16 <=
                                                           (unsigned)a.M * (second ? a.C2 : a.C1) * 4u);
            ra[sl][it] = __builtin_bit_cast(
                f4, __builtin_amdgcn_raw_buffer_load_b128(rsa, second ? a_off2[it] : a_off1[it], sa, 0));
        }
#pragma unroll
        for (int it = 0; it < BIT; ++it) {
            rbh[sl][it] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rwh, b_off[it], cb * 2, 0));
            rbl[sl][it] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rwl, b_off[it], cb * 2, 0));
        }
    };
    auto store_tile = [&](int buf, int sl) {
        char* st = lds + buf * STAGE;
#pragma unroll
        for (int it = 0; it < AIT; ++it) {
            uint2 hv, lv;
            split4_mix_p(ra[sl][it], hv, lv);
            const int off = pswz(rsub + it * RPP, kq >> 1) + (kq & 1) * 8;
            CFD_DASSERT(off >= 0 && off + 8 <= APL);
            *(uint2*)(st + off) = hv;
            *(uint2*)(st + APL + off) = lv;
        }
#pragma unroll
        for (int it = 0; it < BIT; ++it) {
            const int off = pswz(rsub + it * RPP, kq >> 1) + (kq & 1) * 8;
            CFD_DASSERT(off >= 0 && off + 8 <= BPL);
            *(uint2*)(st + 2 * APL + off) = rbh[sl][it];
            *(uint2*)(st + 2 * APL + BPL + off) = rbl[sl][it];
        }
    };

    f4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, li = lane & 15;
    auto compute = [&](int cur) {
        const char* st = lds + cur * STAGE;
        h8v fah[TM], fal[TM], fbh[TN], fbl[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int off = pswz(wm * WM + 16 * i + li, g);
            CFD_DASSERT(off + 16 <= APL);
            fah[i] = *(const h8v*)(st + off);
            fal[i] = *(const h8v*)(st + APL + off);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int off = pswz(wn * WN + 16 * j + li, g);
            CFD_DASSERT(off + 16 <= BPL);
            fbh[j] = *(const h8v*)(st + 2 * APL + off);
            fbl[j] = *(const h8v*)(st + 2 * APL + BPL + off);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fal[i], fbh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fah[i], fbl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fah[i], fbh[j], acc[i][j], 0, 0, 0);
            }
    };

    // the first PF tiles in flight at once (clamped: a repeated last tile keeps
    // every load unconditional, so the wait before a store is a counted vmcnt);
    // step k refills the register slot tile k left, runs the MFMAs of LDS stage
    // k & 1 and parks tile k + 1 in the other stage.  The last step parks its
    // repeated last tile too, which nobody reads: a store skipped on a branch left
    // that slot's loads pending on one path into the loop head, and the compiler
    // then drained every load (vmcnt 0) at the top of each round of PF steps.
#pragma unroll
    for (int p = 0; p < PF; ++p) load_tile(min(p, nkt - 1), p);
    store_tile(0, 0);
    __syncthreads();
    CFD_STAMP(a.stamps, 3, a.seq, 2);
    // (whole rounds of PF steps in the loop, the remaining steps after it: a round
    // whose later steps are skipped on a condition reaches the loop head again in
    // the compiler's view, with the skipped steps' loads pending)
    auto step = [&](int k, int j) {
        load_tile(min(k + PF, nkt - 1), j);
        compute(k & 1);
        store_tile((k & 1) ^ 1, (j + 1) % PF);
        __syncthreads();
        // keep a later step's conversions (register-only work the scheduler is free
        // to hoist) behind this barrier: hoisted, they wait for that step's loads here
        __builtin_amdgcn_sched_barrier(0);
    };
    int k = 0;
    for (; k + PF <= nkt; k += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) step(k + j, j);
    }
#pragma unroll
    for (int j = 0; j < PF - 1; ++j)
        if (k + j < nkt) step(k + j, j);
    CFD_STAMP(a.stamps, 3, a.seq, 3);

    // epilogue through LDS (every wave is past its last fragment read: the K loop
    // ends on a barrier): undo the power-of-two weight scale (exact), then float4
    // rows of BN channels -- bias, optional residual row, store.  Columns
    // XOR-swizzled by 16 ((row >> 2) & 3), as the K1s epilogue.
    float* tile = (float*)lds;
    auto sw = [](int row, int col) { return row * BN + (col ^ (((row >> 2) & 3) << 4)); };
    const int g4 = 4 * g;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            acc[i][j] *= a.acc_scale;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = sw(wm * WM + 16 * i + g4 + r, wn * WN + 16 * j + li);
                CFD_DASSERT(o >= 0 && o < BM * BN);
                tile[o] = acc[i][j][r];
            }
        }
    __syncthreads();
    constexpr int NV = BM * BN / 4 / NT;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int idx = tid + v * NT;
        const int row = idx / (BN / 4), c4 = (idx - row * (BN / 4)) * 4;
        const int m = m0 + row, n = n0 + c4;
        if (m >= a.M || n >= a.Cout) continue;
        f4 val = *(const f4*)&tile[sw(row, c4)];
        const int64_t o = (int64_t)m * a.Cout + n;
        if (a.bias) val = val + *(const f4*)(a.bias + n);
        if (a.res) val = *(const f4*)(a.res + o) + val;
        *(f4*)(a.out + o) = val;
    }
    // qkv convolution: the split attention's K / V fragments from the staged tile,
    // attn_kv_split_kernel's layout and arithmetic -- K = (acc + bias) * scale
    // log2 e, V = acc + bias, each split into f16 hi / lo -- the bits the K1s
    // epilogue writes.  T % 32 == 0 and m0 % 32 == 0 (conv_kv_pack_ok): a 32-key
    // block never straddles two samples or tiles.
    if (a.kvf) {
        const int CH = a.kv_ch, C3 = 3 * CH, T = a.kv_T, nj = CH >> 5, nd = CH >> 4;
        const float ks = kln2(a.kv_scale);
        const float rc3 = 1.0f / (float)C3, rT = 1.0f / (float)T;   // fdiv24: M < 2^24 (launch_conv)
        h8v* kf = (h8v*)a.kvf;
        h8v* vf = kf + a.kv_voff;
        // K: (key row, 8 channels) -> one lane of fragment (key / 16, j)
        for (int it = tid; it < BM * (BN / 8); it += NT) {
            const int row = it / (BN / 8), c8 = (it - row * (BN / 8)) * 8;
            const int m = m0 + row, n = n0 + c8;
            if (m >= a.M || n >= a.Cout) continue;
            const int hh = fdiv24(n, C3, rc3), o = n - hh * C3;
            if (o < CH || o >= 2 * CH) continue;
            const int b = fdiv24(m, T, rT);
            const int kc = o - CH, key = m - b * T;
            f4 v0 = *(const f4*)&tile[sw(row, c8)], v1 = *(const f4*)&tile[sw(row, c8 + 4)];
            v0 = v0 + *(const f4*)(a.bias + n);
            v1 = v1 + *(const f4*)(a.bias + n + 4);
            float v[8];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                v[t] = v0[t] * ks;
                v[t + 4] = v1[t] * ks;
            }
            h8v hi, lo;
            split8_f16(v, hi, lo);
            const int64_t bh = (int64_t)b * a.kv_heads + hh;
            h8v* dst = kf + ((bh * (T >> 4) + (key >> 4)) * nj + (kc >> 5)) * 128 + ((kc & 31) >> 3) * 16 + (key & 15);
            CFD_DASSERT(b * T + key < a.M && hh < a.kv_heads && kc < CH);
            dst[0] = hi;
            dst[64] = lo;
        }
        // V: (32-key block, lane group g, channel) -> one lane of fragment (block, channel / 16)
        for (int it = tid; it < (BM / 32) * 4 * BN; it += NT) {
            const int col = it % BN, r2 = it / BN, gg = r2 & 3, blk = r2 >> 2;
            const int n = n0 + col, mb = m0 + 32 * blk;
            if (n >= a.Cout || mb >= a.M) continue;
            const int hh = fdiv24(n, C3, rc3), o = n - hh * C3;
            if (o < 2 * CH) continue;
            const int b = fdiv24(mb, T, rT);
            const int vc = o - 2 * CH, kb = (mb - b * T) >> 5;
            const float bn = a.bias[n];
            float v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = tile[sw(32 * blk + (t < 4 ? 4 * gg + t : 12 + 4 * gg + t), col)] + bn;
            h8v hi, lo;
            split8_f16(v, hi, lo);
            const int64_t bh = (int64_t)b * a.kv_heads + hh;
            h8v* dst = vf + ((bh * (T >> 5) + kb) * nd + (vc >> 4)) * 128 + gg * 16 + (vc & 15);
            CFD_DASSERT(mb + 32 <= a.M && hh < a.kv_heads && vc < CH);
            dst[0] = hi;
            dst[64] = lo;
        }
    }
#ifdef CFD_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
#endif
    CFD_STAMP(a.stamps, 3, a.seq, 4);
}

// whether K1p takes this convolution: pointwise, split compute, forward, fp32
// sources whose 32-channel K tiles do not straddle the two sources, float4 output
// rows, and (at the real batch) 32-bit operand offsets
bool conv_p_applies(const ConvArgs& a) {
#ifdef CFD_NO_K1P
    return false;
#else
    return a.wbf && a.wlo && !a.tmode && a.ks == 1 && a.stride == 1 && !a.up && !a.src_bf16 && !a.emb &&
           a.C1 % 32 == 0 && a.C2 % 32 == 0 && a.Ctot >= 32 && (a.C2 == 0 || a.src2) && a.Cout % 4 == 0 &&
           a.Hin == a.Hout && a.Win == a.Wout;
#endif
}

void conv_p_tile(int variant, int& bm, int& bn, int& nw) {
    bm = variant == 40 ? 128 : variant == 41 ? 64 : 32;
    bn = variant == 40 ? 128 : 64;
    nw = variant == 40 ? 8 : 4;
}

void launch_conv_p(const ConvArgs& a, int variant, hipStream_t st) {
    CFD_REQUIRE(conv_p_applies(a) && a.K == a.Ctot, CFD_ESTATE, "internal: K1p takes pointwise split-f16 forward convolutions");
    CFD_REQUIRE((int64_t)a.M * std::max(a.C1, a.C2) * 4 < (1ll << 31) && (int64_t)a.Cout * a.K * 2 < (1ll << 31) &&
                    a.M < (1 << 24),
                CFD_ESTATE, "internal: K1p needs 32-bit operand offsets");
    int bm, bn, nw;
    conv_p_tile(variant, bm, bn, nw);
    const dim3 grid((unsigned)ceil_div(a.M, bm), (unsigned)ceil_div(a.Cout, bn), 1);
    switch (variant) {
        // ring depths from tools/convbench: deeper rings were no faster (32x64: 6 as 4;
        // 128x128: 3 and 4 slower than 2, which keeps two workgroups per CU)
        case 40: hipLaunchKernelGGL((conv_p_kernel<128, 128, 8, 2>), grid, dim3(512), 0, st, a); break;
        case 41: hipLaunchKernelGGL((conv_p_kernel<64, 64, 4, 3>), grid, dim3(256), 0, st, a); break;
        case 42: hipLaunchKernelGGL((conv_p_kernel<32, 64, 4, 4>), grid, dim3(256), 0, st, a); break;
        default: throw Error{CFD_ESTATE, "internal: unknown K1p variant"};
    }
    check_launch("conv_p_kernel");
}

}  // namespace cfd
