// Shared pieces of the fused SIREN decoders (siren.hip: exact fp32 MFMA chain;
// siren_split.hip: fp32-accurate split-f16 MFMA chain).
#pragma once
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.hpp"

namespace cfd {

// Compile-time loop: f(std::integral_constant<int, I>) for I in [0, N).  Keeps
// every register-array index static (a runtime index sends the array to scratch).
template <int N, class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl<N>(f, std::make_integer_sequence<int, N>{});
}

struct SirenArgs {
    const float* w0;      // (H, d)            net1.0.weight
    const float* wimg;    // nh * NB blocks of NB*256 floats (packed hidden weights)
    const float* wout;    // (c, H)            net1.{nh+1}.weight
    const float* bout;    // (c)               net1.{nh+1}.bias
    const float* film;    // (b, nh+1, H)      b_i + V_i z
    const float* coords;  // (N, d)
    const float* xmax;
    const float* xmin;
    const float* ymax;
    const float* ymin;
    float* out;           // (b, N, c)
    const float* wscale;  // (nh) power-of-two weight scale of each hidden layer (split-f16 image only)
    const float* wimg_rev; // siren_split32 image of the hidden weights pre-scaled by (w0 / 2pi) s'_i (HWSIN >= 3)
    const float* wrev;     // (2 nh): FiLM scale (w0 / 2pi) s'_i of each hidden layer, then 1 / s'_i
    const float* wimg_rev16; // the same values as wimg_rev in the 16x16x32 form's order (siren_split32, SHAPE 16)
    int64_t N;
    int64_t ystride;
    int64_t b0;           // first latent of this launch (grid.y chunking)
    int d, c, nh;
    float w0f;
    unsigned long long* stamps;   // development (CFD_STAMPS builds): timestamp buffer, else null
};
// Tape kernels of the DPS adjoint and the CNF training backward (siren.hip):
// pre-activations u and deltas of every layer for P = R x Ns (row, sensor) pairs
struct SirenTapeArgs {
    const float* w0;      // (H, d)
    const float* wimg;    // forward weight image (as SirenArgs)
    const float* wimg_t;  // transposed image, layers nh..1: img[j][q][lane][s] = W_i[16q+4g+s][16j+(lane&15)]
    const float* wout;    // (c, H)
    const float* bout;    // (c)
    const float* film;    // (R, nh+1, H)
    const float* coords;  // (Ns, d)
    const float* xmax;
    const float* xmin;
    const float* ymax;
    const float* ymin;
    float* u;             // (P, nh+1, H) tape
    float* delta;         // (P, nh+1, H)
    float* out;           // (P, c)
    const float* gout;    // (P, c)
    const float* wimg16;  // split-f16 image of the hidden weights (pack_split_f16), null: fp32 tape
    const float* wimg16t; // split-f16 image of their transposes, layers nh..1 (pack_split_f16t)
    const float* wscale;  // (nh) the power-of-two scale of both images
    int64_t P;
    int64_t ystride;
    int Ns, d, c, nh;
    float w0f;
};
// the CFD_STAMPS build's timestamp buffer (unet_kernels.hip; null: off)
unsigned long long* stamps_buf();

// LDS-DMA of one weight block (NB pieces of 1 KiB) into an LDS ring slot: one
// global_load_lds_dwordx4 wave-instruction per piece, pieces spread over the waves.
template <int NB, int WAVES>
__device__ __forceinline__ void siren_issue_block(const float* __restrict__ wimg, int J, float* dst,
                                                  int wave, int lane) {
    constexpr int BLK = NB * 256;
    // J through readfirstlane: keeps the block base a scalar (else the compiler
    // precomputes one 64-bit VGPR address per unrolled block)
    const float* src = wimg + (int64_t)__builtin_amdgcn_readfirstlane(J) * BLK;
    for (int piece = wave; piece < NB; piece += WAVES) {
        __builtin_amdgcn_global_load_lds((const void*)(src + piece * 256 + lane * 4),
                                         (__attribute__((address_space(3))) void*)(dst + piece * 256),
                                         16, 0, 0);
    }
}

// The same with the piece loop unrolled (NB % WAVES == 0: NB / WAVES pieces per
// wave, a compile-time count, so the compiler's vmcnt accounting stays exact
// across the issue instead of falling back to vmcnt(0) at the next use of an
// earlier load)
template <int NB, int WAVES>
__device__ __forceinline__ void siren_issue_block_u(const float* __restrict__ wimg, int J, float* dst,
                                                    int wave, int lane) {
    static_assert(NB % WAVES == 0, "whole pieces per wave");
    constexpr int BLK = NB * 256;
    const float* src = wimg + (int64_t)__builtin_amdgcn_readfirstlane(J) * BLK;
    static_for<NB / WAVES>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int piece = wave + m * WAVES;
        __builtin_amdgcn_global_load_lds((const void*)(src + piece * 256 + lane * 4),
                                         (__attribute__((address_space(3))) void*)(dst + piece * 256), 16, 0, 0);
    });
}

// Split-f16 chain (siren_split.hip).  Defined for even NB (H a multiple of 32).
bool siren_split_supported(int NB);
void launch_siren_split(int NB, SirenArgs a, int b, hipStream_t st);
// 32x32x16 form of the chain (K7t, image from pack_split_f16_32)
bool siren_split32_supported(int H, int nh);
void launch_siren_split32(int H, SirenArgs a, int b, hipStream_t st);
// split-f16 K-split tape kernels (K9t, siren_split.hip): null when NB has no form
bool tape_split_supported(int NB);
void launch_tape_split(int NB, const SirenTapeArgs& a, bool bwd, hipStream_t st);
void launch_tape_split_sum(int NB, const SirenTapeArgs& a, int rows, hipStream_t st);

struct SirenParam {
    std::string key;
    std::vector<int64_t> shape;
    bool set = false;
};

}  // namespace cfd

struct cfd_siren {
    cfd_siren_cfg cfg;
    int device = 0;
    int NB = 0;
    std::vector<cfd::SirenParam> params;
    float* w0 = nullptr;    // (H, d)
    float* fbias = nullptr; // (nh+1, H)
    float* V = nullptr;     // (nh+1, H, L)
    float* wimg = nullptr;  // nh * NB * NB*256
    float* wout = nullptr;  // (c, H)
    float* bout = nullptr;  // (c)
    float* wimg_t = nullptr; // transposed weight image, layers nh..1 (latent-gradient path)
    float* wimg16 = nullptr; // split-f16 image (hi, lo) of the scaled hidden weights, same bytes as wimg
    float* wimg16t = nullptr; // the same image of the transposes, layers nh..1 (K9t backward)
    float* wscale = nullptr; // (nh) power-of-two scale of each hidden layer in wimg16
    float* wimg32 = nullptr; // the same split in the 32x32x16 chain's k order (siren_split32)
    float* wimg32r = nullptr; // siren_split32 image of W (w0 / 2pi) s'_i: accumulators in revolutions
    float* wrev = nullptr;    // (2 nh): (w0 / 2pi) s'_i, then 1 / s'_i
    float* wimg16r = nullptr; // wimg32r's words in the order of siren_split32's 16x16x32 form
    int compute = CFD_SIREN_SPLIT_F16;
    int dense_bwd = CFD_DENSE_BWD_SUM;          // dense DPS adjoint forms (dps_dense.hip,
    int dense_compute = CFD_DENSE_COMPUTE_AUTO;  // cfd_siren_dense_set_form)
};

namespace cfd {

// latent-side pieces of siren.hip shared with the dense DPS adjoint (dps_dense.hip)
int gemm_splits(int K);
void launch_gemm_f32(bool bt, const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc,
                     int M, int N, int K, hipStream_t st, float* part = nullptr);
void film_vectors(const cfd_siren* h, const float* latents, int b, float* film, hipStream_t st);
// g_z (R, L) from the tape deltas (R, Ns, nh+1, H); D: R (nh+1) H floats and the GEMM's split-K partials
void latent_grad_from_delta(const cfd_siren* h, const float* delta, float* D, int64_t Ns, int R, float* g_latents,
                            hipStream_t st);
// chunk and tail steps of the dense adjoints (dps_dense.hip; K16 in siren_jdense.hip shares them):
// part[row][slab] = the slab's `per` items of (rows, n_items, nf) in item order;
// D[row] += the chunk's slab partials in slab order and rowss[row] += sspart[row][slab] likewise;
// norm[b] = sqrt(the sample's row sums in row order), g_latents = (D . V) / norm (zero at norm 0)
void launch_dense_slab_sum(const float* items, float* part, int n_items, int per, int64_t nf, int rows, int slabs,
                           hipStream_t st);
void launch_dense_accum(const float* part, const double* sspart, float* D, double* rowss, int rows, int slabs,
                        int64_t nf, hipStream_t st);
void dense_tail(const cfd_siren* h, const float* D, const double* rowss, float* norm, float* g_latents, float* gpart,
                int R, int T, hipStream_t st);

}  // namespace cfd
