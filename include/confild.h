/*
 * confild.h -- C ABI of libconfild_hip.so, the MI355X (gfx950) implementation of
 * CoNFiLD's generation hot path.
 *
 * The reference (semihkacmaz/CoNFiLD, pure Python) has no native FFI: its
 * boundary is a set of Python callables.  Each entry point below replaces the
 * arithmetic behind one of them; the Python mirror in confild_amd/ binds these
 * with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain pointers and sizes only; no framework types;
 *   - tensor pointers are DEVICE pointers on the handle's device unless the
 *     parameter name says host_; fp32 throughout (the reference computes fp32);
 *   - activations are NHWC ("channels last"); the U-Net's (B,1,H,W) input and
 *     output are identical in NCHW and NHWC because C == 1;
 *   - every call is stream-ordered on `stream` (a hipStream_t, NULL = default)
 *     and performs no host synchronisation, no allocation and no host<->device
 *     copy, except the *_create / *_set_param / cfd_sched_create calls;
 *   - return 0 on success, a CFD_E* code otherwise; cfd_last_error() gives a
 *     thread-local message.
 */
#ifndef CONFILD_H
#define CONFILD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CFD_OK = 0, CFD_EARG = 1, CFD_EHIP = 2, CFD_EKEY = 3, CFD_ESHAPE = 4, CFD_ESTATE = 5 };

const char* cfd_last_error(void);
/* Returns the library build tag ("gfx950 ..."); used to prove which .so is loaded. */
const char* cfd_version(void);

/* ------------------------------------------------------------------------ */
/* Latent U-Net (replaces UNetModel, U/src/unet.py:396-663, built by         */
/* create_model, U/src/script_util.py:130-187).                              */
/* ------------------------------------------------------------------------ */
typedef struct cfd_unet cfd_unet;

typedef struct {
    int image_size;          /* informational; H == W == image_size expected   */
    int in_channels;         /* 1 in every CoNFiLD recipe                      */
    int model_channels;      /* num_channels                                   */
    int out_channels;        /* 1 (learn_sigma=False)                          */
    int num_res_blocks;
    int n_mult;              /* len(channel_mult)                              */
    int channel_mult[8];
    int n_attn;              /* len(attention downsample rates)                */
    int attention_ds[8];     /* image_size // res for res in attention_resolutions */
    int num_heads;
    int num_head_channels;   /* -1 => use num_heads                            */
} cfd_unet_cfg;

/* Builds the topology of UNetModel.__init__ (unet.py:427-616) on `device`. */
int  cfd_unet_create(const cfd_unet_cfg* cfg, int device, cfd_unet** out);
void cfd_unet_destroy(cfd_unet* h);
/* Parameter registry in the reference's state_dict order and key names. */
int  cfd_unet_num_params(const cfd_unet* h, int* n);
int  cfd_unet_param_info(const cfd_unet* h, int idx, const char** key, int* ndim, int64_t shape[4]);
/* Copies one reference-layout fp32 tensor (torch (Cout,Cin,kh,kw) etc.) from
 * HOST memory and packs it into the kernel layout.  Replaces load_state_dict. */
int  cfd_unet_set_param(cfd_unet* h, const char* key, const float* host_data, size_t n);
/* Overrides the (model_channels/2) timestep-embedding frequencies
 * exp(-ln(1e4) * i / half) (nn.py:129-131) with host-computed fp32 values so
 * they match the caller's framework bit for bit (default: computed in C++). */
int  cfd_unet_set_time_freqs(cfd_unet* h, const float* host_freqs, int n);
/* Fails with CFD_ESTATE until every parameter has been set. */
int  cfd_unet_ready(const cfd_unet* h);
/* Every parameter at once from a DEVICE buffer: `flat` holds the fp32 tensors
 * in cfd_unet_param_info order, reference layout, n floats in total.  Packs on
 * the device (the same layouts, bf16 copy, split-f16 hi / lo with the same
 * power-of-two scales as cfd_unet_set_param, bit for bit) on `stream` and
 * synchronises it once (the split scales are launch arguments).  The training
 * loop's parameter update (train_util.py: the optimizer writes the weights the
 * next forward reads).                                                         */
int  cfd_unet_load_flat(cfd_unet* h, const float* flat, size_t n, void* stream);
int  cfd_unet_workspace_bytes(const cfd_unet* h, int B, size_t* bytes);
/* eps = UNetModel.forward(x, timesteps): x (B,1,H,W), t (B) int64 (already
 * remapped through timestep_map, respace.py:123-128), eps (B,1,H,W). */
/* Convolution operand precision (config E, BASELINE.json configs[4]):
 * CFD_COMPUTE_BF16 rounds both convolution operands to bf16 (RNE) and
 * accumulates in fp32 on v_mfma_f32_16x16x32_bf16; GroupNorm, softmax, the
 * timestep MLP and the 1-channel in/out convolutions stay fp32, attention runs
 * the fp32-accurate split-f16 kernel.
 * Default CFD_COMPUTE_SPLIT_F16 (fp32-accurate, below); CFD_COMPUTE_F32 is the
 * exact fp32 MFMA path.  This
 * replaces UNetModel's use_fp16 torso conversion (U/src/unet.py:619-633) with
 * bf16 operands. */
/* CFD_COMPUTE_SPLIT_F16: fp32-accurate convolutions on f16 MFMA -- activations
 * and power-of-two-scaled weights split into f16 hi + lo (22-bit operands),
 * three v_mfma_f32_16x16x32_f16 per product (lo*hi + hi*lo + hi*hi), fp32
 * accumulation; error against an fp64 evaluation at the fp32 kernel's level
 * (DESIGN.md K1s).  Activations must stay below 65504 in magnitude. */
#define CFD_COMPUTE_F32       0
#define CFD_COMPUTE_BF16      1
#define CFD_COMPUTE_SPLIT_F16 2
int  cfd_unet_set_compute(cfd_unet* h, int compute);
/* The batch the convolution planner tiles for (tiles, split-K counts, kernel
 * family): 0 = 8 (default).  A per-model setting, never the real batch, so a
 * sample's eps stays bit-identical whatever batch or GPU it runs in; set it to
 * the chains a GPU runs when that is far from 8 (real Case4 at one chain: 2,
 * +8 % steps/s).  No reference counterpart (a performance setting). */
int  cfd_unet_set_plan_batch(cfd_unet* h, int nominal_batch);
int  cfd_unet_forward(cfd_unet* h, const float* x, const int64_t* t, float* eps, int B,
                      void* workspace, size_t ws_bytes, void* stream);
/* Range guard of the split-f16 compute (no reference counterpart: the
 * reference's fp32 aten ops have no f16 range).  Every forward's last
 * convolution raises a device flag when an eps value is not finite -- an
 * activation beyond 65504 makes its f16 hi part infinite and reaches eps as
 * inf / NaN.  Reads the flag accumulated since the previous call (stream-
 * ordered, synchronises `stream`) into *nonfinite and clears it. */
int  cfd_unet_check_finite(cfd_unet* h, int* nonfinite, void* stream);
/* NOT PART OF THE STABLE API: a test and development entry (tests/
 * test_gpu_upsample_phase.py, tools/libdiff.py); it allocates, frees and
 * synchronises on every call and may change or go without notice.
 * One Upsample convolution (nearest 2x, then conv3x3 pad 1 with bias) of the
 * split-f16 compute on its own, planned and launched as the U-Net forward does
 * at planned batch plan_b (0: 8): x (B, H, W, Cin) and out (B, 2H, 2W, Cout) are
 * NHWC fp32 on `device`, w_host (Cout, Cin, 3, 3) and bias_host (Cout) on the
 * host.  *kx receives the planner's kernel variant (24-26: the phase forms).
 * Packs the weights, runs and synchronises: a test and development entry. */
int  cfd_upsample_conv(const float* x, const float* w_host, const float* bias_host, float* out, int B, int H,
                       int W, int Cin, int Cout, int plan_b, int device, int* kx, void* stream);

/* Input-gradient of the U-Net (DPS adjoint; replaces the autograd.grad of
 * grad_and_value through UNetModel.forward, C/src/guided_diffusion/
 * condition_methods.py:31-47, C/unet.py).  cfd_unet_forward_tape is
 * cfd_unet_forward (bit-identical eps) that also keeps every activation the
 * backward needs in `tape`; cfd_unet_input_vjp then computes
 * d_x = (d eps / d x)^T d_eps for that forward (same h, B and tape).  Weights are
 * constants: no parameter gradients. */
int  cfd_unet_tape_bytes(const cfd_unet* h, int B, size_t* bytes);
int  cfd_unet_vjp_workspace_bytes(const cfd_unet* h, int B, size_t* bytes);
int  cfd_unet_forward_tape(cfd_unet* h, const float* x, const int64_t* t, float* eps, int B,
                           void* workspace, size_t ws_bytes, void* tape, size_t tape_bytes, void* stream);
int  cfd_unet_input_vjp(cfd_unet* h, const float* d_eps, float* d_x, int B, const void* tape,
                        size_t tape_bytes, void* workspace, size_t ws_bytes, void* stream);
/* What the next cfd_unet_forward_tape records (and cfd_unet_tape_bytes sizes):
 * CFD_TAPE_INPUT_VJP (default) the activations cfd_unet_input_vjp reads, nothing
 * more (the DPS adjoint); CFD_TAPE_PARAM_GRAD also every GroupNorm(+SiLU) output
 * the convolutions read and its max |.| -- the operands of cfd_unet_param_grad's
 * split weight gradients, which otherwise recompute them (one activation per
 * GroupNorm of tape memory, +0.3 ms per Case1 forward, -2.5 ms per backward).
 * The handle remembers, per tape pointer, the mode, batch and planned batch each
 * cfd_unet_forward_tape recorded (the 64 most recent tapes): input_vjp /
 * param_grad replay THAT tape's layout, so several live tapes of different modes
 * stay valid; replaying a tape the handle did not record (or recorded at another
 * B or plan) fails with CFD_ESTATE / CFD_EARG instead of reading a wrong layout. */
#define CFD_TAPE_INPUT_VJP  0
#define CFD_TAPE_PARAM_GRAD 1
int  cfd_unet_set_tape_mode(cfd_unet* h, int mode);

/* ------------------------------------------------------------------------ */
/* Diffusion step epilogue (replaces p_mean_variance + p_sample / ddim_sample */
/* for EPSILON / FIXED_LARGE, U/src/gaussian_diffusion.py:232-326,395-439,    */
/* 537-585).                                                                   */
/* ------------------------------------------------------------------------ */
typedef struct cfd_sched cfd_sched;
enum { CFD_COEF_SRA = 0, CFD_COEF_SRM1, CFD_COEF_M1, CFD_COEF_M2, CFD_COEF_SIGMA,
       CFD_COEF_SQRT_ABP, CFD_COEF_DIR, CFD_COEF_SIGMA_DDIM, CFD_NCOEF };
enum { CFD_STEP_DDPM = 0, CFD_STEP_DDIM = 1 };

/* host_coefs: n_t rows of CFD_NCOEF fp32 values, the float64 tables of the
 * (respaced) process already cast to fp32 the way _extract_into_tensor does
 * (gaussian_diffusion.py:899-912). */
int  cfd_sched_create(const float* host_coefs, int n_t, int device, cfd_sched** out);
void cfd_sched_destroy(cfd_sched* s);
/* x_out = step(x, eps, t).  t: (B) int64 device indices into the table.
 * noise: (B*n) device normals in the reference's draw order, or NULL to draw
 * them in-kernel with Philox4x32-10 keyed by (seed, counter); element i of
 * this call uses stream position offset + i (offset % 4 == 0), so a batch
 * sharded over ranks draws exactly the normals of the unsharded batch.
 * xstart_out may be NULL.  x_out may alias x. */
int  cfd_sched_step(const cfd_sched* s, int kind, int clip, const float* x, const float* eps,
                    const int64_t* t, const float* noise, uint64_t seed, uint64_t counter,
                    uint64_t offset, float* x_out, float* xstart_out, int64_t n_per_sample, int B,
                    void* stream);
/* cfd_sched_step followed by known-row replacement (no reference counterpart; the
 * cheap route of conditioning on known latent rows).  With s the step's sample
 * at table index i, computed exactly as cfd_sched_step does:
 *   q   = a_i * known + b_i * n2        a_i = sqrt(abar_prev[i]), b_i = sqrt(1 - abar_prev[i])
 *   out = m * q + (1 - m) * s           (fp contraction off, in this order)
 * so the known rows are carried at the noise level of the state the step
 * produces; at i = 0, q = known.  m = 0 leaves s bit for bit, m = 1 gives q.
 * known / mask: (n_per_sample) tables shared by the batch (stride 0) or per sample
 * (stride n_per_sample).  table: (n_t, 2) device fp32 rows (a_i, b_i), float64
 * tables cast to fp32 like host_coefs.  n2: noise2 (B*n device normals), or NULL
 * for Philox (seed, counter2) at stream position offset + element; the loops use
 * counter2 = (1 << 41) + k, apart from the step's k and the initial noise's 1 << 40. */
int  cfd_sched_step_known(const cfd_sched* s, int kind, int clip, const float* x, const float* eps,
                          const int64_t* t, const float* noise, uint64_t seed, uint64_t counter,
                          uint64_t offset, float* x_out, float* xstart_out, int64_t n_per_sample, int B,
                          const float* known, int64_t known_bstride, const float* mask, int64_t mask_bstride,
                          const float* table, const float* noise2, uint64_t counter2, void* stream);
/* cfd_sched_step_known followed by a resampling jump (RePaint, Lugmayr et al. 2022;
 * no reference counterpart).  With out the known-row step's result, at the noise
 * level L = i - 1 the step at table index i produces:
 *   x_out = ja * out + jb * n3          (fp contraction off, in this order)
 * the forward process from level L to level L + J in one merged step,
 *   rho = abar[L + J] / abar[L],  (ja, jb) = (sqrt(rho), sqrt(1 - rho)) as fp32
 * (the distribution of J single steps sqrt(1 - beta) x + sqrt(beta) eps).  jb == 0
 * skips the jump: x_out is cfd_sched_step_known's, bit for bit.  xstart_out is
 * unaffected.  n3: noise3 (B*n device normals), or NULL for Philox (seed, counter3)
 * at stream position offset + element; the loops use counter3 = (1 << 42) + k, a
 * fourth range beside k, 1 << 40 and (1 << 41) + k.  Same argument checks as
 * cfd_sched_step_known. */
int  cfd_sched_step_jump(const cfd_sched* s, int kind, int clip, const float* x, const float* eps,
                         const int64_t* t, const float* noise, uint64_t seed, uint64_t counter,
                         uint64_t offset, float* x_out, float* xstart_out, int64_t n_per_sample, int B,
                         const float* known, int64_t known_bstride, const float* mask, int64_t mask_bstride,
                         const float* table, const float* noise2, uint64_t counter2, float ja, float jb,
                         const float* noise3, uint64_t counter3, void* stream);
/* Native reverse loop (p_sample_loop / ddim_sample_loop, gaussian_diffusion.py:
 * 441-535 / 625-707, with Philox noise): per step the timestep advance, the U-Net
 * forward and the K6 epilogue, with no host work between steps.  graph != 0
 * captures the step once into a HIP graph (`unroll` steps per graph, 1..64) and
 * replays it; the step's timesteps and Philox counter live in device memory.
 * host_tidx[k] / host_tmodel[k]: coefficient-table index / model timestep
 * (timestep_map) of step k in loop order.  The sampler owns its state, eps and
 * U-Net workspace; `unet` and `sched` must outlive it.  Parameters set on
 * `unet` later and compute-mode changes are seen (the graph is re-captured
 * when the handle changed since the last capture).
 * cfd_sampler_run: steps [k0, k1) of the loop; x_in (B * n_per_sample) is
 * copied in first unless NULL (continue from the state), x_out receives the
 * state afterwards unless NULL.  Step k draws Philox(seed, counter = k) at
 * stream position offset + element (offset % 4 == 0), exactly as
 * cfd_sched_step with counter k, so the result is bit-identical to a host loop
 * of cfd_unet_forward + cfd_sched_step. */
typedef struct cfd_sampler cfd_sampler;
int  cfd_sampler_create(const cfd_unet* unet, const cfd_sched* sched, int kind, int clip, int B,
                        int64_t n_per_sample, int n_steps, const int64_t* host_tidx, const int64_t* host_tmodel,
                        int graph, int unroll, cfd_sampler** out);
void cfd_sampler_destroy(cfd_sampler* sp);
/* A stream whose kernels run on CUs [first_cu, first_cu + n_cu) of the device only
 * (hipExtStreamCreateWithCUMask): the sampling loop and the CNF decode of the
 * previous batch run side by side on disjoint halves of the chip (bench.py config
 * B).  No reference counterpart (an execution resource). */
int  cfd_device_cu_count(int device, int* n_cu);
int  cfd_stream_create_cu_range(int device, int first_cu, int n_cu, void** stream);
int  cfd_stream_destroy(void* stream);
int  cfd_sampler_run(cfd_sampler* sp, const float* x_in, float* x_out, int k0, int k1, uint64_t seed,
                     uint64_t offset, void* stream);
/* Known rows for the following cfd_sampler_run calls: every step becomes
 * cfd_sched_step_known with counter2 = (1 << 41) + k read from device memory.
 * known, mask (strides 0 or n_per_sample) and table ((n_t, 2)) are device arrays,
 * copied on `stream` into buffers the sampler owns (graphs capture addresses), so
 * new contents need no re-capture.  The conditioned step has its own captured
 * graphs next to the unconditioned ones; known == NULL clears it, and the runs
 * that follow are the unconditioned loop, its graphs and its bits.
 * cfd_sampler_captures: the number of graph captures the sampler has made. */
int  cfd_sampler_set_known(cfd_sampler* sp, const float* known, int64_t known_bstride, const float* mask,
                           int64_t mask_bstride, const float* table, void* stream);
int  cfd_sampler_captures(const cfd_sampler* sp, uint64_t* n);
/* Resampling jumps for the following cfd_sampler_run calls.  A resampled loop is a
 * sampler created with the expanded step sequence (a level is visited more than
 * once; host_tidx / host_tmodel repeat accordingly); host_jtab is a host array of
 * n_steps rows (ja, jb), (1, 0) where step k does not jump, copied into a table
 * the sampler owns.  Every step then becomes cfd_sched_step_jump with (ja, jb)
 * read from row k and counter3 = (1 << 42) + k, on a third pair of captured graphs:
 * the whole schedule replays one graph, with no host work at the jump points.
 * Needs known rows: cfd_sampler_run returns CFD_EARG while jumps are set and
 * known rows are not.  host_jtab == NULL clears the jumps.  Synchronises the
 * device (the table is rewritten in place). */
int  cfd_sampler_set_jumps(cfd_sampler* sp, const float* host_jtab);
/* n standard normals from Philox4x32-10 (seed, counter) at stream positions
 * offset .. offset+n-1 (offset % 4 == 0): the device-side stand-in for th.randn
 * (gaussian_diffusion.py:513). */
int  cfd_randn(float* out, int64_t n, uint64_t seed, uint64_t counter, uint64_t offset, void* stream);
/* Diagnostic: y = sin(x) by the decoder's device sine -- which 0: Cody-Waite pi
 * reduction + degree-9 polynomial (sin_cw family), 1: Cody-Waite 2pi reduction +
 * v_sin_f32, 2: reduction in revolutions (two-float 1/2pi) + v_sin_f32 (the
 * split32 decoder's default).  Used by the tests to bound each against float64
 * (components.py:19-25 Sine = torch.sin). */
int  cfd_sine_probe(const float* x, float* y, int64_t n, int which, void* stream);
/* Latent de-normalisation (scripts/inference.py:59-61): y = (x+1)*(max-min)/2 + min,
 * max/min broadcast over the trailing `period` elements (period=1: scalars). */
int  cfd_latent_denorm(const float* x, float* y, int64_t n, const float* vmax, const float* vmin,
                       int64_t period, void* stream);

/* DPS glue (Case4 conditional sampling, C/src/guided_diffusion/condition_methods.py:31-47,81-90):
 *   cfd_dps_residual     per sample: norm_b = ||y - A_b||_2, g_A = -(y - A_b) / norm_b
 *                        (y shared when y_batch_stride == 0, else per sample);
 *   cfd_dps_latent_grad  g_z (d norm / d unnormalised latent) -> d_eps = -srm1 * g and
 *                        g_direct = sra * g, g = clamp'(x0) * g_z * (max - min) / 2
 *                        (Case4Operator._unnorm, measurements.py:219-220);
 *   cfd_dps_update       x_out = sample - (g_direct + g_unet) * scale. */
int  cfd_dps_residual(const float* y, int64_t y_batch_stride, const float* A, float* g_A, float* norm,
                      int64_t n_per_sample, int B, void* stream);
int  cfd_dps_latent_grad(const cfd_sched* s, int clip, const float* x, const float* eps, const int64_t* t,
                         const float* g_z, const float* vmax, const float* vmin, int64_t period,
                         float* d_eps, float* g_direct, int64_t n_per_sample, int B, void* stream);
int  cfd_dps_update(const float* sample, const float* g_direct, const float* g_unet, float scale,
                    float* x_out, int64_t n, void* stream);
/* cfd_dps_update followed by known-row replacement, in one launch (no reference
 * counterpart): the last call of a DPS step whose sampler holds latent rows to
 * known values.  Per element, fp contraction off, in this order:
 *   img = sample - (g_direct + g_unet) * scale     cfd_dps_update's x_out, bit for bit
 *   q   = a_i * known + b_i * n2                   (a_i, b_i) = row t[b] of table
 *   out = m * q + (1 - m) * img                    cfd_sched_step_known's replacement, bit for bit
 * so the gradient update acts where m = 0 and the known rows stand, at the noise
 * level the step produces, where m = 1; at t[b] = 0, q = known.  t: (B) int64
 * device indices into table ((n_t, 2) device fp32 rows, as cfd_sched_step_known's).
 * known / mask: shared by the batch (stride 0) or per sample (stride n_per_sample).
 * n2: noise2 (B*n device normals), or NULL for Philox (seed, counter2) at stream
 * position offset + element (offset % 4 == 0): four elements per thread with
 * cfd_sched_step_known's group offset, so the normals are the ones it draws for the
 * same (seed, counter2, offset); the guided loop uses counter2 = (1 << 41) + k.
 * Any n_per_sample (a last group of fewer than 4 elements included); arrays that
 * are 16-byte aligned with n_per_sample % 4 == 0 take 16-byte loads and stores,
 * the same bits.  x_out may alias sample.  CFD_EARG, and no launch, for a null
 * array other than noise2, offset % 4 != 0, an empty step, or a stride that is
 * neither 0 nor n_per_sample. */
int  cfd_dps_update_known(const float* sample, const float* g_direct, const float* g_unet, float scale,
                          float* x_out, const int64_t* t, int64_t n_per_sample, int B, const float* known,
                          int64_t known_bstride, const float* mask, int64_t mask_bstride, const float* table,
                          const float* noise2, uint64_t seed, uint64_t counter2, uint64_t offset, void* stream);
/* The 'inpainting' operator under 'ps' (measurements.py:40-56: A(x0) = mask * x0 on
 * the latent image): what cfd_dps_residual and cfd_dps_latent_grad do for a SIREN
 * operator, in one call and without a decoder.  Per sample b:
 *   x0     = sra * x - srm1 * eps, clamped when clip (cfd_sched_step's pred_xstart, the same bits)
 *   r      = y - m * x0,   norm[b] = ||r||_2
 *   g      = -m * (r / norm[b]); zero where norm[b] == 0 and, with clip, where the
 *            unclamped x0 lies outside [-1, 1]
 *   d_eps  = -g * srm1,    g_direct = g * sra
 * y / mask: (n_per_sample) tables shared by the batch (stride 0) or per sample
 * (stride n_per_sample).  The norm is summed in float64 over fixed 4096-element
 * chunks (one workgroup each) whose partials add in chunk order: the order is a
 * function of n_per_sample alone, not of B or the grid, and there are no atomics.
 * workspace: cfd_dps_latent_residual_workspace_bytes(n_per_sample, B), 8-byte aligned. */
int  cfd_dps_latent_residual_workspace_bytes(int64_t n_per_sample, int B, size_t* bytes);
int  cfd_dps_latent_residual(const cfd_sched* s, int clip, const float* x, const float* eps, const int64_t* t,
                             const float* y, int64_t y_bstride, const float* mask, int64_t mask_bstride,
                             float* norm, float* d_eps, float* g_direct, int64_t n_per_sample, int B,
                             void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------ */
/* Conditional neural field decoder: SIRENAutodecoder_film                    */
/* (N/cnf/nf_networks.py:443-495, BatchLinear/Sine components.py:19-25,55-76) */
/* fused with Normalizer_ts '-11' (N/cnf/utils/normalize.py:100-114).         */
/* ------------------------------------------------------------------------ */
typedef struct cfd_siren cfd_siren;

typedef struct {
    int in_coord_features;   /* d  (<= 4)                                     */
    int in_latent_features;  /* L                                            */
    int out_features;        /* c  (<= 4)                                     */
    int num_hidden_layers;   /* nh                                           */
    int hidden_features;     /* H  (multiple of 16, <= 512)                  */
    float w0;                /* 30 (DEFAULT_W0)                              */
} cfd_siren_cfg;

int  cfd_siren_create(const cfd_siren_cfg* cfg, int device, cfd_siren** out);
void cfd_siren_destroy(cfd_siren* h);
int  cfd_siren_num_params(const cfd_siren* h, int* n);
int  cfd_siren_param_info(const cfd_siren* h, int idx, const char** key, int* ndim, int64_t shape[4]);
/* keys net1.{i}.weight/bias, net2.{i}.weight (host fp32, reference layout). */
int  cfd_siren_set_param(cfd_siren* h, const char* key, const float* host_data, size_t n);
int  cfd_siren_ready(const cfd_siren* h);
int  cfd_siren_workspace_bytes(const cfd_siren* h, int b, size_t* bytes);
/* out (b, N, c) = denorm( NF( norm(coords), latents ) ).
 *   coords (N, d); latents (b, L);
 *   xmax/xmin: (d) coordinate normaliser params, or NULL (coords already normalised);
 *   ymax/ymin: output normaliser params with row stride y_stride (elements) per
 *              coordinate: y_stride = c for a per-point (N, c) table (lumped
 *              latent, train.py:194-201), 0 for a (c) table; NULL = raw output. */
/* Hidden-layer arithmetic of cfd_siren_forward:
 * CFD_SIREN_SPLIT_F16 (default; H a multiple of 32, nh >= 1): every product W x
 *   as three v_mfma_f32_16x16x32_f16 on two-term f16 splits of the power-of-two
 *   scaled weights and of the activations (Wl xh + Wh xl + Wh xh, fp32
 *   accumulate): 22-bit operands, exact products, fp32 accumulation -- the error
 *   against an fp64 evaluation matches the fp32 chain's;
 * CFD_SIREN_F32: the exact fp32 v_mfma_f32_16x16x4_f32 chain.
 * Env CFD_SIREN_COMPUTE overrides the default at handle creation.
 * cfd_siren_get_compute reports the mode a forward actually runs. */
#define CFD_SIREN_F32       0
#define CFD_SIREN_SPLIT_F16 1
int  cfd_siren_set_compute(cfd_siren* h, int compute);
int  cfd_siren_get_compute(const cfd_siren* h, int* compute);
int  cfd_siren_forward(cfd_siren* h, const float* coords, int64_t N, const float* latents, int b,
                       const float* xmax, const float* xmin,
                       const float* ymax, const float* ymin, int64_t y_stride,
                       float* out, void* workspace, size_t ws_bytes, void* stream);
/* cfd_siren_forward together with its coordinate Jacobian, one fused launch
 * (csrc/siren_jac.hip): jac (b, N, c, d), jac[b, n, o, k] = d out[b, n, o] /
 * d coords[n, k] in physical units on both sides (the chain rule through both
 * normalisers is applied: 2 / (xmax_k - xmin_k) in, (ymax - ymin) / 2 out).
 * Arguments, normaliser forms (y_stride 0 or c, NULL pairs), workspace and error
 * codes as cfd_siren_forward; out may be NULL (only the Jacobian is stored).
 * Always the exact fp32 MFMA chain, whatever cfd_siren_set_compute chose; the
 * bits of a (latent row, point) pair depend on neither b, N, the point's index
 * nor the other rows.  in_coord_features = 4 returns CFD_EARG. */
int  cfd_siren_jacobian_workspace_bytes(const cfd_siren* h, int b, size_t* bytes);
int  cfd_siren_forward_jacobian(cfd_siren* h, const float* coords, int64_t N, const float* latents, int b,
                                const float* xmax, const float* xmin,
                                const float* ymax, const float* ymin, int64_t y_stride,
                                float* out, float* jac,
                                void* workspace, size_t ws_bytes, void* stream);
/* cfd_siren_forward_jacobian on the f16 matrix pipes with fp32-level accuracy
 * (csrc/siren_jac_split.hip, K13s): every hidden product as three
 * v_mfma_f32_16x16x32_f16 on hi/lo f16 halves (CFD_SIREN_SPLIT_F16's arithmetic).
 * Each tangent column is split at a power-of-two scale of its own, taken per layer
 * from the column's largest magnitude and undone exactly at the head, so no finite
 * tangent overflows an f16 half and scaling the coordinates by a power of two scales
 * jac by exactly its inverse.  Same parameters, normaliser forms, workspace
 * (cfd_siren_jacobian_workspace_bytes), NULL out and invariances as
 * cfd_siren_forward_jacobian; not selected by cfd_siren_set_compute.  Besides that
 * entry's errors, CFD_EARG before any launch unless hidden_features is
 * 32*{1,2,3,4,6,8,12}, num_hidden_layers >= 1, in_coord_features <= 3 and the LDS
 * staging (2 weight blocks + the FiLM rows) is within 160 KiB. */
int  cfd_siren_forward_jacobian_split(cfd_siren* h, const float* coords, int64_t N, const float* latents, int b,
                                      const float* xmax, const float* xmin,
                                      const float* ymax, const float* ymin, int64_t y_stride,
                                      float* out, float* jac,
                                      void* workspace, size_t ws_bytes, void* stream);
/* The same with the second derivatives, one fused launch (csrc/siren_hess.hip):
 * hess (b, N, c, d, d), hess[b, n, o, k, l] = d2 out[b, n, o] / d coords[n, k]
 * d coords[n, l] in physical units (the coordinate scales of both axes and
 * (ymax - ymin) / 2 applied), symmetric to the bit; with diag_only != 0 hess is
 * (b, N, c, d), the unmixed derivatives d2 / d coords[n, k]^2 alone, with the bits
 * of the full form's diagonal.  out (b, N, c) and jac (b, N, c, d) may each be
 * NULL (that store is skipped); hess is required.  Arguments, normaliser forms,
 * workspace and error codes as cfd_siren_forward_jacobian; always the exact fp32
 * MFMA chain; in_coord_features = 4 returns CFD_EARG before any launch. */
int  cfd_siren_hessian_workspace_bytes(const cfd_siren* h, int b, size_t* bytes);
int  cfd_siren_forward_hessian(cfd_siren* h, const float* coords, int64_t N, const float* latents, int b,
                               const float* xmax, const float* xmin,
                               const float* ymax, const float* ymin, int64_t y_stride,
                               float* out, float* jac, float* hess, int diag_only,
                               void* workspace, size_t ws_bytes, void* stream);
/* cfd_siren_forward_hessian on the f16 matrix pipes with fp32-level accuracy
 * (csrc/siren_hess_split.hip, K14s): cfd_siren_forward_jacobian_split's arithmetic
 * (three v_mfma_f32_16x16x32_f16 on hi/lo f16 halves per 32 features) with the
 * second-order columns.  Every tangent and second-order column is split at a
 * power-of-two scale of its own, taken per layer from the column's largest magnitude;
 * the second-order update, a product of two tangent columns, is formed in the larger
 * of the two frames it meets, and every scale is undone exactly at the head: no
 * finite column overflows an f16 half, and scaling coordinate k by a power of two
 * scales jac[.., k] and hess[.., k, l] by exactly its inverse (twice for k = l).
 * Same parameters, NULL out / jac, diag_only, normaliser forms, workspace
 * (cfd_siren_hessian_workspace_bytes), symmetry and invariances as
 * cfd_siren_forward_hessian; not selected by cfd_siren_set_compute.  Besides that
 * entry's errors, CFD_EARG before any launch unless hidden_features is
 * 32*{1,2,3,4,6,8,12}, num_hidden_layers >= 1, in_coord_features <= 3 and the LDS
 * staging (2 weight blocks + the FiLM rows) is within 160 KiB. */
int  cfd_siren_forward_hessian_split(cfd_siren* h, const float* coords, int64_t N, const float* latents, int b,
                                     const float* xmax, const float* xmin,
                                     const float* ymax, const float* ymin, int64_t y_stride,
                                     float* out, float* jac, float* hess, int diag_only,
                                     void* workspace, size_t ws_bytes, void* stream);

/* Latent-gradient of the Case4 measurement operator (DPS; replaces autograd
 * through Case4Operator.forward -> pass_through_model_batch -> SIRENAutodecoder_film,
 * C/src/guided_diffusion/measurements.py:219-226, N/cnf/inference_function.py:22-48).
 * cfd_siren_tape_forward = cfd_siren_forward over Ns sensor coordinates for R
 * latent rows, keeping each layer's pre-activation in the workspace;
 * cfd_siren_tape_vjp: g_latents (R, L) = d<g_out, out>/d latents for that forward
 * (same h, Ns, R, workspace and y normaliser). */
int  cfd_siren_vjp_workspace_bytes(const cfd_siren* h, int64_t Ns, int R, size_t* bytes);
int  cfd_siren_tape_forward(cfd_siren* h, const float* coords, int64_t Ns, const float* latents, int R,
                            const float* xmax, const float* xmin,
                            const float* ymax, const float* ymin, int64_t y_stride,
                            float* out, void* workspace, size_t ws_bytes, void* stream);
int  cfd_siren_tape_vjp(cfd_siren* h, const float* g_out, int64_t Ns, int R,
                        const float* ymax, const float* ymin, int64_t y_stride,
                        float* g_latents, void* workspace, size_t ws_bytes, void* stream);

/* Latent gradient of a linear functional of the value and the coordinate Jacobian
 * at sensor points (K15: derivative sensors in the DPS sampler; no reference
 * counterpart).  cfd_siren_jtape_forward = cfd_siren_forward_jacobian over Ns sensor
 * coordinates for R latent rows (out (R, Ns, c), jac (R, Ns, c, d), physical units,
 * both required), keeping every layer's value and tangent accumulators in the
 * workspace; cfd_siren_jtape_vjp:
 *   g_latents (R, L) = d( <g_out, out> + <g_jac, jac> ) / d latents
 * for that forward (same h, Ns, R, workspace and y normaliser).  g_out (R, Ns, c) and
 * g_jac (R, Ns, c, d) may each be NULL, which means zero.  Always the exact fp32 MFMA
 * chain, whatever cfd_siren_set_compute chose; deterministic, and a row's result does
 * not depend on R or on the other rows.
 * Workspace (16-byte aligned), with nl = num_hidden_layers + 1, H = hidden_features,
 * P = R Ns, nf = nl H: (2 + d) P nf floats of tape and deltas + 2 R nf (FiLM vectors,
 * sensor sums) + the latent GEMM's split-K partials; ask cfd_siren_jtape_workspace_bytes.
 * CFD_EARG before any launch: a NULL required pointer, Ns < 1 or > 2^20, R < 1,
 * normaliser bounds not in pairs, a workspace even one byte short and
 * in_coord_features = 4.  Widths: hidden_features = 16*{1,2,3,4,6,8,12,16,24,32}
 * (512 runs 4 waves per workgroup, none uses scratch). */
int  cfd_siren_jtape_workspace_bytes(const cfd_siren* h, int64_t Ns, int R, size_t* bytes);
int  cfd_siren_jtape_forward(cfd_siren* h, const float* coords, int64_t Ns, const float* latents, int R,
                             const float* xmax, const float* xmin,
                             const float* ymax, const float* ymin, int64_t y_stride,
                             float* out, float* jac, void* workspace, size_t ws_bytes, void* stream);
int  cfd_siren_jtape_vjp(cfd_siren* h, const float* g_out, const float* g_jac, int64_t Ns, int R,
                         const float* ymax, const float* ymin, int64_t y_stride,
                         float* g_latents, void* workspace, size_t ws_bytes, void* stream);
/* The residual of linear sensor stencils on (out, jac) of cfd_siren_jtape_forward:
 *   A[r, s, m] = sum_o wv[s, m, o] out[r, s, o] + sum_{o,k} wj[s, m, o, k] jac[r, s, o, k]
 * wv (M, c) or, with wv_per_sensor, (Ns, M, c); wj (M, c, d) or (Ns, M, c, d); either
 * may be NULL (with its gradient output), not both.  y: rows_per_sample tables of
 * (Ns, M) shared by the B samples, or with y_per_sample B rows_per_sample of them.
 * Per sample b (rows [b T, (b+1) T), T = rows_per_sample): norm[b] = ||y - A||_2
 * (float64 sum in a fixed order), g_out = wv^T g and g_jac = wj^T g with
 * g = -(y - A) / norm[b] (zero where the norm is zero, as cfd_dps_residual).
 * A (R, Ns, M) is written when not NULL.  c <= 4, d <= 3. */
int  cfd_dps_residual_linear(const float* y, int y_per_sample, const float* out, const float* jac,
                             const float* wv, int wv_per_sensor, const float* wj, int wj_per_sensor,
                             float* g_out, float* g_jac, float* norm, float* A, int64_t Ns, int M, int c,
                             int d, int rows_per_sample, int B, void* stream);

/* Dense masked DPS adjoint (Case2 / Case3 operators: a whole field of N points,
 * measurements.py:58-181): the masked residual norm and its latent gradient in
 * one call whose workspace is bounded by `budget` and does not grow with N.
 * For sample b owning rows [b T, (b+1) T), T = rows_per_sample:
 *   norm[b]   = || y - m (.) A ||_2 over the sample's T N c values, A the value
 *               cfd_siren_forward gives; g_latents (R, L) = d norm / d latents
 *               (zero where the norm is zero, as cfd_dps_residual).
 *   y:    y_rows tables of (N, c), y_rows = rows_per_sample (shared by the samples)
 *         or R; row r reads table r % y_rows.
 *   mask: NULL (all ones) or mask_rows in {1, rows_per_sample, R} tables of (N, c),
 *         row r reads table r % mask_rows.
 * The N points are walked in chunks of whole 64-point slabs (and, where even one
 * slab of all R rows exceeds the budget, in blocks of rows): tape forward,
 * residual, backward, per-slab sums added into D (R, (nh+1) H) in slab order;
 * then g = (D . V) / norm.  The reduction tree is a function of N alone, so
 * g_latents and norm do not depend on budget or on how many samples share the
 * call.  budget = 0: the library default (CFD_DENSE_DEFAULT_BUDGET).  A budget
 * too small for one slab of one row: CFD_EARG before any launch.
 * cfd_siren_dense_plan: the same planner from a configuration alone (no device);
 * also reports the points per chunk and rows per block it chose. */
#define CFD_DENSE_SLAB 64
#define CFD_DENSE_DEFAULT_BUDGET ((size_t)1 << 30)
int  cfd_siren_dense_plan(const cfd_siren_cfg* cfg, int64_t N, int R, size_t budget, int bwd_form,
                          int compute_form, size_t* bytes, int64_t* chunk_points, int* block_rows);
int  cfd_siren_dense_workspace_bytes(const cfd_siren* h, int64_t N, int R, size_t budget, size_t* bytes);
int  cfd_siren_dense_grad(cfd_siren* h, const float* coords, int64_t N,
                          const float* latents, int R, int rows_per_sample,
                          const float* xmax, const float* xmin,
                          const float* ymax, const float* ymin, int64_t y_stride,
                          const float* y, int y_rows,
                          const float* mask, int mask_rows,
                          float* g_latents, float* norm,
                          void* workspace, size_t ws_bytes, size_t budget, void* stream);
/* Forms of the dense adjoint (development: tools/dense_dps_bench.py times them,
 * profiles/dense_dps.json; the defaults are the shipped choice):
 * compute   CFD_DENSE_COMPUTE_AUTO (default): the K9t split-f16 tape kernels for a
 *           handle in CFD_SIREN_SPLIT_F16 whose width they take (H = 128, 256, 384),
 *           else the fp32 MFMA chain; _F32: the fp32 chain.  A handle in
 *           CFD_SIREN_F32 always runs the exact fp32 chain.
 * backward  CFD_DENSE_BWD_SUM (default): the deltas of a tile (16 points in K9t, 64
 *           in the fp32 chain) are summed on chip and one (nh+1) H partial is stored
 *           per tile; CFD_DENSE_BWD_DELTA: the chunk's deltas are stored per pair
 *           and column-summed after.
 * cfd_siren_dense_plan takes the same two forms (for a handle in split compute). */
#define CFD_DENSE_BWD_SUM   0
#define CFD_DENSE_BWD_DELTA 1
#define CFD_DENSE_COMPUTE_AUTO  0
#define CFD_DENSE_COMPUTE_F32   1
int  cfd_siren_dense_set_form(cfd_siren* h, int bwd_form, int compute_form);

/* Dense derivative measurements (K16; no reference counterpart): the dense adjoint
 * above for linear stencils on the value and the exact coordinate Jacobian at every
 * one of N points, M readings per point,
 *   A[r, n, m] = sum_o wv[n, m, o] out[r, n, o] + sum_{o,k} wj[n, m, o, k] jac[r, n, o, k]
 * (out, jac as cfd_siren_forward_jacobian gives them, physical units):
 *   norm[b]   = || y - m (.) A ||_2 over the sample's T N M readings;
 *   g_latents (R, L) = d norm / d latents (zero where the norm is zero).
 *   wv:   (M, c), or with wv_per_point (N, M, c); wj: (M, c, d) or (N, M, c, d).
 *         Either may be NULL (no such term), not both.
 *   y:    NULL (a zero target) or y_rows tables of (N, M), y_rows = rows_per_sample
 *         or R; row r reads table r % y_rows.
 *   mask: NULL (all ones) or mask_rows in {1, rows_per_sample, R} tables of (N, M).
 * Chunks, row blocks, budget and determinism as cfd_siren_dense_grad: K15's chain
 * (cfd_siren_jtape_*) on row-aligned tiles, its tape kept for one chunk only
 * ((1 + d) rows nc (nh+1) H floats) and u-bar summed on chip, no atomics; g_latents
 * and norm do not depend on budget, row blocking or the samples sharing the call.
 * Always the exact fp32 chain, whatever cfd_siren_set_compute chose.
 * CFD_EARG before any launch: a NULL required pointer, both weights NULL, M < 1,
 * N < 1, R < 1, rows_per_sample not dividing R, y_rows / mask_rows outside the sets
 * above, in_coord_features > 3, a workspace even one byte short, a budget too small
 * for one slab of one row; CFD_ESHAPE: in_latent_features % 4 or (nh+1) H % 16.
 * cfd_siren_jdense_plan: the planner from a configuration alone (no device). */
int  cfd_siren_jdense_plan(const cfd_siren_cfg* cfg, int64_t N, int R, int M, size_t budget,
                           size_t* bytes, int64_t* chunk_points, int* block_rows);
int  cfd_siren_jdense_workspace_bytes(const cfd_siren* h, int64_t N, int R, int M, size_t budget, size_t* bytes);
int  cfd_siren_jdense_grad(cfd_siren* h, const float* coords, int64_t N,
                           const float* latents, int R, int rows_per_sample,
                           const float* xmax, const float* xmin,
                           const float* ymax, const float* ymin, int64_t y_stride,
                           const float* wv, int wv_per_point, const float* wj, int wj_per_point, int M,
                           const float* y, int y_rows,
                           const float* mask, int mask_rows,
                           float* g_latents, float* norm,
                           void* workspace, size_t ws_bytes, size_t budget, void* stream);

/* ------------------------------------------------------------------------ */
/* CNF autodecoder training (K10; N/scripts/train.py:334-416 _single_trainer:  */
/* model(coords, latents(idx)) -> MSELoss -> loss.backward(), Adam steps).     */
/* ------------------------------------------------------------------------ */
/* One backward of MSELoss(mean) for a batch: R latent rows (rows[r] indexes   *
 * the (N_samples, L) latent table `latents`, distinct), N raw coordinates     *
 * (N, d) as the model sees them, target (R, N, c).  scale = 2 / (numel of the *
 * whole loss) (ATen mse_loss_backward's factor; a caller that splits the      *
 * coordinates over several calls passes the full count).  Accumulates (+=):   *
 *   grad          flat fp32 gradient, parameters in cfd_siren_param_info order *
 *                 and reference shapes (torch's .grad accumulation);          *
 *   grad_latents  (N_samples, L): the batch's rows;                           *
 *   sse           (1) sum of squared errors of this call.                     *
 * The tape chain (forward with tape, backward to every delta) follows the      *
 * handle's compute mode: in CFD_SIREN_SPLIT_F16 at H = 128 / 256 / 384 with at *
 * least one hidden layer and fewer than 32,768 (row, coordinate) pairs in the  *
 * call it is K9t, the split-f16 tape (fp32-level error); at every other width, *
 * from 32,768 pairs on, and always under CFD_SIREN_F32, the fp32 MFMA tape.    *
 * The weight-gradient products over the pairs, the column sums and the latent  *
 * gradient are fp32 MFMA / fp32 sums in every mode (the activations recomputed *
 * from the tape the chain wrote).  Deterministic: fixed slicing and order.     */
int  cfd_siren_train_workspace_bytes(const cfd_siren* h, int64_t N, int R, size_t* bytes);
int  cfd_siren_train_grad(cfd_siren* h, const float* coords, int64_t N, const float* latents,
                          const int64_t* rows, int R, const float* target, float scale,
                          float* grad, float* grad_latents, float* sse,
                          void* workspace, size_t ws_bytes, void* stream);
/* ------------------------------------------------------------------------ */
/* Latent U-Net parameter gradients (K11; the diffusion TrainLoop's backward,  */
/* U/src/train_util.py:196-240 -> loss.backward() through UNetModel.forward).  */
/* ------------------------------------------------------------------------ */
/* For the forward recorded by cfd_unet_forward_tape(h, x, t, ...) on `tape`:   *
 * grad (flat fp32, cfd_unet_param_info order and reference shapes) +=         *
 * (d eps / d params)^T d_eps -- every convolution weight / bias, GroupNorm    *
 * gamma / beta, emb_layers and time_embed parameter; x is that forward's      *
 * input.  fp32 (fp32 MFMA weight-gradient products over the pixels, fixed     *
 * reduction orders: deterministic).                                           */
int  cfd_unet_param_grad_workspace_bytes(const cfd_unet* h, int B, size_t* bytes);
int  cfd_unet_param_grad(cfd_unet* h, const float* x, const float* d_eps, int B, const void* tape,
                         size_t tape_bytes, float* grad, void* workspace, size_t ws_bytes, void* stream);
/* GaussianDiffusion.training_losses' MSE term on eps (gaussian_diffusion.py    *
 * :775-853) and the backward of (loss * weights).mean() (train_util.py:210):   *
 * d_eps = scale * weights[b] * (eps - noise) (scale = 2 / numel for the batch  *
 * mean of mean_flat; weights may be null = 1), sse[b] = sum over sample b of   *
 * (eps - noise)^2.                                                             */
int  cfd_eps_mse(const float* eps, const float* noise, const float* weights, float* d_eps,
                 int64_t n_per_sample, int B, float scale, float* sse, void* stream);
/* update_ema (U/src/nn.py:71-80): target = target * rate + source * (1 - rate). */
int  cfd_ema_update(float* target, const float* source, int64_t n, double rate, void* stream);
/* q_sample (U/src/gaussian_diffusion.py:188-206): x_t = coef_a[b] x0 +        *
 * coef_s[b] noise per sample, coef_a / coef_s the fp32 casts of              *
 * sqrt(alphas_cumprod[t]) / sqrt(1 - alphas_cumprod[t]).                      */
int  cfd_q_sample(const float* x0, const float* noise, const float* coef_a, const float* coef_s, float* x_t,
                  int64_t n_per_sample, int B, void* stream);
/* torch.optim.Adam / AdamW step (amsgrad off) over n fp32 elements: exp_avg /  *
 * exp_avg_sq updated in place, step = the 1-based step count; weight_decay > 0 *
 * is AdamW's decoupled decay (param *= 1 - lr * weight_decay first).           */
int  cfd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CONFILD_H */
