// Native reverse loop: p_sample_loop / ddim_sample_loop (U/src/gaussian_diffusion.py:
// 441-535, 625-707) without per-step host work.
//
// The Python loop costs, per step, one ctypes U-Net call (~220 kernel launches,
// each a host-side dispatch) plus the timestep bookkeeping as torch ops -- at
// B = 1 the GPU waits on the host (config A: 2.6 ms per 19-GFLOP forward).  Here
// one step (timestep advance, U-Net forward, K6 epilogue in place) is captured
// once into a HIP graph; the step's timesteps and Philox counter live in device
// memory (SamplerCtl) and are advanced by the graph's first node, so the same
// instantiated graph replays every step of every loop.  `unroll` steps are
// captured back to back into one graph to amortise the graph launch.
//
// Results are bit-identical to the Python loop with Philox noise: the same
// kernels run with the same arguments; only the step's (seed, counter, offset)
// come from memory instead of kernel arguments.
#include <vector>

#include "sampler.hpp"

#include <hip/hip_ext.h>

struct cfd_sampler {
    const cfd_unet* unet = nullptr;
    const cfd_sched* sched = nullptr;
    int kind = 0, clip = 1, B = 0, n_steps = 0, device = 0, unroll = 1, graph = 1;
    int64_t n_per_sample = 0;
    float* x = nullptr;             // loop state (B, n_per_sample), updated in place
    float* eps = nullptr;
    int64_t* tseq = nullptr;        // (2, n_steps): table indices, then model timesteps
    int64_t* tbuf = nullptr;        // (2, B): this step's table index / model timestep per sample
    cfd::SamplerCtl* ctl = nullptr;
    void* ws = nullptr;             // U-Net workspace
    size_t ws_bytes = 0;            // (re-sized when the model's planned batch grows its split-K slab)
    // captured graphs: [0] one step, [1] `unroll` steps, and the U-Net handle version
    // they were captured at (a set_param can change a weight's split scale, which
    // is a kernel argument; set_compute changes the kernels)
    hipGraphExec_t exec[2] = {nullptr, nullptr};
    uint64_t exec_version = ~uint64_t(0);
    // known-row replacement (cfd_sampler_set_known): buffers the sampler owns, since
    // the graphs capture their addresses; the conditioned step has graphs of its own
    // (kexec: one step, `unroll` steps), so switching it on or off re-captures nothing
    float* known = nullptr;         // (B, n_per_sample)
    float* kmask = nullptr;         // (B, n_per_sample)
    float* ktab = nullptr;          // (n_t, 2)
    int has_known = 0;
    hipGraphExec_t kexec[2] = {nullptr, nullptr};
    // resampling jumps (cfd_sampler_set_jumps): per step of the loop (ja, jb), (1, 0)
    // where it does not jump; the jump step (known rows, then the jump) has a third
    // pair of graphs
    float* jtab = nullptr;          // (n_steps, 2)
    int has_jumps = 0;
    hipGraphExec_t jexec[2] = {nullptr, nullptr};
    uint64_t captures = 0;          // graph captures so far (cfd_sampler_captures)
};

namespace {

void destroy_graphs(cfd_sampler* sp) {
    for (auto* set : {sp->exec, sp->kexec, sp->jexec})
        for (int i = 0; i < 2; ++i)
            if (set[i]) {
                (void)hipGraphExecDestroy(set[i]);
                set[i] = nullptr;
            }
    sp->exec_version = ~uint64_t(0);
}

// which epilogue a step runs, and which pair of graphs holds it
enum StepMode { STEP_PLAIN = 0, STEP_KNOWN = 1, STEP_JUMP = 2 };

// one reverse step on `st`: advance the timesteps, eps = U-Net(x, t), x = step(x, eps)
void enqueue_step(const cfd_sampler* sp, StepMode mode, hipStream_t st) {
    cfd::launch_sampler_advance(sp->ctl, sp->tseq, sp->tseq + sp->n_steps, sp->tbuf, sp->tbuf + sp->B, sp->B, st);
    cfd::unet_forward_raw(sp->unet, sp->x, sp->tbuf + sp->B, sp->eps, sp->B, sp->ws, st);
    if (mode == STEP_JUMP)
        cfd::launch_sched_step_jump_ctl(sp->sched, sp->kind, sp->clip, sp->x, sp->eps, sp->tbuf, sp->ctl, sp->known,
                                        sp->kmask, sp->ktab, sp->jtab, sp->n_steps, sp->n_per_sample, sp->B, st);
    else if (mode == STEP_KNOWN)
        cfd::launch_sched_step_known_ctl(sp->sched, sp->kind, sp->clip, sp->x, sp->eps, sp->tbuf, sp->ctl, sp->known,
                                         sp->kmask, sp->ktab, sp->n_per_sample, sp->B, st);
    else
        cfd::launch_sched_step_ctl(sp->sched, sp->kind, sp->clip, sp->x, sp->eps, sp->tbuf, sp->ctl,
                                   sp->n_per_sample, sp->B, st);
}

hipGraphExec_t capture(cfd_sampler* sp, StepMode mode, int steps) {
    ++sp->captures;
    hipStream_t cs;
    CFD_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipGraph_t g = nullptr;
    hipGraphExec_t e = nullptr;
    try {
        CFD_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        try {
            for (int i = 0; i < steps; ++i) enqueue_step(sp, mode, cs);
        } catch (...) {
            hipGraph_t dummy = nullptr;
            (void)hipStreamEndCapture(cs, &dummy);
            if (dummy) (void)hipGraphDestroy(dummy);
            throw;
        }
        CFD_HIP(hipStreamEndCapture(cs, &g));
        CFD_HIP(hipGraphInstantiate(&e, g, nullptr, nullptr, 0));
    } catch (...) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipStreamDestroy(cs);
        throw;
    }
    (void)hipGraphDestroy(g);
    (void)hipStreamDestroy(cs);
    return e;
}

}  // namespace

extern "C" int cfd_sampler_create(const cfd_unet* unet, const cfd_sched* sched, int kind, int clip, int B,
                                  int64_t n_per_sample, int n_steps, const int64_t* host_tidx,
                                  const int64_t* host_tmodel, int graph, int unroll, cfd_sampler** out) {
    return cfd::guard([&] {
        CFD_REQUIRE(unet && sched && out && host_tidx && host_tmodel, CFD_EARG, "null argument");
        CFD_REQUIRE(kind == CFD_STEP_DDPM || kind == CFD_STEP_DDIM, CFD_EARG, "unknown step kind");
        CFD_REQUIRE(B > 0 && n_steps > 0 && n_per_sample > 0, CFD_EARG, "empty loop");
        CFD_REQUIRE(unroll >= 1 && unroll <= 64, CFD_EARG, "unroll must be 1..64");
        cfd::unet_check_ready(unet);
        for (int k = 0; k < n_steps; ++k)
            CFD_REQUIRE(host_tidx[k] >= 0 && host_tidx[k] < cfd::sched_nt(sched), CFD_EARG,
                        "timestep index outside the coefficient table");
        cfd::DeviceGuard dg(cfd::unet_device(unet));
        auto* sp = new cfd_sampler();
        sp->unet = unet;
        sp->sched = sched;
        sp->kind = kind;
        sp->clip = clip ? 1 : 0;
        sp->B = B;
        sp->n_steps = n_steps;
        sp->n_per_sample = n_per_sample;
        sp->device = cfd::unet_device(unet);
        sp->graph = graph ? 1 : 0;
        sp->unroll = unroll;
        try {
            CFD_HIP(hipMalloc(&sp->x, sizeof(float) * (size_t)B * n_per_sample));
            CFD_HIP(hipMalloc(&sp->eps, sizeof(float) * (size_t)B * n_per_sample));
            CFD_HIP(hipMalloc(&sp->tseq, sizeof(int64_t) * 2 * (size_t)n_steps));
            CFD_HIP(hipMalloc(&sp->tbuf, sizeof(int64_t) * 2 * (size_t)B));
            CFD_HIP(hipMalloc(&sp->ctl, sizeof(cfd::SamplerCtl)));
            sp->ws_bytes = cfd::unet_ws_bytes(unet, B);
            CFD_HIP(hipMalloc(&sp->ws, sp->ws_bytes));
            CFD_HIP(hipMemcpy(sp->tseq, host_tidx, sizeof(int64_t) * n_steps, hipMemcpyHostToDevice));
            CFD_HIP(hipMemcpy(sp->tseq + n_steps, host_tmodel, sizeof(int64_t) * n_steps, hipMemcpyHostToDevice));
        } catch (...) {
            cfd_sampler_destroy(sp);
            throw;
        }
        *out = sp;
    });
}

extern "C" void cfd_sampler_destroy(cfd_sampler* sp) {
    if (!sp) return;
    destroy_graphs(sp);
    (void)hipFree(sp->x);
    (void)hipFree(sp->eps);
    (void)hipFree(sp->tseq);
    (void)hipFree(sp->tbuf);
    (void)hipFree(sp->ctl);
    (void)hipFree(sp->ws);
    (void)hipFree(sp->known);
    (void)hipFree(sp->kmask);
    (void)hipFree(sp->ktab);
    (void)hipFree(sp->jtab);
    delete sp;
}

extern "C" int cfd_sampler_run(cfd_sampler* sp, const float* x_in, float* x_out, int k0, int k1, uint64_t seed,
                               uint64_t offset, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(sp, CFD_EARG, "null sampler");
        CFD_REQUIRE(0 <= k0 && k0 <= k1 && k1 <= sp->n_steps, CFD_EARG, "step range outside the loop");
        CFD_REQUIRE(offset % 4 == 0, CFD_EARG, "noise offset must be a multiple of 4");
        CFD_REQUIRE(!sp->has_jumps || sp->has_known, CFD_EARG,
                    "resampling jumps need known rows (cfd_sampler_set_known)");
        cfd::unet_check_ready(sp->unet);
        cfd::DeviceGuard dg(sp->device);
        const hipStream_t st = (hipStream_t)stream;
        if (const size_t need = cfd::unet_ws_bytes(sp->unet, sp->B); need > sp->ws_bytes) {
            // the model's planned batch changed (cfd_unet_set_plan_batch): a larger
            // slab, and graphs that captured the old workspace pointer are stale
            CFD_HIP(hipDeviceSynchronize());
            destroy_graphs(sp);
            CFD_HIP(hipFree(sp->ws));
            sp->ws = nullptr;
            sp->ws_bytes = 0;
            CFD_HIP(hipMalloc(&sp->ws, need));
            sp->ws_bytes = need;
        }
        const size_t bytes = sizeof(float) * (size_t)sp->B * sp->n_per_sample;
        if (x_in) CFD_HIP(hipMemcpyAsync(sp->x, x_in, bytes, hipMemcpyDeviceToDevice, st));
        cfd::launch_sampler_set(sp->ctl, (uint64_t)k0, seed, offset / 4, st);
        int k = k0;
        const StepMode mode = sp->has_jumps ? STEP_JUMP : sp->has_known ? STEP_KNOWN : STEP_PLAIN;
        if (sp->graph) {
            if (sp->exec_version != cfd::unet_version(sp->unet)) {
                destroy_graphs(sp);
                sp->exec_version = cfd::unet_version(sp->unet);
            }
            hipGraphExec_t* ex = mode == STEP_JUMP ? sp->jexec : mode == STEP_KNOWN ? sp->kexec : sp->exec;
            if (!ex[0]) {
                // the plain, the conditioned and the jump step are captured when first run
                ex[0] = capture(sp, mode, 1);
                if (sp->unroll > 1) ex[1] = capture(sp, mode, sp->unroll);
            }
            for (; sp->unroll > 1 && k + sp->unroll <= k1; k += sp->unroll) CFD_HIP(hipGraphLaunch(ex[1], st));
            for (; k < k1; ++k) CFD_HIP(hipGraphLaunch(ex[0], st));
        } else {
            for (; k < k1; ++k) enqueue_step(sp, mode, st);
        }
        if (x_out) CFD_HIP(hipMemcpyAsync(x_out, sp->x, bytes, hipMemcpyDeviceToDevice, st));
    });
}

extern "C" int cfd_sampler_set_known(cfd_sampler* sp, const float* known, int64_t known_bstride, const float* mask,
                                     int64_t mask_bstride, const float* table, void* stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(sp, CFD_EARG, "null sampler");
        if (!known) {
            sp->has_known = 0;   // the buffers and the conditioned graphs stay for the next set
            return;
        }
        CFD_REQUIRE(mask && table, CFD_EARG, "known rows need a mask and the (n_t, 2) table");
        const int64_t n = sp->n_per_sample;
        CFD_REQUIRE((known_bstride == 0 || known_bstride == n) && (mask_bstride == 0 || mask_bstride == n), CFD_EARG,
                    "known rows and mask must be shared (stride 0) or per sample (stride n)");
        cfd::DeviceGuard dg(sp->device);
        const hipStream_t st = (hipStream_t)stream;
        const size_t row = sizeof(float) * (size_t)n, tab = sizeof(float) * 2 * (size_t)cfd::sched_nt(sp->sched);
        if (!sp->known) CFD_HIP(hipMalloc(&sp->known, row * sp->B));
        if (!sp->kmask) CFD_HIP(hipMalloc(&sp->kmask, row * sp->B));
        if (!sp->ktab) CFD_HIP(hipMalloc(&sp->ktab, tab));
        for (int b = 0; b < sp->B; ++b) {
            CFD_HIP(hipMemcpyAsync(sp->known + (size_t)b * n, known + (size_t)b * known_bstride, row,
                                   hipMemcpyDeviceToDevice, st));
            CFD_HIP(hipMemcpyAsync(sp->kmask + (size_t)b * n, mask + (size_t)b * mask_bstride, row,
                                   hipMemcpyDeviceToDevice, st));
        }
        CFD_HIP(hipMemcpyAsync(sp->ktab, table, tab, hipMemcpyDeviceToDevice, st));
        sp->has_known = 1;
    });
}

extern "C" int cfd_sampler_set_jumps(cfd_sampler* sp, const float* host_jtab) {
    return cfd::guard([&] {
        CFD_REQUIRE(sp, CFD_EARG, "null sampler");
        if (!host_jtab) {
            sp->has_jumps = 0;   // the table and the jump graphs stay for the next set
            return;
        }
        for (int k = 0; k < sp->n_steps; ++k) {
            const float ja = host_jtab[2 * k], jb = host_jtab[2 * k + 1];
            CFD_REQUIRE(ja >= 0.0f && ja <= 1.0f && jb >= 0.0f && jb <= 1.0f, CFD_EARG,
                        "jump coefficients outside [0, 1]");
        }
        CFD_REQUIRE(host_jtab[2 * (sp->n_steps - 1) + 1] == 0.0f, CFD_EARG, "the last step cannot jump");
        cfd::DeviceGuard dg(sp->device);
        const size_t bytes = sizeof(float) * 2 * (size_t)sp->n_steps;
        if (!sp->jtab) CFD_HIP(hipMalloc(&sp->jtab, bytes));
        // a run in flight still reads the table it was given
        CFD_HIP(hipDeviceSynchronize());
        CFD_HIP(hipMemcpy(sp->jtab, host_jtab, bytes, hipMemcpyHostToDevice));
        sp->has_jumps = 1;
    });
}

extern "C" int cfd_sampler_captures(const cfd_sampler* sp, uint64_t* n) {
    return cfd::guard([&] {
        CFD_REQUIRE(sp && n, CFD_EARG, "null argument");
        *n = sp->captures;
    });
}

extern "C" int cfd_device_cu_count(int device, int* n_cu) {
    return cfd::guard([&] {
        CFD_REQUIRE(n_cu, CFD_EARG, "null argument");
        hipDeviceProp_t p;
        CFD_HIP(hipGetDeviceProperties(&p, device));
        *n_cu = p.multiProcessorCount;
    });
}

extern "C" int cfd_stream_create_cu_range(int device, int first_cu, int n_cu, void** stream) {
    return cfd::guard([&] {
        CFD_REQUIRE(stream, CFD_EARG, "null argument");
        int total = 0;
        CFD_REQUIRE(cfd_device_cu_count(device, &total) == 0, CFD_EARG, "bad device");
        CFD_REQUIRE(first_cu >= 0 && n_cu > 0 && first_cu + n_cu <= total, CFD_EARG, "CU range outside the device");
        std::vector<uint32_t> mask((size_t)(total + 31) / 32, 0u);
        for (int c = first_cu; c < first_cu + n_cu; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
        cfd::DeviceGuard dg(device);
        hipStream_t s = nullptr;
        CFD_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
        *stream = (void*)s;
    });
}

extern "C" int cfd_stream_destroy(void* stream) {
    return cfd::guard([&] {
        if (stream) CFD_HIP(hipStreamDestroy((hipStream_t)stream));
    });
}
