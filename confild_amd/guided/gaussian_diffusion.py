"""Guided samplers (C/src/guided_diffusion/gaussian_diffusion.py): create_sampler,
DDPM / DDIM with the conditional p_sample_loop of the Case4 notebook.

One reverse step of the 'ps' (DPS) loop, reference (gaussian_diffusion.py:
169-206, 362-372; condition_methods.py:31-47,81-90):

    out = p_sample(x)                      # eps = U(x, t); x0 = clamp(c1 x - c2 eps); sample
    norm = ||y - A(x0)||                   # A = the operator's forward (mask * fields with a mask)
    x = out.sample - scale * d norm / d x  # torch autograd through A, clamp, U

Here, with the same arithmetic per link:

    eps     = cfd_unet_forward_tape(x)                   (activations kept)
    sample  = cfd_sched_step(x, eps)                      (bit-exact DDPM/DDIM step)
    A       = cfd_siren_tape_forward(unnorm(x0))          (sensor points only)
    g_A     = cfd_dps_residual(y, A)                      (-(y - A) / ||y - A||)
    g_z     = cfd_siren_tape_vjp(g_A)
    d_eps, g_direct = cfd_dps_latent_grad(g_z)            (unnorm, clamp', c1 / c2 links)
    g_unet  = cfd_unet_input_vjp(d_eps)
    x       = cfd_dps_update(sample, g_direct, g_unet, scale)

Case4Operator without a mask runs exactly that.  Every other operator (case2,
case3, case3_gappy), and any operator with ``partial(cond_method.conditioning,
mask=mask)``, replaces the three SIREN / residual lines by one call,

    g_z, norm = cfd_siren_dense_grad(unnorm(x0), y, mask) (bounded workspace)

SensorStencilOperator ('sensor_stencil': linear stencils on the value and the exact
coordinate Jacobian at the sensors -- vorticity, divergence, wall shear) runs the
Case4 sequence on the Jacobian tape, readings (T, Ns, M):

    out, jac     = cfd_siren_jtape_forward(unnorm(x0))
    g_out, g_jac = cfd_dps_residual_linear(y, out, jac, weights)
    g_z          = cfd_siren_jtape_vjp(g_out, g_jac)

A ``mask`` keyword with it raises NotImplementedError (a zero weight row does that).

DenseStencilOperator ('dense_stencil': the same stencils at every point of a whole
field -- a measured vorticity field, divergence-free guidance at all collocation
points) takes the dense branch instead, readings (T, N, M) and masks of (N, M) tables:

    g_z, norm = cfd_siren_jdense_grad(unnorm(x0), y, weights, mask) (bounded workspace)

InpaintingOperator (A(x0) = mask * x0 on the latent image, measurements.py:40-56)
needs no decoder: the three SIREN lines and cfd_dps_latent_grad become

    d_eps, g_direct, norm = cfd_dps_latent_residual(x, eps, y, mask)

with ``mask`` (required) and the measurement broadcast to (1 | B, 1, T, L).

Batches: the reference loop only runs one sample per call (its ``if t != 0``
needs a one-element t; the notebook loops over samples).  Here a batch of B
samples is B independent DPS chains -- one residual norm per sample -- so a
batched call equals B single-sample calls, and samples shard over GPUs with no
collective.  The measurement is shared by all samples ((T, Ns, c)) or given
per sample ((B*T, Ns, c)).

Known rows (no reference counterpart): ``known=, known_mask=, known_noise=`` hold
latent rows to given values while the measurement guides the free ones.  Only the
last call of the step changes: cfd_dps_update becomes

    x       = cfd_dps_update_known(sample, g_direct, g_unet, scale, known, mask)

which forms cfd_dps_update's image and then replaces it, where the mask is set, by
the known rows at the noise level the step produces (q = a_i known + b_i n2, as
GaussianDiffusion's known-row loops; n2 Philox (seed, (1 << 41) + k) or
``known_noise``).  The gradient therefore acts on the free rows only.  'vanilla'
runs cfd_sched_step_known.  Without ``known`` every call is the one above.

RNG: as the unconditional sampler, Philox(seed, counter=step) by default, or the
reference's draws through ``step_noise`` (the p_sample ``randn_like`` of every
step; the unused q_sample draw of the noisy measurement is not needed).
"""
from __future__ import annotations

import ctypes as C
import functools

import torch

from .. import _lib
from ..gaussian_diffusion import (KNOWN_COUNTER, LossType, ModelMeanType, ModelVarType, STEP_DDIM, STEP_DDPM, _Known,
                                  broadcast_rows, check_model_range, fresh_seed, get_named_beta_schedule)
from ..respace import SpacedDiffusion, space_timesteps
from .condition_methods import Identity, PosteriorSampling
from .measurements import (_STENCIL_MASK, Case4Operator, DenseStencilOperator, InpaintingOperator,
                           SensorStencilOperator)

__SAMPLER__ = {}


def register_sampler(name: str):
    def wrapper(cls):
        if __SAMPLER__.get(name, None):
            raise NameError(f"Name {name} is already registered!")
        __SAMPLER__[name] = cls
        return cls
    return wrapper


def get_sampler(name: str):
    if __SAMPLER__.get(name, None) is None:
        raise NameError(f"Name {name} is not defined!")
    return __SAMPLER__[name]


_MEAN = {"epsilon": ModelMeanType.EPSILON}
_VAR = {"fixed_large": ModelVarType.FIXED_LARGE, "fixed_small": ModelVarType.FIXED_SMALL}


def create_sampler(sampler, steps, noise_schedule, model_mean_type, model_var_type, dynamic_threshold, clip_denoised,
                   rescale_timesteps, timestep_respacing=""):
    """gaussian_diffusion.py:30-52."""
    cls = get_sampler(name=sampler)
    if model_mean_type not in _MEAN:
        raise NotImplementedError(f"model_mean_type {model_mean_type!r} on the HIP path (CoNFiLD uses 'epsilon')")
    if model_var_type not in _VAR:
        raise NotImplementedError(f"model_var_type {model_var_type!r} on the HIP path")
    if dynamic_threshold:
        raise NotImplementedError("dynamic_threshold on the HIP path")
    if rescale_timesteps:
        raise NotImplementedError("rescale_timesteps=True on the HIP path")
    betas = get_named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    return cls(use_timesteps=space_timesteps(steps, timestep_respacing), betas=betas,
               model_mean_type=_MEAN[model_mean_type], model_var_type=_VAR[model_var_type],
               loss_type=LossType.MSE, rescale_timesteps=False, clip_denoised=clip_denoised)


_COND_KEYWORDS = ("mask",)


def _method_of(measurement_cond_fn):
    """(method, keywords) behind ``partial(cond_method.conditioning, **keywords)``: the
    keywords of the whole partial chain (an outer partial's win, as when called).
    ``mask`` is the one the operators take (measurements.py:92); any other raises."""
    fn = measurement_cond_fn
    kw = {}
    while isinstance(fn, functools.partial):
        for k, v in fn.keywords.items():
            kw.setdefault(k, v)
        fn = fn.func
    owner = getattr(fn, "__self__", None)
    if not isinstance(owner, (PosteriorSampling, Identity)):
        raise NotImplementedError("measurement_cond_fn must be partial(cond_method.conditioning) of a 'ps' or "
                                  "'vanilla' method from confild_amd.guided.condition_methods")
    for k in kw:
        if k not in _COND_KEYWORDS:
            raise NotImplementedError(f"keyword {k!r} of measurement_cond_fn is not supported on the HIP path "
                                      f"(supported: {', '.join(_COND_KEYWORDS)})")
    return owner, kw


def _mask_tables(mask, op, B, T, N, c, dev):
    """The mask keyword (and the operator's own mask) as 1, T or B*T tables of (N, c)
    on the device, or None.  Masks broadcastable to (T, N, c) or (B*T, N, c)."""
    own = op.default_mask() if hasattr(op, "default_mask") else None
    if mask is None and own is None:
        return None
    if mask is None:
        return own.to(device=dev, dtype=torch.float32).reshape(1, N, c).contiguous()
    m = torch.as_tensor(mask).to(device=dev, dtype=torch.float32)
    if own is not None:
        m = m * own.to(device=dev, dtype=torch.float32)
    if m.dim() > 3:
        raise ValueError(f"mask of shape {tuple(m.shape)} has more than 3 dimensions")
    lead = m.shape[0] if m.dim() == 3 else 1
    if lead not in (1, T, B * T):
        raise ValueError(f"mask of shape {tuple(m.shape)} broadcasts to neither ({T}, {N}, {c}) nor "
                         f"({B * T}, {N}, {c})")
    return torch.broadcast_to(m, (lead, N, c)).contiguous()


class _LatentMask:
    """An 'inpainting' run on the device: measurement and mask as (1 | B, n) tables with
    their batch strides, and the float64 partial sums cfd_dps_latent_residual needs."""

    def __init__(self, mask, measurement, x):
        if mask is None:
            raise ValueError("Require mask: the 'inpainting' operator needs partial(cond.conditioning, mask=mask)")
        B, tail = x.shape[0], tuple(x.shape[1:])
        self.mask, self.mstride = broadcast_rows(mask, B, tail, x.device, "mask")
        self.y, self.ystride = broadcast_rows(measurement, B, tail, x.device, "measurement")
        nbytes = C.c_size_t()
        _lib.check(_lib.lib().cfd_dps_latent_residual_workspace_bytes(x[0].numel(), B, C.byref(nbytes)),
                   "cfd_dps_latent_residual_workspace_bytes")
        self.ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.float64, device=x.device)


class _GuidedSampler(SpacedDiffusion):
    _kind = STEP_DDPM

    def __init__(self, use_timesteps, clip_denoised=True, **kwargs):
        super().__init__(use_timesteps, **kwargs)
        self.clip_denoised = clip_denoised
        self.distances = None   # (steps, B) residual norms of the last p_sample_loop (GPU)
        self.dense_budget = None  # workspace bytes the dense adjoint may plan for (None: the library default)

    def p_sample_loop(self, model, x_start, measurement, measurement_cond_fn, record=False, save_root=None, *,
                      step_noise=None, seed=None, sample_offset=0, progress=False, resample=None, known=None,
                      known_mask=None, known_noise=None):
        """gaussian_diffusion.py:169-206: guided reverse loop from x_start (B, 1, T, L).
        Per-step residual norms (the reference's progress-bar 'distance') are left in
        ``self.distances`` (steps, B) on the GPU.  ``known`` / ``known_mask`` (broadcast to
        (1 | B, 1, T, L)): rows held to known values inside every step, as
        GaussianDiffusion.p_sample_loop's; ``known_noise`` (steps, B, 1, T, L) replaces
        their Philox normals.  ``resample`` is refused: resampling jumps belong to
        known-row replacement (GaussianDiffusion.p_sample_loop)."""
        if resample is not None:
            raise ValueError("resampling jumps are not built for posterior sampling; use known-row replacement")
        if record:
            raise NotImplementedError("record=True (progress images) is not part of the HIP path")
        method, kw = _method_of(measurement_cond_fn)
        if x_start.device.type != "cuda":
            raise _lib.CfdError("the DPS sampler runs on the GPU only (no CPU fallback)")
        mask = self._device_mask(method, kw, x_start, measurement)
        kn = _Known.of(known, known_mask, known_noise, tuple(x_start.shape), x_start.device)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        x = x_start.detach().to(torch.float32).contiguous().clone()
        self.distances = torch.zeros(self.num_timesteps, x.shape[0], dtype=torch.float32, device=x.device)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for k, i in enumerate(indices):
            nz = None if step_noise is None else step_noise[k]
            nz2 = None if known_noise is None else known_noise[k]
            x = self._guided_step(model, x, i, measurement, method, nz, seed, k, sample_offset, self.distances[k],
                                  mask, kn, nz2)[0]
        check_model_range(model, x.device)
        return x

    def p_sample_step(self, model, x, index, measurement, measurement_cond_fn, noise=None, seed=None, counter=0,
                      sample_offset=0, *, known=None, known_mask=None, known_noise=None):
        """One guided reverse step at respaced index ``index`` (p_sample + conditioning,
        gaussian_diffusion.py:188-199).  Returns dict(sample, pred_xstart, x_t, distance):
        the conditioned image, x0_hat, the unconditioned DDPM/DDIM sample, the norms.
        Without ``noise`` and ``seed`` the step draws a fresh Philox key (fresh_seed).
        ``known`` / ``known_mask`` / ``known_noise`` (one tensor of x's shape): as the loop's;
        ``sample`` then carries the known rows, ``x_t`` stays the step's own sample."""
        method, kw = _method_of(measurement_cond_fn)
        seed = fresh_seed(noise, seed)
        x = x.detach().to(torch.float32).contiguous().clone()
        kn = _Known.of(known, known_mask, known_noise, tuple(x.shape), x.device)
        dist = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
        img, x0, sample = self._guided_step(model, x, index, measurement, method, noise, seed, counter,
                                            sample_offset, dist, self._device_mask(method, kw, x, measurement), kn,
                                            known_noise)
        return {"sample": img, "pred_xstart": x0, "x_t": sample, "distance": dist}

    @staticmethod
    def _device_mask(method, kw, x, measurement=None):
        """The mask tables of a 'ps' run on x's device (once per loop, not per step); for
        the 'inpainting' operator a _LatentMask (mask and measurement, shape-checked
        before the first launch)."""
        if not isinstance(method, PosteriorSampling):
            return None
        op = method.operator
        if isinstance(op, InpaintingOperator):
            if x.device.type != "cuda":
                raise _lib.CfdError("the DPS sampler runs on the GPU only (no CPU fallback)")
            if x.dim() != 4 or x.shape[1] != 1:
                raise ValueError(f"latents must be (B, 1, T, L), got {tuple(x.shape)}")
            return _LatentMask(kw.get("mask"), measurement, x)
        if isinstance(op, SensorStencilOperator):
            if kw.get("mask") is not None:
                raise NotImplementedError(_STENCIL_MASK)
            return None
        # tables of (N, c) values, or of (N, M) readings for 'dense_stencil'
        width = op.readings if isinstance(op, DenseStencilOperator) else op.model.out_features
        return _mask_tables(kw.get("mask"), op, x.shape[0], x.shape[2], op.coords.shape[0], width, x.device)

    def _update(self, sample, g_dir, g_unet, scale, t, seed, counter, offset, kn, nz2):
        """The step's last call: cfd_dps_update, or with known rows (``kn`` a _Known)
        cfd_dps_update_known, which also puts them back at the level the step produces."""
        lib = _lib.lib()
        st = _lib.stream_of(sample.device)
        img = torch.empty_like(sample)
        if kn is None:
            _lib.check(lib.cfd_dps_update(_lib.ptr(sample), _lib.ptr(g_dir), _lib.ptr(g_unet), scale, _lib.ptr(img),
                                          sample.numel(), st), "cfd_dps_update")
            return img
        _lib.check(lib.cfd_dps_update_known(_lib.ptr(sample), _lib.ptr(g_dir), _lib.ptr(g_unet), scale,
                                            _lib.ptr(img), _lib.ptr(t), sample[0].numel(), sample.shape[0],
                                            _lib.ptr(kn.known), kn.kstride, _lib.ptr(kn.mask), kn.mstride,
                                            _lib.ptr(self._ktab(sample.device)), _lib.ptr(nz2), seed,
                                            KNOWN_COUNTER + counter, offset, st), "cfd_dps_update_known")
        return img

    def _guided_step(self, model, x, i, measurement, method, noise, seed, counter, sample_offset, dist_out,
                     mask=None, kn=None, known_noise=None):
        """x (B, 1, T, L) contiguous fp32 on the GPU; updated in place for 'ps'.
        mask: None or the (1 | T | B*T, N, c) device tables of _mask_tables ((N, M) for 'dense_stencil').
        kn: None or the _Known rows; known_noise: their normals (x's shape) or None."""
        dev = x.device
        if dev.type != "cuda":
            raise _lib.CfdError("the DPS sampler runs on the GPU only (no CPU fallback)")
        lib = _lib.lib()
        st = _lib.stream_of(dev)
        B = x.shape[0]
        n = x[0].numel()
        offset = sample_offset * n
        if offset % 4:
            raise ValueError("sharded sampling needs (elements per sample * first sample) % 4 == 0")
        sched = self._sched(dev, 0.0)
        t = torch.full((B,), i, dtype=torch.int64, device=dev)
        tm = self._map_timesteps(t)
        nz = None if noise is None else noise.to(device=dev, dtype=torch.float32).contiguous()
        nz2 = None
        if kn is not None and known_noise is not None:
            nz2 = known_noise.to(device=dev, dtype=torch.float32).contiguous()
            if nz2.shape != x.shape:
                raise ValueError("known_noise must have the shape of x")
        dps = isinstance(method, PosteriorSampling)
        clip = 1 if self.clip_denoised else 0
        eps = (model.forward_tape(x, tm) if dps else model(x, tm)).contiguous()
        sample = torch.empty_like(x)
        x0 = torch.empty_like(x)
        if kn is not None and not dps:
            # 'vanilla': the unconditioned loops' known-row step
            _lib.check(lib.cfd_sched_step_known(sched.handle, self._kind, clip, _lib.ptr(x), _lib.ptr(eps),
                                                _lib.ptr(t), _lib.ptr(nz), seed, counter, offset, _lib.ptr(sample),
                                                _lib.ptr(x0), n, B, _lib.ptr(kn.known), kn.kstride,
                                                _lib.ptr(kn.mask), kn.mstride, _lib.ptr(self._ktab(dev)),
                                                _lib.ptr(nz2), KNOWN_COUNTER + counter, st), "cfd_sched_step_known")
            return sample, x0, sample
        _lib.check(lib.cfd_sched_step(sched.handle, self._kind, clip, _lib.ptr(x), _lib.ptr(eps), _lib.ptr(t),
                                      _lib.ptr(nz), seed, counter, offset, _lib.ptr(sample), _lib.ptr(x0), n, B, st),
                   "cfd_sched_step")
        if not dps:
            return sample, x0, sample
        op = method.operator
        if isinstance(mask, _LatentMask):
            d_eps = torch.empty_like(x)
            g_dir = torch.empty_like(x)
            _lib.check(lib.cfd_dps_latent_residual(sched.handle, clip, _lib.ptr(x), _lib.ptr(eps), _lib.ptr(t),
                                                   _lib.ptr(mask.y), mask.ystride, _lib.ptr(mask.mask), mask.mstride,
                                                   _lib.ptr(dist_out), _lib.ptr(d_eps), _lib.ptr(g_dir), n, B,
                                                   _lib.ptr(mask.ws), mask.ws.numel() * 8, st),
                       "cfd_dps_latent_residual")
            g_unet = model.input_vjp(d_eps)
            img = self._update(sample, g_dir, g_unet, float(method.scale), t, seed, counter, offset, kn, nz2)
            return img, x0, sample
        # a 'dense_stencil' measurement may be None: a zero target (e.g. zero divergence)
        dense_zero = measurement is None and isinstance(op, DenseStencilOperator)
        y = None if dense_zero else measurement.to(device=dev, dtype=torch.float32).contiguous()
        vmax, vmin = op._bounds()
        if n % vmax.numel():
            raise ValueError("latent max/min do not tile the latent")
        if isinstance(op, Case4Operator) and mask is None:
            A = op.forward_tape(x0)                                      # (B*T, Ns, c)
            per = A.numel() // B
            if y.numel() not in (per, A.numel()):
                raise ValueError(f"measurement of {y.numel()} values matches neither one sample ({per}) "
                                 f"nor the batch ({A.numel()})")
            gA = torch.empty_like(A)
            _lib.check(lib.cfd_dps_residual(_lib.ptr(y), 0 if y.numel() == per else per, _lib.ptr(A), _lib.ptr(gA),
                                            _lib.ptr(dist_out), per, B, st), "cfd_dps_residual")
            gz = op.vjp(gA)                                              # (B*T, L)
        elif isinstance(op, SensorStencilOperator):
            # value and derivative sensors: the Jacobian tape and its adjoint (K15)
            out, jac = op.forward_tape(x0)                               # (B*T, Ns, c), (B*T, Ns, c, d)
            _, g_out, g_jac, _ = op.residual(out, jac, y, B, dist_out)
            gz = op.vjp(g_out, g_jac)                                    # (B*T, L)
        else:
            # a dense or masked measurement (values: K12; 'dense_stencil' readings: K16):
            # norm and latent gradient in bounded memory
            gz, norms = op.dense_grad(x0, y, mask, self.dense_budget)
            dist_out.copy_(norms)
        d_eps = torch.empty_like(x)
        g_dir = torch.empty_like(x)
        _lib.check(lib.cfd_dps_latent_grad(sched.handle, clip, _lib.ptr(x), _lib.ptr(eps), _lib.ptr(t), _lib.ptr(gz),
                                           _lib.ptr(vmax), _lib.ptr(vmin), vmax.numel(), _lib.ptr(d_eps),
                                           _lib.ptr(g_dir), n, B, st), "cfd_dps_latent_grad")
        g_unet = model.input_vjp(d_eps)
        img = self._update(sample, g_dir, g_unet, float(method.scale), t, seed, counter, offset, kn, nz2)
        return img, x0, sample


@register_sampler(name="ddpm")
class DDPM(_GuidedSampler):
    _kind = STEP_DDPM


@register_sampler(name="ddim")
class DDIM(_GuidedSampler):
    """DDIM.p_sample with eta = 0 (gaussian_diffusion.py:375-403)."""
    _kind = STEP_DDIM
