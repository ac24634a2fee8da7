"""Latent sequences longer than the U-Net's ``time_length``: overlapping windows.

A latent is an image (B, 1, T, L) whose rows are snapshots.  A rollout chains
windows of T rows: window w >= 1 is sampled conditioned on its first ``overlap``
rows, which are the last ``overlap`` rows of the sequence so far, and contributes
its remaining T - overlap rows.  Three ways to condition (no reference
counterpart for the driver; 'ps' + 'inpainting' is the reference's operator):

  replace  known-row replacement inside the unconditioned loop
           (GaussianDiffusion.p_sample_loop(known=, known_mask=), the native
           graph loop included): one fused elementwise pass per step;
           ``resample=(jump_length, jump_n_sample)`` adds RePaint's resampling
           jumps, which re-denoise free and known rows together (more steps
           per window, the same cost per step);
  ps       posterior sampling with the 'inpainting' operator
           (guided sampler): a U-Net forward and an input VJP per step;
  guided   posterior sampling on a sensor record longer than one window: every
           window, window 0 included, runs the guided loop ('ps' on a SIREN
           operator) on its own rows of the record, and windows w >= 1 also hold
           their overlap rows to the sequence so far (the guided sampler's
           ``known=, known_mask=``; cfd_dps_update_known): the 'ps' step's cost,
           one elementwise launch exchanged for another.

Window w draws from Philox key ``seed + w``; samples shard over ranks through
``sample_offset`` exactly as the unconditioned loops do (dist.sharded_samples).
"""
from __future__ import annotations

import functools

import torch

from . import _lib
from .gaussian_diffusion import STEP_DDIM, GaussianDiffusion

METHODS = ("replace", "ps", "guided")


def plan_windows(T, overlap, n_windows):
    """Row slices of every window in the stitched sequence (host only): window 0 is
    slice(0, T); window w >= 1 starts ``overlap`` rows before the end of window
    w - 1.  The sequence has T + n_windows * (T - overlap) rows."""
    T, overlap, n_windows = int(T), int(overlap), int(n_windows)
    if T < 1 or not 1 <= overlap < T:
        raise ValueError(f"overlap must satisfy 1 <= overlap < T, got overlap {overlap}, T {T}")
    if n_windows < 0:
        raise ValueError(f"n_windows must be >= 0, got {n_windows}")
    stride = T - overlap
    return [slice(w * stride, w * stride + T) for w in range(n_windows + 1)]


def window_noise(shape, seed, sample_offset, device):
    """x_T of one window, as the unconditioned loops draw it: Philox (seed, 1 << 40)
    at the shard's stream position."""
    img = torch.empty(*shape, dtype=torch.float32, device=device)
    offset = sample_offset * img[0].numel()
    if offset % 4:
        raise ValueError("sharded sampling needs (elements per sample * first sample) % 4 == 0")
    _lib.check(_lib.lib().cfd_randn(_lib.ptr(img), img.numel(), seed, 1 << 40, offset, _lib.stream_of(device)),
               "cfd_randn")
    return img


def known_rows(prev, overlap):
    """(known, mask) of the window that follows ``prev`` (B, 1, T, L): its rows
    [0, overlap) are the last ``overlap`` rows of prev, the mask (1, 1, T, L) is 1 there."""
    T = prev.shape[2]
    known = torch.zeros_like(prev)
    known[:, :, :overlap] = prev[:, :, T - overlap:]
    mask = torch.zeros(1, 1, T, prev.shape[3], dtype=torch.float32, device=prev.device)
    mask[:, :, :overlap] = 1.0
    return known, mask


def window_measurement(measurement, mask, sl, B, T_total):
    """(measurement, mask) of the window on rows ``sl`` (a slice of plan_windows) of a
    record of ``T_total`` rows (host only; any device).  ``measurement`` is
    (T_total, Ns, c), shared by the B samples, or (B, T_total, Ns, c), one record per
    sample; the window's is (T, Ns, c) or (B * T, Ns, c), as the guided loop takes it.
    ``mask`` (the ``mask`` keyword of the conditioning): None or an (Ns, c) table pass
    through; (T_total, Ns, c) or (B, T_total, Ns, c) are sliced like the measurement."""
    B, T_total = int(B), int(T_total)
    y = torch.as_tensor(measurement)
    if y.dim() == 3 and y.shape[0] == T_total:
        y_w = y[sl]
    elif y.dim() == 4 and tuple(y.shape[:2]) == (B, T_total):
        y_w = y[:, sl].reshape((-1,) + tuple(y.shape[2:]))
    else:
        raise ValueError(f"measurement of shape {tuple(y.shape)} is neither ({T_total}, Ns, c) nor "
                         f"({B}, {T_total}, Ns, c)")
    if mask is None:
        return y_w, None
    m = torch.as_tensor(mask)
    if m.dim() == 2:
        return y_w, m
    if m.dim() == 3 and m.shape[0] == T_total:
        return y_w, m[sl]
    if m.dim() == 4 and tuple(m.shape[:2]) == (B, T_total):
        return y_w, m[:, sl].reshape((-1,) + tuple(m.shape[2:]))
    raise ValueError(f"mask of shape {tuple(m.shape)} is none of (Ns, c), ({T_total}, Ns, c), "
                     f"({B}, {T_total}, Ns, c)")


def _guided_method(diffusion, cond_fn, measurement):
    """The 'ps' method and conditioning keywords behind ``cond_fn`` of a 'guided' rollout."""
    from .guided.condition_methods import PosteriorSampling
    from .guided.gaussian_diffusion import _GuidedSampler, _method_of
    from .guided.measurements import InpaintingOperator
    if not isinstance(diffusion, _GuidedSampler):
        raise TypeError("method 'guided' takes a guided sampler from "
                        "confild_amd.guided.gaussian_diffusion.create_sampler")
    if cond_fn is None or measurement is None:
        raise TypeError("method 'guided' needs cond_fn=partial(cond_method.conditioning[, mask=...]) and measurement=")
    method, kw = _method_of(cond_fn)
    if not isinstance(method, PosteriorSampling) or isinstance(method.operator, InpaintingOperator):
        raise TypeError("method 'guided' conditions with a 'ps' method on a SIREN operator (case2 / case3 / case4)")
    return method, kw


def _ps_method(device, scale):
    from .guided.condition_methods import get_conditioning_method
    from .guided.measurements import get_noise, get_operator
    return get_conditioning_method("ps", get_operator("inpainting", device=device),
                                   get_noise("gaussian", sigma=0.0), scale=scale)


def sample_window(model, diffusion, shape, method, *, known=None, mask=None, scale=1.0, seed, sample_offset=0,
                  sampler="ddpm", device=None, resample=None, cond_fn=None, measurement=None):
    """One window (B, 1, T, L): unconditioned when ``known`` is None, else conditioned on
    ``known`` where ``mask`` is 1.  ``sampler`` picks the DDPM / DDIM loop for
    'replace'; a guided sampler ('ps', 'guided') carries its own kind.  ``resample``
    (jump_length, jump_n_sample): resampling jumps of a conditioned 'replace' window;
    an unconditioned window has nothing to harmonise and ignores it.  'guided':
    ``cond_fn`` (partial(cond_method.conditioning[, mask=...]) of a 'ps' method on a SIREN
    operator, with the window's mask) and ``measurement`` (the window's (T | B*T, Ns, c))
    guide every row; ``known`` / ``mask`` then hold rows on top of that."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if resample is not None and method != "replace":
        raise ValueError("resample goes with method 'replace'; posterior sampling ('ps', 'guided') has no "
                         "resampling jumps")
    if method == "guided":
        _guided_method(diffusion, cond_fn, measurement)
        if device is None:
            device = next(model.parameters()).device
        x_T = window_noise(shape, seed, sample_offset, device)
        return diffusion.p_sample_loop(model=model, x_start=x_T, measurement=measurement,
                                       measurement_cond_fn=cond_fn, seed=seed, sample_offset=sample_offset,
                                       known=known, known_mask=mask)
    if method == "replace":
        if sampler not in ("ddpm", "ddim"):
            raise ValueError(f"sampler must be 'ddpm' or 'ddim', got {sampler!r}")
        fn = diffusion.p_sample_loop if sampler == "ddpm" else diffusion.ddim_sample_loop
        return fn(model, tuple(shape), device=device, seed=seed, sample_offset=sample_offset, known=known,
                  known_mask=mask, resample=None if known is None else resample)
    from .guided.gaussian_diffusion import _GuidedSampler
    if not isinstance(diffusion, _GuidedSampler):
        raise TypeError("method 'ps' takes a guided sampler from confild_amd.guided.gaussian_diffusion.create_sampler")
    if device is None:
        device = next(model.parameters()).device
    if known is None:
        # window 0: the guided sampler's own schedule and step kind, no measurement
        fn = GaussianDiffusion.ddim_sample_loop if diffusion._kind == STEP_DDIM else GaussianDiffusion.p_sample_loop
        return fn(diffusion, model, tuple(shape), clip_denoised=diffusion.clip_denoised, device=device, seed=seed,
                  sample_offset=sample_offset)
    cond = _ps_method(device, scale)
    x_T = window_noise(shape, seed, sample_offset, device)
    return diffusion.p_sample_loop(model=model, x_start=x_T, measurement=mask * known,
                                   measurement_cond_fn=functools.partial(cond.conditioning, mask=mask), seed=seed,
                                   sample_offset=sample_offset)


def extend_latents(model, diffusion, first, n_windows, overlap, method, *, scale=1.0, seed, sample_offset=0,
                   sampler="ddpm", batch_size=1, resample=None, cond_fn=None, measurement=None):
    """(B, 1, T + n_windows * (T - overlap), L): ``first`` (B, 1, T, L) continued by
    ``n_windows`` conditioned windows.  ``first=None`` samples window 0 unconditionally:
    ``batch_size`` samples of the model's (1, image_size, image_size) input.

    The stitched sequence keeps the earlier window's values on each overlap and
    appends the later window's rows [overlap, T).  method 'replace' takes a
    GaussianDiffusion, 'ps' a guided sampler (create_sampler) and ``scale``.
    Window w uses Philox key seed + w.  ``resample`` (jump_length, jump_n_sample):
    resampling jumps in every conditioned window ('replace' only).

    'guided' takes a guided sampler, ``cond_fn`` (partial(cond_method.conditioning[,
    mask=...]) of a 'ps' method on a SIREN operator; its scale is the method's) and
    ``measurement``, the whole record: (T_total, Ns, c) shared by the samples or
    (B, T_total, Ns, c) per sample (B: this call's samples), T_total = T + n_windows *
    (T - overlap).  Window w runs the guided loop on the record's rows
    plan_windows(...)[w] (window_measurement; a mask with a row dimension is sliced
    likewise) -- window 0 too, from ``first=None`` -- and windows w >= 1 also hold their
    overlap rows to the sequence so far."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if resample is not None and method != "replace":
        raise ValueError("resample goes with method 'replace'; posterior sampling ('ps', 'guided') has no "
                         "resampling jumps")
    guided = method == "guided"
    if guided:
        cond, cond_kw = _guided_method(diffusion, cond_fn, measurement)
    if torch.is_tensor(first):
        if first.dim() != 4 or first.shape[1] != 1:
            raise ValueError(f"first must be (B, 1, T, L), got {tuple(first.shape)}")
        seq = first.detach().to(torch.float32).contiguous()
        device = seq.device
        shape = tuple(seq.shape)
    else:
        if first is not None:
            raise TypeError("first must be a (B, 1, T, L) tensor or None")
        device = next(model.parameters()).device
        shape = (int(batch_size), 1, model.image_size, model.image_size)
        seq = None
    T = shape[2]
    windows = plan_windows(T, overlap, n_windows)   # argument checks
    seed = int(seed)

    def guide(w):
        """The window's measurement and conditioning (its rows of the record and of the mask)."""
        if not guided:
            return {}
        y_w, m_w = window_measurement(measurement, cond_kw.get("mask"), windows[w], shape[0], windows[-1].stop)
        fn = functools.partial(cond.conditioning) if m_w is None else functools.partial(cond.conditioning, mask=m_w)
        return {"cond_fn": fn, "measurement": y_w}

    if guided:
        guide(0)   # the record's and the mask's shapes, before any launch
    if seq is None:
        seq = sample_window(model, diffusion, shape, method, seed=seed, sample_offset=sample_offset, sampler=sampler,
                            device=device, **guide(0))
    for w in range(1, n_windows + 1):
        known, mask = known_rows(seq[:, :, -T:], overlap)
        win = sample_window(model, diffusion, shape, method, known=known, mask=mask, scale=scale, seed=seed + w,
                            sample_offset=sample_offset, sampler=sampler, device=device, resample=resample,
                            **guide(w))
        seq = torch.cat([seq, win[:, :, overlap:]], dim=2)
    return seq
