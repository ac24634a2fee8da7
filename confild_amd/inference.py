"""Drop-in for UnconditionalDiffusionTraining_and_Generation/scripts/inference.py.

    python -m confild_amd.inference case.yml                      # 1 GPU
    torchrun --nproc-per-node 8 -m confild_amd.inference case.yml # 8 GPUs

Same YAML keys as the reference (training_recipes/*.yml).  Optional keys, with
reference-preserving defaults:
  timestep_respacing: ""      (reference: full `steps`)
  sampler: ddpm | ddim        (reference: ddpm, p_sample_loop)
  coords_path: null           (reference: the CNF trainer's training points)
  seed: 42                    (reference: torch.manual_seed(42), inference.py:17)
  precision: fp32 | bf16      (reference: fp32.  fp32 runs the U-Net convolutions as
                               split-f16, fp32-level error; bf16 = config E, bf16
                               operands with fp32 accumulation, GroupNorm/softmax fp32)
  compute: split_f16 | fp32 | bf16   (explicit U-Net compute mode; overrides precision)
  rollout_windows: 0          (reference: one window of time_length rows.  W > 0 continues
                               every sample by W conditioned windows, confild_amd.rollout:
                               T_total = T + W * (T - rollout_overlap) rows, saved as
                               (B*T_total, N, c))
  rollout_overlap: T // 2     (rows a window shares with the sequence before it)
  rollout_method: replace | ps | guided   (replace: known-row replacement in the native loop;
                               ps: posterior sampling with the 'inpainting' operator;
                               guided: every window, window 0 included, is posterior sampling
                               on its rows of a sensor record, and windows w >= 1 also hold
                               their overlap rows to the sequence so far.  rollout_windows: 0
                               then runs one guided window)
  rollout_scale: 1.0          (the 'ps' / 'guided' step size)
  rollout_sensor_coords:      ('guided', required: npy (Ns, d), the sensors' physical coordinates)
  rollout_measurement:        ('guided', required: npy (T_total, Ns, c), the record in physical
                               values, shared by the samples: the B samples are B posterior
                               draws.  Any other row count is a ValueError before sampling)
  rollout_sensor_mask: null   ('guided': npy (Ns, c) or (T_total, Ns, c), 1 where a value was measured)
                               The operator is Case4Operator.from_parts on the driver's own CNF
                               (network, x / y normalisers) and max_val / min_val.
  rollout_jump_length: 10     (RePaint resampling in the conditioned 'replace' windows: after every
  rollout_jump_n_sample: 1     jump_length levels the state is noised back up by jump_length levels
                               and re-denoised, jump_n_sample times in all, which harmonises free and
                               known rows at (jump_n_sample - 1) more steps per level.  1: off)
  derived: []                 (a subset of jacobian | vorticity | divergence | q_criterion: exact spatial
                               derivatives of the decoded fields at the query points, from the fused
                               value-and-Jacobian decode (trainer.infer_jacobian, confild_amd.derived).
                               Each is saved beside save_path as <stem>_<name>.npy with the fields'
                               leading shape: jacobian (..., c, d), vorticity (...) in 2-D or (..., 3),
                               divergence and q_criterion (...).  The fields and out.npy do not change.
                               Also hessian | laplacian | grad_divergence: exact second derivatives from
                               the fused value-Jacobian-Hessian decode (trainer.infer_hessian), one more
                               launch per chunk, which leaves the files above as they are: hessian
                               (..., c, d, d), laplacian (..., c), grad_divergence (..., d).  laplacian
                               alone runs the diagonal form)
                               Also the PDE residuals of confild_amd.derived, from the launches above and
                               the chunk's saved fields: convective_acceleration (..., d), (u . grad) u
                               from the Jacobian launch; momentum_residual (..., d), the steady form
                               u . grad u + grad p / rho - nu lap u from the Hessian launch's Jacobian and
                               Hessian (no time derivative: dudt is not a driver feature);
                               pressure_poisson_residual (...), lap p + rho d_i u_k d_k u_i from the
                               Hessian launch.  The two residuals need the Laplacian only: with no hessian
                               or grad_divergence beside them the diagonal form runs)
  derived_compute: f32        (f32 | split_f16: the arithmetic of the Jacobian launch behind jacobian |
                               vorticity | divergence | q_criterion.  f32: the exact fp32 MFMA chain;
                               split_f16: the same chain on the f16 matrix pipes with fp32-level
                               accuracy (decode_jacobian(compute="split_f16")), for CNF widths
                               hidden_features 32*{1,2,3,4,6,8,12}, num_hidden_layers >= 1, dims <= 3 --
                               any other value or width is a ValueError before sampling starts.  The
                               fields and the Hessian names do not depend on it)
  derived_hessian_compute: f32 (f32 | split_f16: the arithmetic of the Hessian launch behind hessian |
                               laplacian | grad_divergence | momentum_residual | pressure_poisson_residual.
                               split_f16 is decode_hessian(compute="split_f16"), with derived_compute's
                               widths and the same ValueError before sampling starts.  derived_compute
                               stays the Jacobian launch's alone)
  derived_velocity_channels:  (which d output channels are the velocity, default the first d)
  derived_nu:                 (float, the kinematic viscosity: required with momentum_residual)
  derived_rho: 1.0            (float, the density of the two residuals)
  derived_pressure_channel: null   (int, the output channel that is the pressure: required with
                               pressure_poisson_residual; null drops the pressure term of momentum_residual.
                               It must not be one of the velocity channels)
Known deviation (fixed on purpose): ``channel_mult`` from the YAML IS passed to
create_model (the reference reads but drops it, inference.py:38-44, so its own
case4.yml raises ValueError).

Flow (inference.py:20-81; with rollout_method: guided the CNF is loaded first,
nothing else moves): sample (B, 1, T, L) latents on the GPU(s) ->
de-normalise with max_val/min_val -> CNF decode of every latent row over the
query points (one fused launch per chunk) -> np.save((B*T, N, c)) on rank 0.
Multi-GPU: samples are sharded over ranks (dist.sharded_samples) with the
unsharded Philox stream, weights are broadcast from rank 0 once, decoded
fields are gathered to rank 0.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from . import _lib, dist
from .read_input import basic_input
from .script_util import create_gaussian_diffusion, create_model
from .trainer import trainer


def latent_denorm(gen: torch.Tensor, vmax: torch.Tensor, vmin: torch.Tensor) -> torch.Tensor:
    """(gen + 1) * (max - min) / 2 + min on the GPU (cfd_latent_denorm); max/min are
    scalars or broadcast over gen's trailing dimensions."""
    period = vmax.numel()
    if vmin.numel() != period or gen.numel() % period or (period > 1 and
                                                          tuple(gen.shape[-vmax.dim():]) != tuple(vmax.shape)):
        raise ValueError(f"max/min of shape {tuple(vmax.shape)} do not broadcast over the latents' trailing dims")
    out = torch.empty_like(gen)
    _lib.check(_lib.lib().cfd_latent_denorm(_lib.ptr(gen), _lib.ptr(out), gen.numel(), _lib.ptr(vmax),
                                            _lib.ptr(vmin), period, _lib.stream_of(gen.device)), "latent_denorm")
    return out


PRECISIONS = {"fp32": "split_f16", "float32": "split_f16", "bf16": "bf16", "bfloat16": "bf16"}


def unet_compute(inp) -> str:
    """U-Net compute mode from the optional ``compute`` / ``precision`` YAML keys."""
    explicit = getattr(inp, "compute", None)
    if explicit is not None:
        return str(explicit)
    prec = str(getattr(inp, "precision", "fp32")).lower()
    if prec not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {prec!r}")
    return PRECISIONS[prec]


def rollout_sampler(inp, diff, sampler):
    """(diffusion, method) of a rollout run: ``diff`` for 'replace', for 'ps' and 'guided' a
    guided sampler on the same schedule (fixed-large variance, clipped x0, as ``diff`` runs)."""
    method = str(getattr(inp, "rollout_method", "replace"))
    if method == "replace":
        return diff, method
    if method not in ("ps", "guided"):
        raise ValueError(f"rollout_method must be 'replace', 'ps' or 'guided', got {method!r}")
    from .guided.gaussian_diffusion import create_sampler
    return create_sampler(sampler=sampler, steps=inp.steps, noise_schedule=inp.noise_schedule,
                          model_mean_type="epsilon", model_var_type="fixed_large", dynamic_threshold=False,
                          clip_denoised=True, rescale_timesteps=False,
                          timestep_respacing=getattr(inp, "timestep_respacing", "")), method


RESIDUAL_DERIVED = ("momentum_residual", "pressure_poisson_residual")   # the Laplacian is all they need
# from infer_hessian, the rest from infer_jacobian
HESSIAN_DERIVED = ("hessian", "laplacian", "grad_divergence") + RESIDUAL_DERIVED
DERIVED = ("jacobian", "vorticity", "divergence", "q_criterion", "convective_acceleration") + HESSIAN_DERIVED


def derived_names(inp):
    """The ``derived`` YAML key as a list of names (empty: today's run)."""
    names = getattr(inp, "derived", None) or []
    if isinstance(names, str):
        names = [names]
    names = [str(n) for n in names]
    bad = [n for n in names if n not in DERIVED]
    if bad or len(set(names)) != len(names):
        raise ValueError(f"derived must be distinct names out of {list(DERIVED)}, got {names}")
    return names


def derived_compute(inp):
    """The ``derived_compute`` YAML key: "f32" (default) or "split_f16".  split_f16 is
    checked here against the widths in the CNF case file (no model is loaded), so a
    run the kernel would refuse stops before sampling."""
    from .nf_networks import JACOBIAN_COMPUTE, jacobian_split_refusal
    mode = str(getattr(inp, "derived_compute", None) or "f32")
    if mode not in JACOBIAN_COMPUTE:
        raise ValueError(f"derived_compute must be one of {list(JACOBIAN_COMPUTE)}, got {mode!r}")
    if mode == "split_f16":
        cnf = basic_input(inp.cnf_case_file_path)
        why = jacobian_split_refusal(int(cnf.dims), int(cnf.NF["num_hidden_layers"]), int(cnf.NF["hidden_features"]))
        if why:
            raise ValueError(f"derived_compute: split_f16 does not take this CNF: {why}")
    return mode


def derived_hessian_compute(inp):
    """The ``derived_hessian_compute`` YAML key: "f32" (default) or "split_f16", the
    arithmetic of the Hessian launch, checked against the CNF case file as
    derived_compute() checks the Jacobian launch's."""
    from .nf_networks import HESSIAN_COMPUTE, hessian_split_refusal
    mode = str(getattr(inp, "derived_hessian_compute", None) or "f32")
    if mode not in HESSIAN_COMPUTE:
        raise ValueError(f"derived_hessian_compute must be one of {list(HESSIAN_COMPUTE)}, got {mode!r}")
    if mode == "split_f16":
        cnf = basic_input(inp.cnf_case_file_path)
        why = hessian_split_refusal(int(cnf.dims), int(cnf.NF["num_hidden_layers"]), int(cnf.NF["hidden_features"]))
        if why:
            raise ValueError(f"derived_hessian_compute: split_f16 does not take this CNF: {why}")
    return mode


def derived_physics(inp, names=None):
    """{nu, rho, pressure_channel} of the residual names, from ``derived_nu``,
    ``derived_rho`` and ``derived_pressure_channel``, checked against ``names`` (default:
    the ``derived`` key) and the CNF case file's out_features (no model is loaded)."""
    names = derived_names(inp) if names is None else names
    nu, rho, pch = (getattr(inp, k, None) for k in ("derived_nu", "derived_rho", "derived_pressure_channel"))

    def number(key, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise ValueError(f"{key} must be a finite number, got {v!r}")
        return float(v)
    nu = None if nu is None else number("derived_nu", nu)
    rho = 1.0 if rho is None else number("derived_rho", rho)
    if rho == 0.0:
        raise ValueError("derived_rho must not be 0")
    if "momentum_residual" in names and nu is None:
        raise ValueError("derived: momentum_residual needs derived_nu")
    if "pressure_poisson_residual" in names and pch is None:
        raise ValueError("derived: pressure_poisson_residual needs derived_pressure_channel")
    if pch is not None:
        if isinstance(pch, bool) or not isinstance(pch, int):
            raise ValueError(f"derived_pressure_channel must be an integer or null, got {pch!r}")
        c = int(basic_input(inp.cnf_case_file_path).NF["out_features"])
        if pch < 0 or pch >= c:
            raise ValueError(f"derived_pressure_channel {pch} out of range for {c} components")
        # the pressure is not a velocity component: derived_velocity_channels, or the first d
        vch = getattr(inp, "derived_velocity_channels", None)
        vch = list(range(int(basic_input(inp.cnf_case_file_path).dims))) if vch is None else [int(v) for v in vch]
        if pch in vch:
            raise ValueError(f"derived_pressure_channel {pch} is one of the velocity channels {vch}")
    return {"nu": nu, "rho": rho, "pressure_channel": pch}


def derived_quantity(name, jac, velocity_channels=None, hess=None, diag=False, fields=None, physics=None):
    """One ``derived`` quantity of a Jacobian (..., c, d) or, for HESSIAN_DERIVED, of a
    Hessian (..., c, d, d) (``diag``: its diagonal form (..., c, d), enough for laplacian
    and the residuals).  convective_acceleration and momentum_residual also read the
    ``fields`` (..., c); the residuals take ``physics`` (derived_physics())."""
    from . import derived
    if name == "convective_acceleration":
        return derived.convective_acceleration(fields, jac, velocity_channels)
    if name == "momentum_residual":
        return derived.momentum_residual(fields, jac, hess, physics["nu"], physics["pressure_channel"],
                                         physics["rho"], velocity_channels=velocity_channels)
    if name == "pressure_poisson_residual":
        return derived.pressure_poisson_residual(jac, hess, physics["pressure_channel"], physics["rho"],
                                                 velocity_channels)
    if name == "jacobian":
        return jac
    if name == "hessian":
        return hess
    if name == "laplacian":
        return derived.laplacian(hess, diag=diag)
    if name == "grad_divergence":
        return derived.grad_divergence(hess, velocity_channels)
    return getattr(derived, name)(jac, velocity_channels)


def load_cnf(inp, device):
    """The CNF decoder of the run on ``device`` (trainer: network and normalisers)."""
    cnf = trainer(basic_input(inp.cnf_case_file_path), infer_mode=getattr(inp, "coords_path", None) is not None)
    cnf.load(-1, siren_only=True)
    cnf.nf.to(device)
    return cnf


def guided_rollout(inp, cnf, device, T, windows, overlap):
    """{cond_fn, measurement} of ``rollout_method: guided``: a 'ps' method on a Case4Operator
    built in memory from the driver's CNF and latent bounds, and the sensor record on
    ``device``.  Shapes are checked here, before any sampling launch."""
    from functools import partial

    from .guided.condition_methods import get_conditioning_method
    from .guided.measurements import Case4Operator, get_noise
    from .rollout import plan_windows
    for key in ("rollout_sensor_coords", "rollout_measurement"):
        if getattr(inp, key, None) is None:
            raise ValueError(f"rollout_method: guided needs {key}")
    coords = np.load(inp.rollout_sensor_coords)
    y = np.load(inp.rollout_measurement)
    total = plan_windows(T, overlap, windows)[-1].stop
    c = cnf.nf.out_features
    if coords.ndim != 2 or y.shape != (total, coords.shape[0], c):
        raise ValueError(f"rollout_measurement of shape {tuple(y.shape)} with rollout_sensor_coords of shape "
                         f"{tuple(coords.shape)}: the record must be ({total}, Ns, {c}), T_total = {T} + "
                         f"{windows} * ({T} - {overlap}) rows")
    op = Case4Operator.from_parts(device, coords, cnf.in_normalizer, cnf.out_normalizer, cnf.nf, np.load(inp.max_val),
                                  np.load(inp.min_val))
    cond = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.0),
                                   scale=float(getattr(inp, "rollout_scale", 1.0)))
    fn = partial(cond.conditioning)
    if getattr(inp, "rollout_sensor_mask", None) is not None:
        mask = np.load(inp.rollout_sensor_mask)
        if mask.shape not in ((coords.shape[0], c), y.shape):
            raise ValueError(f"rollout_sensor_mask of shape {tuple(mask.shape)} is neither ({coords.shape[0]}, {c}) "
                             f"nor {tuple(y.shape)}")
        fn = partial(cond.conditioning, mask=torch.as_tensor(mask, dtype=torch.float32).to(device))
    return {"cond_fn": fn, "measurement": torch.as_tensor(y, dtype=torch.float32).to(device)}


def run(yaml_path: str):
    rank, world, device = dist.init_from_env()
    if device.type != "cuda":
        raise _lib.CfdError("confild_amd.inference needs a GPU")
    inp = basic_input(yaml_path)
    jcompute = derived_compute(inp)                          # raises before any model is built
    hcompute = derived_hessian_compute(inp)                  # the same for the Hessian launch
    physics = derived_physics(inp)                           # and the residuals' keys
    seed = int(getattr(inp, "seed", 42))
    torch.manual_seed(seed)
    np.random.seed(seed)
    # Philox key of the reverse loop, drawn first so it depends only on `seed`
    # (identical on every rank)
    loop_seed = int(torch.randint(0, 2 ** 62, (1,)).item())

    model = create_model(image_size=inp.image_size, num_channels=inp.num_channels,
                         num_res_blocks=inp.num_res_blocks, num_heads=inp.num_heads,
                         num_head_channels=inp.num_head_channels,
                         attention_resolutions=inp.attention_resolutions,
                         channel_mult=getattr(inp, "channel_mult", None))
    model.set_compute(unet_compute(inp))
    if rank == 0:
        model.load_state_dict(torch.load(inp.ema_path, weights_only=True, map_location="cpu"))
    model.to(device)
    dist.broadcast_module(model)
    diff = create_gaussian_diffusion(steps=inp.steps, noise_schedule=inp.noise_schedule,
                                     timestep_respacing=getattr(inp, "timestep_respacing", ""))
    sampler = getattr(inp, "sampler", "ddpm")
    B, T, L = inp.test_batch_size, inp.time_length, inp.latent_length

    windows = int(getattr(inp, "rollout_windows", 0))
    if windows < 0:
        raise ValueError(f"rollout_windows must be >= 0, got {windows}")

    guided = str(getattr(inp, "rollout_method", "replace")) == "guided"
    overlap = int(getattr(inp, "rollout_overlap", T // 2))
    cnf, guide = None, {}
    if guided:
        # the measurement operator decodes with the driver's own CNF: load it before sampling
        cnf = load_cnf(inp, device)
        guide = guided_rollout(inp, cnf, device, T, windows, overlap)

    def sample(start, count):
        if windows or guided:
            from .rollout import extend_latents
            if (T, L) != (model.image_size, model.image_size):
                raise ValueError("a rollout needs time_length == latent_length == image_size")
            kind = "ddpm" if sampler == "ddpm" else "ddim"     # as the plain run picks its loop
            rdiff, method = rollout_sampler(inp, diff, kind)
            n_sample = int(getattr(inp, "rollout_jump_n_sample", 1))
            resample = None if n_sample == 1 else (int(getattr(inp, "rollout_jump_length", 10)), n_sample)
            return extend_latents(model, rdiff, None, windows, overlap, method,
                                  scale=float(getattr(inp, "rollout_scale", 1.0)), seed=loop_seed,
                                  sample_offset=start, sampler=kind, batch_size=count, resample=resample,
                                  **guide)[:, 0]
        fn = diff.p_sample_loop if sampler == "ddpm" else diff.ddim_sample_loop
        return fn(model, (count, 1, T, L), seed=loop_seed, sample_offset=start)[:, 0]

    gen = dist.sharded_samples(sample, B)                    # (B, T, L) on every rank
    T = gen.shape[1]                                         # T_total of a rollout

    max_val = torch.as_tensor(np.load(inp.max_val), dtype=torch.float32).to(device).contiguous()
    min_val = torch.as_tensor(np.load(inp.min_val), dtype=torch.float32).to(device).contiguous()
    gen = latent_denorm(gen.contiguous(), max_val, min_val)   # inference.py:59-61

    if cnf is None:
        cnf = load_cnf(inp, device)
    coord = cnf.train_coord
    if getattr(inp, "coords_path", None):
        coord = torch.as_tensor(np.load(inp.coords_path), dtype=torch.float32)
    # lumped (N, d) points, or an (h, w, d) grid: the reference keeps the grid
    # shape and saves (B*T, h, w, c) (train.py:274-277, inference.py:75-81)
    coord = coord.to(device)
    spatial = tuple(coord.shape[:-1])
    npts = int(np.prod(spatial))
    lat = gen.reshape(B * T, L)
    names = derived_names(inp)
    vch = getattr(inp, "derived_velocity_channels", None)
    c, d = cnf.nf.out_features, cnf.nf.in_coord_features
    jnames = [n for n in names if n not in HESSIAN_DERIVED]
    hnames = [n for n in names if n in HESSIAN_DERIVED]
    # the unmixed derivatives are all a Laplacian needs, and the residuals need the Laplacian only
    diag = bool(hnames) and all(n == "laplacian" or n in RESIDUAL_DERIVED for n in hnames)
    hd = d if diag else d * d
    # rows per launch bounded by ~2 GiB of output (with `derived`: the fields and their (c, d) Jacobian;
    # with a Hessian name also that launch's fields, Jacobian and (c, d, d) or (c, d) Hessian; the
    # PDE-residual names keep up to (c, d) floats of intermediates of their own per point and name)
    nres = sum(n in RESIDUAL_DERIVED or n == "convective_acceleration" for n in names)
    rows = max(1, (2 << 30) // (npts * c * 4 * ((1 + d if jnames else 1) + (1 + d + hd if hnames else 0) +
                                                nres * d)))
    fields, extra = [], {n: [] for n in names}
    s, e = dist.shard_range(B * T, rank, world)
    for a in range(s, e, rows):
        chunk = lat[a:min(e, a + rows)]
        # the fields are the plain decode's whether or not `derived` is set (the Jacobian
        # launch's values are not the ones saved, whatever derived_compute it runs)
        fields.append(cnf.infer(coord, chunk))
        if jnames:
            jac = cnf.infer_jacobian(coord, chunk, compute=jcompute)[1]
            for n in jnames:
                extra[n].append(derived_quantity(n, jac, vch, fields=fields[-1]))
        if hnames:
            _, hjac, hess = cnf.infer_hessian(coord, chunk, diag=diag, compute=hcompute)
            for n in hnames:
                extra[n].append(derived_quantity(n, hjac, vch, hess, diag, fields[-1], physics))
    local = {"": torch.cat(fields) if fields else torch.empty((0,) + spatial + (c,), device=device)}
    for n in names:
        local[n] = (torch.cat(extra[n]) if extra[n] else
                    derived_quantity(n, torch.empty((0,) + spatial + (c, d), device=device), vch,
                                     torch.empty((0,) + spatial + (c,) + (d,) * (1 if diag else 2), device=device),
                                     diag, torch.empty((0,) + spatial + (c,), device=device),
                                     physics)).contiguous()
    if world > 1:   # gather the decoded fields to rank 0 over RCCL
        sizes = [dist.shard_range(B * T, r, world)[1] - dist.shard_range(B * T, r, world)[0] for r in range(world)]
        local = {n: dist.gather_cat(v, 0, sizes, dst=0) for n, v in local.items()}
    if rank == 0:
        out = local[""].cpu().numpy()
        np.save(inp.save_path, out)                          # (B*T, N, c) or (B*T, h, w, c), inference.py:79-81
        stem = os.path.splitext(str(inp.save_path))[0]
        for n in names:
            np.save(f"{stem}_{n}.npy", local[n].cpu().numpy())
        return out
    return None


if __name__ == "__main__":
    run(sys.argv[1])
