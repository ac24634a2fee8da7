"""GPU: known rows in the guided (DPS) sampler and the sensor-guided rollout
(cfd_dps_update_known; _GuidedSampler.p_sample_loop / p_sample_step(known=, known_mask=,
known_noise=); rollout.*("guided", cond_fn=, measurement=); the driver's rollout_sensor_* keys).

With known rows the last call of a guided step writes, per element,
    img = sample - (g_direct + g_unet) * scale
    q   = a_i * known + b_i * n2
    out = m * q + (1 - m) * img           (fp32, contraction off, in this order)
with (a_i, b_i) = GaussianDiffusion.known_table()[t] and n2 Philox (seed, (1 << 41) + k).
Everything runs on the tiny16 U-Net at 4 respaced steps with the operator of
tests/golden/dps_tiny16.npz (5 sensors, 3 channels).  Every comparison is bit-exact
(the kernel against the same expression evaluated by torch on the CPU, mask 0 against
the loop without known rows, scale 0 against GaussianDiffusion's known-row loop, a
batch against its chains, the rollout against the direct calls it chains, the
bounds-checked build against the shipped library) except one: the inference driver
against the CPU oracle decode, at 2e-5."""
import ast
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import golden
from confild_amd import _lib, inference, rollout, synth
from confild_amd import gaussian_diffusion as gd
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts
from confild_amd.script_util import create_gaussian_diffusion, create_model
from oracle import siren as osn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")
S, T, OV, W, SEED = 16, 16, 5, 2, 4242
TOTAL = T + W * (T - OV)
EARG = 1


def _sampler(kind="ddpm"):
    from confild_amd.guided.gaussian_diffusion import create_sampler
    return create_sampler(sampler=kind, steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                          model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=False, timestep_respacing="4")


def _cond_fn(op, scale, name="ps", **kw):
    from confild_amd.guided.condition_methods import get_conditioning_method
    from confild_amd.guided.measurements import get_noise
    cond = get_conditioning_method(name, op, get_noise("gaussian", sigma=0.0), scale=scale)
    return functools.partial(cond.conditioning, **kw)


@pytest.fixture(scope="module")
def dps():
    """(model, op, y): the tiny16 U-Net, the Case4 operator and the (16, 5, 3) measurement of
    dps_tiny16.npz, built as _dps_setup of test_gpu_dps.py does."""
    from confild_amd.guided.measurements import Case4Operator
    from confild_amd.guided.unet import create_model as guided_model
    g = golden("dps_tiny16.npz")
    model = guided_model(**ast.literal_eval(str(g["kwargs"])))
    sd = synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.to(DEV)
    d, L, c, nh, H = (int(v) for v in g["siren_dims"])
    nf = SIRENAutodecoder_film(d, L, c, nh, H)
    nf.load_state_dict({k: torch.from_numpy(v) for k, v in
                        synth.siren_state_dict(int(g["siren_seed"]), d, L, c, nh, H).items()})
    A = lambda k: torch.from_numpy(g[k])  # noqa: E731
    op = Case4Operator.from_parts(DEV, A("coords"), Normalizer_ts(params=(A("xhi"), A("xlo")), method="-11", dim=0),
                                  Normalizer_ts(params=(A("yhi"), A("ylo")), method="-11", dim=0), nf, A("vmax"),
                                  A("vmin"), batch_size=int(g["op_batch"]))
    return model, op, A("measurement").to(DEV)


def _known(B, tag="gk", rows=OV):
    known = torch.from_numpy(synth.uniform(9, f"{tag}/known", (B, 1, S, S), -0.9, 0.9)).to(DEV)
    mask = torch.zeros(1, 1, S, S, device=DEV)
    mask[:, :, :rows] = 1.0
    return known, mask


def _x_start(B, tag="gk"):
    return torch.from_numpy(synth.normal(3, f"{tag}/xs", (B, 1, S, S))).to(DEV)


# ---------------------------------------------------------------------------
# 1, 2: the kernel on the C ABI
# ---------------------------------------------------------------------------
def _expression(sample, g_dir, g_unet, scale, tab, t, known, mask, n2):
    """The stated fp32 expression, one torch op per operation, on the CPU."""
    B = sample.shape[0]
    sc = torch.tensor(scale, dtype=torch.float32)
    a = tab[t, 0].reshape(B, 1, 1, 1)
    b = tab[t, 1].reshape(B, 1, 1, 1)
    img = sample - (g_dir + g_unet) * sc
    q = a * known + b * n2
    return mask * q + (1.0 - mask) * img


def _c_update(hip, d, sample, g_dir, g_unet, scale, t, known, mask, nz2, seed=0, counter2=0, offset=0, out=None):
    kn = gd._Known(known, mask, tuple(sample.shape), DEV)
    out = torch.empty_like(sample) if out is None else out
    _lib.check(hip.cfd_dps_update_known(_lib.ptr(sample), _lib.ptr(g_dir), _lib.ptr(g_unet), scale, _lib.ptr(out),
                                        _lib.ptr(t), sample[0].numel(), sample.shape[0], _lib.ptr(kn.known),
                                        kn.kstride, _lib.ptr(kn.mask), kn.mstride, _lib.ptr(d._ktab(DEV)),
                                        _lib.ptr(nz2), seed, counter2, offset, _lib.stream_of(DEV)),
               "cfd_dps_update_known")
    return out


def _kernel_case(B, rows, cols, shared, t):
    shape = (B, 1, rows, cols)
    tag = f"uk/{B}x{rows}x{cols}"
    f = lambda name: torch.from_numpy(synth.normal(4, f"{tag}/{name}", shape))  # noqa: E731
    lead = 1 if shared else B
    known = torch.from_numpy(synth.uniform(4, tag + "/kn", (lead, 1, rows, cols), -0.9, 0.9))
    mask = torch.from_numpy(synth.uniform(4, tag + "/m", (lead, 1, rows, cols), 0.0, 1.0))
    mask[:, :, :3] = 1.0
    mask[:, :, 3] = 0.0
    return f("s"), f("gd"), f("gu"), f("nz2"), known, mask, torch.tensor(t, dtype=torch.int64)


@pytest.mark.parametrize("B,rows,cols,shared,t", [
    (2, 24, 32, True, [0, 3]), (2, 24, 32, False, [0, 3]), (3, 24, 48, True, [0, 3, 2]),
    (3, 24, 48, False, [0, 3, 2]), (1, 25, 27, True, [0]), (1, 25, 27, True, [2]), (3, 15, 15, False, [0, 3, 1])])
def test_update_known_is_the_stated_expression(hip, B, rows, cols, shared, t):
    """B x n = 2 x 768 and 3 x 1,152 (16-byte loads and stores), 1 x 675 (168 groups of 4 and a
    tail of 3) and 3 x 225 (groups that straddle two samples): table index 0 (q = known) and mixed
    indices within a batch; a fractional mask with rows of exactly 1 and 0; explicit n2, then
    Philox n2 against cfd_randn at (seed, counter2, offset) for offsets 0 and 148."""
    d = _sampler()
    scale = 0.37
    s, g_dir, g_unet, nz2, known, mask, t = _kernel_case(B, rows, cols, shared, t)
    tab = d.known_table()
    assert tab[0, 0].item() == 1.0 and tab[0, 1].item() == 0.0
    dev = lambda v: v.to(DEV).contiguous()  # noqa: E731
    got = _c_update(hip, d, dev(s), dev(g_dir), dev(g_unet), scale, dev(t), known, mask, dev(nz2))
    want = _expression(s, g_dir, g_unet, scale, tab, t, known, mask, nz2)
    assert torch.equal(got.cpu(), want)
    if t[0] == 0:
        # table index 0: q is `known` itself, so rows of mask 1 carry it
        assert torch.equal(got[0, :, :3].cpu(), known[0, :, :3])
    # rows of mask 0: cfd_dps_update's bits
    plain = torch.empty_like(got)
    ds, dgd, dgu = dev(s), dev(g_dir), dev(g_unet)
    _lib.check(hip.cfd_dps_update(_lib.ptr(ds), _lib.ptr(dgd), _lib.ptr(dgu), scale, _lib.ptr(plain), s.numel(),
                                  _lib.stream_of(DEV)), "cfd_dps_update")
    assert torch.equal(got[:, :, 3], plain[:, :, 3])
    for offset in (0, 148):
        seed, counter2 = 77, gd.KNOWN_COUNTER + 5
        n2 = torch.empty(s.numel(), dtype=torch.float32, device=DEV)
        _lib.check(hip.cfd_randn(_lib.ptr(n2), n2.numel(), seed, counter2, offset, _lib.stream_of(DEV)), "cfd_randn")
        got = _c_update(hip, d, dev(s), dev(g_dir), dev(g_unet), scale, dev(t), known, mask, None, seed, counter2,
                        offset)
        want = _expression(s, g_dir, g_unet, scale, tab, t, known, mask, n2.cpu().reshape(s.shape))
        assert torch.equal(got.cpu(), want), offset


def test_update_known_unaligned_arrays_and_aliasing(hip):
    """Arrays that start 4 bytes off a 16-byte boundary take the scalar path: the same bits.
    x_out may alias sample."""
    d = _sampler()
    s, g_dir, g_unet, nz2, known, mask, t = _kernel_case(2, 24, 32, False, [0, 3])
    want = _expression(s, g_dir, g_unet, 0.37, d.known_table(), t, known, mask, nz2)

    def off(v):
        buf = torch.empty(v.numel() + 1, dtype=torch.float32, device=DEV)
        buf[1:] = v.reshape(-1).to(DEV)
        view = buf[1:].reshape(v.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    sample = off(s)
    got = _c_update(hip, d, sample, off(g_dir), off(g_unet), 0.37, t.to(DEV), known, mask, off(nz2))
    assert torch.equal(got.cpu(), want)
    aligned = s.to(DEV)
    _c_update(hip, d, aligned, g_dir.to(DEV), g_unet.to(DEV), 0.37, t.to(DEV), known, mask, nz2.to(DEV), out=aligned)
    assert torch.equal(aligned.cpu(), want)


def test_update_known_argument_errors(hip):
    d = _sampler()
    s, g_dir, g_unet, _, known, mask, t = (v.to(DEV).contiguous() for v in _kernel_case(2, 24, 32, False, [0, 3]))
    n, B = s[0].numel(), s.shape[0]
    out = torch.full_like(s, 7.0)

    def call(offset=0, kstride=n, mstride=n, known_ptr=_lib.ptr(known), nB=B, sample_ptr=_lib.ptr(s)):
        return hip.cfd_dps_update_known(sample_ptr, _lib.ptr(g_dir), _lib.ptr(g_unet), 0.5, _lib.ptr(out),
                                        _lib.ptr(t), n, nB, known_ptr, kstride, _lib.ptr(mask), mstride,
                                        _lib.ptr(d._ktab(DEV)), None, 1, 2, offset, _lib.stream_of(DEV))
    assert call(offset=2) == EARG and b"multiple of 4" in hip.cfd_last_error()
    assert call(offset=5) == EARG
    assert call(kstride=n // 2) == EARG and b"stride" in hip.cfd_last_error()
    assert call(mstride=1) == EARG
    assert call(known_ptr=None) == EARG and b"null" in hip.cfd_last_error()
    assert call(sample_ptr=None) == EARG
    assert call(nB=0) == EARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---------------------------------------------------------------------------
# 3 - 7: the guided sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,operator", [("ddpm", "case4"), ("ddim", "case4"), ("ddpm", "inpainting")])
def test_mask_zero_is_the_loop_without_known_rows(hip, dps, kind, operator):
    model, op, y = dps
    sampler = _sampler(kind)
    xs = _x_start(2)
    known, _ = _known(2)
    if operator == "case4":
        fn, meas = _cond_fn(op, 0.5), y
    else:
        from confild_amd.guided.measurements import get_operator
        _, m = _known(1, rows=7)
        fn, meas = _cond_fn(get_operator("inpainting", device=DEV), 0.5, mask=m), m * _known(2, "gk/inp")[0]
    plain = sampler.p_sample_loop(model=model, x_start=xs, measurement=meas, measurement_cond_fn=fn, seed=SEED)
    dist = sampler.distances.clone()
    zero = sampler.p_sample_loop(model=model, x_start=xs, measurement=meas, measurement_cond_fn=fn, seed=SEED,
                                 known=known, known_mask=torch.zeros(1, 1, S, S))
    assert torch.isfinite(plain).all()
    assert torch.equal(zero, plain)
    assert sampler.distances.shape == (4, 2) and torch.equal(sampler.distances, dist)


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_scale_zero_is_the_unconditioned_known_row_loop(hip, dps, monkeypatch, kind):
    """scale = 0 switches the measurement off: what is left is GaussianDiffusion's
    known-row loop (its Python loop: cfd_sched_step_known per step), so the step noise,
    n2 and the replacement are the same bits in both families."""
    model, op, y = dps
    B = 2
    known, mask = _known(B)
    x_T = rollout.window_noise((B, 1, S, S), SEED, 0, DEV)
    got = _sampler(kind).p_sample_loop(model=model, x_start=x_T, measurement=y, measurement_cond_fn=_cond_fn(op, 0.0),
                                       seed=SEED, known=known, known_mask=mask)
    plain = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="4")
    monkeypatch.setattr(gd, "NATIVE_MODE", 0)
    loop = plain.p_sample_loop if kind == "ddpm" else plain.ddim_sample_loop
    want = loop(model, (B, 1, S, S), seed=SEED, known=known, known_mask=mask)
    assert torch.equal(got, want)
    assert torch.equal(got[:, :, :OV], known[:, :, :OV])
    # 'vanilla' with known rows is that loop too (cfd_sched_step_known)
    van = _sampler(kind).p_sample_loop(model=model, x_start=x_T, measurement=y,
                                       measurement_cond_fn=_cond_fn(op, 1.0, "vanilla"), seed=SEED, known=known,
                                       known_mask=mask)
    assert torch.equal(van, want)


def test_mask_one_and_the_gradient_acts_on_free_rows_only(hip, dps):
    model, op, y = dps
    sampler = _sampler()
    B = 2
    xs = _x_start(B)
    known, mask = _known(B)
    run = lambda scale, m: sampler.p_sample_loop(model=model, x_start=xs, measurement=y,  # noqa: E731
                                                 measurement_cond_fn=_cond_fn(op, scale), seed=SEED, known=known,
                                                 known_mask=m)
    assert torch.equal(run(0.5, torch.ones(1, 1, S, S)), known)
    guided, free = run(0.5, mask), run(0.0, mask)
    assert torch.equal(guided[:, :, :OV], known[:, :, :OV]) and torch.equal(free[:, :, :OV], known[:, :, :OV])
    assert torch.isfinite(guided).all()
    assert not torch.equal(guided[:, :, OV:], free[:, :, OV:])
    assert bool((guided[:, :, OV:] != free[:, :, OV:]).any(dim=3).all())     # every free row moved


def test_batch_of_chains_with_per_sample_known_rows(hip, dps):
    model, op, y = dps
    sampler = _sampler()
    fn = _cond_fn(op, 0.5)
    xs = _x_start(3)
    known, mask = _known(3)
    kw = dict(model=model, measurement=y, measurement_cond_fn=fn, seed=99, known_mask=mask)
    full = sampler.p_sample_loop(x_start=xs, known=known, **kw)
    dfull = sampler.distances.clone()
    assert torch.equal(sampler.p_sample_loop(x_start=xs, known=known, **kw), full)
    for s in range(3):
        one = sampler.p_sample_loop(x_start=xs[s:s + 1], known=known[s:s + 1], sample_offset=s, **kw)
        assert torch.equal(one, full[s:s + 1]), s
        assert torch.equal(sampler.distances[:, 0], dfull[:, s]), s
    assert not torch.equal(full[0], full[1])


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_p_sample_step_with_known_rows(hip, dps, kind):
    """The step with known rows returns the same x_t, x0 and distance as the step without,
    and its sample is the stated expression of that step's conditioned image."""
    model, op, y = dps
    sampler = _sampler(kind)
    B, index = 2, 2
    x = _x_start(B, "gk/step")
    known = torch.from_numpy(synth.uniform(9, "gk/step/known", (B, 1, S, S), -0.9, 0.9))
    mask = torch.from_numpy(synth.uniform(9, "gk/step/m", (1, 1, S, S), 0.0, 1.0))
    mask[:, :, :OV] = 1.0
    nz = torch.from_numpy(synth.normal(9, "gk/step/nz", (B, 1, S, S)))
    nz2 = torch.from_numpy(synth.normal(9, "gk/step/nz2", (B, 1, S, S)))
    fn = _cond_fn(op, 0.5)
    base = sampler.p_sample_step(model, x, index, y, fn, noise=nz)
    out = sampler.p_sample_step(model, x, index, y, fn, noise=nz, known=known, known_mask=mask, known_noise=nz2)
    for key in ("x_t", "pred_xstart", "distance"):
        assert torch.equal(out[key], base[key]), key
    tab = sampler.known_table()
    q = tab[index, 0] * known + tab[index, 1] * nz2
    want = mask * q + (1.0 - mask) * base["sample"].cpu()
    assert torch.equal(out["sample"].cpu(), want)
    assert not torch.equal(out["sample"], base["sample"])
    # Philox n2: counter (1 << 41) + counter of the step's key
    n2 = torch.empty(B * S * S, dtype=torch.float32, device=DEV)
    _lib.check(hip.cfd_randn(_lib.ptr(n2), n2.numel(), 31, gd.KNOWN_COUNTER + 3, 0, _lib.stream_of(DEV)), "cfd_randn")
    out = sampler.p_sample_step(model, x, index, y, fn, noise=nz, seed=31, counter=3, known=known, known_mask=mask)
    q = tab[index, 0] * known + tab[index, 1] * n2.cpu().reshape(B, 1, S, S)
    assert torch.equal(out["sample"].cpu(), mask * q + (1.0 - mask) * base["sample"].cpu())
    # the argument faults of GaussianDiffusion.p_sample_loop
    with pytest.raises(ValueError, match="go together"):
        sampler.p_sample_step(model, x, index, y, fn, noise=nz, known=known)
    with pytest.raises(ValueError, match="known_noise without known rows"):
        sampler.p_sample_step(model, x, index, y, fn, noise=nz, known_noise=nz2)
    with pytest.raises(ValueError, match="broadcasts to neither"):
        sampler.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=fn, seed=1,
                              known=known[:, :, :5], known_mask=mask)
    with pytest.raises(ValueError, match="resampling jumps"):
        sampler.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=fn, seed=1, known=known,
                              known_mask=mask, resample=(2, 2))


# ---------------------------------------------------------------------------
# 8: the rollout
# ---------------------------------------------------------------------------
def _record(op, B):
    """(B, 38, 5, 3): the operator on a seeded latent sequence clamped to [-1, 1]."""
    seq = torch.from_numpy(synth.normal(6, "gk/seq", (B, 1, TOTAL, S))).clamp(-1.0, 1.0).to(DEV)
    rec = op.forward(seq)
    assert rec.shape == (B * TOTAL, 5, 3)
    return rec.reshape(B, TOTAL, 5, 3)


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_guided_rollout_is_the_chain_of_direct_calls(hip, dps, kind):
    model, op, _ = dps
    B = 2
    sampler = _sampler(kind)
    fn = _cond_fn(op, 0.5)
    rec = _record(op, B)[0]
    out = rollout.extend_latents(model, sampler, None, W, OV, "guided", seed=SEED, batch_size=B, cond_fn=fn,
                                 measurement=rec)
    assert out.shape == (B, 1, 38, 16) == (B, 1, TOTAL, S)
    assert torch.isfinite(out).all()
    windows = rollout.plan_windows(T, OV, W)
    direct = lambda w, **kw: sampler.p_sample_loop(  # noqa: E731
        model=model, x_start=rollout.window_noise((B, 1, T, S), SEED + w, 0, DEV), measurement=rec[windows[w]],
        measurement_cond_fn=fn, seed=SEED + w, **kw)
    assert torch.equal(out[:, :, windows[0]], direct(0))
    for w in range(1, W + 1):
        sl = windows[w]
        known, mask = rollout.known_rows(out[:, :, windows[w - 1]], OV)
        assert torch.equal(known[:, :, :OV], out[:, :, sl.start:sl.start + OV])
        win = direct(w, known=known, known_mask=mask)
        assert torch.equal(out[:, :, sl.start + OV:sl.stop], win[:, :, OV:]), w
        # the overlap rows are the earlier window's values, in the window and in the sequence
        assert sl.start == windows[w - 1].stop - OV
        assert torch.equal(win[:, :, :OV], out[:, :, sl.start:sl.start + OV]), w
    assert not torch.equal(out[:, :, 5:16], out[:, :, 16:27]) and not torch.equal(out[:, :, 16:27], out[:, :, 27:38])
    # continuing a given first window gives the same sequence
    again = rollout.extend_latents(model, sampler, out[:, :, :T].clone(), W, OV, "guided", seed=SEED, cond_fn=fn,
                                   measurement=rec)
    assert torch.equal(again, out)
    # the measurement steers the free rows: another record, another sequence
    other = rollout.extend_latents(model, sampler, None, W, OV, "guided", seed=SEED, batch_size=B, cond_fn=fn,
                                   measurement=rec * 0.5)
    assert not torch.equal(other[:, :, OV:T], out[:, :, OV:T])


def test_guided_rollout_shards_and_per_sample_records(hip, dps):
    model, op, _ = dps
    B = 2
    sampler = _sampler()
    fn = _cond_fn(op, 0.5)
    per = _record(op, B)
    run = lambda meas, **kw: rollout.extend_latents(model, sampler, None, W, OV, "guided", seed=SEED,  # noqa: E731
                                                    cond_fn=fn, measurement=meas, **kw)
    full = run(per[0], batch_size=B)
    for s in range(B):
        assert torch.equal(run(per[0], batch_size=1, sample_offset=s), full[s:s + 1]), s
    both = run(per, batch_size=B)
    assert torch.equal(both[0:1], full[0:1]) and not torch.equal(both[1:2], full[1:2])
    for s in range(B):
        assert torch.equal(run(per[s:s + 1], batch_size=1, sample_offset=s), both[s:s + 1]), s
        assert torch.equal(run(per[s], batch_size=1, sample_offset=s), both[s:s + 1]), s
    # a mask with a row dimension is cut like the record: sensor 0 switched off in rows 16..37
    mask = torch.ones(TOTAL, 5, 3, device=DEV)
    mask[T:, 0] = 0.0
    masked = rollout.extend_latents(model, sampler, None, W, OV, "guided", seed=SEED, batch_size=B,
                                    cond_fn=_cond_fn(op, 0.5, mask=mask), measurement=per[0])
    windows = rollout.plan_windows(T, OV, W)
    x_T = rollout.window_noise((B, 1, T, S), SEED, 0, DEV)
    win0 = sampler.p_sample_loop(model=model, x_start=x_T, measurement=per[0][windows[0]],
                                 measurement_cond_fn=_cond_fn(op, 0.5, mask=mask[windows[0]]), seed=SEED)
    assert torch.equal(masked[:, :, :T], win0)
    assert torch.isfinite(masked).all() and not torch.equal(masked[:, :, T:], full[:, :, T:])


def test_guided_rollout_argument_errors(hip, dps):
    model, op, _ = dps
    sampler = _sampler()
    fn = _cond_fn(op, 0.5)
    rec = _record(op, 1)[0]
    plain = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="4")
    with pytest.raises(TypeError):
        rollout.extend_latents(model, sampler, None, W, OV, "guided", seed=1)
    with pytest.raises(TypeError):
        rollout.extend_latents(model, plain, None, W, OV, "guided", seed=1, cond_fn=fn, measurement=rec)
    with pytest.raises(ValueError):
        rollout.extend_latents(model, sampler, None, W, OV, "guided", seed=1, cond_fn=fn, measurement=rec,
                               resample=(2, 2))
    with pytest.raises(ValueError, match="measurement of shape"):
        rollout.extend_latents(model, sampler, None, W, OV, "guided", seed=1, cond_fn=fn, measurement=rec[:-1])
    from confild_amd.guided.measurements import get_operator
    with pytest.raises(TypeError):
        rollout.extend_latents(model, sampler, None, W, OV, "guided", seed=1, measurement=rec,
                               cond_fn=_cond_fn(get_operator("inpainting", device=DEV), 0.5))


# ---------------------------------------------------------------------------
# 9: the driver's keys, end to end
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["sensors", "masked"])
def test_inference_driver_guided_rollout_keys(hip, tmp_path, masked):
    """python -m confild_amd.inference with rollout_method: guided: the saved array is
    (B * T_total, N, c), the decode of extend_latents' sequence on an operator built from
    the same CNF (CPU oracle decode, the tolerance of test_gpu_rollout.py's driver test);
    rollout_windows: 0 is one guided window; a record of another length is refused."""
    from confild_amd.guided.measurements import Case4Operator
    g = golden("unet_tiny16.npz")
    kw = ast.literal_eval(str(g["kwargs"]))
    tiny = create_model(**kw)
    tiny.load_state_dict({k: torch.from_numpy(v) for k, v in synth.unet_state_dict(
        int(g["seed"]), {k: tuple(v.shape) for k, v in tiny.state_dict().items()}).items()})
    tiny.to(DEV)
    torch.save({k: v.detach().cpu() for k, v in tiny.state_dict().items()}, tmp_path / "ema.pt")
    d, L, c, nh, H, N, Ns = 3, 16, 3, 2, 32, 300, 6
    yhi = torch.from_numpy(synth.uniform(5, "yhi", (c,), 0.5, 2.0))
    ssd = {k: torch.from_numpy(v) for k, v in synth.siren_state_dict(5, d, L, c, nh, H).items()}
    cnf_dir = tmp_path / "cnf"
    cnf_dir.mkdir()
    torch.save({"x_normalizer_params": (torch.ones(1, d), torch.zeros(1, d)),
                "y_normalizer_params": (yhi, -yhi)}, cnf_dir / "normalizer_params.pt")
    torch.save({"epoch": 1, "model_state_dict": ssd}, cnf_dir / "checkpoint_1.pt")
    coords = synth.uniform(5, "coords", (N, d), 0.0, 1.0)
    np.save(tmp_path / "coords.npy", coords)
    cnf_cfg = {"save_path": str(cnf_dir), "coor_path": str(tmp_path / "coords.npy"), "lumped_latent": True,
               "normalizer": {"method": "-11", "dim": 0}, "multiGPU": 1, "hidden_size": L, "dims": d,
               "NF": {"name": "SIRENAutodecoder_film", "out_features": c, "num_hidden_layers": nh,
                      "hidden_features": H}}
    (tmp_path / "cnf.yml").write_text(yaml.safe_dump(cnf_cfg))
    np.save(tmp_path / "max.npy", np.float32(1.5))
    np.save(tmp_path / "min.npy", np.float32(-1.5))
    # the sensors and their record: the CNF's decode of a seeded latent sequence, physical values
    sensors = synth.uniform(5, "sensors", (Ns, d), 0.0, 1.0)
    nf = SIRENAutodecoder_film(d, L, c, nh, H)
    nf.load_state_dict(ssd)
    op = Case4Operator.from_parts(DEV, sensors, Normalizer_ts(params=(torch.ones(1, d), torch.zeros(1, d)),
                                                              method="-11", dim=0),
                                  Normalizer_ts(params=(yhi, -yhi), method="-11", dim=0), nf, np.float32(1.5),
                                  np.float32(-1.5))
    rec = _record_of(op)
    np.save(tmp_path / "sensors.npy", sensors)
    np.save(tmp_path / "record.npy", rec.cpu().numpy())
    mask = None
    B = 2
    cfg = {"test_batch_size": B, "time_length": T, "latent_length": T, "image_size": T,
           "num_channels": kw["num_channels"], "num_res_blocks": kw["num_res_blocks"],
           "channel_mult": kw["channel_mult"], "num_heads": kw["num_heads"],
           "num_head_channels": kw["num_head_channels"], "attention_resolutions": kw["attention_resolutions"],
           "ema_path": str(tmp_path / "ema.pt"), "steps": 1000, "noise_schedule": "cosine",
           "timestep_respacing": "4", "max_val": str(tmp_path / "max.npy"), "min_val": str(tmp_path / "min.npy"),
           "cnf_case_file_path": str(tmp_path / "cnf.yml"), "save_path": str(tmp_path / "out.npy"),
           "rollout_windows": W, "rollout_overlap": OV, "rollout_method": "guided", "rollout_scale": 0.5,
           "rollout_sensor_coords": str(tmp_path / "sensors.npy"),
           "rollout_measurement": str(tmp_path / "record.npy")}
    if masked:
        mask = torch.ones(TOTAL, Ns, c)
        mask[T:, 0] = 0.0
        mask[:, 3, 1] = 0.0
        np.save(tmp_path / "mask.npy", mask.numpy())
        cfg["rollout_sensor_mask"] = str(tmp_path / "mask.npy")
    (tmp_path / "case.yml").write_text(yaml.safe_dump(cfg))
    out = inference.run(str(tmp_path / "case.yml"))
    saved = np.load(tmp_path / "out.npy")
    assert saved.shape == (B * TOTAL, N, c) and np.array_equal(saved, out)

    torch.manual_seed(42)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    fn = _cond_fn(op, 0.5) if mask is None else _cond_fn(op, 0.5, mask=mask.to(DEV))
    lat = rollout.extend_latents(tiny, _sampler(), None, W, OV, "guided", seed=seed, batch_size=B, cond_fn=fn,
                                 measurement=rec)[:, 0]

    def decode(v):
        rows = ((v + 1) * (1.5 + 1.5) / 2. - 1.5).reshape(-1, T).cpu()
        return osn.decode(ssd, torch.from_numpy(coords), rows, torch.ones(1, d), torch.zeros(1, d), yhi, -yhi)
    ref = decode(lat)
    print("guided rollout driver against the CPU oracle decode:", np.abs(saved - ref.numpy()).max(),
          "max|ref|", float(ref.abs().max()))
    assert np.abs(saved - ref.numpy()).max() <= 2e-5 * max(1.0, float(ref.abs().max()))
    if masked:
        return
    # rollout_windows: 0 is one guided window on a record of T rows
    np.save(tmp_path / "record.npy", rec[:T].cpu().numpy())
    cfg["rollout_windows"] = 0
    (tmp_path / "case.yml").write_text(yaml.safe_dump(cfg))
    one = inference.run(str(tmp_path / "case.yml"))
    assert one.shape == (B * T, N, c)
    x_T = rollout.window_noise((B, 1, T, T), seed, 0, DEV)
    win = _sampler().p_sample_loop(model=tiny, x_start=x_T, measurement=rec[:T], measurement_cond_fn=fn, seed=seed)
    ref = decode(win[:, 0])
    assert np.abs(one - ref.numpy()).max() <= 2e-5 * max(1.0, float(ref.abs().max()))
    # a record whose row count is not T_total, or a missing key: ValueError before any launch
    cfg["rollout_windows"] = W
    (tmp_path / "case.yml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="T_total"):
        inference.run(str(tmp_path / "case.yml"))
    del cfg["rollout_sensor_coords"]
    (tmp_path / "case.yml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="rollout_sensor_coords"):
        inference.run(str(tmp_path / "case.yml"))


def _record_of(op):
    """(38, Ns, c): the operator on one seeded latent sequence clamped to [-1, 1]."""
    seq = torch.from_numpy(synth.normal(6, "gk/drv", (1, 1, TOTAL, S))).clamp(-1.0, 1.0).to(DEV)
    return op.forward(seq)


# ---------------------------------------------------------------------------
# 10: the bounds-checked build
# ---------------------------------------------------------------------------
DEBUG_CHILD = r"""
import ast, functools, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from confild_amd import synth
from confild_amd.guided.condition_methods import get_conditioning_method
from confild_amd.guided.gaussian_diffusion import create_sampler
from confild_amd.guided.measurements import Case4Operator, get_noise
from confild_amd.guided.unet import create_model
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts
g = np.load(sys.argv[1] + "/tests/golden/dps_tiny16.npz")
dev = torch.device("cuda", 0)
m = create_model(**ast.literal_eval(str(g["kwargs"])))
shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.unet_state_dict(int(g["seed"]), shapes).items()})
m.to(dev)
d, L, c, nh, H = (int(v) for v in g["siren_dims"])
nf = SIRENAutodecoder_film(d, L, c, nh, H)
ssd = synth.siren_state_dict(int(g["siren_seed"]), d, L, c, nh, H)
nf.load_state_dict({k: torch.from_numpy(v) for k, v in ssd.items()})
A = lambda k: torch.from_numpy(g[k])
op = Case4Operator.from_parts(dev, A("coords"), Normalizer_ts(params=(A("xhi"), A("xlo")), method="-11", dim=0),
                              Normalizer_ts(params=(A("yhi"), A("ylo")), method="-11", dim=0), nf, A("vmax"), A("vmin"),
                              batch_size=int(g["op_batch"]))
cond = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.0), scale=0.5)
sampler = create_sampler(sampler="ddpm", steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                         model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=False, timestep_respacing="4")
xs = torch.from_numpy(synth.normal(3, "gk/xs", (3, 1, 16, 16))).to(dev)
known = torch.from_numpy(synth.uniform(9, "gk/known", (3, 1, 16, 16), -0.9, 0.9)).to(dev)
mask = torch.zeros(1, 1, 16, 16, device=dev)
mask[:, :, :5] = 1.0
out = sampler.p_sample_loop(model=m, x_start=xs, measurement=A("measurement").to(dev),
                            measurement_cond_fn=functools.partial(cond.conditioning), seed=1234, known=known,
                            known_mask=mask)
torch.cuda.synchronize()
np.save(sys.argv[2], out.cpu().numpy())
"""


def test_debug_library_runs_the_guided_known_row_loop(hip, dps, tmp_path):
    """The 4-step guided loop with a row mask on the bounds-checked build (CFD_DASSERT in
    cfd_dps_update_known's 16-byte path, and every check of the U-Net's and the SIREN's
    kernels), in a child process: it exits clean, no assertion fires, and the final
    sample has the shipped library's bits."""
    if not os.path.exists(DEBUG_SO):
        pytest.skip("debug build absent (make -C confild_amd/csrc DEBUG=1)")
    env = dict(os.environ, CFD_LIB="libconfild_hip_debug.so")
    path = str(tmp_path / "dbg.npy")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD, ROOT, path], capture_output=True, text=True, env=env,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CFD_DASSERT" not in r.stdout + r.stderr
    dbg = torch.from_numpy(np.load(path))
    model, op, y = dps
    known, mask = _known(3)
    rel = _sampler().p_sample_loop(model=model, x_start=_x_start(3), measurement=y,
                                   measurement_cond_fn=_cond_fn(op, 0.5), seed=1234, known=known,
                                   known_mask=mask).cpu()
    print("debug build against the shipped library:", (dbg - rel).abs().max().item())
    assert torch.equal(dbg[:, :, :5], known[:, :, :5].cpu())
    assert torch.equal(dbg, rel)
