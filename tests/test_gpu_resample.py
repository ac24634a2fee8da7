"""GPU: RePaint resampling jumps on top of known-row replacement (cfd_sched_step_jump,
cfd_sampler_set_jumps; GaussianDiffusion.*(resample=(jump_length, jump_n_sample)),
p_sample / ddim_sample(jump_to=, jump_noise=), rollout.*(resample=), the driver's
rollout_jump_* keys).

A jumping step writes, after the known-row step's result s,
    out = ja * s + jb * n3        (fp32, contraction off)
with (ja, jb) = GaussianDiffusion.jump_coefs and n3 Philox (seed, (1 << 42) + k).
Every comparison is bit-exact (the step against the same expression evaluated by
torch on the CPU, the native graph loop against the Python loop, shards against the
batch, degenerate schedules against the known-row loop, the bounds-checked build
against the shipped library) except one: the inference driver against the CPU oracle
decode, at 2e-5."""
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
from confild_amd.script_util import create_gaussian_diffusion, create_model
from oracle import siren as osn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")
S = 16


@pytest.fixture(scope="module")
def tiny():
    g = golden("unet_tiny16.npz")
    kw = ast.literal_eval(str(g["kwargs"]))
    m = create_model(**kw)
    sd = synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _diff(respacing="8"):
    return create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing=respacing)


def _run(monkeypatch, mode, unroll, fn, *a, **k):
    monkeypatch.setattr(gd, "NATIVE_MODE", mode)
    monkeypatch.setattr(gd, "GRAPH_UNROLL", unroll)
    return fn(*a, **k)


def _known(B, tag="k"):
    known = torch.from_numpy(synth.uniform(9, f"{tag}/known", (B, 1, S, S), -0.9, 0.9)).to(DEV)
    mask = torch.zeros(1, 1, S, S, device=DEV)
    mask[:, :, :5] = 1.0
    return known, mask


class _Eps(torch.nn.Module):
    """A stand-in model returning a fixed eps: the step at shapes other than the U-Net's."""

    def __init__(self, eps):
        super().__init__()
        self.eps = eps

    def forward(self, x, t):
        return self.eps


def _c_step(hip, d, kind, x, eps, t, nz, kn, nz2, jump=None, seed=0, counter=0):
    """cfd_sched_step_known, or with ``jump`` = (ja, jb, nz3 | None) cfd_sched_step_jump, on the C ABI."""
    out, xs = torch.empty_like(x), torch.empty_like(x)
    head = (d._sched(DEV, 0.0).handle, kind, 1, _lib.ptr(x), _lib.ptr(eps), _lib.ptr(t), _lib.ptr(nz), seed, counter,
            0, _lib.ptr(out), _lib.ptr(xs), x[0].numel(), x.shape[0], _lib.ptr(kn.known), kn.kstride,
            _lib.ptr(kn.mask), kn.mstride, _lib.ptr(d._ktab(DEV)), _lib.ptr(nz2), gd.KNOWN_COUNTER + counter)
    if jump is None:
        _lib.check(hip.cfd_sched_step_known(*head, _lib.stream_of(DEV)), "cfd_sched_step_known")
    else:
        ja, jb, nz3 = jump
        _lib.check(hip.cfd_sched_step_jump(*head, ja, jb, _lib.ptr(nz3), gd.JUMP_COUNTER + counter,
                                           _lib.stream_of(DEV)), "cfd_sched_step_jump")
    return out, xs


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
@pytest.mark.parametrize("B,side,shared", [(3, 16, True), (3, 16, False), (2, 24, True), (2, 24, False),
                                           (3, 15, True), (3, 15, False)])
def test_jump_step_is_the_stated_expression(hip, ddim, B, side, shared):
    """B * n = 768, 1152 and 675 elements (675 = 168 groups of 4 and a tail of 3); table
    indices 1 (a jump from level 0), 3 and 7 in one launch; a fractional mask; explicit
    noise, known noise and jump noise, then Philox for all three."""
    d = _diff()
    kind = gd.STEP_DDIM if ddim else gd.STEP_DDPM
    shape = (B, 1, side, side)
    tag = f"js/{side}"
    x = torch.from_numpy(synth.normal(4, tag + "/x", shape)).to(DEV)
    eps = torch.from_numpy(synth.normal(4, tag + "/eps", shape)).to(DEV)
    nz = torch.from_numpy(synth.normal(4, tag + "/nz", shape)).to(DEV)
    nz2 = torch.from_numpy(synth.normal(4, tag + "/nz2", shape)).to(DEV)
    nz3 = torch.from_numpy(synth.normal(4, tag + "/nz3", shape)).to(DEV)
    lead = 1 if shared else B
    known = torch.from_numpy(synth.uniform(4, tag + "/kn", (lead, 1, side, side), -0.9, 0.9))
    mask = torch.from_numpy(synth.uniform(4, tag + "/m", (lead, 1, side, side), 0.0, 1.0))
    mask[:, :, :3] = 1.0
    mask[:, :, 3:6] = 0.0
    kn = gd._Known(known, mask, shape, DEV)
    t = torch.tensor([1, 3, 7][:B], dtype=torch.int64, device=DEV)
    s, xs = _c_step(hip, d, kind, x, eps, t, nz, kn, nz2)
    ja, jb = d.jump_coefs(3, 4)
    got, gxs = _c_step(hip, d, kind, x, eps, t, nz, kn, nz2, (ja, jb, nz3))
    assert torch.equal(gxs, xs)                                   # pred_xstart is unaffected
    want = ja * s.cpu() + jb * nz3.cpu()
    assert torch.equal(got.cpu(), want)
    assert not torch.equal(got, s)
    # jb == 0 is no jump: the known-row step's bits, whatever ja
    for ja0 in (1.0, 0.5):
        same, _ = _c_step(hip, d, kind, x, eps, t, nz, kn, nz2, (ja0, 0.0, nz3))
        assert torch.equal(same, s), ja0
    # Philox n3: counter (1 << 42) + k of the same key, a fourth stream
    k = 2
    sp, _ = _c_step(hip, d, kind, x, eps, t, None, kn, None, seed=7, counter=k)
    p1, _ = _c_step(hip, d, kind, x, eps, t, None, kn, None, (ja, jb, None), seed=7, counter=k)
    p2, _ = _c_step(hip, d, kind, x, eps, t, None, kn, None, (ja, jb, None), seed=7, counter=k)
    assert torch.equal(p1, p2)
    n3 = torch.empty(shape, device=DEV)
    _lib.check(hip.cfd_randn(_lib.ptr(n3), n3.numel(), 7, (1 << 42) + k, 0, _lib.stream_of(DEV)), "cfd_randn")
    assert torch.equal(p1.cpu(), ja * sp.cpu() + jb * n3.cpu())
    # the public single steps: one table index for the batch, (ja, jb) from jump_coefs
    step = d.ddim_sample if ddim else d.p_sample
    model = _Eps(eps)
    for i, to in ((1, 2), (1, 7), (3, 4), (7, 7)):
        ti = torch.full((B,), i, dtype=torch.int64, device=DEV)
        base = step(model, x, ti, noise=nz, known=known, known_mask=mask, known_noise=nz2)
        out = step(model, x, ti, noise=nz, known=known, known_mask=mask, known_noise=nz2, jump_to=to, jump_noise=nz3)
        a, b = d.jump_coefs(i, to)
        assert torch.equal(out["sample"].cpu(), a * base["sample"].cpu() + b * nz3.cpu()), (i, to)
        assert torch.equal(out["pred_xstart"], base["pred_xstart"])
    ph = step(model, x, ti, seed=7, counter=k, known=known, known_mask=mask, jump_to=7)
    ti_s, _ = _c_step(hip, d, kind, x, eps, ti, None, kn, None, seed=7, counter=k)
    assert torch.equal(ph["sample"].cpu(), a * ti_s.cpu() + b * n3.cpu())


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
@pytest.mark.parametrize("resample,n_rev", [((2, 2), 14), ((3, 3), 20)])
def test_native_resampled_loop_bit_identical_to_python_loop(hip, monkeypatch, tiny, ddim, resample, n_rev):
    """8 levels, 14 and 20 executed steps, B = 3, Philox noise, per-sample known rows and
    a per-sample fractional mask; the host loop without a graph and graphs of 1, 4 and 7
    steps (unrolled graphs plus single-step remainders, jumps at any place in a graph)."""
    d = _diff()
    assert len(gd.resample_schedule(d.num_timesteps, *resample)) == n_rev
    loop = d.ddim_sample_loop if ddim else d.p_sample_loop
    prog = d.ddim_sample_loop_progressive if ddim else d.p_sample_loop_progressive
    known, mask = _known(3)
    mask = mask.repeat(3, 1, 1, 1)
    mask[1, :, 9, ::3] = 0.5
    kw = dict(seed=1234, known=known, known_mask=mask)
    ref = _run(monkeypatch, 0, 1, loop, tiny, (3, 1, S, S), resample=resample, **kw)
    steps = list(prog(tiny, (3, 1, S, S), resample=resample, **kw))
    assert len(steps) == n_rev and torch.equal(steps[-1]["sample"], ref)     # one item per executed step
    for mode, unroll in ((1, 1), (2, 1), (2, 4), (2, 7)):
        got = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), resample=resample, **kw)
        assert torch.equal(got, ref), (resample, mode, unroll, (got - ref).abs().max().item())
    plain = _run(monkeypatch, 2, 4, loop, tiny, (3, 1, S, S), **kw)
    assert torch.equal(plain[:, :, :5], ref[:, :, :5])                      # the fully masked rows end at known
    for b in range(3):
        assert not torch.equal(plain[b, :, 10:], ref[b, :, 10:]), b


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
def test_degenerate_schedules_are_the_known_row_loop(hip, monkeypatch, tiny, ddim):
    d = _diff()
    loop = d.ddim_sample_loop if ddim else d.p_sample_loop
    known, mask = _known(3)
    kw = dict(seed=99, known=known, known_mask=mask)
    for mode, unroll in ((0, 1), (2, 4)):
        ref = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), **kw)
        for resample in ((3, 1), (8, 2)):
            got = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), resample=resample, **kw)
            assert torch.equal(got, ref), (mode, resample)


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
def test_mask_one_ends_at_known_and_row_mask_keeps_rows(hip, monkeypatch, tiny, ddim):
    d = _diff()
    loop = d.ddim_sample_loop if ddim else d.p_sample_loop
    known, mask = _known(3)
    for mode, unroll in ((0, 1), (2, 4)):
        ones = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), seed=5, known=known,
                    known_mask=torch.ones(1, 1, S, S), resample=(2, 2))
        assert torch.equal(ones, known), mode
        rows = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), seed=5, known=known, known_mask=mask,
                    resample=(2, 2))
        assert torch.equal(rows[:, :, :5], known[:, :, :5]), mode
        assert torch.isfinite(rows).all()


def test_resampled_loop_shards(hip, monkeypatch, tiny):
    d = _diff()
    known, mask = _known(3)
    for mode, unroll in ((2, 4), (0, 1)):
        full = _run(monkeypatch, mode, unroll, d.p_sample_loop, tiny, (3, 1, S, S), seed=77, known=known,
                    known_mask=mask, resample=(2, 2))
        for s in range(3):
            one = _run(monkeypatch, mode, unroll, d.p_sample_loop, tiny, (1, 1, S, S), seed=77, sample_offset=s,
                       known=known[s:s + 1], known_mask=mask, resample=(2, 2))
            assert torch.equal(one, full[s:s + 1]), (mode, s)
    other = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, (3, 1, S, S), seed=78, known=known, known_mask=mask,
                 resample=(2, 2))
    assert not torch.equal(other[:, :, 5:], full[:, :, 5:])


def test_resampled_loop_reuses_its_graphs(hip, monkeypatch, tiny):
    """The whole expanded schedule replays the jump step's two graphs (one step, `unroll`
    steps): new known rows, and a repeat with the same (J, r), capture nothing."""
    d = _diff()
    shape = (2, 1, S, S)
    k1, mask = _known(2, "a")
    k2, _ = _known(2, "b")
    r1 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3, known=k1, known_mask=mask, resample=(2, 2))
    c1 = d.native_captures()
    assert c1 == 2
    r2 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3, known=k2, known_mask=mask, resample=(2, 2))
    assert d.native_captures() == c1
    r3 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3, known=k2, known_mask=mask, resample=(2, 2))
    assert d.native_captures() == c1
    assert torch.equal(r3, r2) and not torch.equal(r1, r2)
    assert torch.equal(r1[:, :, :5], k1[:, :, :5]) and torch.equal(r2[:, :, :5], k2[:, :, :5])
    ref2 = _run(monkeypatch, 0, 1, d.p_sample_loop, tiny, shape, seed=3, known=k2, known_mask=mask, resample=(2, 2))
    assert torch.equal(r2, ref2)
    # the plain loop lives next to the resampled one (a rollout alternates: window 0,
    # then resampled windows): going back and forth re-creates and re-captures neither
    p1 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3)
    c2 = d.native_captures()
    assert c2 == c1 + 2 and len(d._natives) == 2
    r4 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3, known=k2, known_mask=mask, resample=(2, 2))
    p2 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3)
    assert d.native_captures() == c2 and len(d._natives) == 2
    assert torch.equal(r4, r2) and torch.equal(p2, p1)
    # another (J, r) replaces the resampled loop only
    _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3, known=k2, known_mask=mask, resample=(3, 3))
    assert len(d._natives) == 2 and d.native_captures() == 4
    assert torch.equal(_run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3), p1)
    assert d.native_captures() == 4


def test_clearing_the_jumps_gives_the_known_row_graphs_back(hip, tiny):
    """cfd_sampler_set_jumps on one sampler: a table of (1, 0) rows runs the jump step's
    graphs and writes the known-row loop's bits; a jumping row changes them; NULL clears
    the jumps, and the run that follows is the known-row loop on the graphs captured
    before (kexec), with no new capture."""
    d = _diff()
    shape = (2, 1, S, S)
    known, mask = _known(2)
    kn = gd._Known(known, mask, shape, DEV)
    n = d.num_timesteps
    tidx = list(range(n))[::-1]
    nl = gd._NativeLoop(tiny, d._sched(DEV, 0.0), tiny._handle(DEV), gd.STEP_DDPM, True, 2, S * S, tidx,
                        d._model_timesteps_host(tidx), True, 4)
    x = torch.from_numpy(synth.normal(11, "clr/x", shape)).to(DEV)

    def run():
        out = torch.empty_like(x)
        nl.run(x, out, 0, n, 21, 0, DEV)
        torch.cuda.synchronize()
        return out

    nl.set_known(kn, d._ktab(DEV), DEV)
    base = run()
    assert nl.captures() == 2
    none = np.tile(np.array([[1.0, 0.0]], dtype=np.float32), (n, 1))
    nl.set_jumps(none)
    assert torch.equal(run(), base) and nl.captures() == 4          # the jump step's own two graphs
    jt = none.copy()
    jt[2] = d.jump_coefs(tidx[2], tidx[2] + 1)
    nl.set_jumps(jt)
    jumped = run()
    assert not torch.equal(jumped[:, :, 5:], base[:, :, 5:]) and torch.equal(jumped[:, :, :5], known[:, :, :5])
    nl.set_jumps(None)
    assert torch.equal(run(), base) and nl.captures() == 4
    nl.set_jumps(jt)
    assert torch.equal(run(), jumped) and nl.captures() == 4


def test_resample_argument_errors(hip, monkeypatch, tiny):
    d = _diff()
    known, mask = _known(2)
    shape = (2, 1, S, S)
    for mode in (0, 2):
        with pytest.raises(ValueError):
            _run(monkeypatch, mode, 4, d.p_sample_loop, tiny, shape, seed=1, resample=(2, 2))
        with pytest.raises(ValueError):
            _run(monkeypatch, mode, 4, d.ddim_sample_loop, tiny, shape, seed=1, resample=(2, 2))
        for bad in ((2,), (2, 2, 2), "ab", 3, (0, 2), (2, 0), (1.5, 2), (2, None)):
            with pytest.raises(ValueError):
                _run(monkeypatch, mode, 4, d.p_sample_loop, tiny, shape, seed=1, known=known, known_mask=mask,
                     resample=bad)
    with pytest.raises(ValueError):
        list(d.p_sample_loop_progressive(tiny, shape, seed=1, resample=(2, 2)))
    x = torch.zeros(shape, device=DEV)
    t0 = torch.zeros(2, dtype=torch.int64, device=DEV)
    t3 = torch.full((2,), 3, dtype=torch.int64, device=DEV)
    for step in (d.p_sample, d.ddim_sample):
        with pytest.raises(ValueError):
            step(tiny, x, t0, seed=1, known=known, known_mask=mask, jump_to=2)         # the clean sample does not jump
        with pytest.raises(ValueError):
            step(tiny, x, t3, seed=1, jump_to=4)                                       # no known rows
        with pytest.raises(ValueError):
            step(tiny, x, t3, seed=1, known=known, known_mask=mask, jump_to=8)         # past the last level
        with pytest.raises(ValueError):
            step(tiny, x, torch.tensor([3, 4], device=DEV), seed=1, known=known, known_mask=mask, jump_to=5)
        with pytest.raises(ValueError):
            step(tiny, x, t3, seed=1, known=known, known_mask=mask, jump_noise=x)      # noise without a jump
    # the guided sampler refuses the keyword
    from confild_amd.guided.condition_methods import get_conditioning_method
    from confild_amd.guided.gaussian_diffusion import create_sampler
    from confild_amd.guided.measurements import get_noise, get_operator
    g = create_sampler(sampler="ddpm", steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                       model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                       rescale_timesteps=False, timestep_respacing="4")
    cond = get_conditioning_method("ps", get_operator("inpainting", device=DEV), get_noise("gaussian", sigma=0.0),
                                   scale=0.5)
    with pytest.raises(ValueError):
        g.p_sample_loop(model=tiny, x_start=x, measurement=mask * known,
                        measurement_cond_fn=functools.partial(cond.conditioning, mask=mask), seed=1, resample=(2, 2))
    # the C loop refuses jumps without known rows
    sched, jtab = d._resampled((2, 2))
    tidx = [i for i, _ in sched]
    nl = gd._NativeLoop(tiny, d._sched(DEV, 0.0), tiny._handle(DEV), gd.STEP_DDPM, True, 2, S * S, tidx,
                        d._model_timesteps_host(tidx), True, 4)
    nl.set_jumps(jtab)
    out = torch.empty_like(x)
    with pytest.raises(_lib.CfdError, match="bad argument"):
        nl.run(x, out, 0, len(tidx), 1, 0, DEV)
    with pytest.raises(ValueError):
        nl.set_jumps(jtab[:-1])
    assert nl.captures() == 0


T, OV, W, SEED = 16, 5, 2, 4242


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_rollout_with_resampling(hip, tiny, sampler):
    """3 windows (window 0 and two conditioned ones), overlap 5, 8 levels, resample (2, 2)."""
    B, rs = 2, (2, 2)
    d = _diff()
    out = rollout.extend_latents(tiny, d, None, W, OV, "replace", seed=SEED, sampler=sampler, batch_size=B,
                                 resample=rs)
    assert out.shape == (B, 1, T + W * (T - OV), T) and torch.isfinite(out).all()
    windows = rollout.plan_windows(T, OV, W)
    plain = _diff()
    loop = plain.p_sample_loop if sampler == "ddpm" else plain.ddim_sample_loop
    assert torch.equal(out[:, :, windows[0]], loop(tiny, (B, 1, T, T), seed=SEED))     # window 0 ignores resample
    for w in range(1, W + 1):
        sl = windows[w]
        known = torch.zeros(B, 1, T, T, device=DEV)
        known[:, :, :OV] = out[:, :, sl.start:sl.start + OV]
        mask = torch.zeros(1, 1, T, T, device=DEV)
        mask[:, :, :OV] = 1.0
        win = loop(tiny, (B, 1, T, T), seed=SEED + w, known=known, known_mask=mask, resample=rs)
        assert torch.equal(out[:, :, sl.start + OV:sl.stop], win[:, :, OV:]), w
        assert torch.equal(win[:, :, :OV], out[:, :, sl.start:sl.start + OV]), w
        unres = loop(tiny, (B, 1, T, T), seed=SEED + w, known=known, known_mask=mask)
        assert not torch.equal(unres[:, :, OV:], win[:, :, OV:]), w
    for s in range(B):
        one = rollout.extend_latents(tiny, d, None, W, OV, "replace", seed=SEED, sampler=sampler, sample_offset=s,
                                     batch_size=1, resample=rs)
        assert torch.equal(one, out[s:s + 1]), s
    one_win = rollout.sample_window(tiny, d, (B, 1, T, T), "replace", seed=SEED, sampler=sampler, resample=rs)
    assert torch.equal(one_win, out[:, :, windows[0]])


def test_rollout_ps_refuses_resampling(hip, tiny):
    from confild_amd.guided.gaussian_diffusion import create_sampler
    g = create_sampler(sampler="ddpm", steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                       model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                       rescale_timesteps=False, timestep_respacing="4")
    with pytest.raises(ValueError):
        rollout.extend_latents(tiny, g, None, 1, OV, "ps", seed=1, resample=(2, 2))
    with pytest.raises(ValueError):
        rollout.sample_window(tiny, g, (1, 1, T, T), "ps", seed=1, resample=(2, 2))
    with pytest.raises(ValueError):
        rollout.extend_latents(tiny, _diff(), None, 1, OV, "replace", seed=1, resample=(2, 2, 2))


def test_inference_driver_jump_keys(hip, tiny, tmp_path):
    """python -m confild_amd.inference with rollout_jump_length / rollout_jump_n_sample: the
    saved array is the decode of extend_latents(resample=) (CPU oracle decode, <= 2e-5, the
    tolerance of test_gpu_rollout.py's driver test); rollout_jump_n_sample absent or 1
    gives the bits of a run without the keys."""
    kw = ast.literal_eval(str(golden("unet_tiny16.npz")["kwargs"]))
    torch.save({k: v.detach().cpu() for k, v in tiny.state_dict().items()}, tmp_path / "ema.pt")
    d, L, c, nh, H, N = 3, 16, 3, 2, 32, 300
    yhi = torch.from_numpy(synth.uniform(5, "yhi", (1, N, c), 0.5, 2.0))
    ssd = synth.siren_state_dict(5, d, L, c, nh, H)
    cnf_dir = tmp_path / "cnf"
    cnf_dir.mkdir()
    torch.save({"x_normalizer_params": (torch.ones(1, d), torch.zeros(1, d)),
                "y_normalizer_params": (yhi, -yhi)}, cnf_dir / "normalizer_params.pt")
    torch.save({"epoch": 1, "model_state_dict": {k: torch.from_numpy(v) for k, v in ssd.items()}},
               cnf_dir / "checkpoint_1.pt")
    coords = synth.uniform(5, "coords", (N, d), 0.0, 1.0)
    np.save(tmp_path / "coords.npy", coords)
    cnf_cfg = {"save_path": str(cnf_dir), "coor_path": str(tmp_path / "coords.npy"), "lumped_latent": True,
               "normalizer": {"method": "-11", "dim": 0}, "multiGPU": 1, "hidden_size": L, "dims": d,
               "NF": {"name": "SIRENAutodecoder_film", "out_features": c, "num_hidden_layers": nh,
                      "hidden_features": H}}
    (tmp_path / "cnf.yml").write_text(yaml.safe_dump(cnf_cfg))
    np.save(tmp_path / "max.npy", np.float32(1.5))
    np.save(tmp_path / "min.npy", np.float32(-1.5))
    B = 2
    cfg = {"test_batch_size": B, "time_length": T, "latent_length": T, "image_size": T,
           "num_channels": kw["num_channels"], "num_res_blocks": kw["num_res_blocks"],
           "channel_mult": kw["channel_mult"], "num_heads": kw["num_heads"],
           "num_head_channels": kw["num_head_channels"], "attention_resolutions": kw["attention_resolutions"],
           "ema_path": str(tmp_path / "ema.pt"), "steps": 1000, "noise_schedule": "cosine",
           "timestep_respacing": "4", "max_val": str(tmp_path / "max.npy"), "min_val": str(tmp_path / "min.npy"),
           "cnf_case_file_path": str(tmp_path / "cnf.yml"), "save_path": str(tmp_path / "out.npy"),
           "rollout_windows": W, "rollout_overlap": OV, "rollout_method": "replace",
           "rollout_jump_length": 2, "rollout_jump_n_sample": 2}

    def drive():
        (tmp_path / "case.yml").write_text(yaml.safe_dump(cfg))
        return inference.run(str(tmp_path / "case.yml"))

    out = drive()
    saved = np.load(tmp_path / "out.npy")
    total = T + W * (T - OV)
    assert saved.shape == (B * total, N, c) and np.array_equal(saved, out)
    torch.manual_seed(42)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    lat = rollout.extend_latents(tiny, _diff("4"), None, W, OV, "replace", seed=seed, batch_size=B,
                                 resample=(2, 2))[:, 0]
    lat = ((lat + 1) * (1.5 + 1.5) / 2. - 1.5).reshape(B * total, T).cpu()
    ref = osn.decode({k: torch.from_numpy(v) for k, v in ssd.items()}, torch.from_numpy(coords), lat,
                     torch.ones(1, d), torch.zeros(1, d), yhi, -yhi)
    err = np.abs(saved - ref.numpy()).max()
    print("driver against the oracle decode:", err, "scale", float(ref.abs().max()))
    assert err <= 2e-5 * max(1.0, float(ref.abs().max()))
    # the jumps are off by default
    del cfg["rollout_jump_n_sample"]
    off = drive()
    cfg["rollout_jump_n_sample"] = 1
    one = drive()
    del cfg["rollout_jump_n_sample"], cfg["rollout_jump_length"]
    none = drive()
    assert np.array_equal(off, none) and np.array_equal(one, none)
    assert np.array_equal(none[:T], out[:T]) and not np.array_equal(none, out)     # window 0 has no jumps
    cfg.update(rollout_method="ps", rollout_jump_n_sample=2)
    with pytest.raises(ValueError):
        drive()


DEBUG_CHILD = r"""
import ast, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from confild_amd import synth
from confild_amd.script_util import create_gaussian_diffusion, create_model
g = np.load(sys.argv[1] + "/tests/golden/unet_tiny16.npz")
m = create_model(**ast.literal_eval(str(g["kwargs"])))
m.load_state_dict({k: torch.from_numpy(v) for k, v in
                   synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in m.state_dict().items()}).items()})
dev = torch.device("cuda", 0)
m.to(dev)
known = torch.from_numpy(synth.uniform(9, "k/known", (3, 1, 16, 16), -0.9, 0.9)).to(dev)
mask = torch.zeros(1, 1, 16, 16, device=dev)
mask[:, :, :5] = 1.0
d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="8")
out = d.p_sample_loop(m, (3, 1, 16, 16), seed=1234, known=known, known_mask=mask, resample=(2, 2))
torch.cuda.synchronize()
assert d.native_captures() == 2
np.save(sys.argv[2], out.cpu().numpy())
"""


def test_debug_library_runs_the_resampled_graph_loop(hip, tiny, tmp_path):
    """The 14-step native loop on the bounds-checked build (CFD_DASSERT on the jump
    table's row, and every check of the U-Net's kernels), in a child process: it exits
    clean, no assertion fires, and the final sample has the shipped library's bits."""
    if not os.path.exists(DEBUG_SO):
        pytest.skip("debug build absent (make -C confild_amd/csrc DEBUG=1)")
    env = dict(os.environ, CFD_LIB="libconfild_hip_debug.so", CFD_SAMPLER="2", CFD_SAMPLER_UNROLL="4")
    path = str(tmp_path / "dbg.npy")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD, ROOT, path], capture_output=True, text=True, env=env,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CFD_DASSERT" not in r.stdout + r.stderr
    dbg = torch.from_numpy(np.load(path))
    known, mask = _known(3)
    rel = _diff().p_sample_loop(tiny, (3, 1, S, S), seed=1234, known=known, known_mask=mask, resample=(2, 2)).cpu()
    err = (dbg - rel).abs().max().item()
    print("debug build against the shipped library:", err)
    assert torch.equal(dbg[:, :, :5], known[:, :, :5].cpu())
    assert torch.equal(dbg, rel)
