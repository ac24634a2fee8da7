"""GPU: known-row replacement in the unconditioned loops (cfd_sched_step_known,
cfd_sampler_set_known; GaussianDiffusion.*(known=, known_mask=, known_noise=)).

After its sample s, the step at table index i writes
    q = a_i * known + b_i * n2,   out = m * q + (1 - m) * s
(a_i, b_i) = (sqrt(abar_prev[i]), sqrt(1 - abar_prev[i])) as fp32, contraction off.
Everything here is bit-exact: the step against the same fp32 expression evaluated
by torch on the CPU (IEEE multiplies and adds in the stated order), the native
graph loop against the Python loop, a sharded batch against the unsharded one, a
zero mask against the loops without known rows.
"""
import ast

import pytest
import torch

from conftest import golden
from confild_amd import gaussian_diffusion as gd
from confild_amd import synth
from confild_amd.script_util import create_gaussian_diffusion, create_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
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


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
@pytest.mark.parametrize("B,n,shared", [(3, 256, True), (3, 256, False), (2, 576, True), (2, 576, False)])
def test_known_step_is_the_stated_expression(hip, ddim, B, n, shared):
    """B * n = 768 and 1152 elements; table indices 0 (q == known), 3 and 7; a
    fractional mask; explicit noise and known_noise."""
    d = _diff()
    side = {256: 16, 576: 24}[n]
    shape = (B, 1, side, side)
    tag = f"ks/{n}"
    x = torch.from_numpy(synth.normal(4, tag + "/x", shape)).to(DEV)
    eps = torch.from_numpy(synth.normal(4, tag + "/eps", shape)).to(DEV)
    nz = torch.from_numpy(synth.normal(4, tag + "/nz", shape))
    nz2 = torch.from_numpy(synth.normal(4, tag + "/nz2", shape))
    lead = 1 if shared else B
    known = torch.from_numpy(synth.uniform(4, tag + "/kn", (lead, 1, side, side), -0.9, 0.9))
    mask = torch.from_numpy(synth.uniform(4, tag + "/m", (lead, 1, side, side), 0.0, 1.0))
    mask[:, :, :3] = 1.0
    mask[:, :, 3:6] = 0.0
    t = torch.tensor([0, 3, 7][:B], dtype=torch.int64, device=DEV)
    step = d.ddim_sample if ddim else d.p_sample
    model = _Eps(eps)
    plain = step(model, x, t, noise=nz)
    got = step(model, x, t, noise=nz, known=known, known_mask=mask, known_noise=nz2)
    assert torch.equal(got["pred_xstart"], plain["pred_xstart"])
    s = plain["sample"].cpu()
    tab = d.known_table()[t.cpu()]
    a, b = tab[:, 0].reshape(B, 1, 1, 1), tab[:, 1].reshape(B, 1, 1, 1)
    q = a * known + b * nz2
    want = mask * q + (1.0 - mask) * s
    assert torch.equal(got["sample"].cpu(), want)
    g = got["sample"].cpu()
    assert torch.equal(g[:, :, :3][0], (known.expand(B, -1, -1, -1))[0, :, :3])       # index 0, mask 1: known itself
    assert torch.equal(g[:, :, 3:6], s[:, :, 3:6])                                    # mask 0: the sample's bits
    # Philox n2: counter (1 << 41) + k of the same key, another stream than the step's own
    p1 = step(model, x, t, seed=7, counter=2, known=known, known_mask=mask)
    p2 = step(model, x, t, seed=7, counter=2, known=known, known_mask=mask)
    assert torch.equal(p1["sample"], p2["sample"])
    n2 = torch.empty(shape, device=DEV)
    from confild_amd import _lib
    _lib.check(hip.cfd_randn(_lib.ptr(n2), n2.numel(), 7, (1 << 41) + 2, 0, _lib.stream_of(DEV)), "cfd_randn")
    sp = step(model, x, t, seed=7, counter=2)["sample"].cpu()
    want = mask * (a * known + b * n2.cpu()) + (1.0 - mask) * sp
    assert torch.equal(p1["sample"].cpu(), want)


def test_known_argument_errors(hip, tiny):
    d = _diff("4")
    known, mask = _known(2)
    with pytest.raises(ValueError):
        d.p_sample_loop(tiny, (2, 1, S, S), seed=1, known=known)
    with pytest.raises(ValueError):
        d.p_sample_loop(tiny, (2, 1, S, S), seed=1, known=known, known_mask=torch.ones(3, 1, S, S))
    with pytest.raises(ValueError):
        d.p_sample_loop(tiny, (2, 1, S, S), seed=1, known=known[:, :, :8], known_mask=mask)
    with pytest.raises(ValueError):
        d.p_sample_loop(tiny, (2, 1, S, S), seed=1, known_noise=torch.zeros(4, 2, 1, S, S))


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
def test_mask_zero_is_the_unconditioned_loop(hip, monkeypatch, tiny, ddim):
    d = _diff()
    loop = d.ddim_sample_loop if ddim else d.p_sample_loop
    known, _ = _known(3)
    zero = torch.zeros(1, 1, S, S)
    for mode, unroll in ((0, 1), (2, 4)):
        ref = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), seed=1234)
        got = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), seed=1234, known=known, known_mask=zero)
        assert torch.equal(got, ref), mode


@pytest.mark.parametrize("ddim", [False, True], ids=["ddpm", "ddim"])
def test_mask_one_ends_at_known_and_row_mask_keeps_rows(hip, monkeypatch, tiny, ddim):
    d = _diff()
    loop = d.ddim_sample_loop if ddim else d.p_sample_loop
    known, mask = _known(3)
    for mode, unroll in ((0, 1), (2, 4)):
        ones = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), seed=5, known=known,
                    known_mask=torch.ones(1, 1, S, S))
        assert torch.equal(ones, known), mode
        plain = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), seed=5)
        rows = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), seed=5, known=known, known_mask=mask)
        assert torch.equal(rows[:, :, :5], known[:, :, :5]), mode
        assert torch.isfinite(rows).all()
        for b in range(3):
            assert not torch.equal(rows[b, :, 5:], plain[b, :, 5:]), (mode, b)


@pytest.mark.parametrize("respacing,ddim", [("8", False), ("8", True), ("10,20,30", False)])
def test_native_known_loop_bit_identical_to_python_loop(hip, monkeypatch, tiny, respacing, ddim):
    """8 steps (and 60: the loop crosses no range-check boundary; unrolled graphs plus
    single-step remainders at unroll 7), B = 3, Philox noise, per-sample known rows
    and a per-sample fractional mask."""
    d = _diff(respacing)
    loop = d.ddim_sample_loop if ddim else d.p_sample_loop
    known, mask = _known(3)
    mask = mask.repeat(3, 1, 1, 1)
    mask[1, :, 9, ::3] = 0.5
    ref = _run(monkeypatch, 0, 1, loop, tiny, (3, 1, S, S), seed=1234, known=known, known_mask=mask)
    for mode, unroll in ((1, 1), (2, 1), (2, 4), (2, 7)):
        got = _run(monkeypatch, mode, unroll, loop, tiny, (3, 1, S, S), seed=1234, known=known, known_mask=mask)
        assert torch.equal(got, ref), (respacing, mode, unroll, (got - ref).abs().max().item())
    # explicit known_noise takes the Python loop and differs from the Philox run
    kn = torch.from_numpy(synth.normal(6, "kn", (d.num_timesteps, 3, 1, S, S)))
    a = _run(monkeypatch, 2, 4, loop, tiny, (3, 1, S, S), seed=1234, known=known, known_mask=mask, known_noise=kn)
    b = _run(monkeypatch, 0, 1, loop, tiny, (3, 1, S, S), seed=1234, known=known, known_mask=mask, known_noise=kn)
    assert torch.equal(a, b) and not torch.equal(a, ref)


def test_known_loop_shards_and_repeats(hip, monkeypatch, tiny):
    d = _diff()
    known, mask = _known(3)
    for mode, unroll in ((2, 4), (0, 1)):
        full = _run(monkeypatch, mode, unroll, d.p_sample_loop, tiny, (3, 1, S, S), seed=77, known=known,
                    known_mask=mask)
        again = _run(monkeypatch, mode, unroll, d.p_sample_loop, tiny, (3, 1, S, S), seed=77, known=known,
                     known_mask=mask)
        assert torch.equal(full, again)
        for s in range(3):
            one = _run(monkeypatch, mode, unroll, d.p_sample_loop, tiny, (1, 1, S, S), seed=77, sample_offset=s,
                       known=known[s:s + 1], known_mask=mask)
            assert torch.equal(one, full[s:s + 1]), (mode, s)
    other = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, (3, 1, S, S), seed=78, known=known, known_mask=mask)
    assert not torch.equal(other[:, :, 5:], full[:, :, 5:])


def test_set_known_reuses_the_graphs(hip, monkeypatch, tiny):
    """New known rows are copied into the sampler's buffers: no capture after the
    first conditioned run; clearing them gives the unconditioned bits back, on the
    unconditioned graphs captured before."""
    d = _diff()
    shape = (2, 1, S, S)
    plain = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3)
    c0 = d.native_captures()
    assert c0 == 2                                        # one step, and `unroll` steps
    k1, mask = _known(2, "a")
    k2, _ = _known(2, "b")
    r1 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3, known=k1, known_mask=mask)
    c1 = d.native_captures()
    assert c1 == 4                                        # the conditioned step's own two graphs
    r2 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3, known=k2, known_mask=mask)
    m2 = mask.clone()
    m2[:, :, 8:10] = 1.0
    r3 = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3, known=k2, known_mask=m2)
    assert d.native_captures() == c1
    assert torch.equal(r1[:, :, :5], k1[:, :, :5]) and torch.equal(r2[:, :, :5], k2[:, :, :5])
    assert torch.equal(r3[:, :, 8:10], k2[:, :, 8:10]) and not torch.equal(r3[:, :, 8:10], r2[:, :, 8:10])
    assert not torch.equal(r1, r2)
    ref2 = _run(monkeypatch, 0, 1, d.p_sample_loop, tiny, shape, seed=3, known=k2, known_mask=mask)
    assert torch.equal(r2, ref2)
    back = _run(monkeypatch, 2, 4, d.p_sample_loop, tiny, shape, seed=3)
    assert torch.equal(back, plain)
    assert d.native_captures() == c1
