"""GPU parity of the dense / masked DPS adjoint (cfd_siren_dense_grad)
and of the guided loop with the case2 / case3 / case3_gappy operators.

Bounds (none is a free number):
* g_z against an fp64 autograd evaluation of the oracle: at most 2x the error of the
  present tape_forward / tape_vjp route on the same problem, seeded with the fp64
  d(sum of norms)/dA cast to fp32, plus 1e-7 of the gradient's maximum;
* norms within 1e-4 max(1, norm), the bound test_gpu_dps.py uses for distances;
* the guided loop: the tolerances of test_gpu_dps.py::test_dps_loop_matches_reference;
* budget, batch and repeat invariance: torch.equal.
"""
import ast
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from confild_amd import _lib, synth
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts
from oracle import siren as osn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SHAPES = {   # (d, L, c, nh, H), N, R, T: N is never a multiple of 16 (tiles end inside a row)
    "h128": ((2, 32, 4, 3, 128), 203, 6, 3),
    "case2w": ((2, 64, 4, 10, 256), 203, 6, 3),
    "case3w": ((2, 64, 2, 17, 256), 27, 4, 2),
    "case4w": ((3, 64, 3, 15, 384), 45, 4, 4),
}


def _problem(dims, N, R, T, seed=51):
    d, L, c, nh, H = dims
    sd_np = synth.siren_state_dict(seed, d, L, c, nh, H)
    p = dict(dims=dims, N=N, R=R, T=T, sd_np=sd_np)
    p["coords"] = torch.from_numpy(synth.uniform(seed, "c", (N, d), -0.5, 2.0))
    p["xhi"], p["xlo"] = torch.full((1, d), 2.2), torch.full((1, d), -0.7)
    p["yhi"] = torch.from_numpy(synth.uniform(seed, "yhi", (c,), 0.5, 2.0))
    p["ylo"] = -p["yhi"]
    p["z"] = torch.from_numpy(synth.normal(seed, "z", (R, L))) * 0.5
    p["y"] = {"shared": torch.from_numpy(synth.normal(seed, "ys", (T, N, c))),
              "per_sample": torch.from_numpy(synth.normal(seed, "yp", (R, N, c)))}
    bits = lambda tag, shape: torch.from_numpy((synth.uniform(seed, tag, shape, 0., 1.) < 0.6).astype(np.float32))  # noqa: E731
    p["mask"] = {"none": None, "table": bits("m1", (N, c)), "rows": bits("mT", (T, N, c)), "all": bits("mR", (R, N, c))}
    return p


def _rows_of(t, R, N, c):
    """(R, N, c) view of 1 / T / R tables: row r reads table r % rows."""
    t = t.reshape(-1, N, c)
    return t.repeat(R // t.shape[0], 1, 1)


def _fp64_reference(p, yk, mk):
    """norms (B), d sum(norms) / d z (R, L) and d sum(norms) / d A (R, N, c) in fp64."""
    d, L, c, nh, H = p["dims"]
    N, R, T = p["N"], p["R"], p["T"]
    sd64 = {k: torch.from_numpy(v).double() for k, v in p["sd_np"].items()}
    z64 = p["z"].double().requires_grad_()
    A = osn.decode(sd64, p["coords"].double(), z64, p["xhi"].double(), p["xlo"].double(), p["yhi"].double(),
                   p["ylo"].double())
    y = _rows_of(p["y"][yk].double(), R, N, c)
    m = torch.ones(R, N, c, dtype=torch.float64) if p["mask"][mk] is None else _rows_of(p["mask"][mk].double(), R, N, c)
    norms = torch.linalg.norm((y - m * A).reshape(R // T, -1), dim=1)
    gz, gA = torch.autograd.grad(norms.sum(), (z64, A))
    return norms.detach(), gz.detach(), gA.detach()


def _module(p, mode, form=("sum", "auto")):
    d, L, c, nh, H = p["dims"]
    nf = SIRENAutodecoder_film(d, L, c, nh, H)
    nf.load_state_dict({k: torch.from_numpy(v) for k, v in p["sd_np"].items()})
    nf.to(DEV).set_compute(mode).set_dense_form(*form)
    xn = Normalizer_ts(params=(p["xhi"], p["xlo"]), method="-11", dim=0)
    yn = Normalizer_ts(params=(p["yhi"], p["ylo"]), method="-11", dim=0)
    return nf, xn, yn


def _dense(nf, xn, yn, p, yk, mk, budget=None, rows=None):
    rows = slice(None) if rows is None else rows
    y = p["y"][yk] if yk == "shared" else p["y"][yk][rows]
    m = p["mask"][mk]
    if mk == "all":
        m = m[rows]
    return nf.dense_grad(p["coords"].to(DEV), p["z"][rows].to(DEV), p["T"], y.to(DEV), None if m is None else m.to(DEV),
                         xn, yn, budget)


@pytest.fixture(scope="module")
def references():
    """The fp64 references, computed once per (shape, y, mask) and left unchanged."""
    cache = {}

    def get(shape, yk, mk):
        key = (shape, yk, mk)
        if key not in cache:
            dims, N, R, T = SHAPES[shape]
            cache[key] = _fp64_reference(_problem(dims, N, R, T), yk, mk)
        return cache[key]
    return get


_PARITY = [(shape, mode, ("sum", "auto")) for shape in SHAPES for mode in ("f32", "split_f16")]
# the other forms at the Case2 widths: the K9t delta tape, and the fp32 delta tape
# (what a handle runs whose on-chip sums do not fit in LDS)
_PARITY += [("case2w", "split_f16", ("delta", "auto")), ("case2w", "f32", ("delta", "f32"))]


@pytest.mark.parametrize("shape,mode,form", _PARITY, ids=[f"{s}-{m}-{f[0]}" for s, m, f in _PARITY])
def test_dense_grad_matches_fp64_autograd(hip, references, shape, mode, form):
    dims, N, R, T = SHAPES[shape]
    p = _problem(dims, N, R, T)
    nf, xn, yn = _module(p, mode, form)
    for yk in ("shared", "per_sample"):
        for mk in ("none", "table", "rows", "all"):
            norms64, gz64, gA64 = references(shape, yk, mk)
            # the present route on the same problem, seeded with the fp64 gradient cast to fp32
            nf.tape_forward(p["coords"].to(DEV), p["z"].to(DEV), xn, yn)
            e_tape = float((nf.tape_vjp(gA64.float().to(DEV)).cpu().double() - gz64).abs().max())
            gz, norms = _dense(nf, xn, yn, p, yk, mk)
            e_dense = float((gz.cpu().double() - gz64).abs().max())
            gmax = float(gz64.abs().max())
            en = (norms.cpu().double() - norms64).abs() / norms64.clamp(min=1.0)
            print(f"{shape} {mode} y={yk} mask={mk}: g_z error dense {e_dense:.3e} tape {e_tape:.3e} "
                  f"(max {gmax:.3e}); norm error {float(en.max()):.3e}")
            assert e_dense <= 2 * e_tape + 1e-7 * gmax, (yk, mk, e_dense, e_tape, gmax)
            assert float(en.max()) < 1e-4, (yk, mk, norms, norms64)


_FORM_IDS = {"sum": 0, "delta": 1, "auto": 0, "f32": 1}


def _plan(nf, N, R, budget, form=("sum", "auto")):
    cfg = _lib.SirenCfg(nf.in_coord_features, nf.in_latent_features, nf.out_features, nf.num_hidden_layers,
                        nf.hidden_features, nf.w0)
    b, pts, rows = C.c_size_t(), C.c_int64(), C.c_int()
    _lib.check(_lib.load().cfd_siren_dense_plan(C.byref(cfg), N, R, budget, _FORM_IDS[form[0]],
                                                _FORM_IDS[form[1]], C.byref(b), C.byref(pts), C.byref(rows)), "cfd_siren_dense_plan")
    return b.value, pts.value, rows.value


FORMS = [("sum", "auto"), ("delta", "auto"), ("sum", "f32"), ("delta", "f32")]
FORM_NAMES = ["sum-k9t", "delta-k9t", "sum-f32", "delta-f32"]      # the first is the default in split compute


@pytest.mark.parametrize("form", FORMS, ids=FORM_NAMES)
def test_dense_grad_bits_do_not_depend_on_budget_or_batch(hip, form):
    dims, N, R, T = (2, 64, 4, 10, 256), 2500, 6, 3
    p = _problem(dims, N, R, T, seed=52)
    nf, xn, yn = _module(p, "split_f16", form)
    fid = form
    MiB = 1 << 20
    budgets = {"one chunk": None, "several chunks": 64 * MiB, "many chunks": 24 * MiB, "row blocks": 3 * MiB}
    # what the budgets make the planner do (all R rows, and one sample's rows)
    _, pts, rows = _plan(nf, N, R, 0, fid)
    assert pts >= N and rows == R
    _, pts, rows = _plan(nf, N, R, 64 * MiB, fid)
    assert rows == R and -(-N // pts) >= 3 and N % pts != 0      # >= 3 chunks, a short last one
    _, pts2, rows = _plan(nf, N, R, 24 * MiB, fid)
    assert rows == R and pts2 < pts
    _, pts3, rows = _plan(nf, N, R, 3 * MiB, fid)
    assert pts3 == 64 and rows < R
    out = {k: _dense(nf, xn, yn, p, "per_sample", "rows", b) for k, b in budgets.items()}
    gz, norms = out["one chunk"]
    assert torch.isfinite(gz).all() and float(gz.abs().max()) > 0 and (norms > 0).all()
    for k, (g, n) in out.items():
        assert torch.equal(g, gz) and torch.equal(n, norms), k
    # two samples in one call equal the two single-sample calls (at another budget each)
    for s, b in ((0, 64 * MiB), (1, None)):
        g, n = _dense(nf, xn, yn, p, "per_sample", "rows", b, rows=slice(s * T, (s + 1) * T))
        assert torch.equal(g, gz[s * T:(s + 1) * T]) and torch.equal(n, norms[s:s + 1]), s
    # and a repeat equals itself
    g, n = _dense(nf, xn, yn, p, "per_sample", "rows", None)
    assert torch.equal(g, gz) and torch.equal(n, norms)


def test_budget_too_small_is_an_argument_error(hip):
    dims, N, R, T = SHAPES["h128"]
    p = _problem(dims, N, R, T)
    nf, xn, yn = _module(p, "f32")
    with pytest.raises(_lib.CfdError, match="budget"):
        _dense(nf, xn, yn, p, "shared", "none", budget=4096)


def test_all_ones_mask_agrees_with_the_case4_route(hip, references):
    """A Case4-shaped problem (10 sensors, H = 384): dense_grad with an all-ones mask
    against the present route end to end (tape_forward, cfd_dps_residual, tape_vjp).
    The two gradients differ by at most bound 1's figure, 2 e_tape + 1e-7 max, e_tape
    the present route's own error against the fp64 gradient; and the dense gradient's
    error against fp64 is within the same figure."""
    dims, N, R, T = (3, 64, 3, 15, 384), 10, 24, 12
    p = _problem(dims, N, R, T, seed=53)
    p["mask"]["table"] = torch.ones(N, dims[2])
    norms64, gz64, gA64 = _fp64_reference(p, "shared", "none")
    for mode in ("f32", "split_f16"):
        nf, xn, yn = _module(p, mode)
        A = nf.tape_forward(p["coords"].to(DEV), p["z"].to(DEV), xn, yn)
        # the present route end to end: cfd_dps_residual's seed from its own A
        gA = torch.empty_like(A)
        dist = torch.empty(R // T, device=DEV)
        y = p["y"]["shared"].to(DEV).contiguous()
        _lib.check(_lib.lib().cfd_dps_residual(_lib.ptr(y), 0, _lib.ptr(A), _lib.ptr(gA), _lib.ptr(dist),
                                               T * N * dims[2], R // T, _lib.stream_of(DEV)), "cfd_dps_residual")
        gz_tape = nf.tape_vjp(gA)
        e_tape = float((gz_tape.cpu().double() - gz64).abs().max())
        gmax = float(gz64.abs().max())
        for mk in ("none", "table"):
            gz, norms = _dense(nf, xn, yn, p, "shared", mk)
            diff = float((gz - gz_tape).abs().max())
            e_dense = float((gz.cpu().double() - gz64).abs().max())
            print(f"{mode} mask={mk}: dense vs tape {diff:.3e}, dense error {e_dense:.3e}, tape error {e_tape:.3e}, "
                  f"max {gmax:.3e}")
            assert diff <= 2 * e_tape + 1e-7 * gmax, (mode, mk, diff, e_tape)
            assert e_dense <= 2 * e_tape + 1e-7 * gmax, (mode, mk, e_dense, e_tape)
            assert float(((norms - dist).abs() / dist.clamp(min=1.0)).max()) < 1e-4
            assert float(((norms.cpu().double() - norms64).abs() / norms64.clamp(min=1.0)).max()) < 1e-4


# ---------------------------------------------------------------------------
# the guided loop vs the reference's recorded masked runs
# ---------------------------------------------------------------------------
def _dense_setup(name):
    from confild_amd.guided import measurements as ms
    from confild_amd.guided.condition_methods import get_conditioning_method
    from confild_amd.guided.gaussian_diffusion import create_sampler
    from confild_amd.guided.unet import create_model as guided_model
    g = golden(f"{name}.npz")
    kw = ast.literal_eval(str(g["kwargs"]))
    model = guided_model(**kw)
    sd = synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.to(DEV)
    d, L, c, nh, H = (int(v) for v in g["siren_dims"])
    nf = SIRENAutodecoder_film(d, L, c, nh, H)
    nf.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(int(g["siren_seed"]), d, L, c, nh,
                                                                                   H).items()})
    T = lambda k: torch.from_numpy(g[k])  # noqa: E731
    cls = {"case2": ms.Case2Operator, "case3": ms.Case3Operator}[str(g["operator"])]
    op = cls.from_parts(DEV, T("coords"), Normalizer_ts(params=(T("xhi"), T("xlo")), method="-11", dim=0),
                        Normalizer_ts(params=(T("yhi"), T("ylo")), method="-11", dim=0), nf, T("vmax"), T("vmin"),
                        batch_size=int(g["op_batch"]))
    cond = get_conditioning_method(operator=op, noiser=ms.get_noise(sigma=0.0, name="gaussian"), name="ps",
                                   scale=float(g["scale"]))
    sampler = create_sampler(sampler="ddpm", steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                             model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                             rescale_timesteps=False, timestep_respacing=str(g["respacing"]))
    return g, model, op, cond, sampler


@pytest.mark.parametrize("name", ["dps_dense_case2", "dps_dense_case3gappy"])
def test_masked_dps_loop_matches_reference(hip, name):
    g, model, op, cond, sampler = _dense_setup(name)
    y = torch.from_numpy(g["measurement"]).to(DEV)
    mask = torch.from_numpy(g["mask"])
    A = op.forward(torch.from_numpy(g["x_true"]).to(DEV), mask=mask).cpu().numpy()
    assert np.abs(A - g["measurement"]).max() < 2e-5 * max(1.0, np.abs(g["measurement"]).max())
    steps = len(g["img"])
    fn = functools.partial(cond.conditioning, mask=mask)
    for k in range(steps):
        xin = torch.from_numpy(g["x_start"] if k == 0 else g["img"][k - 1]).to(DEV)
        out = sampler.p_sample_step(model, xin, steps - 1 - k, y, fn, noise=torch.from_numpy(g["step_noise"][k]))
        lat = max(1.0, float(np.abs(g["img"][k]).max()))
        for key, ref in (("pred_xstart", g["x0"][k]), ("x_t", g["sample"][k]), ("sample", g["img"][k])):
            err = float(np.abs(out[key].cpu().numpy() - ref).max()) / lat
            assert err < 1e-4, (k, key, err)
        assert abs(float(out["distance"][0]) - g["dist"][k]) < 1e-4 * max(1.0, g["dist"][k])
    x = torch.from_numpy(g["x_start"]).to(DEV)
    out = sampler.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=fn, record=False,
                                save_root=None, step_noise=torch.from_numpy(g["step_noise"]))
    err = float(np.abs(out.cpu().numpy() - g["out"]).max()) / max(1.0, float(np.abs(g["out"]).max()))
    assert err < 5e-4, err
    dist = sampler.distances[:, 0].cpu().numpy()
    assert np.abs(dist - g["dist"]).max() < 1e-3 * max(1.0, g["dist"].max())


def test_gappy_operator_applies_its_own_mask(hip):
    """case3_gappy without a mask keyword runs what Case3 runs with the gappy table."""
    from confild_amd.guided import measurements as ms
    g, model, op, cond, sampler = _dense_setup("dps_dense_case3gappy")
    gop = ms.Case3Operator_gappy.from_parts(DEV, op.coords, op.x_normalizer, op.y_normalizer, op.model, op.max_val,
                                            op.min_val)
    assert np.array_equal(gop.default_mask().cpu().numpy(), g["mask"])
    x_true = torch.from_numpy(g["x_true"]).to(DEV)
    assert torch.equal(gop.forward(x_true), op.forward(x_true, mask=torch.from_numpy(g["mask"])))
    from confild_amd.guided.condition_methods import get_conditioning_method
    gcond = get_conditioning_method(operator=gop, noiser=ms.get_noise(sigma=0.0, name="gaussian"), name="ps",
                                    scale=float(g["scale"]))
    y = torch.from_numpy(g["measurement"]).to(DEV)
    x = torch.from_numpy(g["x_start"]).to(DEV)
    nz = torch.from_numpy(g["step_noise"][0])
    a = sampler.p_sample_step(model, x, 5, y, functools.partial(gcond.conditioning), noise=nz)
    b = sampler.p_sample_step(model, x, 5, y, functools.partial(cond.conditioning, mask=torch.from_numpy(g["mask"])),
                              noise=nz)
    assert torch.equal(a["sample"], b["sample"]) and torch.equal(a["distance"], b["distance"])


def test_all_zero_mask_gives_zero_norm_and_no_guidance(hip):
    g, model, op, cond, sampler = _dense_setup("dps_dense_case2")
    y = torch.zeros_like(torch.from_numpy(g["measurement"])).to(DEV)
    fn = functools.partial(cond.conditioning, mask=torch.zeros(g["mask"].shape))
    x = torch.from_numpy(g["x_start"]).to(DEV)
    out = sampler.p_sample_step(model, x, 5, y, fn, noise=torch.from_numpy(g["step_noise"][0]))
    assert float(out["distance"][0]) == 0.0
    assert torch.isfinite(out["sample"]).all()
    assert torch.equal(out["sample"], out["x_t"])               # img == sample: no guidance
    gz, norms = op.dense_grad(out["pred_xstart"], y, torch.zeros(g["mask"].shape))
    assert float(norms[0]) == 0.0 and not gz.any() and torch.isfinite(gz).all()


def test_masked_chains_in_a_batch_equal_single_chains(hip):
    g, model, op, cond, sampler = _dense_setup("dps_dense_case2")
    mask = torch.from_numpy(g["mask"])
    fn = functools.partial(cond.conditioning, mask=mask)
    xs = torch.from_numpy(synth.normal(3, "dense/xs", (3, 1, 16, 16))).to(DEV)
    # a measurement per sample, one mask shared by the samples
    xt = torch.from_numpy(synth.uniform(3, "dense/xt", (3, 1, 16, 16), -0.9, 0.9)).to(DEV)
    y = op.forward(xt, mask=mask.repeat(3, 1, 1))              # (3*16, 37, 4)
    per = y.shape[0] // 3
    full = sampler.p_sample_loop(model=model, x_start=xs, measurement=y, measurement_cond_fn=fn, seed=99)
    dfull = sampler.distances.clone()
    for s in range(3):
        one = sampler.p_sample_loop(model=model, x_start=xs[s:s + 1], measurement=y[s * per:(s + 1) * per],
                                    measurement_cond_fn=fn, seed=99, sample_offset=s)
        assert torch.equal(one, full[s:s + 1]), s
        assert torch.equal(sampler.distances[:, 0], dfull[:, s]), s
    assert torch.isfinite(full).all() and (dfull > 0).all()


def test_case4_without_a_mask_keeps_its_bits(hip):
    """Case4Operator without a mask runs the tape route as before: the loop's output
    and distances on dps_tiny16 equal the bits recorded from the library before the
    dense path existed (tests/golden/dps_case4_pinned.npz, written by
    tests/golden/make_pinned_case4.py from a checkout of that commit)."""
    from test_gpu_dps import _dps_setup
    g, model, op, cond, sampler = _dps_setup("dps_tiny16")
    pin = golden("dps_case4_pinned.npz")
    y = torch.from_numpy(g["measurement"]).to(DEV)
    fn = functools.partial(cond.conditioning)
    out = sampler.p_sample_loop(model=model, x_start=torch.from_numpy(g["x_start"]).to(DEV), measurement=y,
                                measurement_cond_fn=fn, step_noise=torch.from_numpy(g["step_noise"]))
    assert np.array_equal(out.cpu().numpy(), pin["out_noise"])
    assert np.array_equal(sampler.distances.cpu().numpy(), pin["dist_noise"])
    xs = torch.from_numpy(synth.normal(3, "dps/xs", (3, 1, 16, 16))).to(DEV)
    out = sampler.p_sample_loop(model=model, x_start=xs, measurement=y, measurement_cond_fn=fn, seed=99)
    assert np.array_equal(out.cpu().numpy(), pin["out_seed"])
    assert np.array_equal(sampler.distances.cpu().numpy(), pin["dist_seed"])


_DEBUG_CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
from confild_amd import _lib
assert _lib.LIB_PATH.endswith("libconfild_hip_debug.so"), _lib.LIB_PATH
import test_gpu_dps_dense as t
dims, N, R, T = t.SHAPES["h128"]
p = t._problem(dims, N, R, T)
for mode in ("f32", "split_f16"):
    for form in t.FORMS:
        nf, xn, yn = t._module(p, mode, form)
        for budget in (None, 2 << 20):
            gz, norms = t._dense(nf, xn, yn, p, "per_sample", "rows", budget)
            torch.cuda.synchronize()
            assert torch.isfinite(gz).all() and torch.isfinite(norms).all()
print("DENSE_DEBUG_OK")
"""


def test_dense_grad_under_the_bounds_checked_build(hip):
    lib = os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")
    assert os.path.exists(lib), "build() makes the bounds-checked library"
    env = dict(os.environ, CFD_LIB="libconfild_hip_debug.so")
    code = _DEBUG_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "DENSE_DEBUG_OK" in r.stdout and "CFD_DASSERT" not in r.stdout + r.stderr
