"""GPU: dense derivative measurements in bounded memory (K16: cfd_siren_jdense_grad,
SIRENAutodecoder_film.jac_dense_grad): per-sample residual norms of linear stencils on
the decoded value and its coordinate Jacobian at every point, and their latent
gradient, against fp64 double autograd through the CPU oracle (tests/
test_gpu_siren_jvjp.py::_oracle extended with the stencil, the mask and the norm);
against K15 on the same inputs; bit for bit across budgets, row blocks, batches and
runs; edge behaviour, errors and the bounds-checked build.

The yardstick is K13's, K14's and K15's: |g_z - g64| <= K_BOUND * max(e32, 1e-7 |g64|max)
for the maximum and the mean, e32 the CPU fp32 double autograd's own error against fp64
at the same inputs, K_BOUND = 4; norms relative 1e-5.  Measured on an MI355X over the
fifteen variants (profiles/dense_stencil.json has every case): g_z ratio max 0.75 ... 1.32,
mean 0.69 ... 1.59 (largest at (2, 8, 2, 3, 48), N = 63); norms 8.0e-9 ... 5.6e-7 relative.
Against K15 on the eight unmasked core cases: max 0.10 ... 0.78, mean 0.07 ... 0.53 of the
yardstick (bound 2 K_BOUND), no case with K15's bits (another summation order)."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

from confild_amd import _lib, synth
from confild_amd.guided.measurements import SensorStencilOperator
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts
from oracle import siren as osn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_BOUND = 4.0
NORM_TOL = 1e-5

# (d, L, c, nh, H), N, R, T
CASES = [((2, 8, 4, 1, 32), 150, 6, 3),       # idle column at d = 2, ragged last slab
         ((3, 16, 1, 0, 64), 65, 2, 1),       # no hidden layer, a slab and one point
         ((1, 8, 1, 2, 16), 130, 4, 2),       # RS = 2: the 64-pair tile
         ((2, 8, 2, 3, 48), 63, 2, 2),        # odd NB, under one slab
         ((2, 128, 2, 2, 256), 70, 3, 3),     # H = 256
         ((3, 64, 3, 2, 384), 40, 2, 1),      # Case4 width
         ((3, 8, 3, 2, 512), 33, 1, 1),       # NB = 32: the 4-wave form, 16-pair tiles
         ((2, 8, 4, 1, 32), 1, 2, 1)]         # one point
# variant: weights ("both" / "value" / "jac"), value / jac weights per point, mask rows
# (None, 1, "T", "R"), y rows ("T", "R", None: a zero target), y normaliser ("point": a
# (1, N, c) table, "chan": (c), "none": no normalisers), M readings
MAIN = dict(weights="both", wv_pp=True, wj_pp=False, mask="T", y="T", norm="point", M=3)
VARIANTS = [(ci, MAIN) for ci in range(len(CASES))] + [
    (0, dict(MAIN, weights="value", wv_pp=False, mask=None, norm="chan")),
    (0, dict(MAIN, weights="jac", wj_pp=True, mask=1, y="R", norm="none")),
    (0, dict(MAIN, wv_pp=False, wj_pp=True, mask="R", y=None, M=1)),
    (2, dict(MAIN, weights="jac", wj_pp=False, mask=None, y="R", M=2)),
    (3, dict(MAIN, weights="value", wv_pp=True, mask="R", y=None, norm="chan", M=5)),
    (4, dict(MAIN, wv_pp=True, wj_pp=True, mask=1, norm="none", M=2)),
    (6, dict(MAIN, weights="jac", wj_pp=True, mask=None, y="T", M=1))]


def _vid(ci, v):
    dims, N, R, T = CASES[ci]
    return (f"{'x'.join(map(str, dims))}-N{N}-R{R}T{T}-{v['weights']}{int(v['wv_pp'])}{int(v['wj_pp'])}-m{v['mask']}"
            f"-y{v['y']}-{v['norm']}-M{v['M']}")


IDS = [_vid(ci, v) for ci, v in VARIANTS]

def _key(v):
    return tuple(sorted(v.items(), key=lambda kv: kv[0]))


@functools.lru_cache(maxsize=None)
def _problem(case, ci, vkey):
    """The synthetic problem of shape `case` = (dims, N, R, T), variant `vkey`, stream tag `ci`."""
    v = dict(vkey)
    dims, N, R, T = case
    d, L, c, nh, H = dims
    M = v["M"]
    tag = f"jdense/{ci}"
    p = {"dims": dims, "N": N, "R": R, "T": T, "M": M}
    p["sd"] = {k: torch.from_numpy(a) for k, a in synth.siren_state_dict(61 + H, *dims).items()}
    p["coords"] = torch.from_numpy(synth.uniform(71, tag + "/x", (N, d), -0.3, 1.7))
    p["lat"] = torch.from_numpy(synth.normal(72, tag + "/z", (R, L))) * 0.5
    p["xmax"] = p["xmin"] = p["ymax"] = p["ymin"] = None
    if v["norm"] != "none":
        p["xmax"] = torch.from_numpy(synth.uniform(73, tag + "/xmax", (1, d), 1.5, 2.0))
        p["xmin"] = torch.from_numpy(synth.uniform(74, tag + "/xmin", (1, d), -0.5, -0.2))
        shape = (1, N, c) if v["norm"] == "point" else (c,)
        p["ymax"] = torch.from_numpy(synth.uniform(75, tag + "/ymax", shape, 0.5, 2.0))
        p["ymin"] = torch.from_numpy(synth.uniform(76, tag + "/ymin", shape, -2.0, -0.5))
    p["wv"] = p["wj"] = None
    if v["weights"] in ("both", "value"):
        p["wv"] = torch.from_numpy(synth.normal(77, tag + "/wv", ((N, M, c) if v["wv_pp"] else (M, c))))
    if v["weights"] in ("both", "jac"):
        p["wj"] = torch.from_numpy(synth.normal(78, tag + "/wj", ((N, M, c, d) if v["wj_pp"] else (M, c, d)))) * 0.3
    rows = {None: 0, 1: 1, "T": T, "R": R}
    p["y"] = None if v["y"] is None else torch.from_numpy(synth.normal(79, tag + "/y", (rows[v["y"]], N, M)))
    p["mask"] = None
    if v["mask"] is not None:   # about a third of the readings off, the rest weighted
        m = torch.from_numpy(synth.uniform(80, tag + "/m", (rows[v["mask"]], N, M), -0.5, 1.0))
        p["mask"] = torch.where(m < 0, torch.zeros_like(m), m)
    return p


def _inputs(ci, v):
    return _problem(CASES[ci], ci, _key(v))


def _oracle(p, dtype):
    """(g_z (R, L), norms (R / T)) by autograd through the oracle in `dtype`: out, its
    Jacobian by autograd with create_graph, the stencil, the mask, per-sample norms."""
    cast = lambda t: None if t is None else t.to(dtype)
    sdt = {k: a.to(dtype) for k, a in p["sd"].items()}
    R, N, T, M = p["R"], p["N"], p["T"], p["M"]
    z = cast(p["lat"]).clone().requires_grad_(True)
    x = cast(p["coords"])[None].expand(R, -1, -1).clone().requires_grad_(True)
    cn = x if p["xmax"] is None else osn.normalize(x, cast(p["xmax"]), cast(p["xmin"]))
    raw = osn.forward(sdt, cn, z[:, None])
    out = raw if p["ymax"] is None else osn.denormalize(raw, cast(p["ymax"]), cast(p["ymin"]))
    J = torch.stack([torch.autograd.grad(out[..., o].sum(), x, create_graph=True)[0] for o in range(out.shape[-1])],
                    -2)
    A = 0.0
    if p["wv"] is not None:
        wv = cast(p["wv"])
        A = A + torch.einsum("nmo,rno->rnm", wv if wv.dim() == 3 else wv[None].expand(N, -1, -1), out)
    if p["wj"] is not None:
        wj = cast(p["wj"])
        A = A + torch.einsum("nmok,rnok->rnm", wj if wj.dim() == 4 else wj[None].expand(N, -1, -1, -1), J)
    if p["mask"] is not None:
        A = cast(p["mask"]).repeat(R // p["mask"].shape[0], 1, 1) * A
    y = torch.zeros((R, N, M), dtype=dtype) if p["y"] is None else cast(p["y"]).repeat(R // p["y"].shape[0], 1, 1)
    norms = (y - A).reshape(R // T, -1).pow(2).sum(1).sqrt()
    g = torch.autograd.grad(norms.sum(), z)[0]
    return g.detach(), norms.detach()


@functools.lru_cache(maxsize=None)
def _reference_cached(ci, vkey):
    p = _problem(CASES[ci], ci, vkey)
    g64, n64 = _oracle(p, torch.float64)
    g32, _ = _oracle(p, torch.float32)
    eg = (g32.double() - g64).abs()
    return {"g64": g64, "n64": n64, "eg_max": float(eg.max()), "eg_mean": float(eg.mean())}


def _reference(ci, v):
    return _reference_cached(ci, _key(v))


def _net(p):
    net = SIRENAutodecoder_film(*p["dims"])
    net.load_state_dict(p["sd"])
    net.to(DEV)
    xn = yn = None
    if p["xmax"] is not None:
        xn = Normalizer_ts(params=(p["xmax"], p["xmin"]), method="-11", dim=0)
        yn = Normalizer_ts(params=(p["ymax"], p["ymin"]), method="-11", dim=0)
    return net, xn, yn


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(net, xn, yn, p, budget=None, rows=None, **over):
    """jac_dense_grad on the problem (or on its rows [rows[0], rows[1]))."""
    q = dict(p, **over)
    lat, y, mask = q["lat"], q["y"], q["mask"]
    if rows is not None:
        lat = lat[rows[0]:rows[1]]
        y = y if y is None or y.shape[0] != p["R"] else y[rows[0]:rows[1]]
        mask = mask if mask is None or mask.shape[0] != p["R"] else mask[rows[0]:rows[1]]
    return net.jac_dense_grad(_dev(q["coords"]), _dev(lat), p["T"], _dev(y), _dev(q["wv"]), _dev(q["wj"]), _dev(mask),
                              xn, yn, budget)


def _bits(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _ratios(got, ref64, e_max, e_mean):
    err = (got.cpu().double() - ref64).abs()
    floor = 1e-7 * float(ref64.abs().max())
    return float(err.max()) / max(e_max, floor), float(err.mean()) / max(e_mean, floor)


@pytest.mark.parametrize("ci,v", VARIANTS, ids=IDS)
def test_gradient_and_norms_against_fp64_autograd(hip, ci, v):
    """1. g_z and the norms under the yardstick.  Ratios are printed as JSON."""
    p = _inputs(ci, v)
    ref = _reference(ci, v)
    net, xn, yn = _net(p)
    gz, norms = _run(net, xn, yn, p)
    assert gz.shape == (p["R"], p["dims"][1]) and norms.shape == (p["R"] // p["T"],)
    g_max, g_mean = _ratios(gz, ref["g64"], ref["eg_max"], ref["eg_mean"])
    n_rel = float(((norms.cpu().double() - ref["n64"]).abs() / ref["n64"]).max())
    print(json.dumps({"case": _vid(ci, v), "g_scale": float(ref["g64"].abs().max()), "e32_max": ref["eg_max"],
                      "e32_mean": ref["eg_mean"], "ratio_max": g_max, "ratio_mean": g_mean, "norm_rel": n_rel}))
    assert torch.isfinite(gz).all()
    assert g_max <= K_BOUND and g_mean <= K_BOUND, (g_max, g_mean)
    assert n_rel <= NORM_TOL, n_rel


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_vid(ci, MAIN) for ci in range(len(CASES))])
def test_agrees_with_the_whole_tape_adjoint(hip, ci):
    """2. Against K15 (jac_tape_forward + cfd_dps_residual_linear + jac_tape_vjp) on the
    same inputs, no mask: two fp32 summation orders, each within the yardstick."""
    v = dict(MAIN, mask=None)
    p = _inputs(ci, v)
    ref = _reference(ci, v)
    net, xn, yn = _net(p)
    gz, norms = _run(net, xn, yn, p)
    out, jac = net.jac_tape_forward(_dev(p["coords"]), _dev(p["lat"]), xn, yn)
    L = p["dims"][1]
    op = SensorStencilOperator.from_parts(DEV, p["coords"], xn, yn, net, torch.ones(L), -torch.ones(L),
                                          value_weights=p["wv"], jac_weights=p["wj"])
    n15, g_out, g_jac, _ = op.residual(out, jac, _dev(p["y"]), p["R"] // p["T"])
    g15 = net.jac_tape_vjp(g_out, g_jac)
    d_max, d_mean = _ratios(gz, g15.cpu().double(), ref["eg_max"], ref["eg_mean"])
    n_rel = float(((norms - n15).abs() / n15).max())
    print(json.dumps({"case": _vid(ci, v), "vs_k15_max": d_max, "vs_k15_mean": d_mean, "norm_rel_vs_k15": n_rel,
                      "equal_bits": torch.equal(gz, g15)}))
    assert d_max <= 2 * K_BOUND and d_mean <= 2 * K_BOUND, (d_max, d_mean)
    assert n_rel <= 2 * NORM_TOL, n_rel


def _plan(dims, N, R, M, budget):
    cfg = _lib.SirenCfg(*dims, 30.0)
    b, pts, rows = C.c_size_t(), C.c_int64(), C.c_int()
    rc = _lib.load().cfd_siren_jdense_plan(C.byref(cfg), N, R, M, budget, C.byref(b), C.byref(pts), C.byref(rows))
    return rc, b.value, pts.value, rows.value


BITS = [((2, 8, 2, 3, 48), 300, 6, 3), ((1, 8, 1, 2, 16), 200, 4, 2), ((3, 8, 3, 2, 512), 100, 2, 1)]


@pytest.mark.parametrize("bi", range(len(BITS)), ids=["odd-NB", "RS2", "4-wave"])
def test_bits_do_not_depend_on_budget_row_blocks_batch_or_run(hip, bi):
    """3. One chunk, several chunks and row blocks with rb < R (each read back from the
    planner); a sample alone against its rows inside the batch; run to run."""
    dims, N, R, T = BITS[bi]
    p = _problem(BITS[bi], f"bits{bi}", _key(dict(MAIN, y="R", mask="R")))
    M = p["M"]
    net, xn, yn = _net(p)
    rc, full, pts, rows = _plan(dims, N, R, M, 0)
    assert rc == 0 and pts >= N and rows == R                           # one chunk of all rows
    gz, norms = _run(net, xn, yn, p)
    assert net.dense_workspace_bytes == full
    seen = {"chunks": None, "blocks": None}
    for k in range(1, 400):                                             # shrink the budget by 2 % steps
        budget = int(full * 0.98 ** k)
        rc, b, pts, rows = _plan(dims, N, R, M, budget)
        if rc != 0:
            break
        assert b <= budget and pts % 64 == 0
        if rows == R and 64 <= pts < N and seen["chunks"] is None:
            seen["chunks"] = budget
        if rows < R and seen["blocks"] is None:
            assert pts == 64
            seen["blocks"] = budget
    assert seen["chunks"] is not None and seen["blocks"] is not None, seen
    rc, _, _, rows_small = _plan(dims, N, R, M, seen["blocks"] // 2)
    budgets = [seen["chunks"], seen["blocks"]] + ([seen["blocks"] // 2] if rc == 0 and rows_small >= 1 else [])
    for budget in budgets:
        g2, n2 = _run(net, xn, yn, p, budget=budget)
        assert net.dense_workspace_bytes <= budget
        assert torch.equal(g2, gz) and torch.equal(n2, norms), budget
    g3, n3 = _run(net, xn, yn, p)                                       # run to run
    assert torch.equal(g3, gz) and torch.equal(n3, norms)
    for b in range(R // T):                                             # a sample alone
        g1, n1 = _run(net, xn, yn, p, rows=(b * T, (b + 1) * T))
        assert torch.equal(g1, gz[b * T:(b + 1) * T]) and torch.equal(n1, norms[b:b + 1]), b


def test_compute_mode_does_not_change_the_result(hip):
    p = _inputs(4, MAIN)
    net, xn, yn = _net(p)
    net.set_compute("split_f16")
    g1, n1 = _run(net, xn, yn, p)
    net.set_compute("f32")
    g2, n2 = _run(net, xn, yn, p)
    assert torch.equal(g1, g2) and torch.equal(n1, n2)


def test_zero_residual_gives_a_zero_gradient(hip):
    p = _inputs(0, MAIN)
    net, xn, yn = _net(p)
    gz, norms = _run(net, xn, yn, p, y=None, mask=torch.zeros(1, p["N"], p["M"]))
    assert not norms.any() and not gz.any() and torch.isfinite(gz).all()
    gz, norms = _run(net, xn, yn, p, y=None, mask=None, wv=torch.zeros(p["M"], p["dims"][2]), wj=None)
    assert not norms.any() and not gz.any() and torch.isfinite(gz).all()


def test_a_masked_reading_equals_a_zero_weight_row(hip):
    """A masked-out point, and one masked-out reading of another, contribute exactly
    nothing: bit-equal to zero rows in per-point weight tables."""
    v = dict(MAIN, wv_pp=True, wj_pp=True, mask=None)
    p = _inputs(0, v)
    net, xn, yn = _net(p)
    N, M = p["N"], p["M"]
    mask = torch.ones(1, N, M)
    mask[0, 70] = 0.0          # a whole point
    mask[0, 149, 1] = 0.0      # one reading of the last point (the ragged slab)
    wv, wj = p["wv"].clone(), p["wj"].clone()
    for w in (wv, wj):
        w[70] = 0.0
        w[149, 1] = 0.0
    g_m, n_m = _run(net, xn, yn, p, mask=mask)
    g_w, n_w = _run(net, xn, yn, p, wv=wv, wj=wj)
    assert torch.equal(g_m, g_w) and torch.equal(n_m, n_w)
    g_0, n_0 = _run(net, xn, yn, p)
    assert not torch.equal(g_0, g_m) and not torch.equal(n_0, n_m)


def _raw(net, p, gz, norm, ws, ws_bytes, budget=0, T=None, M=None, wv=True, wj=True, y_rows=None, mask=None,
         mask_rows=0, N=None):
    """cfd_siren_jdense_grad with no normalisers; keeps every device tensor alive over the call."""
    c, d = p["dims"][2], p["dims"][0]
    N = p["N"] if N is None else N
    M = p["M"] if M is None else M
    coords, lat = _dev(p["coords"]).contiguous(), _dev(p["lat"]).contiguous()
    wvt = torch.ones((max(M, 1), c), device=DEV) if wv else None
    wjt = torch.ones((max(M, 1), c, d), device=DEV) if wj else None
    y = torch.ones((p["R"], N, max(M, 1)), device=DEV)
    rc = _lib.load().cfd_siren_jdense_grad(
        net._handle(DEV), _lib.ptr(coords), N, _lib.ptr(lat), p["R"], p["T"] if T is None else T, None, None, None,
        None, 0, _lib.ptr(wvt), 0, _lib.ptr(wjt), 0, M, _lib.ptr(y), p["R"] if y_rows is None else y_rows,
        _lib.ptr(mask), mask_rows, _lib.ptr(gz), _lib.ptr(norm), _lib.ptr(ws), ws_bytes, budget, _lib.stream_of(DEV))
    torch.cuda.synchronize()
    return rc, _lib.load().cfd_last_error()


def test_errors_raise_before_any_launch(hip):
    """5. Every shape error: CFD_EARG (1), g_latents and norm untouched."""
    p = _inputs(0, dict(MAIN, norm="none"))
    dims, N, R, T, M = p["dims"], p["N"], p["R"], p["T"], p["M"]
    net, xn, yn = _net(p)
    lib = _lib.load()
    n = C.c_size_t()
    _lib.check(lib.cfd_siren_jdense_workspace_bytes(net._handle(DEV), N, R, M, 0, C.byref(n)), "workspace")
    need = n.value
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    gz = torch.zeros((R, dims[1]), device=DEV)
    norm = torch.zeros((R // T,), device=DEV)
    ones = torch.ones((R, N, M), device=DEV)

    def refused(word, **kw):
        rc, msg = _raw(net, p, gz, norm, ws, kw.pop("ws_bytes", need), **kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
        assert not gz.any() and not norm.any(), kw

    refused(b"workspace", ws_bytes=need - 1)                        # one byte short
    refused(b"too small", budget=4096)                              # below one slab of one row
    refused(b"rows_per_sample", T=4)                                # 4 does not divide 6
    refused(b"rows_per_sample", T=0)
    refused(b"y_rows", y_rows=2)                                    # neither T nor R
    refused(b"mask_rows", mask=ones, mask_rows=2)                   # neither 1, T nor R
    refused(b"reading", M=0)
    refused(b"weights", wv=False, wj=False)
    refused(b"point", N=0)
    rc, msg = _raw(net, p, gz, norm, ws, need)
    assert rc == 0 and gz.any() and norm.all(), msg                 # and the same call, well-formed, runs
    # the Python guards
    with pytest.raises(ValueError, match="needs value_weights"):
        _run(net, xn, yn, p, wv=None, wj=None)
    with pytest.raises(ValueError, match="rows_per_sample"):
        net.jac_dense_grad(_dev(p["coords"]), _dev(p["lat"]), 4, None, _dev(p["wv"]))
    with pytest.raises(ValueError, match="measurement"):
        _run(net, xn, yn, p, y=torch.zeros(2, N, M))
    with pytest.raises(ValueError, match="mask"):
        _run(net, xn, yn, p, mask=torch.zeros(2, N, M))
    with pytest.raises(ValueError, match="readings"):
        _run(net, xn, yn, p, wj=torch.zeros(M + 1, dims[2], dims[0]))
    with pytest.raises(_lib.CfdError):
        net.jac_dense_grad(p["coords"], p["lat"], T, None, p["wv"])
    msn = Normalizer_ts(params=(torch.zeros(1, dims[0]), torch.ones(1, dims[0])), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        _run(net, msn, None, p)


def test_four_coordinates_raise_before_any_launch(hip):
    dims = (4, 8, 2, 1, 32)
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict({k: torch.from_numpy(a) for k, a in synth.siren_state_dict(3, *dims).items()})
    net.to(DEV)
    p = {"dims": dims, "N": 10, "R": 2, "T": 1, "M": 1,
         "coords": torch.from_numpy(synth.uniform(4, "jdense/d4", (10, 4), 0.0, 1.0)),
         "lat": torch.from_numpy(synth.normal(5, "jdense/d4z", (2, 8)))}
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    gz = torch.zeros((2, 8), device=DEV)
    norm = torch.zeros((2,), device=DEV)
    rc, msg = _raw(net, p, gz, norm, ws, ws.numel())
    assert rc == 1 and b"in_coord_features" in msg and not gz.any() and not norm.any()
    with pytest.raises(_lib.CfdError, match="in_coord_features"):
        net.jac_dense_grad(_dev(p["coords"]), _dev(p["lat"]), 1, None, torch.ones(1, 2))


CHILD = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_siren_jdense as t
res = {}
for ci in range(len(t.CASES)):
    p = t._inputs(ci, t.MAIN)
    net, xn, yn = t._net(p)
    gz, norms = t._run(net, xn, yn, p)
    g2, n2 = t._run(net, xn, yn, p, budget=int(sys.argv[2]) if ci == 0 else None)
    torch.cuda.synchronize()
    res[str(ci)] = {"gz": gz.cpu().tolist(), "norms": norms.cpu().tolist(), "blocks_equal": bool(
        torch.equal(gz, g2) and torch.equal(norms, n2))}
print(json.dumps(res))
"""


def test_debug_library_bits_and_the_d1_tolerance(hip):
    """6. The bounds-checked build (CFD_LIB, a child process as tests/test_debug_build.py
    selects it) on the core cases, case 0 also in row blocks of one slab: every index
    assertion of the new kernels live and none fails, and the shipped build's bits at
    d >= 2, as K15's test asserts them.  The d = 1 case (RS = 2) is held to 1e-5 of
    |g_z|max and 1e-6 relative on the norms instead: the two builds differ in
    optimisation level, and at RS = 2 the compiler contracts a multiply-add of the
    shared forward chain in one and not in the other (their instruction mixes differ
    there, in K15's instantiations too), which moves single roundings of 6e-8
    relative; a wrong index moves g_z by its own size."""
    assert os.path.exists(os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")), \
        "debug build absent (make -C confild_amd/csrc DEBUG=1)"
    dims, N, R, T = CASES[0]
    rc, full, _, _ = _plan(dims, N, R, MAIN["M"], 0)
    budget = full // 3
    rc, _, pts, rows = _plan(dims, N, R, MAIN["M"], budget)
    assert rc == 0 and (pts < N or rows < R)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(budget)], capture_output=True, text=True,
                       env=dict(os.environ, CFD_LIB="libconfild_hip_debug.so"), timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CFD_DASSERT failed" not in r.stdout + r.stderr
    dbg = json.loads(r.stdout.strip().splitlines()[-1])
    for ci in range(len(CASES)):
        p = _inputs(ci, MAIN)
        net, xn, yn = _net(p)
        gz, norms = _run(net, xn, yn, p)
        dg, dn = torch.tensor(dbg[str(ci)]["gz"]), torch.tensor(dbg[str(ci)]["norms"])
        same = torch.equal(dg, gz.cpu()) and torch.equal(dn, norms.cpu())   # the lists carry every fp32 bit
        print(json.dumps({"case": _vid(ci, MAIN), "debug_build_same_bits": same}))
        assert dbg[str(ci)]["blocks_equal"], ci
        if CASES[ci][0][0] >= 2:
            assert same, ci
        else:
            assert float((dg - gz.cpu()).abs().max()) <= 1e-5 * float(gz.abs().max()), ci
            assert float(((dn - norms.cpu()).abs() / norms.cpu()).max()) <= 1e-6, ci
