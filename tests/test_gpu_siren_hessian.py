"""GPU: the fused value-Jacobian-Hessian decode (cfd_siren_forward_hessian,
SIRENAutodecoder_film.decode_hessian) against double autograd through the CPU oracle
in fp64, its invariances (bit-exact), its errors and the bounds-checked build.

The yardstick and the bound are the Jacobian test's (tests/test_gpu_siren_jacobian.py):
max|hess - H64| <= K_BOUND * max(e32, 1e-7 |H64|max) and the means alike, e32 the CPU
fp32 double autograd's own error against fp64 on the same inputs; the same call's jac
meets that bound against J64 and its out 2e-5 against the fp32 oracle decode.

Measured on an MI355X over the 14 variants: the Hessian's ratio max 0.49 ... 1.28, mean
0.83 ... 1.69 (largest at (3, 64, 3, 15, 384)), the Jacobian's 0.76 ... 1.71; out and jac
were bit-identical to decode_jacobian's in every variant (profiles/siren_hessian.json
has every case)."""
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
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts
from oracle import siren as osn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (d, L, c, nh, H), N, b; no N is a multiple of its form's points per workgroup
# (32 at d = 1, 16 at d = 2 and for the diagonal at d = 3, 8 for the full form at d = 3;
# halved at H = 512)
CASES = [((2, 8, 4, 1, 32), 129, 3),
         ((3, 16, 1, 0, 64), 100, 2),      # no hidden layer: layer 0 feeds the head
         ((1, 8, 1, 2, 16), 70, 2),        # d = 1 packing
         ((2, 8, 2, 3, 48), 100, 2),       # odd NB
         ((2, 128, 2, 17, 256), 77, 2),
         ((3, 64, 3, 15, 384), 65, 2),     # Case4 width, NB = 24
         ((3, 8, 3, 2, 512), 33, 1),       # NB = 32: the 4-wave form
         ((3, 16, 3, 2, 64), 1, 1)]        # N = 1
# normaliser forms: "point" a (1, N, c) output table, "chan" a (c) table, "none" no normalisers;
# every d = 3 case in the full and in the diagonal form
VARIANTS = ([(i, "point", False) for i in range(len(CASES))] + [(0, "chan", False), (0, "none", False)]
            + [(i, "point", True) for i in range(len(CASES)) if CASES[i][0][0] == 3])
IDS = [f"{'x'.join(map(str, CASES[i][0]))}-N{CASES[i][1]}-b{CASES[i][2]}-{v}-{'diag' if dg else 'full'}"
       for i, v, dg in VARIANTS]

# max|hess - H64| <= K_BOUND * max(e32_max, 1e-7 |H64|max), and the means alike
K_BOUND = 4.0


def _inputs(ci, form):
    dims, N, b = CASES[ci]
    d, L, c, nh, H = dims
    tag = f"hess/{ci}"
    sd = {k: torch.from_numpy(v) for k, v in synth.siren_state_dict(11 + ci, *dims).items()}
    coords = torch.from_numpy(synth.uniform(21, tag + "/x", (N, d), -0.3, 1.7))
    lat = torch.from_numpy(synth.normal(22, tag + "/z", (b, L))) * 0.5
    xmax = xmin = ymax = ymin = None
    if form != "none":
        xmax = torch.from_numpy(synth.uniform(23, tag + "/xmax", (1, d), 1.5, 2.0))
        xmin = torch.from_numpy(synth.uniform(24, tag + "/xmin", (1, d), -0.5, -0.2))
        shape = (1, N, c) if form == "point" else (c,)
        ymax = torch.from_numpy(synth.uniform(25, tag + "/ymax", shape, 0.5, 2.0))
        ymin = torch.from_numpy(synth.uniform(26, tag + "/ymin", shape, -2.0, -0.5))
    return dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin


def _oracle(sd, coords, lat, xmax, xmin, ymax, ymin, dtype):
    """(out (b, N, c), J (b, N, c, d), H (b, N, c, d, d)) by double autograd through the oracle in `dtype`."""
    cast = lambda t: None if t is None else t.to(dtype)
    sdt = {k: v.to(dtype) for k, v in sd.items()}
    b = lat.shape[0]
    x = cast(coords)[None].expand(b, -1, -1).clone().requires_grad_(True)
    cn = x if xmax is None else osn.normalize(x, cast(xmax), cast(xmin))
    raw = osn.forward(sdt, cn, cast(lat)[:, None])
    out = raw if ymax is None else osn.denormalize(raw, cast(ymax), cast(ymin))
    d = x.shape[-1]
    J, Hs = [], []
    for o in range(out.shape[-1]):
        Jo = torch.autograd.grad(out[..., o].sum(), x, create_graph=True)[0]        # (b, N, d)
        J.append(Jo)
        Hs.append(torch.stack([torch.autograd.grad(Jo[..., k].sum(), x, retain_graph=True)[0] for k in range(d)], -2))
    return out.detach(), torch.stack(J, -2).detach(), torch.stack(Hs, -3).detach()


@functools.lru_cache(maxsize=None)
def _reference(ci, form):
    """fp64 Jacobian and Hessian, the CPU fp32 double autograd's errors against them
    ((max, mean) of each), and the fp32 oracle decode."""
    dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = _inputs(ci, form)
    _, J64, H64 = _oracle(sd, coords, lat, xmax, xmin, ymax, ymin, torch.float64)
    out32, J32, H32 = _oracle(sd, coords, lat, xmax, xmin, ymax, ymin, torch.float32)
    ej, eh = (J32.double() - J64).abs(), (H32.double() - H64).abs()
    ehd = torch.diagonal(eh, dim1=-2, dim2=-1)
    return {"J64": J64, "H64": H64, "ej": (float(ej.max()), float(ej.mean())),
            "eh": (float(eh.max()), float(eh.mean())), "ehd": (float(ehd.max()), float(ehd.mean())), "out32": out32}


def _net(ci, form):
    dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = _inputs(ci, form)
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict(sd)
    net.to(DEV)
    xn = yn = None
    if form != "none":
        xn = Normalizer_ts(params=(xmax, xmin), method="-11", dim=0)
        yn = Normalizer_ts(params=(ymax, ymin), method="-11", dim=0)
    return net, coords.to(DEV), lat.to(DEV)[:, None], xn, yn


def _bits(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _ratios(got, ref, e32):
    err = (got.cpu().double() - ref).abs()
    scale = float(ref.abs().max())
    floor = 1e-7 * scale
    return float(err.max()) / max(e32[0], floor), float(err.mean()) / max(e32[1], floor), scale, err


@pytest.mark.parametrize("ci,form,diag", VARIANTS, ids=IDS)
def test_hessian_against_fp64_double_autograd(hip, ci, form, diag):
    dims, N, b = CASES[ci]
    d, L, c, nh, H = dims
    ref = _reference(ci, form)
    net, coords, lat, xn, yn = _net(ci, form)
    out, jac, hess = net.decode_hessian(coords, lat, xn, yn, diag=diag)
    assert out.shape == (b, N, c) and jac.shape == (b, N, c, d)
    assert hess.shape == ((b, N, c, d) if diag else (b, N, c, d, d))
    H64 = torch.diagonal(ref["H64"], dim1=-2, dim2=-1) if diag else ref["H64"]
    # the diagonal form is judged on the diagonal's own scale and fp32 error
    h_max, h_mean, h_scale, herr = _ratios(hess, H64, ref["ehd"] if diag else ref["eh"])
    j_max, j_mean, j_scale, _ = _ratios(jac, ref["J64"], ref["ej"])
    oerr = float((out.cpu() - ref["out32"]).abs().max())
    o13, j13 = net.decode_jacobian(coords, lat, xn, yn)
    print(json.dumps({"case": IDS[VARIANTS.index((ci, form, diag))], "hess_scale": h_scale,
                      "e32_max": (ref["ehd"] if diag else ref["eh"])[0],
                      "e32_mean": (ref["ehd"] if diag else ref["eh"])[1], "err_max": float(herr.max()),
                      "err_mean": float(herr.mean()), "ratio_max": h_max, "ratio_mean": h_mean,
                      "jac_ratio_max": j_max, "jac_ratio_mean": j_mean, "out_err": oerr,
                      "out_equals_decode_jacobian": torch.equal(out, o13),
                      "jac_equals_decode_jacobian": torch.equal(jac, j13)}))
    assert h_max <= K_BOUND and h_mean <= K_BOUND, (h_max, h_mean)
    assert j_max <= K_BOUND and j_mean <= K_BOUND, (j_max, j_mean)
    assert oerr <= 2e-5 * max(1.0, float(ref["out32"].abs().max()))
    if not diag:
        assert torch.equal(hess, hess.transpose(-1, -2))           # both halves from one lane


@pytest.mark.parametrize("ci", [0, 4, 5, 6, 7], ids=["d2", "d2-H256", "d3-H384", "d3-H512", "d3-N1"])
def test_diagonal_of_the_full_form_equals_the_diagonal_form(hip, ci):
    net, coords, lat, xn, yn = _net(ci, "point")
    of, jf, hf = net.decode_hessian(coords, lat, xn, yn)
    od, jd, hd = net.decode_hessian(coords, lat, xn, yn, diag=True)
    assert torch.equal(torch.diagonal(hf, dim1=-2, dim2=-1), hd)
    assert torch.equal(of, od) and torch.equal(jf, jd)


def test_compute_mode_does_not_change_the_hessian(hip):
    """Always the exact fp32 chain: split_f16 and f32 handles give the same bits, and
    the handle's mode is what it was."""
    net, coords, lat, xn, yn = _net(4, "point")
    net.set_compute("split_f16")
    r1 = net.decode_hessian(coords, lat, xn, yn)
    assert net.compute_mode(DEV) == "split_f16"
    net.set_compute("f32")
    r2 = net.decode_hessian(coords, lat, xn, yn)
    assert net.compute_mode(DEV) == "f32"
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))


@pytest.mark.parametrize("ci,diag", [(0, False), (2, False), (5, False), (5, True)],
                         ids=["d2", "d1", "d3-H384", "d3-H384-diag"])
def test_invariance_is_bit_exact(hip, ci, diag):
    dims, N, b = CASES[ci]
    net, coords, lat, xn, yn = _net(ci, "chan")     # a (c) table: the same for every point order
    lat3 = torch.cat([lat, lat.flip(0)])[:3]
    dec = lambda x, z: net.decode_hessian(x, z, xn, yn, diag=diag)
    same = lambda r, s: all(torch.equal(a, b) for a, b in zip(r, s))
    full = dec(coords, lat3)
    assert same(full, dec(coords, lat3))                                           # run to run
    for r in range(3):                                                             # batch
        assert same([t[0] for t in dec(coords, lat3[r:r + 1])], [t[r] for t in full]), r
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).to(DEV)   # point order
    assert same(dec(coords[perm], lat3), [t[:, perm] for t in full])
    for keep in (1, N // 2 + 1, N - 1):                                            # point count
        assert same(dec(coords[:keep], lat3), [t[:, :keep] for t in full]), keep


def _raw_call(net, coords, lat, hess, out=None, jac=None, diag=0, ws_bytes=None):
    """cfd_siren_forward_hessian through ctypes, no normalisers; returns the code."""
    lib = _lib.load()
    h = net._handle(DEV)
    n = C.c_size_t()
    _lib.check(lib.cfd_siren_hessian_workspace_bytes(h, lat.shape[0], C.byref(n)), "workspace")
    ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=DEV)
    rc = lib.cfd_siren_forward_hessian(h, _lib.ptr(coords), coords.shape[0], _lib.ptr(lat), lat.shape[0], None, None,
                                       None, None, 0, _lib.ptr(out), _lib.ptr(jac), _lib.ptr(hess), diag,
                                       _lib.ptr(ws), n.value if ws_bytes is None else ws_bytes, _lib.stream_of(DEV))
    torch.cuda.synchronize()
    return rc, n.value


@pytest.mark.parametrize("ci", [0, 7], ids=["d2", "d3"])
def test_null_out_and_null_jac_give_the_same_hessian(hip, ci):
    dims, N, b = CASES[ci]
    net, coords, lat, _, _ = _net(ci, "none")
    out, jac, hess = net.decode_hessian(coords, lat)
    x, z = coords.contiguous(), lat.reshape(b, -1).contiguous()
    for with_out, with_jac in ((False, False), (True, False), (False, True)):
        h2 = torch.full_like(hess, float("nan"))
        o2 = torch.full_like(out, float("nan")) if with_out else None
        j2 = torch.full_like(jac, float("nan")) if with_jac else None
        rc, _ = _raw_call(net, x, z, h2, out=o2, jac=j2)
        assert rc == 0 and torch.equal(h2, hess)
        assert o2 is None or torch.equal(o2, out)
        assert j2 is None or torch.equal(j2, jac)
    hd = torch.full_like(jac, float("nan"))
    rc, _ = _raw_call(net, x, z, hd, diag=1)
    assert rc == 0 and torch.equal(hd, torch.diagonal(hess, dim1=-2, dim2=-1))


def test_errors(hip):
    dims, N, b = CASES[0]
    d, L, c, nh, H = dims
    net, coords, lat, xn, yn = _net(0, "point")
    with pytest.raises(_lib.CfdError):
        net.decode_hessian(coords.cpu(), lat.cpu(), xn, yn)
    ms = Normalizer_ts(params=(torch.zeros(1, d), torch.ones(1, d)), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        net.decode_hessian(coords, lat, ms, yn)
    msy = Normalizer_ts(params=(torch.zeros(c), torch.ones(c)), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        net.decode_hessian(coords, lat, xn, msy)
    # a workspace one byte short: CFD_EARG (1), nothing launched
    hess = torch.zeros((b, N, c, d, d), device=DEV)
    x, z = coords.contiguous(), lat.reshape(b, -1).contiguous()
    rc, need = _raw_call(net, x, z, hess, ws_bytes=0)
    assert need > 0 and rc == 1 and b"workspace" in _lib.load().cfd_last_error()
    rc, _ = _raw_call(net, x, z, hess, ws_bytes=need - 1)
    assert rc == 1 and not hess.any()
    # hess is required
    rc, _ = _raw_call(net, x, z, None, out=torch.zeros((b, N, c), device=DEV))
    assert rc == 1 and b"null" in _lib.load().cfd_last_error()


def test_four_coordinates_raise_before_any_launch(hip):
    dims = (4, 8, 2, 1, 32)
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(3, *dims).items()})
    net.to(DEV)
    coords = torch.from_numpy(synth.uniform(4, "hess/d4", (10, 4), 0.0, 1.0)).to(DEV)
    lat = torch.from_numpy(synth.normal(5, "hess/d4z", (2, 1, 8))).to(DEV)
    for diag in (0, 1):
        hess = torch.zeros((2, 10, 2, 4) + (() if diag else (4,)), device=DEV)
        rc, _ = _raw_call(net, coords, lat.reshape(2, 8).contiguous(), hess, diag=diag)
        assert rc == 1 and b"in_coord_features" in _lib.load().cfd_last_error() and not hess.any()
    with pytest.raises(_lib.CfdError, match="in_coord_features"):
        net.decode_hessian(coords, lat)


CHILD = r"""
import hashlib, json, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_siren_hessian as t
res = {}
for ci in (int(v) for v in sys.argv[2:]):
    net, coords, lat, xn, yn = t._net(ci, "point")
    out, jac, hess = net.decode_hessian(coords, lat, xn, yn)
    torch.cuda.synchronize()
    res[str(ci)] = {"out": t._bits(out), "jac": t._bits(jac), "hess": t._bits(hess)}
print(json.dumps(res))
"""


def test_debug_library_same_bits(hip):
    """The bounds-checked build (CFD_LIB, a child process as tests/test_debug_build.py
    selects it): every index assertion of the new kernel live at d = 2 and at d = 3
    (full form), same bits."""
    assert os.path.exists(os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")), \
        "debug build absent (make -C confild_amd/csrc DEBUG=1)"
    cis = (3, 7, 1)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT] + [str(ci) for ci in cis], capture_output=True, text=True,
                       env=dict(os.environ, CFD_LIB="libconfild_hip_debug.so"), timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CFD_DASSERT failed" not in r.stdout + r.stderr
    dbg = json.loads(r.stdout.strip().splitlines()[-1])
    for ci in cis:
        net, coords, lat, xn, yn = _net(ci, "point")
        out, jac, hess = net.decode_hessian(coords, lat, xn, yn)
        assert dbg[str(ci)] == {"out": _bits(out), "jac": _bits(jac), "hess": _bits(hess)}, ci
