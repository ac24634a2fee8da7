"""GPU: the split-f16 value-Jacobian-Hessian decode (K14s, cfd_siren_forward_hessian_split,
decode_hessian(compute="split_f16")): accuracy against fp64 double autograd through the
CPU oracle, exact homogeneity in each coordinate's scale, range, invariances (bit-exact),
the untouched default, NULL outputs, refusals, errors and the bounds-checked build.

Inputs, references and the bound are those of tests/test_gpu_siren_hessian.py:
|hess - H64| max and mean <= K_BOUND * max(e32, 1e-7 |H64|max), K_BOUND = 4, e32 the CPU
fp32 double autograd's own error, the Jacobian alike; the value <= 2e-5 max(1, |out|max)
off the fp32 oracle decode.

Measured on an MI355X over the 11 variants: the Hessian's ratio max 0.59 ... 1.54, mean
0.93 ... 1.48 (largest at (3, 64, 3, 15, 384)), the Jacobian's max 0.60 ... 1.49, mean
0.96 ... 1.77; out and jac had decode_jacobian(compute="split_f16")'s bits in every variant
(profiles/siren_hessian_split.json has every case)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_siren_hessian as base
from confild_amd import _lib, synth
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts

pytestmark = pytest.mark.gpu
DEV = base.DEV
ROOT = base.ROOT
K_BOUND = base.K_BOUND
SPLIT = "split_f16"

# (d, L, c, nh, H), N, b: the smallest shapes at which each piece can go wrong
CASES = [((2, 8, 4, 1, 32), 129, 3),       # one hidden layer is first and last; idle columns; N % tile != 0
         ((2, 128, 2, 17, 256), 77, 2),    # config E's width
         ((3, 64, 3, 15, 384), 65, 2),     # Case4's width
         ((3, 16, 3, 2, 64), 1, 1),        # a single point
         ((1, 8, 1, 2, 64), 70, 2),        # RS = 4 packing at d = 1
         ((2, 8, 2, 3, 96), 100, 2)]       # odd number of 32-feature chunks
RANGE = len(CASES)                         # the growing-tangent network of test_range
RANGE_CASE = ((2, 8, 2, 12, 64), 50, 2)
# every d = 3 case in the full and in the diagonal form; case 0 in every normaliser form
VARIANTS = ([(i, "point", False) for i in range(len(CASES))] + [(0, "chan", False), (0, "none", False)]
            + [(i, "point", True) for i in range(len(CASES)) if CASES[i][0][0] == 3])


def _id(ci, form, diag):
    dims, N, b = RANGE_CASE if ci == RANGE else CASES[ci]
    return f"{'x'.join(map(str, dims))}-N{N}-b{b}-{form}-{'diag' if diag else 'full'}"


IDS = [_id(*v) for v in VARIANTS]


@functools.lru_cache(maxsize=None)
def _inputs(ci, form, k=0, k0=0):
    """The Hessian test's input recipe (its own inputs where the case is one of its
    cases); k: coords, xmax and xmin times 2^k; k0: coordinate 0 alone times 2^k0."""
    if ci != RANGE and CASES[ci] in base.CASES:
        dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = base._inputs(base.CASES.index(CASES[ci]), form)
    else:
        dims, N, b = RANGE_CASE if ci == RANGE else CASES[ci]
        d, L, c, nh, H = dims
        tag = f"hesss/{ci}"
        sd = {k_: torch.from_numpy(v) for k_, v in synth.siren_state_dict(31 if ci == RANGE else 11 + ci, *dims).items()}
        if ci == RANGE:                   # tangents that grow in every layer
            for i in range(1, nh + 1):
                sd[f"net1.{i}.weight"] = sd[f"net1.{i}.weight"] * 2
        coords = torch.from_numpy(synth.uniform(21, tag + "/x", (N, d), -0.3, 1.7))
        lat = torch.from_numpy(synth.normal(22, tag + "/z", (b, L))) * 0.5
        xmax = xmin = ymax = ymin = None
        if form != "none":
            xmax = torch.from_numpy(synth.uniform(23, tag + "/xmax", (1, d), 1.5, 2.0))
            xmin = torch.from_numpy(synth.uniform(24, tag + "/xmin", (1, d), -0.5, -0.2))
            shape = (1, N, c) if form == "point" else (c,)
            ymax = torch.from_numpy(synth.uniform(25, tag + "/ymax", shape, 0.5, 2.0))
            ymin = torch.from_numpy(synth.uniform(26, tag + "/ymin", shape, -2.0, -0.5))
    if k or k0:                           # powers of two: exact in fp32
        s = torch.full((dims[0],), 2.0 ** k)
        s[0] *= 2.0 ** k0
        coords, xmax, xmin = coords * s, xmax * s, xmin * s
    return dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin


@functools.lru_cache(maxsize=None)
def _reference(ci, form):
    """fp64 value, Jacobian and Hessian, the CPU fp32 double autograd's errors against
    them ((max, mean) of each), and the fp32 oracle decode.  Computed once per case."""
    if ci != RANGE and CASES[ci] in base.CASES:
        return base._reference(base.CASES.index(CASES[ci]), form)
    dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = _inputs(ci, form)
    out64, J64, H64 = base._oracle(sd, coords, lat, xmax, xmin, ymax, ymin, torch.float64)
    out32, J32, H32 = base._oracle(sd, coords, lat, xmax, xmin, ymax, ymin, torch.float32)
    ej, eh = (J32.double() - J64).abs(), (H32.double() - H64).abs()
    ehd = torch.diagonal(eh, dim1=-2, dim2=-1)
    return {"J64": J64, "H64": H64, "ej": (float(ej.max()), float(ej.mean())),
            "eh": (float(eh.max()), float(eh.mean())), "ehd": (float(ehd.max()), float(ehd.mean())), "out32": out32,
            "out64": out64}


def _net(ci, form, k=0, k0=0):
    dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = _inputs(ci, form, k, k0)
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict(sd)
    net.to(DEV)
    xn = yn = None
    if form != "none":
        xn = Normalizer_ts(params=(xmax, xmin), method="-11", dim=0)
        yn = Normalizer_ts(params=(ymax, ymin), method="-11", dim=0)
    return net, coords.to(DEV), lat.to(DEV)[:, None], xn, yn


def _check_against_fp64(ci, form, diag, chaotic=False):
    dims, N, b = RANGE_CASE if ci == RANGE else CASES[ci]
    d, L, c, nh, H = dims
    ref = _reference(ci, form)
    net, coords, lat, xn, yn = _net(ci, form)
    out, jac, hess = net.decode_hessian(coords, lat, xn, yn, diag=diag, compute=SPLIT)
    assert out.shape == (b, N, c) and jac.shape == (b, N, c, d)
    assert hess.shape == ((b, N, c, d) if diag else (b, N, c, d, d))
    finite = all(bool(torch.isfinite(t).all()) for t in (out, jac, hess))
    H64 = torch.diagonal(ref["H64"], dim1=-2, dim2=-1) if diag else ref["H64"]
    e32 = ref["ehd"] if diag else ref["eh"]      # the diagonal form on the diagonal's own scale and fp32 error
    h_max, h_mean, h_scale, herr = base._ratios(hess, H64, e32)
    j_max, j_mean, j_scale, _ = base._ratios(jac, ref["J64"], ref["ej"])
    oerr = float((out.cpu() - ref["out32"]).abs().max())
    o13, j13 = net.decode_jacobian(coords, lat, xn, yn, compute=SPLIT)
    print(json.dumps({"case": _id(ci, form, diag), "compute": SPLIT, "hess_scale": h_scale, "e32_max": e32[0],
                      "e32_mean": e32[1], "err_max": float(herr.max()), "err_mean": float(herr.mean()),
                      "ratio_max": h_max, "ratio_mean": h_mean, "jac_ratio_max": j_max, "jac_ratio_mean": j_mean,
                      "out_err": oerr, "finite": finite,
                      "out_equals_decode_jacobian_split": torch.equal(out, o13),
                      "jac_equals_decode_jacobian_split": torch.equal(jac, j13)}))
    assert finite
    assert h_max <= K_BOUND and h_mean <= K_BOUND, (h_max, h_mean)
    assert j_max <= K_BOUND and j_mean <= K_BOUND, (j_max, j_mean)
    if not chaotic:     # the value: the suite's standing bound against the fp32 oracle decode
        assert oerr <= 2e-5 * max(1.0, float(ref["out32"].abs().max()))
    else:               # two fp32 evaluations differ by more than that here: K13s's chaotic form
        out64 = ref["out64"]
        o32 = float((ref["out32"].double() - out64).abs().max())
        o = float((out.cpu().double() - out64).abs().max())
        print(json.dumps({"case": _id(ci, form, diag), "out_e32_max": o32, "out_err_fp64": o}))
        assert o <= K_BOUND * max(o32, 2e-5 * max(1.0, float(out64.abs().max())))
    if not diag:
        assert torch.equal(hess, hess.transpose(-1, -2))           # both halves from one lane


@pytest.mark.parametrize("ci,form,diag", VARIANTS, ids=IDS)
def test_split_hessian_against_fp64_double_autograd(hip, ci, form, diag):
    _check_against_fp64(ci, form, diag)


@pytest.mark.parametrize("ci", [0, 1, 2, 3], ids=["d2", "d2-H256", "d3-H384", "d3-N1"])
def test_diagonal_of_the_full_form_equals_the_diagonal_form(hip, ci):
    """d = 3: the 8-column form against the 16-column one; d = 2: the diagonal call
    against the diagonal of the full call."""
    net, coords, lat, xn, yn = _net(ci, "point")
    of, jf, hf = net.decode_hessian(coords, lat, xn, yn, compute=SPLIT)
    od, jd, hd = net.decode_hessian(coords, lat, xn, yn, diag=True, compute=SPLIT)
    assert torch.equal(torch.diagonal(hf, dim1=-2, dim2=-1), hd)
    assert torch.equal(of, od) and torch.equal(jf, jd)


@pytest.mark.parametrize("ci", [1, 0], ids=["H256", "H32"])
def test_coordinate_scale_is_exactly_homogeneous(hip, ci):
    """coords, xmax, xmin times 2^k: hess 2^(2k), jac 2^k and out keep their bits.  With
    coordinate 0 alone scaled, hess[.., i, j] 2^(k ([i = 0] + [j = 0])) keeps them: every
    column has a frame of its own, which one scale shared by a point's columns cannot do."""
    net, coords, lat, xn, yn = _net(ci, "point")
    d = CASES[ci][0][0]
    out0, jac0, hess0 = net.decode_hessian(coords, lat, xn, yn, compute=SPLIT)
    assert bool(torch.isfinite(hess0).all()) and bool(hess0.any()) and bool(jac0.any())
    for k in (-20, -12, 12, 20):
        net, coords, lat, xn, yn = _net(ci, "point", k)
        out, jac, hess = net.decode_hessian(coords, lat, xn, yn, compute=SPLIT)
        assert torch.equal(hess * 2.0 ** (2 * k), hess0), k
        assert torch.equal(jac * 2.0 ** k, jac0), k
        assert torch.equal(out, out0), k
    for k in (-20, 20):
        net, coords, lat, xn, yn = _net(ci, "point", 0, k)
        out, jac, hess = net.decode_hessian(coords, lat, xn, yn, compute=SPLIT)
        # the exact powers of two as Python floats (a device pow() need not be exact)
        s1 = torch.tensor([2.0 ** (k if i == 0 else 0) for i in range(d)], device=DEV)
        assert torch.equal(hess * (s1[:, None] * s1[None, :]), hess0), k
        assert torch.equal(jac * s1, jac0), k
        assert torch.equal(out, out0), k


def test_range_growing_tangents(hip):
    """K13s's recipe: hidden weights doubled, the tangents and the second-order columns
    grow in every layer, past f16's 65504 without the per-column frames.  Finite and
    within the same bound; the value is held to the fp64 decode in K13s's chaotic form."""
    _check_against_fp64(RANGE, "chan", False, chaotic=True)


@pytest.mark.parametrize("ci,diag", [(0, False), (4, False), (2, False), (2, True)],
                         ids=["d2", "d1", "d3-H384", "d3-H384-diag"])
def test_invariance_is_bit_exact(hip, ci, diag):
    dims, N, b = CASES[ci]
    net, coords, lat, xn, yn = _net(ci, "chan")     # a (c) table: the same for every point order
    lat3 = torch.cat([lat, lat.flip(0)])[:3]
    dec = lambda x, z: net.decode_hessian(x, z, xn, yn, diag=diag, compute=SPLIT)
    same = lambda r, s: all(torch.equal(a, b) for a, b in zip(r, s))
    full = dec(coords, lat3)
    assert same(full, dec(coords, lat3))                                           # run to run
    for r in range(3):                                                             # rows alone
        assert same([t[0] for t in dec(coords, lat3[r:r + 1])], [t[r] for t in full]), r
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).to(DEV)   # point order
    assert same(dec(coords[perm], lat3), [t[:, perm] for t in full])
    for keep in (1, N // 2 + 1, N - 1):                                            # point count
        assert same(dec(coords[:keep], lat3), [t[:, :keep] for t in full]), keep


def test_default_is_untouched(hip):
    """No keyword and compute="f32" are the same call under both handle modes, and a
    split_f16 call leaves the handle's mode alone."""
    net, coords, lat, xn, yn = _net(1, "point")
    same = lambda r, s: all(torch.equal(a, b) for a, b in zip(r, s))
    first = None
    for mode in ("split_f16", "f32"):
        net.set_compute(mode)
        r1 = net.decode_hessian(coords, lat, xn, yn)
        assert same(r1, net.decode_hessian(coords, lat, xn, yn, compute="f32")), mode
        before = net.compute_mode(DEV)
        rs = net.decode_hessian(coords, lat, xn, yn, compute=SPLIT)
        assert net.compute_mode(DEV) == before == mode
        assert same(r1, net.decode_hessian(coords, lat, xn, yn)), mode
        assert not torch.equal(rs[2], r1[2])           # another kernel ran
        first = first or r1
        assert same(first, r1), mode                   # the same bits under either handle mode


def _raw_call(net, coords, lat, hess, out=None, jac=None, diag=0, ws_bytes=None):
    """cfd_siren_forward_hessian_split through ctypes, no normalisers; returns the code."""
    lib = _lib.load()
    h = net._handle(DEV)
    n = C.c_size_t()
    _lib.check(lib.cfd_siren_hessian_workspace_bytes(h, lat.shape[0], C.byref(n)), "workspace")
    ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=DEV)
    rc = lib.cfd_siren_forward_hessian_split(h, _lib.ptr(coords), coords.shape[0], _lib.ptr(lat), lat.shape[0], None,
                                             None, None, None, 0, _lib.ptr(out), _lib.ptr(jac), _lib.ptr(hess), diag,
                                             _lib.ptr(ws), n.value if ws_bytes is None else ws_bytes,
                                             _lib.stream_of(DEV))
    torch.cuda.synchronize()
    return rc, n.value


@pytest.mark.parametrize("ci", [0, 3], ids=["d2", "d3"])
def test_null_out_and_null_jac_give_the_same_hessian(hip, ci):
    dims, N, b = CASES[ci]
    net, coords, lat, _, _ = _net(ci, "none")
    out, jac, hess = net.decode_hessian(coords, lat, compute=SPLIT)
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


@pytest.mark.parametrize("dims,reason", [((2, 8, 2, 2, 48), "multiple of 32"), ((2, 8, 2, 1, 512), "512"),
                                         ((2, 8, 2, 0, 64), "num_hidden_layers"),
                                         ((4, 8, 2, 1, 32), "in_coord_features")],
                         ids=["H48", "H512", "nh0", "d4"])
def test_refused_widths_raise_before_any_launch(hip, dims, reason):
    d, L, c = dims[:3]
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(3, *dims).items()})
    net.to(DEV)
    coords = torch.from_numpy(synth.uniform(4, "hesss/err", (10, d), 0.0, 1.0)).to(DEV)
    lat = torch.from_numpy(synth.normal(5, "hesss/errz", (2, 1, L))).to(DEV)
    for diag in (0, 1):
        hess = torch.full((2, 10, c, d) + (() if diag else (d,)), 7.0, device=DEV)
        rc, _ = _raw_call(net, coords, lat.reshape(2, L).contiguous(), hess, diag=diag)
        assert rc == 1 and reason.encode() in _lib.load().cfd_last_error() and bool((hess == 7.0).all())
    with pytest.raises(_lib.CfdError, match=reason):
        net.decode_hessian(coords, lat, compute=SPLIT)


def test_errors(hip):
    dims, N, b = CASES[0]
    d, L, c, nh, H = dims
    net, coords, lat, xn, yn = _net(0, "point")
    with pytest.raises(_lib.CfdError):
        net.decode_hessian(coords.cpu(), lat.cpu(), xn, yn, compute=SPLIT)
    ms = Normalizer_ts(params=(torch.zeros(1, d), torch.ones(1, d)), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        net.decode_hessian(coords, lat, ms, yn, compute=SPLIT)
    msy = Normalizer_ts(params=(torch.zeros(c), torch.ones(c)), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        net.decode_hessian(coords, lat, xn, msy, compute=SPLIT)
    for bad in ("f16", "split", "bf16", ""):
        with pytest.raises(ValueError, match="compute"):
            net.decode_hessian(coords, lat, xn, yn, compute=bad)
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


CHILD = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_siren_hessian_split as t
res = {}
for ci in (int(v) for v in sys.argv[2:]):
    net, coords, lat, xn, yn = t._net(ci, "point")
    out, jac, hess = net.decode_hessian(coords, lat, xn, yn, compute="split_f16")
    torch.cuda.synchronize()
    res[str(ci)] = {"out": t.base._bits(out), "jac": t.base._bits(jac), "hess": t.base._bits(hess)}
print(json.dumps(res))
"""


def test_debug_library_same_bits(hip):
    """The bounds-checked build (CFD_LIB, a fresh child process as
    tests/test_debug_build.py selects it): every index assertion of the kernel live at
    d = 1, d = 2 and d = 3 (full form), same bits."""
    assert os.path.exists(os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")), \
        "debug build absent (make -C confild_amd/csrc DEBUG=1)"
    cis = (5, 3, 4)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT] + [str(ci) for ci in cis], capture_output=True, text=True,
                       env=dict(os.environ, CFD_LIB="libconfild_hip_debug.so"), timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CFD_DASSERT failed" not in r.stdout + r.stderr
    dbg = json.loads(r.stdout.strip().splitlines()[-1])
    for ci in cis:
        net, coords, lat, xn, yn = _net(ci, "point")
        out, jac, hess = net.decode_hessian(coords, lat, xn, yn, compute=SPLIT)
        assert dbg[str(ci)] == {"out": base._bits(out), "jac": base._bits(jac), "hess": base._bits(hess)}, ci
