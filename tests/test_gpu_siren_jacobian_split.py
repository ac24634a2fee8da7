"""GPU: the split-f16 value-and-Jacobian decode (K13s, cfd_siren_forward_jacobian_split,
decode_jacobian(compute="split_f16")): accuracy against fp64 autograd through the CPU
oracle, exact homogeneity in the coordinate scale, range, invariances (bit-exact), the
untouched default, errors and the bounds-checked build.

Inputs, references and the bound are those of tests/test_gpu_siren_jacobian.py:
|jac - J64| max and mean <= K_BOUND * max(e32, 1e-7 |J64|max), K_BOUND = 4, e32 the CPU
fp32 autograd's own error; the value <= 2e-5 max(1, |out|max) off the fp32 oracle decode.
The measured ratios are in profiles/siren_jacobian_split.json."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_siren_jacobian as base
from confild_amd import _lib, synth
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts

pytestmark = pytest.mark.gpu
DEV = base.DEV
ROOT = base.ROOT
K_BOUND = base.K_BOUND
SPLIT = "split_f16"

# (d, L, c, nh, H), N, b: the smallest shapes at which each piece can go wrong
CASES = [((2, 8, 4, 1, 32), 129, 3),       # one hidden layer is first and last; idle column; N % tile != 0
         ((1, 8, 1, 2, 64), 70, 2),        # RS = 2 packing
         ((2, 8, 2, 3, 96), 100, 2),       # odd number of 32-feature chunks
         ((3, 16, 3, 2, 64), 1, 1),        # a single point
         ((2, 128, 2, 17, 256), 77, 2),    # config E's width
         ((3, 64, 3, 15, 384), 257, 2)]    # Case4's width
RANGE = len(CASES)                         # the growing-tangent network of test_range
RANGE_CASE = ((2, 8, 2, 12, 64), 50, 2)
VARIANTS = [(i, "point") for i in range(len(CASES))] + [(0, "chan"), (0, "none")]


def _id(ci, form):
    dims, N, b = CASES[ci]
    return f"{'x'.join(map(str, dims))}-N{N}-b{b}-{form}"


IDS = [_id(ci, form) for ci, form in VARIANTS]


@functools.lru_cache(maxsize=None)
def _inputs(ci, form, k=0):
    """The Jacobian test's input recipe (its own inputs where the case is one of its
    cases); k: coords, xmax and xmin times 2^k."""
    if ci != RANGE and CASES[ci] in base.CASES:
        dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = base._inputs(base.CASES.index(CASES[ci]), form)
    else:
        dims, N, b = RANGE_CASE if ci == RANGE else CASES[ci]
        d, L, c, nh, H = dims
        tag = f"jacs/{ci}"
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
    if k:
        coords, xmax, xmin = coords * 2.0 ** k, xmax * 2.0 ** k, xmin * 2.0 ** k     # exact in fp32
    return dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin


@functools.lru_cache(maxsize=None)
def _reference(ci, form):
    """The fp64 Jacobian, the CPU fp32 autograd's error against it, the fp32 oracle
    decode and the fp64 one."""
    dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = _inputs(ci, form)
    out64, J64 = base._oracle(sd, coords, lat, xmax, xmin, ymax, ymin, torch.float64)
    out32, J32 = base._oracle(sd, coords, lat, xmax, xmin, ymax, ymin, torch.float32)
    err = (J32.double() - J64).abs()
    return J64, float(err.max()), float(err.mean()), out32, out64


def _net(ci, form, k=0):
    dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = _inputs(ci, form, k)
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict(sd)
    net.to(DEV)
    xn = yn = None
    if form != "none":
        xn = Normalizer_ts(params=(xmax, xmin), method="-11", dim=0)
        yn = Normalizer_ts(params=(ymax, ymin), method="-11", dim=0)
    return net, coords.to(DEV), lat.to(DEV)[:, None], xn, yn


def _check_against_fp64(ci, form, name, chaotic=False):
    J64, e32_max, e32_mean, out32, out64 = _reference(ci, form)
    net, coords, lat, xn, yn = _net(ci, form)
    out, jac = net.decode_jacobian(coords, lat, xn, yn, compute=SPLIT)
    assert out.shape == out32.shape and jac.shape == J64.shape
    finite = bool(torch.isfinite(jac).all()) and bool(torch.isfinite(out).all())
    err = (jac.cpu().double() - J64).abs()
    scale = float(J64.abs().max())
    floor = 1e-7 * scale
    r_max = float(err.max()) / max(e32_max, floor)
    r_mean = float(err.mean()) / max(e32_mean, floor)
    oerr = float((out.cpu() - out32).abs().max())
    print(json.dumps({"case": name, "compute": SPLIT, "jac_scale": scale, "e32_max": e32_max, "e32_mean": e32_mean,
                      "err_max": float(err.max()), "err_mean": float(err.mean()), "ratio_max": r_max,
                      "ratio_mean": r_mean, "out_err": oerr, "finite": finite}))
    assert finite
    assert r_max <= K_BOUND and r_mean <= K_BOUND, (r_max, r_mean)
    if not chaotic:     # the value: the suite's standing bound against the fp32 oracle decode
        assert oerr <= 2e-5 * max(1.0, float(out32.abs().max()))
    else:               # two fp32 evaluations differ by more than that here: the Jacobian's form of bound
        o32 = float((out32.double() - out64).abs().max())
        o = float((out.cpu().double() - out64).abs().max())
        print(json.dumps({"case": name, "out_e32_max": o32, "out_err_fp64": o}))
        assert o <= K_BOUND * max(o32, 2e-5 * max(1.0, float(out64.abs().max())))


@pytest.mark.parametrize("ci,form", VARIANTS, ids=IDS)
def test_split_jacobian_against_fp64_autograd(hip, ci, form):
    _check_against_fp64(ci, form, _id(ci, form))


@pytest.mark.parametrize("ci", [4, 0], ids=["H256", "H32"])
def test_coordinate_scale_is_exactly_homogeneous(hip, ci):
    """coords, xmax, xmin times 2^k: jac 2^k and out keep their bits (each tangent column
    is split at a scale of its own, so the chain sees the same mantissas; a chain
    without it loses the small scales to f16 underflow and drifts at the large ones)."""
    net, coords, lat, xn, yn = _net(ci, "point")
    out0, jac0 = net.decode_jacobian(coords, lat, xn, yn, compute=SPLIT)
    assert bool(torch.isfinite(jac0).all()) and bool(jac0.any())
    for k in (-20, -12, 12, 20):
        net, coords, lat, xn, yn = _net(ci, "point", k)
        out, jac = net.decode_jacobian(coords, lat, xn, yn, compute=SPLIT)
        assert torch.equal(jac * 2.0 ** k, jac0), k
        assert torch.equal(out, out0), k


def test_range_growing_tangents(hip):
    """Hidden weights doubled: the tangents grow in every layer, past f16's 65504 without
    the per-column scale.  Finite, and within the same bound (e32 is about 1 % of
    |J64|max here, a chaotic regime, so the value is held to the fp64 decode in the
    same form: K_BOUND times the fp32 oracle's own error)."""
    _check_against_fp64(RANGE, "chan", "range-2x8x2x12x64-N50-b2-chan", chaotic=True)


@pytest.mark.parametrize("ci", [0, 1, 5], ids=["d2", "d1", "d3-H384"])
def test_invariance_is_bit_exact(hip, ci):
    dims, N, b = CASES[ci]
    net, coords, lat, xn, yn = _net(ci, "chan")     # a (c) table: the same for every point order
    dj = functools.partial(net.decode_jacobian, compute=SPLIT)
    lat3 = torch.cat([lat, lat.flip(0)])[:3]
    out, jac = dj(coords, lat3, xn, yn)
    out2, jac2 = dj(coords, lat3, xn, yn)
    assert torch.equal(jac, jac2) and torch.equal(out, out2)                       # run to run
    for r in range(3):                                                             # batch
        o1, j1 = dj(coords, lat3[r:r + 1], xn, yn)
        assert torch.equal(j1[0], jac[r]) and torch.equal(o1[0], out[r]), r
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).to(DEV)   # point order
    op, jp = dj(coords[perm], lat3, xn, yn)
    assert torch.equal(jp, jac[:, perm]) and torch.equal(op, out[:, perm])
    for keep in (1, N // 2 + 1, N - 1):                                            # point count
        ot, jt = dj(coords[:keep], lat3, xn, yn)
        assert torch.equal(jt, jac[:, :keep]) and torch.equal(ot, out[:, :keep]), keep


def test_default_is_untouched(hip):
    """No keyword and compute="f32" are the same call under both handle modes, and a
    split_f16 call leaves the handle's mode alone."""
    net, coords, lat, xn, yn = _net(4, "point")
    for mode in ("split_f16", "f32"):
        net.set_compute(mode)
        o1, j1 = net.decode_jacobian(coords, lat, xn, yn)
        o2, j2 = net.decode_jacobian(coords, lat, xn, yn, compute="f32")
        assert torch.equal(j1, j2) and torch.equal(o1, o2), mode
        before = net.compute_mode(DEV)
        net.decode_jacobian(coords, lat, xn, yn, compute=SPLIT)
        assert net.compute_mode(DEV) == before == mode
        o3, j3 = net.decode_jacobian(coords, lat, xn, yn)
        assert torch.equal(j3, j1) and torch.equal(o3, o1), mode


def _raw_call(net, coords, lat, jac, out=None, ws_bytes=None):
    """cfd_siren_forward_jacobian_split through ctypes, no normalisers; returns the code."""
    lib = _lib.load()
    h = net._handle(DEV)
    n = C.c_size_t()
    _lib.check(lib.cfd_siren_jacobian_workspace_bytes(h, lat.shape[0], C.byref(n)), "workspace")
    ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=DEV)
    rc = lib.cfd_siren_forward_jacobian_split(h, _lib.ptr(coords), coords.shape[0], _lib.ptr(lat), lat.shape[0], None,
                                              None, None, None, 0, _lib.ptr(out), _lib.ptr(jac), _lib.ptr(ws),
                                              n.value if ws_bytes is None else ws_bytes, _lib.stream_of(DEV))
    torch.cuda.synchronize()
    return rc, n.value


def test_null_out_gives_the_same_jacobian(hip):
    dims, N, b = CASES[0]
    net, coords, lat, _, _ = _net(0, "none")
    out, jac = net.decode_jacobian(coords, lat, compute=SPLIT)
    j2 = torch.full_like(jac, float("nan"))
    rc, _ = _raw_call(net, coords.contiguous(), lat.reshape(b, -1).contiguous(), j2, out=None)
    assert rc == 0 and torch.equal(j2, jac)


@pytest.mark.parametrize("dims,reason", [((2, 8, 2, 2, 48), "multiple of 32"), ((2, 8, 2, 1, 512), "512"),
                                         ((2, 8, 2, 0, 64), "num_hidden_layers"),
                                         ((4, 8, 2, 1, 32), "in_coord_features")],
                         ids=["H48", "H512", "nh0", "d4"])
def test_refused_widths_raise_before_any_launch(hip, dims, reason):
    d, L, c = dims[:3]
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(3, *dims).items()})
    net.to(DEV)
    coords = torch.from_numpy(synth.uniform(4, "jacs/err", (10, d), 0.0, 1.0)).to(DEV)
    lat = torch.from_numpy(synth.normal(5, "jacs/errz", (2, 1, L))).to(DEV)
    jac = torch.full((2, 10, c, d), 7.0, device=DEV)
    rc, _ = _raw_call(net, coords, lat.reshape(2, L).contiguous(), jac)
    assert rc == 1 and reason.encode() in _lib.load().cfd_last_error() and bool((jac == 7.0).all())
    with pytest.raises(_lib.CfdError, match=reason):
        net.decode_jacobian(coords, lat, compute=SPLIT)


def test_errors(hip):
    dims, N, b = CASES[0]
    d, L, c, nh, H = dims
    net, coords, lat, xn, yn = _net(0, "point")
    with pytest.raises(_lib.CfdError):
        net.decode_jacobian(coords.cpu(), lat.cpu(), xn, yn, compute=SPLIT)
    ms = Normalizer_ts(params=(torch.zeros(1, d), torch.ones(1, d)), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        net.decode_jacobian(coords, lat, ms, yn, compute=SPLIT)
    msy = Normalizer_ts(params=(torch.zeros(c), torch.ones(c)), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        net.decode_jacobian(coords, lat, xn, msy, compute=SPLIT)
    for bad in ("f16", "split", "bf16", ""):
        with pytest.raises(ValueError, match="compute"):
            net.decode_jacobian(coords, lat, xn, yn, compute=bad)
    # a workspace one byte short: CFD_EARG (1), nothing launched
    jac = torch.zeros((b, N, c, d), device=DEV)
    rc, need = _raw_call(net, coords.contiguous(), lat.reshape(b, -1).contiguous(), jac, ws_bytes=0)
    assert need > 0 and rc == 1 and b"workspace" in _lib.load().cfd_last_error()
    rc, _ = _raw_call(net, coords.contiguous(), lat.reshape(b, -1).contiguous(), jac, ws_bytes=need - 1)
    assert rc == 1 and not jac.any()


CHILD = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_siren_jacobian_split as t
net, coords, lat, xn, yn = t._net(int(sys.argv[2]), "point")
out, jac = net.decode_jacobian(coords, lat, xn, yn, compute="split_f16")
torch.cuda.synchronize()
print(json.dumps({"out": t.base._bits(out), "jac": t.base._bits(jac)}))
"""


def test_debug_library_same_bits(hip):
    """The bounds-checked build (CFD_LIB, a fresh child process as
    tests/test_debug_build.py selects it): every index assertion of the kernel live,
    same bits."""
    assert os.path.exists(os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")), \
        "debug build absent (make -C confild_amd/csrc DEBUG=1)"
    ci = 2
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(ci)], capture_output=True, text=True,
                       env=dict(os.environ, CFD_LIB="libconfild_hip_debug.so"), timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CFD_DASSERT failed" not in r.stdout + r.stderr
    dbg = json.loads(r.stdout.strip().splitlines()[-1])
    net, coords, lat, xn, yn = _net(ci, "point")
    out, jac = net.decode_jacobian(coords, lat, xn, yn, compute=SPLIT)
    assert dbg == {"out": base._bits(out), "jac": base._bits(jac)}
