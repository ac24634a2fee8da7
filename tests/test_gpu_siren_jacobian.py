"""GPU: the fused value-and-Jacobian decode (cfd_siren_forward_jacobian,
SIRENAutodecoder_film.decode_jacobian) against autograd through the CPU oracle in
fp64, its invariances (bit-exact), its errors and the bounds-checked build.

Measured on an MI355X, the ratio of |jac - J64| to max(e32, 1e-7 |J64|max) (e32: the
CPU fp32 autograd's own error against fp64, same inputs) over the ten cases: max
0.90 ... 1.87, mean 0.71 ... 1.76, largest at (3, 64, 3, 15, 384) and (2, 128, 2, 17,
256) (profiles/siren_jacobian.json has every case); K_BOUND = 4 is about twice the
largest.  The value output was bit-identical to the f32 decode in every case."""
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

# (d, L, c, nh, H), N, b
CASES = [((2, 8, 4, 1, 32), 129, 3),
         ((3, 16, 1, 0, 64), 100, 2),      # no hidden layer: layer 0 feeds the head
         ((1, 8, 1, 2, 16), 70, 2),        # d = 1 packing
         ((2, 8, 2, 3, 48), 100, 2),       # odd NB
         ((2, 128, 2, 17, 256), 77, 2),
         ((3, 64, 3, 15, 384), 257, 2),    # Case4 width, NB = 24
         ((3, 8, 3, 2, 512), 33, 1),       # NB = 32
         ((3, 16, 3, 2, 64), 1, 1)]        # N = 1
# normaliser forms: "point" a (1, N, c) output table, "chan" a (c) table, "none" no normalisers
VARIANTS = [(i, "point") for i in range(len(CASES))] + [(0, "chan"), (0, "none")]
IDS = [f"{'x'.join(map(str, CASES[i][0]))}-N{CASES[i][1]}-b{CASES[i][2]}-{v}" for i, v in VARIANTS]

# max|jac - J64| <= K_BOUND * max(e32_max, 1e-7 |J64|max), and the means alike
K_BOUND = 4.0


def _inputs(ci, form):
    dims, N, b = CASES[ci]
    d, L, c, nh, H = dims
    tag = f"jac/{ci}"
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
    """(out (b, N, c), J (b, N, c, d)) by autograd through the oracle in `dtype`."""
    cast = lambda t: None if t is None else t.to(dtype)
    sdt = {k: v.to(dtype) for k, v in sd.items()}
    b = lat.shape[0]
    x = cast(coords)[None].expand(b, -1, -1).clone().requires_grad_(True)
    cn = x if xmax is None else osn.normalize(x, cast(xmax), cast(xmin))
    raw = osn.forward(sdt, cn, cast(lat)[:, None])
    out = raw if ymax is None else osn.denormalize(raw, cast(ymax), cast(ymin))
    J = torch.stack([torch.autograd.grad(out[..., o].sum(), x, retain_graph=True)[0] for o in range(out.shape[-1])], -2)
    return out.detach(), J.detach()


@functools.lru_cache(maxsize=None)
def _reference(ci, form):
    """The fp64 Jacobian, the CPU fp32 autograd's error against it, and the fp32 oracle decode."""
    dims, N, b, sd, coords, lat, xmax, xmin, ymax, ymin = _inputs(ci, form)
    _, J64 = _oracle(sd, coords, lat, xmax, xmin, ymax, ymin, torch.float64)
    out32, J32 = _oracle(sd, coords, lat, xmax, xmin, ymax, ymin, torch.float32)
    err = (J32.double() - J64).abs()
    return J64, float(err.max()), float(err.mean()), out32


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


@pytest.mark.parametrize("ci,form", VARIANTS, ids=IDS)
def test_jacobian_against_fp64_autograd(hip, ci, form):
    dims, N, b = CASES[ci]
    d, L, c, nh, H = dims
    J64, e32_max, e32_mean, out32 = _reference(ci, form)
    net, coords, lat, xn, yn = _net(ci, form)
    out, jac = net.decode_jacobian(coords, lat, xn, yn)
    assert out.shape == (b, N, c) and jac.shape == (b, N, c, d)
    err = (jac.cpu().double() - J64).abs()
    scale = float(J64.abs().max())
    floor = 1e-7 * scale
    r_max = float(err.max()) / max(e32_max, floor)
    r_mean = float(err.mean()) / max(e32_mean, floor)
    # the value: the suite's standing bound against the fp32 oracle decode
    oerr = float((out.cpu() - out32).abs().max())
    same = torch.equal(out, net.set_compute("f32").decode(coords, lat, xn, yn))
    print(json.dumps({"case": IDS[VARIANTS.index((ci, form))], "jac_scale": scale, "e32_max": e32_max,
                      "e32_mean": e32_mean, "err_max": float(err.max()), "err_mean": float(err.mean()),
                      "ratio_max": r_max, "ratio_mean": r_mean, "out_err": oerr, "out_equals_f32_decode": same}))
    assert r_max <= K_BOUND and r_mean <= K_BOUND, (r_max, r_mean)
    assert oerr <= 2e-5 * max(1.0, float(out32.abs().max()))


def test_compute_mode_does_not_change_the_jacobian(hip):
    """Always the exact fp32 chain: split_f16 and f32 handles give the same bits, and
    the handle's mode is what it was."""
    net, coords, lat, xn, yn = _net(4, "point")
    net.set_compute("split_f16")
    o1, j1 = net.decode_jacobian(coords, lat, xn, yn)
    assert net.compute_mode(DEV) == "split_f16"
    net.set_compute("f32")
    o2, j2 = net.decode_jacobian(coords, lat, xn, yn)
    assert torch.equal(j1, j2) and torch.equal(o1, o2)


@pytest.mark.parametrize("ci", [0, 2, 5], ids=["d2", "d1", "d3-H384"])
def test_invariance_is_bit_exact(hip, ci):
    dims, N, b = CASES[ci]
    net, coords, lat, xn, yn = _net(ci, "chan")     # a (c) table: the same for every point order
    lat3 = torch.cat([lat, lat.flip(0)])[:3]
    out, jac = net.decode_jacobian(coords, lat3, xn, yn)
    out2, jac2 = net.decode_jacobian(coords, lat3, xn, yn)
    assert torch.equal(jac, jac2) and torch.equal(out, out2)                       # run to run
    for r in range(3):                                                             # batch
        o1, j1 = net.decode_jacobian(coords, lat3[r:r + 1], xn, yn)
        assert torch.equal(j1[0], jac[r]) and torch.equal(o1[0], out[r]), r
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).to(DEV)   # point order
    op, jp = net.decode_jacobian(coords[perm], lat3, xn, yn)
    assert torch.equal(jp, jac[:, perm]) and torch.equal(op, out[:, perm])
    for keep in (1, N // 2 + 1, N - 1):                                            # point count
        ot, jt = net.decode_jacobian(coords[:keep], lat3, xn, yn)
        assert torch.equal(jt, jac[:, :keep]) and torch.equal(ot, out[:, :keep]), keep


def _raw_call(net, coords, lat, jac, out=None, ws_bytes=None):
    """cfd_siren_forward_jacobian through ctypes, no normalisers; returns the code."""
    lib = _lib.load()
    h = net._handle(DEV)
    n = C.c_size_t()
    _lib.check(lib.cfd_siren_jacobian_workspace_bytes(h, lat.shape[0], C.byref(n)), "workspace")
    ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=DEV)
    rc = lib.cfd_siren_forward_jacobian(h, _lib.ptr(coords), coords.shape[0], _lib.ptr(lat), lat.shape[0], None, None,
                                        None, None, 0, _lib.ptr(out), _lib.ptr(jac), _lib.ptr(ws),
                                        n.value if ws_bytes is None else ws_bytes, _lib.stream_of(DEV))
    torch.cuda.synchronize()
    return rc, n.value


def test_null_out_gives_the_same_jacobian(hip):
    dims, N, b = CASES[0]
    net, coords, lat, _, _ = _net(0, "none")
    out, jac = net.decode_jacobian(coords, lat)
    j2 = torch.full_like(jac, float("nan"))
    rc, _ = _raw_call(net, coords.contiguous(), lat.reshape(b, -1).contiguous(), j2, out=None)
    assert rc == 0 and torch.equal(j2, jac)


def test_errors(hip):
    dims, N, b = CASES[0]
    d, L, c, nh, H = dims
    net, coords, lat, xn, yn = _net(0, "point")
    with pytest.raises(_lib.CfdError):
        net.decode_jacobian(coords.cpu(), lat.cpu(), xn, yn)
    ms = Normalizer_ts(params=(torch.zeros(1, d), torch.ones(1, d)), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        net.decode_jacobian(coords, lat, ms, yn)
    msy = Normalizer_ts(params=(torch.zeros(c), torch.ones(c)), method="ms", dim=0)
    with pytest.raises(NotImplementedError):
        net.decode_jacobian(coords, lat, xn, msy)
    # a workspace one byte short: CFD_EARG (1), nothing launched
    jac = torch.zeros((b, N, c, d), device=DEV)
    rc, need = _raw_call(net, coords.contiguous(), lat.reshape(b, -1).contiguous(), jac, ws_bytes=0)
    assert need > 0 and rc == 1 and b"workspace" in _lib.load().cfd_last_error()
    rc, _ = _raw_call(net, coords.contiguous(), lat.reshape(b, -1).contiguous(), jac, ws_bytes=need - 1)
    assert rc == 1 and not jac.any()


def test_four_coordinates_raise_before_any_launch(hip):
    dims = (4, 8, 2, 1, 32)
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(3, *dims).items()})
    net.to(DEV)
    coords = torch.from_numpy(synth.uniform(4, "jac/d4", (10, 4), 0.0, 1.0)).to(DEV)
    lat = torch.from_numpy(synth.normal(5, "jac/d4z", (2, 1, 8))).to(DEV)
    assert net.decode(coords, lat).shape == (2, 10, 2)        # the plain decode takes d = 4
    jac = torch.zeros((2, 10, 2, 4), device=DEV)
    rc, _ = _raw_call(net, coords, lat.reshape(2, 8).contiguous(), jac)
    assert rc == 1 and b"in_coord_features" in _lib.load().cfd_last_error() and not jac.any()
    with pytest.raises(_lib.CfdError, match="in_coord_features"):
        net.decode_jacobian(coords, lat)


CHILD = r"""
import hashlib, json, sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_siren_jacobian as t
net, coords, lat, xn, yn = t._net(int(sys.argv[2]), "point")
out, jac = net.decode_jacobian(coords, lat, xn, yn)
torch.cuda.synchronize()
print(json.dumps({"out": t._bits(out), "jac": t._bits(jac)}))
"""


def test_debug_library_same_bits(hip):
    """The bounds-checked build (CFD_LIB, a child process as tests/test_debug_build.py
    selects it): every index assertion of the new kernel live, same bits."""
    assert os.path.exists(os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")), \
        "debug build absent (make -C confild_amd/csrc DEBUG=1)"
    ci = 3
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(ci)], capture_output=True, text=True,
                       env=dict(os.environ, CFD_LIB="libconfild_hip_debug.so"), timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CFD_DASSERT failed" not in r.stdout + r.stderr
    dbg = json.loads(r.stdout.strip().splitlines()[-1])
    net, coords, lat, xn, yn = _net(ci, "point")
    out, jac = net.decode_jacobian(coords, lat, xn, yn)
    assert dbg == {"out": _bits(out), "jac": _bits(jac)}
