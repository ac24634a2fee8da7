"""The two MFMA shapes of the split-f16 decoder (siren_split32 in
confild_amd/csrc/siren_split.hip): v_mfma_f32_32x32x16_f16 on one 32-coordinate
column block per wave, or v_mfma_f32_16x16x32_f16 on two 16-coordinate column
groups per wave (16-row output blocks, two per ring slot, lane group g storing
output g).  The library picks one per width; the other is a development build
(make VARIANT=shape16 VFLAGS=-DCFD_SPLIT32_SHAPE=16, or shape32 / =32).

Shapes: one layer per width (as many blocks as ring slots), a layer wrap at the
narrowest and the widest width, and the output-store lane roles at c = 1 and c = 4.
Point counts: a second column group with no valid point (N <= 16: it decodes the
clamped point N - 1 and stores nothing), a short group, a short wave, a short tile,
more than one tile.  Checked per shape, as in test_gpu_siren_ring.py:

  accuracy     error against the fp64 oracle <= 2x the larger of the f32 kernel's
               and the CPU fp32 oracle's, + 1e-7 of the output scale
  determinism  five repeats, a decode of another width between them, bit-identical
  placement    a row's bits do not depend on the batch, a point's bits not on its
               column group, wave, tile or the call's N

Each case is at most 3 x 385 (row, point) pairs.  The same properties run on every
development build of the other shape that is present (a child pytest with CFD_LIB).
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from confild_amd import synth
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts
from oracle import siren as osn

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# (d, L, c, nh, H)
ONE_LAYER = [(3, 8, 3, 1, 64), (3, 16, 3, 1, 128), (2, 16, 2, 1, 256), (3, 16, 3, 1, 384)]
WRAPPING = [(2, 8, 2, 2, 64), (3, 16, 3, 2, 384)]
STORE_ROLES = [(1, 8, 1, 2, 64), (2, 16, 4, 3, 128)]
DIMS = ONE_LAYER + WRAPPING + STORE_ROLES
NS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 385)
BS = (1, 3)
NMAX, BMAX = max(NS), max(BS)
VARIANTS = ("libconfild_hip_shape16.so", "libconfild_hip_shape32.so")


@functools.lru_cache(maxsize=None)
def _case(dims):
    """The net, the inputs of the largest call and both oracles on them (computed
    once per shape; every smaller call is a slice: the decode is pointwise)."""
    d, L, c, nh, H = dims
    sd = {k: torch.from_numpy(v) for k, v in synth.siren_state_dict(1234, d, L, c, nh, H).items()}
    net = SIRENAutodecoder_film(d, L, c, nh, H)
    net.load_state_dict(sd)
    net.to(DEV)
    coords = torch.from_numpy(synth.uniform(7, "co", (NMAX, d), 0.0, 1.0))
    lat = torch.from_numpy(synth.normal(11, "la", (BMAX, L))) * 0.5
    ymax = torch.from_numpy(synth.uniform(9, "yx", (1, NMAX, c), 0.5, 2.0))
    ymin = -torch.from_numpy(synth.uniform(9, "yn", (1, NMAX, c), 0.5, 2.0))
    one, zero = torch.ones(1, d), torch.zeros(1, d)
    ref64 = osn.decode({k: v.double() for k, v in sd.items()}, coords.double(), lat.double(), one.double(),
                       zero.double(), ymax.double(), ymin.double())
    ref32 = osn.decode(sd, coords, lat, one, zero, ymax, ymin).double()
    return net, coords, lat, ymax, ymin, ref64, ref32


def _decode(dims, mode, rows, pts):
    """Decode latent rows `rows` at points `pts` (index lists into the shape's inputs)."""
    net, coords, lat, ymax, ymin, _, _ = _case(dims)
    d = dims[0]
    net.set_compute(mode)
    xn = Normalizer_ts(params=(torch.ones(1, d), torch.zeros(1, d)), method="-11", dim=0)
    yn = Normalizer_ts(params=(ymax[:, pts], ymin[:, pts]), method="-11", dim=0)
    out = net.decode(coords[pts].to(DEV), lat[rows].to(DEV)[:, None], xn, yn).cpu()
    assert net.compute_mode(DEV) == mode
    return out


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dims", DIMS)
def test_shape_keeps_fp32_accuracy(hip, dims, N, b):
    _, _, _, _, _, ref64, ref32 = _case(dims)
    rows, pts = list(range(b)), list(range(N))
    r64, r32 = ref64[:b, :N], ref32[:b, :N]
    split = _decode(dims, "split_f16", rows, pts).double()
    f32 = _decode(dims, "f32", rows, pts).double()
    assert split.shape == r64.shape
    scale = r64.abs().max().item()
    e_split, e_f32, e_cpu = (split - r64).abs().max().item(), (f32 - r64).abs().max().item(), \
        (r32 - r64).abs().max().item()
    print(f"{dims} N={N} b={b}: max err vs fp64 split {e_split:.3e} f32-MFMA {e_f32:.3e} cpu-fp32 {e_cpu:.3e}")
    assert e_split <= 2 * max(e_f32, e_cpu) + 1e-7 * scale


@pytest.mark.parametrize("dims", DIMS)
def test_shape_is_deterministic(hip, dims):
    """Five repeats are bit-identical, with a decode of another width between them."""
    other = DIMS[(DIMS.index(dims) + 1) % len(DIMS)]
    if other[4] == dims[4]:
        other = DIMS[(DIMS.index(dims) + 2) % len(DIMS)]
    assert other[4] != dims[4]
    rows, pts = list(range(BMAX)), list(range(NMAX))
    first = _decode(dims, "split_f16", rows, pts)
    for _ in range(4):
        _decode(other, "split_f16", rows, pts)
        assert torch.equal(_decode(dims, "split_f16", rows, pts), first)


@pytest.mark.parametrize("dims", DIMS)
def test_shape_result_does_not_depend_on_placement(hip, dims):
    rows, pts = list(range(BMAX)), list(range(NMAX))
    full = _decode(dims, "split_f16", rows, pts)
    # row r of the b = 3 call is the b = 1 call of that row
    for r in rows:
        assert torch.equal(_decode(dims, "split_f16", [r], pts)[0], full[r]), r
    # the calls of every N are slices of the largest
    for N in NS:
        assert torch.equal(_decode(dims, "split_f16", rows, pts[:N]), full[:, :N]), N
    # point n of the N = 385 call (column group 0 or 1, first or later wave and tile):
    # decoded alone (group 0, the other group empty), moved into group 1 of wave 0,
    # into wave 1, and as the last point of an N = 129 call
    for n in (0, 15, 16, 31, 32, 127, 128, 384):
        assert torch.equal(_decode(dims, "split_f16", rows, [n])[:, 0], full[:, n]), n
        for at in (16, 31, 47, 128):
            others = [(n + 1 + i) % NMAX for i in range(at)]
            assert torch.equal(_decode(dims, "split_f16", rows, others + [n])[:, at], full[:, n]), (n, at)


@pytest.mark.parametrize("lib", VARIANTS)
def test_other_shape_build_has_the_same_properties(hip, lib):
    """The three properties above on a development build that runs one shape at every
    width, when it has been built."""
    if os.environ.get("CFD_LIB"):
        pytest.skip("already running on a named build")
    if not os.path.exists(os.path.join(ROOT, "confild_amd", "lib", lib)):
        pytest.skip(f"{lib} absent (make -C confild_amd/csrc VARIANT=shape16 VFLAGS=-DCFD_SPLIT32_SHAPE=16)")
    env = dict(os.environ, CFD_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__)],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
