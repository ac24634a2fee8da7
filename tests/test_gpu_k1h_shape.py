"""K1h, the halo-tiled split-f16 3x3 convolution, on v_mfma_f32_16x16x32_f16
(conv_x.hip: conv_h_kernel<..., SHAPE = 16>, conv_h16_body; LDS layout: k1h_lds.hpp).

The forward's K1h launches (variant 20, and 24: the phase form of an Upsample
convolution) run the 16x16x32 form; K1hb, K1x, the transposed launches and the
adjoint's mirrored-pack K1h launches (ConvPlan::adjoint) keep 32x32x16.  Same
tiles, halo, ring, grid, split-K ranges and step order, so a sample's bits still
depend only on its shape and the planned batch -- but not the parent's bits: a
32-deep MFMA sums a chunk's channels in another order.

Probes (built as tests/test_gpu_upsample_phase.py builds its probes), B samples:

  probe32   B = 3, image 32, 64 base channels, channel_mult "2,3": halo tiles at
            32^2 (TW = 32) and 16^2 (TW = 16), Cout = 128 / 192, the concatenated
            widths of the output blocks (256 / 320 / 384 input channels), the phase
            form 192 -> 192 at 16^2; every K1h launch split over K (3 to 8 splits:
            bias, embedding and residual are then added by the reduction)
  probe64   B = 3, image 64, 32 base channels, channel_mult "1,2": its 3x3
            convolutions have 32 / 64 output channels, below the 128 from which the
            planner takes K1h at all (test_probes_take_k1h_plans asserts this): such a
            model stays on its K1s plans, whatever the 64-wide tiles do
  probe64w  B = 3, image 64, 128 base channels, channel_mult "1": K1h at 64^2 -- TW =
            64, split over K, at planned batch 1 / 2 the 64-channel workgroups
  probe64x  B = 2, image 64, 256 base channels, channel_mult "1": at planned batch 8
            its 256 -> 256 and 512 -> 256 convolutions have 128 x 2 = 256 tiles and
            plan ONE split, so the kernel's own epilogue adds the bias, the timestep
            embedding (in_layers) and the residual (out_layers)
  config B's widths at image 16, as test_pointwise_config_b_widths.

Each at planned batch 8, 2 and 1.  Accuracy follows
test_split_unet_has_fp32_accuracy: error against the fp64 oracle at most 2 x the
larger of the fp32 HIP path's and the fp32 CPU oracle's, plus 1e-7 (max) / 1e-8
(mean) of the output scale.

Single convolutions go through cfd_upsample_conv (the phase form; there is no
entry for one plain convolution): low-resolution 16 x 16, 8 x 32 and 4 x 64 (TW =
16 / 32 / 64), Cin of 1, 2 and 3 chunks (3 chunks over 2 splits, uneven ranges;
1 chunk unsplit: test_single_conv_plans asserts both), Cout = 160 and 96 (channel
tails inside a 16-wide block; 96 is below the phase form's 128 and stays on K1s),
and larger images whose samples hold 2 x 3 / 2 x 2 tiles, with an impulse at
every corner and edge midpoint of every tile, so on both sides of every seam.
Element-wise bound, reasoned from the formats (K <= 1440): an activation's hi + lo
pair holds 22 bits and lo * lo is dropped (3 * 2^-22 per product), the fp32
accumulation adds about sqrt(K) * 2^-24 of S = sum |w| |x| + |bias|: within 2^-18 *
S; a phase pack is scaled by one power of two and exact to 2^-24 of that scale: 2^-21
* max |w| * X, X the window's sum of |x|.  |err| <= 2^-18 * S + 2^-21 * max |w| * X;
one wrong tap or halo offset is an error of order |w| |x|, five decades above it.

Against the 32x32x16 development build (make VARIANT=k1h32 VFLAGS=-DCFD_K1H_MFMA32),
where it is present, the errors of both forms to fp64 are printed side by side;
the assertion is the accuracy rule, for both libraries.  Measured on MI355X, new /
old: max 0.81 - 1.05, mean 0.98 - 1.00.
"""
import ast
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from confild_amd import _lib, synth
from confild_amd.script_util import create_model
from oracle import unet as ou

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1H32_SO = os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_k1h32.so")


def _kw(image, ch, mult):
    return dict(image_size=image, num_channels=ch, num_res_blocks=1, num_heads=4, num_head_channels=32,
                attention_resolutions="16", channel_mult=mult)


# name -> (model kwargs, seed, batch)
PROBES = {"probe32": (_kw(32, 64, "2,3"), 61, 3), "probe64": (_kw(64, 32, "1,2"), 62, 3),
          "probe64w": (_kw(64, 128, "1"), 63, 3), "probe64x": (_kw(64, 256, "1"), 64, 2)}
_TS = [999, 420, 3]
_cache = {}


def _build(kw, seed):
    m = create_model(**kw)
    sd = synth.unet_state_dict(seed, {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV), sd


def _oracles(sd, kw, x, t):
    with torch.no_grad():
        cfg = ou.Config(**kw)
        ref64 = ou.forward({k: torch.from_numpy(v).double() for k, v in sd.items()}, cfg, x.double(), t).double()
        cpu32 = ou.forward({k: torch.from_numpy(v) for k, v in sd.items()}, cfg, x, t).double()
    return ref64, (cpu32 - ref64).abs()


def _assert_fp32_accuracy(tag, split, fp32, ref64, e_cpu):
    e32 = (fp32.cpu().double() - ref64).abs()
    esp = (split.cpu().double() - ref64).abs()
    scale = ref64.abs().max().item()
    print(f"{tag}: max|err| vs fp64 / max|ref|: split {esp.max() / scale:.3e} fp32-HIP {e32.max() / scale:.3e} "
          f"cpu-fp32 {e_cpu.max() / scale:.3e}; mean split {esp.mean() / scale:.3e} fp32 {e32.mean() / scale:.3e} "
          f"cpu-fp32 {e_cpu.mean() / scale:.3e}")
    assert esp.max().item() <= 2 * max(e32.max().item(), e_cpu.max().item()) + 1e-7 * scale
    assert esp.mean().item() <= 2 * max(e32.mean().item(), e_cpu.mean().item()) + 1e-8 * scale


def _probe(name):
    """model (left in split compute), inputs, fp64 reference, CPU fp32 error, fp32 HIP output: computed once"""
    if name not in _cache:
        kw, seed, B = PROBES[name]
        S = kw["image_size"]
        m, sd = _build(kw, seed)
        x = torch.from_numpy(synth.normal(seed, "k1h/x", (B, 1, S, S)))
        t = torch.tensor(_TS[:B], dtype=torch.int64)
        ref64, e_cpu = _oracles(sd, kw, x, t)
        m.set_compute("fp32")
        fp32 = m(x.to(DEV), t.to(DEV)).clone()
        m.set_compute("split_f16")
        _cache[name] = (m, x.to(DEV), t.to(DEV), ref64, e_cpu, fp32)
    return _cache[name]


@pytest.fixture(params=list(PROBES))
def probe(request, hip):
    return (request.param,) + _probe(request.param)


@pytest.mark.parametrize("pb", [8, 2, 1])
def test_k1h_shape_has_fp32_accuracy(probe, pb):
    name, m, x, t, ref64, e_cpu, fp32 = probe
    m.set_plan_batch(pb)
    try:
        _assert_fp32_accuracy(f"{name} plan {pb}", m(x, t), fp32, ref64, e_cpu)
    finally:
        m.set_plan_batch(0)


def test_k1h_shape_config_b_widths(hip):
    """Config B's widths at image 16: 256 / 384 / 512 channels at 16^2 (TW = 16) and below, B = 2."""
    g = golden("unet_cfgB64.npz")
    kw = dict(ast.literal_eval(str(g["kwargs"])), image_size=16, channel_mult="1,2,3,4", attention_resolutions="8,4,2")
    m, sd = _build(kw, int(g["seed"]))
    x = torch.from_numpy(synth.normal(34, "k1h/xb", (2, 1, 16, 16)))
    t = torch.tensor([650, 17], dtype=torch.int64)
    ref64, e_cpu = _oracles(sd, kw, x, t)
    out = {}
    for mode in ("fp32", "split_f16"):
        m.set_compute(mode)
        out[mode] = m(x.to(DEV), t.to(DEV)).clone()
    _assert_fp32_accuracy("cfgB widths at 16^2", out["split_f16"], out["fp32"], ref64, e_cpu)
    assert torch.equal(m(x.to(DEV), t.to(DEV)), m.forward_tape(x.to(DEV), t.to(DEV)))


@pytest.mark.parametrize("pb", [8, 2, 1])
def test_k1h_shape_invariants(probe, pb):
    """forward == forward_tape; each sample of the batch == its own B = 1 run; two runs identical."""
    name, m, x, t = probe[:4]
    m.set_plan_batch(pb)
    try:
        full = m(x, t).clone()
        assert torch.equal(m(x, t), full)
        assert torch.equal(m.forward_tape(x, t), full)
        for s in range(x.shape[0]):
            assert torch.equal(m(x[s:s + 1], t[s:s + 1]), full[s:s + 1]), (name, pb, s)
    finally:
        m.set_plan_batch(0)


# --- single convolutions (the phase form) ---------------------------------------------------

# (B, H, W, Cin, Cout): TW = 16, 32, 64 with Cin of 2, 1, 3 chunks; 3 chunks at TW = 16; Cout = 96
SHAPES = [(6, 16, 16, 64, 160), (6, 8, 32, 32, 160), (6, 4, 64, 96, 160), (3, 16, 16, 96, 160), (6, 16, 16, 64, 96)]
# samples of 2 x 3, 2 x 3 and 2 x 2 tiles (tile rows x columns: 16 x 16, 8 x 32, 4 x 64)
SEAMS = [(1, 32, 48, 32, 160, 16, 16), (1, 16, 96, 32, 160, 8, 32), (2, 8, 128, 64, 160, 4, 64)]


def _upconv(x, w, bias, pb):
    """x (B, Cin, H, W) -> (B, Cout, 2H, 2W) through cfd_upsample_conv, and its kernel variant."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.empty((B, 2 * H, 2 * W, Cout), dtype=torch.float32, device=DEV)
    wh, bh = w.contiguous(), bias.contiguous()
    kx = C.c_int(-2)
    _lib.check(_lib.lib().cfd_upsample_conv(_lib.ptr(xd), C.c_void_p(wh.data_ptr()), C.c_void_p(bh.data_ptr()),
                                            _lib.ptr(out), B, H, W, Cin, Cout, pb, 0, C.byref(kx),
                                            _lib.stream_of(DEV)), "cfd_upsample_conv")
    return out.permute(0, 3, 1, 2).cpu(), kx.value


def _ref64(x, w, bias):
    up = F.interpolate(x.double(), scale_factor=2, mode="nearest")
    return F.conv2d(up, w.double(), bias.double(), padding=1)


def _bound(x, w, bias):
    up = F.interpolate(x.double().abs(), scale_factor=2, mode="nearest")
    X = F.conv2d(up, torch.ones((1, x.shape[1], 3, 3), dtype=torch.float64), padding=1)   # >= the window's sum of |x|
    return 2.0 ** -18 * F.conv2d(up, w.double().abs(), bias.double().abs(), padding=1) + \
        2.0 ** -21 * w.abs().max().item() * X


def _weights(shape, seed):
    B, H, W, Cin, Cout = shape
    w = torch.from_numpy(synth.normal(seed, f"k1h/w{shape}", (Cout, Cin, 3, 3))) * 0.1
    b = torch.from_numpy(synth.normal(seed, f"k1h/b{shape}", (Cout,))) * 0.1
    return w, b


@pytest.mark.parametrize("pb", [8, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_single_conv_random(hip, shape, pb):
    B, H, W, Cin, Cout = shape
    w, b = _weights(shape, 71)
    x = torch.from_numpy(synth.normal(72, f"k1h/x{shape}", (B, Cin, H, W)))
    got, kx = _upconv(x, w, b, pb)
    ref = _ref64(x, w, b)
    err, bound = (got.double() - ref).abs(), _bound(x, w, b)
    print(f"{shape} plan {pb} kx {kx}: max err / bound {(err / bound).max():.3f}, "
          f"max err / max ref {err.max() / ref.abs().max():.3e}")
    if os.path.basename(_lib.LIB_PATH) == "libconfild_hip.so":
        assert kx == (24 if Cout >= 128 else -1), (shape, kx)
    assert (err <= bound).all()
    got2, _ = _upconv(x, w, b, pb)
    assert torch.equal(got, got2)
    one, _ = _upconv(x[1:2], w, b, pb)
    assert torch.equal(one, got[1:2])


@pytest.mark.parametrize("pb", [8, 1])
@pytest.mark.parametrize("shape", SEAMS, ids=[str(s) for s in SEAMS])
def test_single_conv_tile_edge_impulses(hip, shape, pb):
    """An impulse at every corner and edge midpoint of every tile (each in its own
    channel and size): the pixels on both sides of every seam between two tiles, and
    the image border, where the halo is zero."""
    B, H, W, Cin, Cout, TR, TW = shape
    w, b = _weights(shape[:5], 73)
    x = torch.zeros((B, Cin, H, W))
    k = 0
    for s in range(B):
        for y0 in range(0, H, TR):
            for x0 in range(0, W, TW):
                for dy in (0, TR // 2, TR - 1):
                    for dx in (0, TW // 2, TW - 1):
                        if (dy, dx) == (TR // 2, TW // 2):
                            continue
                        x[s, (5 * k + 3) % Cin, y0 + dy, x0 + dx] += (1.0 + 0.125 * (k % 7)) * (-1) ** k
                        k += 1
    got, kx = _upconv(x, w, b, pb)
    ref = _ref64(x, w, b)
    err, bound = (got.double() - ref).abs(), _bound(x, w, b)
    print(f"{shape} plan {pb} kx {kx}: {k} impulses, max err {err.max():.3e}, max ref {ref.abs().max():.3e}")
    if os.path.basename(_lib.LIB_PATH) == "libconfild_hip.so":
        assert kx == 24, (shape, kx)
    for py in range(2):
        for px in range(2):
            ok = err[:, :, py::2, px::2] <= bound[:, :, py::2, px::2]
            assert ok.all(), (py, px, err[:, :, py::2, px::2].max().item())


# --- the plans these cases take (CFD_CONV_LOG=1, one child process) ---------------------------

PLAN_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import test_gpu_k1h_shape as T
for name, (kw, seed, B) in T.PROBES.items():
    m, _ = T._build(kw, seed)
    m.set_compute("split_f16")
    S = kw["image_size"]
    x, t = torch.zeros((B, 1, S, S), device=T.DEV), torch.zeros(B, dtype=torch.int64, device=T.DEV)
    for pb in (8, 2, 1):
        m.set_plan_batch(pb)
        print(f"PROBE {name} {pb}", file=sys.stderr, flush=True)
        m(x, t)
        torch.cuda.synchronize()
    del m
for shape in T.SHAPES:
    w, b = T._weights(shape, 71)
    for pb in (8, 1):
        print(f"PROBE {shape} {pb}".replace(", ", ","), file=sys.stderr, flush=True)
        T._upconv(torch.zeros((shape[0], shape[3], shape[1], shape[2])), w, b, pb)
"""
_CONV = re.compile(r"CONV (\S+) (\d+)x(\d+) C=(\d+)\+(\d+)->(\d+) ks=(\d) .* kx=(-?\d+) .* splits=(\d+)")


@pytest.fixture(scope="module")
def plans(hip):
    """(case, planned batch) -> [(name, H, Ctot, Cout, ks, kx, splits)] in launch order"""
    if os.path.basename(_lib.LIB_PATH) != "libconfild_hip.so":
        pytest.skip("a development build is loaded: " + os.path.basename(_lib.LIB_PATH))
    env = dict(os.environ, CFD_CONV_LOG="1")
    r = subprocess.run([sys.executable, "-c", PLAN_CHILD, ROOT], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("PROBE "):
            cur = tuple(line.split()[1:3])
            out[cur] = []
        m = _CONV.match(line)
        if m and cur:
            g = m.groups()
            out[cur].append((g[0], int(g[1]), int(g[3]) + int(g[4]), int(g[5]), int(g[6]), int(g[7]), int(g[8])))
    return out


def test_probes_take_k1h_plans(plans):
    """probe32 and probe64w take K1h (kx 20) split over K at every planned batch, probe32
    the phase form on halo tiles (kx 24) too; probe64x takes K1h with ONE split at
    planned batch 8, in convolutions that carry the embedding (in_layers) and the
    residual (out_layers), and with several at planned batch 2 and 1; probe64's 32 / 64
    output channels never take K1h."""
    for name in PROBES:
        for pb in ("8", "2", "1"):
            convs = plans[(name, pb)]
            k1h = [c for c in convs if c[5] == 20]
            print(name, "plan", pb, "K1h (H, Ctot, Cout, splits):", sorted({(c[1], c[2], c[3], c[6]) for c in k1h}),
                  "phase K1h:", sorted({(c[1], c[2], c[3], c[6]) for c in convs if c[5] == 24}))
            if name == "probe64":
                assert not k1h and not any(c[5] == 24 for c in convs)
                assert all(c[3] < 128 for c in convs if c[4] == 3 and c[1] >= 16)
                continue
            assert {c[1] for c in k1h} == ({32, 16} if name == "probe32" else {64}), (name, pb)
            if name == "probe64x" and pb == "8":
                assert k1h and all(c[6] == 1 for c in k1h), k1h
                assert any("in_layers" in c[0] for c in k1h) and any("out_layers" in c[0] for c in k1h)
                assert any(c[2] > c[3] for c in k1h)   # the output blocks' 512 -> 256
            else:
                assert all(c[6] > 1 for c in k1h), (name, pb, k1h)
            if name == "probe32":
                # the phase form; the concatenated widths (a GroupNorm's output: one source)
                assert any(c[5] == 24 for c in convs) and any(c[2] > c[3] for c in k1h)


def test_single_conv_plans(plans):
    """The single convolutions at planned batch 8: phase form on halo tiles, 1 chunk
    unsplit, 3 chunks over 2 splits (ranges of 2 and 1 chunks); Cout = 96 on K1s."""
    want = {SHAPES[0]: (24, 2), SHAPES[1]: (24, 1), SHAPES[2]: (24, 2), SHAPES[3]: (24, 2)}
    for shape in SHAPES:
        (c,) = plans[(str(shape).replace(", ", ","), "8")]
        print(shape, "kx", c[5], "splits", c[6])
        if shape in want:
            assert (c[5], c[6]) == want[shape], (shape, c)
        else:
            assert c[5] == -1, (shape, c)


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import test_gpu_k1h_shape as T
out = {}
for shape in T.SHAPES[:3]:
    w, b = T._weights(shape, 71)
    x = torch.from_numpy(T.synth.normal(72, f"k1h/x{shape}", (shape[0], shape[3], shape[1], shape[2])))
    got, kx = T._upconv(x, w, b, 8)
    ref = T._ref64(x, w, b)
    err = (got.double() - ref).abs()
    out[str(shape)] = {"max": err.max().item(), "mean": err.mean().item(), "scale": ref.abs().max().item()}
for name in ("probe32", "probe64w"):
    m, x, t, ref64, e_cpu, fp32 = T._probe(name)
    err = (m(x, t).cpu().double() - ref64).abs()
    e32 = (fp32.cpu().double() - ref64).abs()
    out[name] = {"max": err.max().item(), "mean": err.mean().item(), "scale": ref64.abs().max().item(),
                 "lim_max": 2 * max(e32.max().item(), e_cpu.max().item()),
                 "lim_mean": 2 * max(e32.mean().item(), e_cpu.mean().item())}
print(json.dumps(out))
"""


def _child(lib):
    env = dict(os.environ)
    env.pop("CFD_LIB", None)
    if lib:
        env["CFD_LIB"] = lib
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_both_mfma_shapes_have_fp32_accuracy():
    """The 32x32x16 development build and the default build on the same inputs: each
    probe obeys the accuracy rule under both, and the errors to fp64 are printed side
    by side (ratio of max and of mean, new / old)."""
    if not os.path.exists(K1H32_SO):
        pytest.skip("the 32x32x16 development build is absent (make VARIANT=k1h32 VFLAGS=-DCFD_K1H_MFMA32)")
    new, old = _child(None), _child("libconfild_hip_k1h32.so")
    for k in new:
        scale = new[k]["scale"]
        print(f"{k}: 16x16x32 max {new[k]['max']:.3e} mean {new[k]['mean']:.3e}; 32x32x16 max {old[k]['max']:.3e} "
              f"mean {old[k]['mean']:.3e}; ratios {new[k]['max'] / old[k]['max']:.3f} "
              f"{new[k]['mean'] / old[k]['mean']:.3f}")
        for r in (new[k], old[k]):
            if "lim_max" in r:
                assert r["max"] <= r["lim_max"] + 1e-7 * scale, k
                assert r["mean"] <= r["lim_mean"] + 1e-8 * scale, k
