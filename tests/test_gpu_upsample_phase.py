"""The phase form of the split-f16 Upsample convolutions (nearest 2x, then conv3x3):
four 2x2 convolutions of the low-resolution input on pre-summed taps, one per
output parity (conv_x.hip: conv_h_kernel / conv_x_kernel with PH; the packs:
unet.hip, phase_pack_host).

The planner takes the phase form from 128 output channels (below that an Upsample
convolution keeps its 9-tap K1s plan, as it never ran on K1h / K1x either), so the
probes (built as tests/test_gpu_pointwise.py builds its probe) are the issue's
smallest probe at twice its width:

  PROBE16  image 16, 64 base channels, channel_mult "1,2,3": Upsample convolutions
           192->192 at 4^2 -> 8^2 and 128->128 at 8^2 -> 16^2 on the K1x phase tiles
           (Cout = 192 is no multiple of 128; a sample of 16 or 64 low-resolution
           pixels is smaller than a 128-row tile; B = 3 leaves partial tiles)
  PROBE32  image 32, channel_mult "2,3": 192->192 at 16^2 -> 32^2 on the halo tiles
  config B's widths at image 16 (256 / 384 / 512 channels at 8^2, 4^2, 2^2)

and, through cfd_upsample_conv (one Upsample convolution on its own, planned as the
forward plans it), input channel counts of one, two and three 32-deep chunks with
Cout = 160 (no multiple of 64 or 128): the K1x phase tiles at 4^2 and 8^2, and the
halo-tile kernel at its three tile widths, low-resolution 16 x 16 (TW = 16), 8 x 32
(TW = 32) and 4 x 64 (TW = 64).

Accuracy of the probes follows test_split_unet_has_fp32_accuracy: error against the
fp64 oracle at most 2 x the larger of the fp32 HIP path's and the fp32 CPU oracle's,
plus 1e-7 (max) / 1e-8 (mean) of the output scale.

The single convolutions on random inputs are held to the same rule against torch's
fp32 convolution of the upsampled input (2 x its error plus the 1e-7 / 1e-8 terms).
The element-wise bound of the impulse and random tests is reasoned from the formats.  Relative part: an
activation's hi + lo pair holds 22 bits and the lo * lo term is dropped (at most
3 * 2^-22 per product); the fp32 accumulation of K <= 1440 terms adds about
sqrt(K) * 2^-24 <= 2^-18.7 of S = sum |w| |x| + |bias|: together within 2^-18 * S.
Absolute part: a pack is scaled by one power of two 2^-e per phase, 2^e <= 2 max
|tap sum| <= 8 max |w|, and its hi + lo pair is exact to 2^-24 of that scale whatever
the size of the single weight, so a product is off by up to 2^-21 max |w| |x|: in all
2^-21 * max |w| * X, X the sum of |x| over the window.  The test asserts
|err| <= 2^-18 * S + 2^-21 * max |w| * X per output element.  A tap assigned to the
wrong phase or input is an error of order |w| |x|, five decades above it.
"""
import ast
import ctypes as C
import json
import os
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
NOUP_SO = os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_noupphase.so")

PROBE16 = dict(image_size=16, num_channels=64, num_res_blocks=1, num_heads=4, num_head_channels=32,
               attention_resolutions="16,8,4", channel_mult="1,2,3")
PROBE32 = dict(image_size=32, num_channels=64, num_res_blocks=1, num_heads=4, num_head_channels=32,
               attention_resolutions="16", channel_mult="2,3")


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


def _probe(kw, seed):
    S = kw["image_size"]
    m, sd = _build(kw, seed)
    x = torch.from_numpy(synth.normal(seed, "up/x", (3, 1, S, S)))
    t = torch.tensor([999, 420, 3], dtype=torch.int64)
    ref64, e_cpu = _oracles(sd, kw, x, t)
    m.set_compute("fp32")
    fp32 = m(x.to(DEV), t.to(DEV)).clone()
    m.set_compute("split_f16")
    return m, x.to(DEV), t.to(DEV), ref64, e_cpu, fp32, sd


@pytest.fixture(scope="module")
def probe16(hip):
    return _probe(PROBE16, 41)


@pytest.fixture(scope="module")
def probe32(hip):
    return _probe(PROBE32, 42)


@pytest.fixture(params=["probe16", "probe32"])
def probe(request):
    return request.getfixturevalue(request.param)


@pytest.mark.parametrize("pb", [8, 1])
def test_upsample_phase_has_fp32_accuracy(probe, pb):
    m, x, t, ref64, e_cpu, fp32 = probe[:6]
    m.set_plan_batch(pb)
    try:
        _assert_fp32_accuracy(f"image {m.image_size} plan {pb}", m(x, t), fp32, ref64, e_cpu)
    finally:
        m.set_plan_batch(0)


def test_upsample_phase_config_b_widths(hip):
    """Config B's widths at image 16 (as test_pointwise_config_b_widths): the 512-,
    384- and 256-channel Upsample convolutions at 2^2, 4^2 and 8^2, B = 2."""
    g = golden("unet_cfgB64.npz")
    kw = dict(ast.literal_eval(str(g["kwargs"])), image_size=16, channel_mult="1,2,3,4", attention_resolutions="8,4,2")
    m, sd = _build(kw, int(g["seed"]))
    x = torch.from_numpy(synth.normal(33, "up/xb", (2, 1, 16, 16)))
    t = torch.tensor([700, 11], dtype=torch.int64)
    ref64, e_cpu = _oracles(sd, kw, x, t)
    out = {}
    for mode in ("fp32", "split_f16"):
        m.set_compute(mode)
        out[mode] = m(x.to(DEV), t.to(DEV)).clone()
    _assert_fp32_accuracy("cfgB widths at 16^2", out["split_f16"], out["fp32"], ref64, e_cpu)
    assert torch.equal(m(x.to(DEV), t.to(DEV)), m.forward_tape(x.to(DEV), t.to(DEV)))


@pytest.mark.parametrize("pb", [8, 1])
def test_upsample_phase_tape_equals_plain(probe, pb):
    m, x, t = probe[:3]
    m.set_plan_batch(pb)
    try:
        assert torch.equal(m(x, t), m.forward_tape(x, t))
    finally:
        m.set_plan_batch(0)


@pytest.mark.parametrize("pb", [1, 2, 8])
def test_upsample_phase_batch_invariant(probe, pb):
    m, x, t = probe[:3]
    m.set_plan_batch(pb)
    try:
        full = m(x, t).clone()
        for s in range(3):
            assert torch.equal(m(x[s:s + 1], t[s:s + 1]), full[s:s + 1]), (pb, s)
    finally:
        m.set_plan_batch(0)


def test_upsample_phase_deterministic(probe):
    m, x, t = probe[:3]
    a = m(x, t).clone()
    assert torch.equal(m(x, t), a)


def test_set_param_rebuilds_the_phase_pack(probe16):
    """cfd_unet_set_param on an Upsample weight alone: the forward follows the new
    weight (bit-equal to a model built with it), so the phase pack was rebuilt."""
    m0, x, t = probe16[:3]
    sd = dict(probe16[6])
    keys = [k for k in sd if k.endswith(".conv.weight") and sd[k].ndim == 4 and "output_blocks" in k]
    assert len(keys) == 2 and all(sd[k].shape[0] >= 128 for k in keys), keys
    m, _ = _build(PROBE16, 41)
    before = m(x, t).clone()
    assert torch.equal(before, m0(x, t))
    lib = _lib.lib()
    h = m._handle(DEV)
    for k in keys:
        w = torch.from_numpy(synth.normal(77, "up/neww/" + k, tuple(sd[k].shape))) * float(abs(sd[k]).max()) * 3.0
        sd[k] = w.numpy()
        host = w.contiguous()
        _lib.check(lib.cfd_unet_set_param(h, k.encode(), C.c_void_p(host.data_ptr()), host.numel()), "set_param")
    after = m(x, t).clone()
    fresh = create_model(**PROBE16)
    fresh.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    want = fresh.to(DEV)(x, t)
    assert not torch.equal(after, before)
    assert torch.equal(after, want)


# --- one Upsample convolution on its own ------------------------------------------------

# (B, H, W, Cin, Cout): K1x phase tiles (sub-tile and partial row counts), then the
# halo tiles at TW = 16, 32, 64; Cout is no multiple of 64
SHAPES = [(3, 4, 4, 96, 160), (3, 8, 8, 32, 160), (6, 16, 16, 64, 160), (6, 8, 32, 32, 160), (6, 4, 64, 96, 160)]


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
    w = torch.from_numpy(synth.normal(seed, f"up1/w{shape}", (Cout, Cin, 3, 3))) * 0.1
    b = torch.from_numpy(synth.normal(seed, f"up1/b{shape}", (Cout,))) * 0.1
    return w, b


@pytest.mark.parametrize("pb", [8, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_single_upsample_conv_impulses(hip, shape, pb):
    """An impulse at each corner, on an edge and in the interior (one per sample,
    samples cycling over them, each in another channel): every output phase against the
    float64 convolution of the upsampled impulse."""
    B, H, W, Cin, Cout = shape
    w, b = _weights(shape, 51)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W // 2 - 1)]
    x = torch.zeros((B, Cin, H, W))
    for s in range(B):
        y, xx = spots[s % 6] if B >= 6 else spots[2 * s]
        x[s, (7 * s + 5) % Cin, y, xx] = 1.0 + 0.25 * s
    if B < 6:   # the other three spots, in other channels of the same samples
        for s in range(B):
            y, xx = spots[2 * s + 1]
            x[s, (11 * s + 8) % Cin, y, xx] = -0.75
    got, kx = _upconv(x, w, b, pb)
    ref = _ref64(x, w, b)
    err = (got.double() - ref).abs()
    print(f"{shape} plan {pb} kx {kx}: max err {err.max():.3e}, max ref {ref.abs().max():.3e}")
    bound = _bound(x, w, b)
    for py in range(2):     # each phase on its own, so a message names it
        for px in range(2):
            ok = err[:, :, py::2, px::2] <= bound[:, :, py::2, px::2]
            assert ok.all(), (py, px, err[:, :, py::2, px::2].max().item())


@pytest.mark.parametrize("pb", [8, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_single_upsample_conv_random(hip, shape, pb):
    B, H, W, Cin, Cout = shape
    w, b = _weights(shape, 52)
    x = torch.from_numpy(synth.normal(53, f"up1/x{shape}", (B, Cin, H, W)))
    got, kx = _upconv(x, w, b, pb)
    ref = _ref64(x, w, b)
    err = (got.double() - ref).abs()
    bound = _bound(x, w, b)
    print(f"{shape} plan {pb} kx {kx}: max err / bound {(err / bound).max():.3f}, "
          f"max err / max ref {err.max() / ref.abs().max():.3e}")
    assert (err <= bound).all()
    # the fp32-parity rule on the same inputs: at most 2 x the error of torch's fp32
    # convolution of the upsampled input, plus 1e-7 (max) / 1e-8 (mean) of the output scale
    f32 = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1).double()
    e32, scale = (f32 - ref).abs(), ref.abs().max().item()
    print(f"   fp32 conv: max {e32.max():.3e} mean {e32.mean():.3e}; split: max {err.max():.3e} mean {err.mean():.3e}")
    assert err.max().item() <= 2 * e32.max().item() + 1e-7 * scale
    assert err.mean().item() <= 2 * e32.mean().item() + 1e-8 * scale
    got2, _ = _upconv(x, w, b, pb)
    assert torch.equal(got, got2)
    # batch invariance of the single convolution: sample 1 alone
    one, _ = _upconv(x[1:2], w, b, pb)
    assert torch.equal(one, got[1:2])


def test_default_build_runs_the_phase_forms(hip):
    """The planner sends these shapes to the phase kernels (24: halo tiles, 25 / 26: K1x),
    and an Upsample convolution of fewer than 128 output channels to its 9-tap plan."""
    # the default library only: a development build named by CFD_LIB (the 9-tap one) plans otherwise
    if os.path.basename(_lib.LIB_PATH) != "libconfild_hip.so":
        pytest.skip("a development build is loaded: " + os.path.basename(_lib.LIB_PATH))
    for shape, want in zip(SHAPES, (25, 25, 24, 24, 24)):
        w, b = _weights(shape, 52)
        _, kx = _upconv(torch.zeros((shape[0], shape[3], shape[1], shape[2])), w, b, 8)
        assert kx == want, (shape, kx)
    w = torch.zeros((96, 64, 3, 3))
    _, kx = _upconv(torch.zeros((1, 64, 8, 8)), w, torch.zeros(96), 8)
    assert kx not in (24, 25, 26), kx


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import test_gpu_upsample_phase as T
out = {}
for shape in T.SHAPES:
    w, b = T._weights(shape, 52)
    x = torch.from_numpy(T.synth.normal(53, f"up1/x{shape}", (shape[0], shape[3], shape[1], shape[2])))
    got, kx = T._upconv(x, w, b, 8)
    ref = T._ref64(x, w, b)
    err = (got.double() - ref).abs()
    out[str(shape)] = {"kx": kx, "max": err.max().item(), "mean": err.mean().item(), "scale": ref.abs().max().item()}
m, x, t, ref64 = T._probe(T.PROBE32, 42)[:4]
err = (m(x, t).cpu().double() - ref64).abs()
out["probe32"] = {"max": err.max().item(), "mean": err.mean().item(), "scale": ref64.abs().max().item()}
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


def test_phase_form_is_as_accurate_as_the_nine_tap_build():
    """Against the 9-tap development build (make VARIANT=noupphase VFLAGS=-DCFD_NO_UPPHASE),
    on the same inputs: the phase form's error to fp64 is at most 2 x the 9-tap form's,
    plus 1e-7 (max) / 1e-8 (mean) of the output scale."""
    if not os.path.exists(NOUP_SO):
        pytest.skip("the 9-tap development build is absent (make VARIANT=noupphase VFLAGS=-DCFD_NO_UPPHASE)")
    ph, nine = _child(None), _child("libconfild_hip_noupphase.so")
    for k in ph:
        scale = ph[k]["scale"]
        print(f"{k}: phase max {ph[k]['max']:.3e} mean {ph[k]['mean']:.3e}; 9-tap max {nine[k]['max']:.3e} "
              f"mean {nine[k]['mean']:.3e}; ratios {ph[k]['max'] / nine[k]['max']:.3f} "
              f"{ph[k]['mean'] / nine[k]['mean']:.3f}")
        if "kx" in ph[k]:
            assert ph[k]["kx"] in (24, 25, 26) and nine[k]["kx"] not in (24, 25, 26), (k, ph[k], nine[k])
        assert ph[k]["max"] <= 2 * nine[k]["max"] + 1e-7 * scale, k
        assert ph[k]["mean"] <= 2 * nine[k]["mean"] + 1e-8 * scale, k
