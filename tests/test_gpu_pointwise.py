"""K1p, the pointwise split-f16 GEMM kernel of the 1x1 convolutions (qkv, proj_out,
skip_connection; conv_p.hip), on a probe model whose shapes exercise its edges:

  create_model(image_size=16, num_channels=32, num_res_blocks=1, num_heads=4,
               num_head_channels=32, attention_resolutions="16,8,4", channel_mult="1,2,3")

has 10 attention blocks with qkv 32->96, 64->192 and 96->288 (K of one, two and
three 32-deep tiles, Cout no multiple of 64 or 128) and 8 skip convolutions, six
of them two-source (96+96, 96+64, 64+32, 32+32).  At B = 3 the GEMMs have M = 768,
192 and 48 rows: partial and sub-tile row counts.  The 4^2 attention (T = 16) does
not pack K / V in the qkv epilogue, the 16^2 and 8^2 ones do.

Accuracy follows the rule of test_split_unet_has_fp32_accuracy: the split-f16
error against an fp64 evaluation of the reference forward is at most twice the
larger of the fp32 HIP path's and the fp32 CPU oracle's, plus 1e-7 (maximum) or
1e-8 (mean) of the output scale.
"""
import ast

import pytest
import torch

from conftest import golden
from confild_amd import synth
from confild_amd.script_util import create_model
from oracle import unet as ou

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

PROBE_KW = dict(image_size=16, num_channels=32, num_res_blocks=1, num_heads=4, num_head_channels=32,
                attention_resolutions="16,8,4", channel_mult="1,2,3")


def _build(kw, seed):
    m = create_model(**kw)
    sd = synth.unet_state_dict(seed, {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV), sd


def _oracles(sd, kw, x, t):
    """fp64 reference and the fp32 CPU oracle's error against it."""
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


@pytest.fixture(scope="module")
def probe(hip):
    """The probe model, its B = 3 input, the fp64 reference, the fp32 oracle's error
    and the fp32 HIP forward: computed once, read by every test."""
    m, sd = _build(PROBE_KW, 31)
    x = torch.from_numpy(synth.normal(31, "pw/x", (3, 1, 16, 16)))
    t = torch.tensor([999, 420, 3], dtype=torch.int64)
    ref64, e_cpu = _oracles(sd, PROBE_KW, x, t)
    m.set_compute("fp32")
    fp32 = m(x.to(DEV), t.to(DEV)).clone()
    m.set_compute("split_f16")
    return m, x.to(DEV), t.to(DEV), ref64, e_cpu, fp32


@pytest.mark.parametrize("pb", [8, 1])
def test_pointwise_has_fp32_accuracy(probe, pb):
    m, x, t, ref64, e_cpu, fp32 = probe
    m.set_plan_batch(pb)
    try:
        _assert_fp32_accuracy(f"probe plan {pb}", m(x, t), fp32, ref64, e_cpu)
    finally:
        m.set_plan_batch(0)


@pytest.mark.parametrize("pb", [8, 1])
def test_pointwise_tape_equals_plain(probe, pb):
    m, x, t = probe[:3]
    m.set_plan_batch(pb)
    try:
        assert torch.equal(m(x, t), m.forward_tape(x, t))
    finally:
        m.set_plan_batch(0)


@pytest.mark.parametrize("pb", [1, 2, 8])
def test_pointwise_batch_invariant(probe, pb):
    m, x, t = probe[:3]
    m.set_plan_batch(pb)
    try:
        full = m(x, t).clone()
        for s in range(3):
            assert torch.equal(m(x[s:s + 1], t[s:s + 1]), full[s:s + 1]), (pb, s)
    finally:
        m.set_plan_batch(0)


def test_pointwise_deterministic(probe):
    m, x, t = probe[:3]
    a = m(x, t).clone()
    assert torch.equal(m(x, t), a)


def test_pointwise_config_b_widths(hip):
    """Config B's widths (128-512 channels, the qkv K / V pack, the 512+512 skip) at
    the smallest image: 16^2 ... 2^2, B = 2.  The fixture's kwargs with image_size 16;
    its channel_mult (None: the 64^2 default) and attention_resolutions (image-size
    ratios) are written out for that size so the widths and the attention levels
    (downsampling 2, 4, 8: qkv 256->768, 384->1152, 512->1536) stay config B's."""
    g = golden("unet_cfgB64.npz")
    kw = dict(ast.literal_eval(str(g["kwargs"])), image_size=16, channel_mult="1,2,3,4", attention_resolutions="8,4,2")
    m, sd = _build(kw, int(g["seed"]))
    x = torch.from_numpy(synth.normal(32, "pw/xb", (2, 1, 16, 16)))
    t = torch.tensor([700, 11], dtype=torch.int64)
    ref64, e_cpu = _oracles(sd, kw, x, t)
    out = {}
    for mode in ("fp32", "split_f16"):
        m.set_compute(mode)
        out[mode] = m(x.to(DEV), t.to(DEV)).clone()
    _assert_fp32_accuracy("cfgB widths at 16^2", out["split_f16"], out["fp32"], ref64, e_cpu)
