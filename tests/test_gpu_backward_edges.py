"""The U-Net backward -- the input VJP (K9 / K9s: cfd_unet_input_vjp) and the
parameter gradients (K11: cfd_unet_param_grad) -- against float64 autograd
through the CPU oracle U-Net, at the shapes, plans and workgroup sizes the
golden topologies (tiny16 ... wide128: power-of-two images, default plan,
T % 32 == 0, head channels <= 64) never reach.

Topologies (num_res_blocks 1, num_heads 4, inputs and d_eps from synth.normal):

  probe16  test_gpu_pointwise.py's probe model (16^2, 32 ch, mult "1,2,3", head
           channels 32, attention at 16^2 / 8^2 / 4^2), B = 3: T = 256 with one head,
           T = 64 with two, T = 16 with three (the backward pads it to T32 = 32;
           heads x B = 9: no XCD map); 96-channel GroupNorms (3 channels per
           group); 96+64, 96+96 and 64+32 two-source skips in the weight gradients.
  odd24    24^2, 32 ch, mult "1,2", head channels 32, attention at 24^2 / 12^2,
           B = 2: T = 576 (18 key blocks) and T = 144 (5 key blocks, the last half
           masked; K / V packed by attn_kv_split_kernel, not the qkv epilogue);
           non-power-of-two tiles in every convolution and GroupNorm.
  head128  16^2, 128 ch, mult "1,2", head channels 128, attention at 16^2 / 8^2,
           B = 2: the CH = 128 instantiations of K4d (key-chunked at T = 256, plain
           at T = 64), attn_combine_kernel and the split attention backward.

Key chunks of the forward attention (attention_kv_chunks(T, heads, plan) of
unet_kernels.hip, mirrored by _kv_chunks below and asserted against this table
in test_backward_matches_fp64_autograd; the library does not export its plan):

  T = 256, 1 head  (probe16, head128)  plans 8, 1, 2: kc = 4
  T = 64,  2 heads (probe16, head128)  plans 8, 1, 2: kc = 1
  T = 16,  3 heads (probe16)           plans 8, 1, 2: kc = 1
  T = 576, 1 head  (odd24)             plan 8: kc = 2; plans 1, 2: kc = 8, 3 blocks
                                       per chunk, so chunks 6 and 7 are empty and
                                       hand (m, l) = (-inf, 0) to the combine pass
  T = 144, 2 heads (odd24)             plans 8, 1, 2: kc = 2 (3 + 2 blocks)
  T = 1024, 2 heads (wave-count case)  plan 8: kc = 1

Bounds.  fp32 compute, the project's existing ones: eps within 1e-5 of
max(1, max|ref|) (test_gpu_parity.py), g_x within 2e-4 of max|g_x|
(test_gpu_dps.py), each parameter gradient within 2e-4 of
max(max|ref_k|, 1e-3 gmax) (test_gpu_unet_train.py).  The fp32 CPU oracle alone,
against the same float64 reference, reaches eps 8.4e-7 / g_x 1.8e-6 / worst
parameter gradient 5.0e-5 (probe16), 6.8e-7 / 1.4e-6 / 5.6e-5 (odd24) and
6.9e-7 / 7.7e-7 / 2.4e-6 (head128): the bounds hold for the reference by itself.
(The worst parameter gradients are biases in front of a GroupNorm, which vanish
analytically and sit at the floor; over synth seeds 31, 32, 33 and 41 the oracle's
own error there is 4.5e-5 ... 1.2e-4, and the seeds used are its quietest.)
(On another host the oracle's float32 sums come out in another order: the GPU
machine's figures are in the table below.)  Split compute, the project's split
criterion: for eps, g_x and every parameter gradient tensor the error against
float64 is at most 2 x max(fp32-HIP error, fp32-CPU-oracle error) + 1e-7 of
the scale (max|ref| for eps and g_x, gmax for the parameter gradients), and for
eps the same rule on the mean error with 1e-8.

Measured on an MI355X (error / scale; "pg" the worst parameter gradient under
the floor rule; worst over plans 8, 1, 2 and both tapes):
             fp32 HIP                      split                         fp32 CPU oracle (that host)
  probe16    eps 1.3e-6 g_x 1.6e-6 pg 2.3e-5   6.7e-7 / 2.2e-6 / 5.4e-5      8.1e-7 / 1.9e-6 / 5.7e-5
  odd24      eps 7.1e-7 g_x 1.6e-6 pg 2.9e-5   6.9e-7 / 1.3e-6 / 6.7e-5      7.0e-7 / 1.3e-6 / 9.2e-5
  head128    eps 8.1e-7 g_x 1.0e-6 pg 2.5e-6   6.8e-7 / 1.4e-6 / 5.8e-6      7.0e-7 / 1.1e-6 / 2.4e-6

(the two tapes give the same figures; the plans differ only on odd24's split eps,
5.9e-7 at plan 8 and 6.9e-7 at plans 1 / 2, and its pg, 6.7e-5 / 6.6e-5).  The
B = 16 wave-count case: eps 8.0e-7 / 5.6e-7 / 5.9e-7 and g_x 7.6e-7 / 1.6e-6 /
6.7e-7 (fp32 HIP / split / oracle).  The T = 36 forward: 4.3e-7 / 4.3e-7 / 4.4e-7.

Mutation checks (scratch builds): a combine pass that drops chunk 5 of kc = 8 and
chunk 3 of the CH = 128 instantiation fails odd24 at plans 1 and 2 and head128 at
every plan, and no earlier gradient test (test_gpu_dps.py, test_gpu_unet_train.py,
test_gpu_plan_batch.py); one that drops chunk 3 at every head width is also caught
by small32 and heads16 there (kc = 4 at the default plan).  A split attention
backward whose packs pad with the last token instead of zeros and whose dq kernel
does not mask the padded keys fails probe16 and odd24 at every plan (T = 16, 144),
and of the earlier tests only cfgA32's input VJP (its 4^2 middle block).
"""
import pytest
import torch

from confild_amd import _lib, synth
from confild_amd.script_util import create_model
from oracle import unet as ou
from test_gpu_pointwise import PROBE_KW

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

_COMMON = dict(num_res_blocks=1, num_heads=4)
TOPOLOGIES = {
    # name: (keyword arguments, B, seed, timesteps)
    "probe16": (PROBE_KW, 3, 41, [999, 420, 3]),
    "odd24": (dict(_COMMON, image_size=24, num_channels=32, num_head_channels=32, attention_resolutions="24,12",
                   channel_mult="1,2"), 2, 32, [870, 15]),
    "head128": (dict(_COMMON, image_size=16, num_channels=128, num_head_channels=128, attention_resolutions="16,8",
                     channel_mult="1,2"), 2, 31, [640, 7]),
}
# (T, heads) of every attention level, and the key chunks at plans (8, 1, 2)
KV_CHUNKS = {
    "probe16": {(256, 1): (4, 4, 4), (64, 2): (1, 1, 1), (16, 3): (1, 1, 1)},
    "odd24": {(576, 1): (2, 8, 8), (144, 2): (2, 2, 2)},
    "head128": {(256, 1): (4, 4, 4), (64, 2): (1, 1, 1)},
}
WAVES_KW = dict(_COMMON, image_size=32, num_channels=128, num_head_channels=64, attention_resolutions="32",
                channel_mult="1")
T36_KW = dict(_COMMON, image_size=6, num_channels=32, num_head_channels=32, attention_resolutions="6",
              channel_mult="1")


def _kv_chunks(T, heads, plan):
    """attention_kv_chunks of unet_kernels.hip: chunks of >= 2 key blocks while the
    planned batch's 64-query grid times the chunks stays within 256 workgroups."""
    nblk, wgs, kc = (T + 31) // 32, plan * heads * ((T + 63) // 64), 1
    while kc * 4 <= nblk and wgs * kc * 2 <= 256:
        kc *= 2
    return kc


def _build(kw, seed):
    m = create_model(**kw)
    sd = synth.unet_state_dict(seed, {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV), sd


def _autograd(kw, sd, x, t, d, dtype, params=True):
    """eps, g_x and the parameter gradients of the oracle forward in ``dtype``, as float64."""
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(params) for k, v in sd.items()}
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    eps = ou.forward(p, ou.Config(**kw), xr, t)
    grads = torch.autograd.grad(eps, [xr] + (list(p.values()) if params else []), d.to(dtype))
    return eps.detach().double(), grads[0].double(), {k: g.double() for k, g in zip(p, grads[1:])}


class _Case:
    """One topology: the model, its inputs, the float64 reference (eps, g_x, every
    parameter gradient) and the fp32 CPU oracle's errors against it -- computed
    once, read by every test, never modified."""

    def __init__(self, kw, B, seed, ts, params=True):
        self.kw, self.B = kw, B
        self.m, sd = _build(kw, seed)
        S = kw["image_size"]
        x = torch.from_numpy(synth.normal(seed, "bwd/x", (B, 1, S, S)))
        d = torch.from_numpy(synth.normal(seed, "bwd/deps", (B, 1, S, S)))
        t = torch.tensor(ts, dtype=torch.int64)
        self.ref = _autograd(kw, sd, x, t, d, torch.float64, params)
        self.gmax = max((float(g.abs().max()) for g in self.ref[2].values()), default=0.0)
        self.e_cpu = self.errors(_autograd(kw, sd, x, t, d, torch.float32, params))
        self.x, self.t, self.d = x.to(DEV), t.to(DEV), d.to(DEV)

    def errors(self, got):
        """(|eps error| tensor, max g_x error, {key: max parameter-gradient error})."""
        eps, gx, pg = got
        return ((eps - self.ref[0]).abs(), float((gx - self.ref[1]).abs().max()),
                {k: float((pg[k] - r).abs().max()) for k, r in self.ref[2].items()})

    def unpack(self, flat):
        named, out, o = dict(self.m.named_parameters()), {}, 0
        flat = flat.cpu().double()
        for k in self.m.param_keys():
            n = named[k].numel()
            out[k] = flat[o:o + n].reshape(named[k].shape)
            o += n
        assert o == flat.numel()
        return out

    def backward(self, kept, params=True):
        """Plain forward, taped forward (the same bits), input VJP and parameter
        gradients of the batch in the model's current compute and plan."""
        m = self.m
        plain = m(self.x, self.t).clone()
        eps = m.forward_tape(self.x, self.t, for_param_grad=kept)
        assert torch.equal(eps, plain), "forward_tape differs from the plain forward"
        gx = m.input_vjp(self.d).clone()
        flat = m.param_grad(self.d) if params else None
        for name, v in (("eps", eps), ("g_x", gx), ("param_grad", flat)):
            assert v is None or bool(torch.isfinite(v).all()), f"{name} is not finite"
        return eps.cpu().double(), gx.cpu().double(), self.unpack(flat) if params else {}

    def pg_rel(self, e_pg):
        """The worst parameter-gradient error under the floor rule, with its key."""
        return max((e / max(float(self.ref[2][k].abs().max()), 1e-3 * self.gmax), k) for k, e in e_pg.items())

    def check(self, tag, kept, params=True):
        """The fp32 bounds and the split criterion of one (plan, tape) on this case."""
        err = {}
        for mode in ("fp32", "split_f16"):
            self.m.set_compute(mode)
            err[mode] = self.errors(self.backward(kept, params))
        ref_eps, ref_gx, _ = self.ref
        s_eps, s_gx, ec = float(ref_eps.abs().max()), float(ref_gx.abs().max()), self.e_cpu
        e32, esp = err["fp32"], err["split_f16"]
        line = f"{tag} {'kept' if kept else 'recomputed'} tape:"
        for mode, e in (("fp32-HIP", e32), ("split", esp), ("cpu-fp32", ec)):
            line += (f" {mode} eps {e[0].max() / s_eps:.2e} (mean {e[0].mean() / s_eps:.2e}) g_x {e[1] / s_gx:.2e}"
                     + (f" pg {self.pg_rel(e[2])[0]:.2e};" if params else ";"))
        print(line)
        # fp32 compute: the existing absolute bounds
        assert float(e32[0].max()) <= 1e-5 * max(1.0, s_eps), (tag, float(e32[0].max()), s_eps)
        assert e32[1] <= 2e-4 * s_gx, (tag, e32[1], s_gx)
        if params:
            worst = self.pg_rel(e32[2])
            assert worst[0] <= 2e-4, (tag, worst)
        # split compute: within twice the fp32 level, tensor by tensor
        assert float(esp[0].max()) <= 2 * max(float(e32[0].max()), float(ec[0].max())) + 1e-7 * s_eps, tag
        assert float(esp[0].mean()) <= 2 * max(float(e32[0].mean()), float(ec[0].mean())) + 1e-8 * s_eps, tag
        assert esp[1] <= 2 * max(e32[1], ec[1]) + 1e-7 * s_gx, (tag, esp[1], e32[1], ec[1])
        for k in esp[2]:
            assert esp[2][k] <= 2 * max(e32[2][k], ec[2][k]) + 1e-7 * self.gmax, (tag, k, esp[2][k], e32[2][k],
                                                                                    ec[2][k], self.gmax)


@pytest.fixture(scope="module", params=list(TOPOLOGIES))
def topo(hip, request):
    return request.param, _Case(*TOPOLOGIES[request.param])


@pytest.mark.parametrize("pb", [8, 1, 2])
def test_backward_matches_fp64_autograd(topo, pb):
    """eps, the input VJP and every parameter gradient of fp32 and split compute at
    plans 8, 1 and 2, with the recomputed and the kept-output tape, against float64
    autograd: forward_tape bit-equal to the plain forward, every output finite (the
    empty key chunks of odd24 at plans 1 and 2 included), the bounds of the module
    docstring."""
    name, case = topo
    for (T, heads), kcs in KV_CHUNKS[name].items():
        assert tuple(_kv_chunks(T, heads, p) for p in (8, 1, 2)) == kcs, (T, heads)
    case.m.set_plan_batch(pb)
    try:
        for kept in (False, True):
            case.check(f"{name} plan {pb}", kept)
    finally:
        case.m.set_plan_batch(0)
        case.m.set_compute("split_f16")


@pytest.mark.parametrize("pb", [8, 1])
def test_backward_bits_are_batch_invariant(topo, pb):
    """Split compute: each sample's input VJP taped alone equals its rows of the
    batch's, bit for bit (the key chunks, the T32 padding and the 4- / 8-wave choice
    depend on the plan and T only), and the batch's parameter gradients repeat."""
    name, case = topo
    m, x, t, d = case.m, case.x, case.t, case.d
    m.set_compute("split_f16")
    m.set_plan_batch(pb)
    try:
        m.forward_tape(x, t)
        full = m.input_vjp(d).clone()
        g1 = m.param_grad(d).clone()
        for s in range(case.B):
            m.forward_tape(x[s:s + 1], t[s:s + 1])
            assert torch.equal(m.input_vjp(d[s:s + 1]), full[s:s + 1]), (name, pb, s)
        m.forward_tape(x, t)
        assert torch.equal(m.param_grad(d), g1), (name, pb)
    finally:
        m.set_plan_batch(0)


def test_attention_wave_count_changes_no_bits(hip):
    """32^2, 128 ch, one level, head channels 64: T = 1024 with 2 heads (kc = 1 at the
    default plan).  At B = 16 the attention forward (ceil(T / 128) x heads x B = 256
    workgroups: the threshold) and the split backward take their 8-wave
    workgroups, at B = 8 the 4-wave ones: eps and the input VJP of the batch of 16
    equal those of its two halves bit for bit, and g_x of the batch meets the split
    criterion against float64 autograd."""
    case = _Case(WAVES_KW, 16, 54, [999, 3, 500, 40, 700, 250, 120, 880, 1, 333, 610, 75, 940, 460, 20, 808],
                 params=False)
    assert _kv_chunks(1024, 2, 8) == 1
    m, x, t, d = case.m, case.x, case.t, case.d
    try:
        case.check("waves B=16", False, params=False)
        m.set_compute("split_f16")
        eps = m.forward_tape(x, t).clone()
        gx = m.input_vjp(d).clone()
        for lo in (0, 8):
            sl = slice(lo, lo + 8)
            assert torch.equal(m.forward_tape(x[sl], t[sl]), eps[sl]), lo
            assert torch.equal(m.input_vjp(d[sl]), gx[sl]), lo
    finally:
        m.set_compute("split_f16")


def test_attention_backward_refuses_t36(hip):
    """A 6^2 one-level model: its attention has T = 36, T % 16 != 0.  The Python
    layer accepts the model and the forward runs in both computes and matches
    float64; the backward (input_vjp and param_grad alike) raises CfdError naming
    the T % 16 requirement before its first launch, and the model stays usable."""
    case = _Case(T36_KW, 2, 55, [900, 30], params=False)
    m, x, t, d = case.m, case.x, case.t, case.d
    ref = case.ref[0]
    scale = float(ref.abs().max())
    out = {}
    for mode in ("fp32", "split_f16"):
        m.set_compute(mode)
        out[mode] = m(x, t).clone()
        e = {k: (v.cpu().double() - ref).abs() for k, v in out.items()}
        assert torch.equal(m.forward_tape(x, t), out[mode])
        with pytest.raises(_lib.CfdError, match="T % 16"):
            m.input_vjp(d)
        with pytest.raises(_lib.CfdError, match="T % 16"):
            m.param_grad(d)
        assert torch.equal(m(x, t), out[mode])
    ec = case.e_cpu[0]
    print(f"T = 36 forward: fp32-HIP {e['fp32'].max() / scale:.2e} split {e['split_f16'].max() / scale:.2e} "
          f"cpu-fp32 {ec.max() / scale:.2e}")
    assert float(e["fp32"].max()) <= 1e-5 * max(1.0, scale)
    assert float(e["split_f16"].max()) <= 2 * max(float(e["fp32"].max()), float(ec.max())) + 1e-7 * scale
    assert float(e["split_f16"].mean()) <= 2 * max(float(e["fp32"].mean()), float(ec.mean())) + 1e-8 * scale
