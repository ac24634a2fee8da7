"""GPU: the 'inpainting' operator under 'ps' (A(x0) = mask * x0 on the latent image).

* the guided DDPM / DDIM loops against the reference's own runs
  (tests/golden/dps_inpaint_*.npz, make_golden_dps_inpaint.py), replaying its
  recorded noise, at the tolerances of test_gpu_dps.py::test_dps_loop_matches_reference;
* cfd_dps_latent_residual alone against a float64 restatement of the same fp32 inputs
  (one pass, a tail, and more than one workgroup per sample);
* a zero residual norm gives a zero gradient: the conditioned image is the
  unconditioned sample, bit for bit;
* a batch of chains with per-sample measurements and masks equals the chains run
  one by one (bit-exact), at 24^2 (not a multiple of the 4096-element chunk or of
  256) and at attention plans 8 and 1.

Bound of the kernel test: x0, m * x0, y - m * x0, r / norm, the product with m and
the product with sra / srm1 are at most six fp32 roundings per element (2^-24
relative each), on operands no larger than the tensors' own scale -- the inputs
are chosen that way: |sra x|, |srm1 eps| of order 1 and residuals up to about 1 --
so 1e-6 of each tensor's maximum; the norm is a float64 sum cast to fp32, 1e-6
relative.
"""
import ast
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from confild_amd import _lib, synth
from confild_amd.script_util import create_gaussian_diffusion

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _ps(scale):
    from confild_amd.guided.condition_methods import get_conditioning_method
    from confild_amd.guided.measurements import get_noise, get_operator
    return get_conditioning_method(operator=get_operator("inpainting", device=DEV),
                                   noiser=get_noise(sigma=0.0, name="gaussian"), name="ps", scale=scale)


def _sampler(name, respacing):
    from confild_amd.guided.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                          model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=False, timestep_respacing=respacing)


def _tiny16(g):
    from confild_amd.guided.unet import create_model as guided_model
    kw = ast.literal_eval(str(g["kwargs"]))
    model = guided_model(**kw)                         # no model_path: random init (weights set below)
    sd = synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(DEV)


@pytest.mark.parametrize("name", ["dps_inpaint_rows", "dps_inpaint_frac"])
def test_inpaint_loop_matches_reference(hip, name):
    g = golden(f"{name}.npz")
    model = _tiny16(g)
    cond = _ps(float(g["scale"]))
    sampler = _sampler(str(g["sampler"]), str(g["respacing"]))
    y = torch.from_numpy(g["measurement"]).to(DEV)
    mask = torch.from_numpy(g["mask"])
    fn = functools.partial(cond.conditioning, mask=mask)
    steps = len(g["img"])
    # per step, from the reference's own state (isolates each step's arithmetic)
    for k in range(steps):
        xin = torch.from_numpy(g["x_start"] if k == 0 else g["img"][k - 1]).to(DEV)
        out = sampler.p_sample_step(model, xin, steps - 1 - k, y, fn, noise=torch.from_numpy(g["step_noise"][k]))
        lat = max(1.0, float(np.abs(g["img"][k]).max()))
        for key, ref in (("pred_xstart", g["x0"][k]), ("x_t", g["sample"][k]), ("sample", g["img"][k])):
            err = float(np.abs(out[key].cpu().numpy() - ref).max()) / lat
            print(f"{name} step {k} {key}: {err:.3e}")
            assert err < 1e-4, (k, key, err)
        derr = abs(float(out["distance"][0]) - g["dist"][k])
        print(f"{name} step {k} distance: {derr:.3e} of {g['dist'][k]:.4f}")
        assert derr < 1e-4 * max(1.0, g["dist"][k])
    # and the whole loop from x_start
    x = torch.from_numpy(g["x_start"]).to(DEV)
    out = sampler.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=fn, record=False,
                                save_root=None, step_noise=torch.from_numpy(g["step_noise"]))
    err = float(np.abs(out.cpu().numpy() - g["out"]).max()) / max(1.0, float(np.abs(g["out"]).max()))
    dist = sampler.distances[:, 0].cpu().numpy()
    print(f"{name} loop: {err:.3e}, distances {np.abs(dist - g['dist']).max():.3e}")
    assert err < 5e-4, err
    assert np.abs(dist - g["dist"]).max() < 1e-3 * max(1.0, g["dist"].max())


def test_inpaint_argument_errors(hip):
    g = golden("dps_inpaint_rows.npz")
    model = _tiny16(g)
    cond = _ps(1.0)
    sampler = _sampler("ddpm", "4")
    x = torch.zeros(2, 1, 16, 16, device=DEV)
    y = torch.zeros(1, 1, 16, 16, device=DEV)
    with pytest.raises(ValueError, match="Require mask"):
        sampler.p_sample_loop(model, x, y, functools.partial(cond.conditioning))
    for bad_mask, bad_y in ((torch.ones(3, 1, 16, 16), y), (torch.ones(1, 1, 16, 8), y),
                            (torch.ones(16, 16), torch.zeros(3, 1, 16, 16)),
                            (torch.ones(1, 1, 1, 16, 16), y), (torch.ones(16, 16), torch.zeros(5, 16, 3))):
        with pytest.raises(ValueError):
            sampler.p_sample_loop(model, x, bad_y, functools.partial(cond.conditioning, mask=bad_mask))


# ---------------------------------------------------------------------------
# cfd_dps_latent_residual alone
# ---------------------------------------------------------------------------
def _residual_case(n, B, y_shared, m_shared):
    d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="8")
    tab = d.coef_table().double()
    t = torch.tensor([0, 2, 1], dtype=torch.int64)[:B]
    tag = f"lr/{n}"
    # |x| up to ~2.5: with sra in [1, 1.12] and srm1 <= 0.5 some x0 leave [-1, 1]
    x = torch.from_numpy(synth.normal(11, tag + "/x", (B, n))) * 0.75
    eps = torch.from_numpy(synth.normal(11, tag + "/eps", (B, n)))
    mask = torch.from_numpy(synth.uniform(11, tag + "/m", (1 if m_shared else B, n), 0.0, 1.0))
    mask[:, ::5] = 1.0
    mask[:, 1::7] = 0.0
    sra, srm1 = tab[t, 0][:, None], tab[t, 1][:, None]
    x0u = sra * x.double() - srm1 * eps.double()
    x0 = x0u.clamp(-1.0, 1.0)
    # residuals of rms 0.25 around a shared / per-sample "true" latent
    base = (mask.double() * x0)[:1] if y_shared else mask.double() * x0
    y = (base + 0.25 * torch.from_numpy(synth.normal(11, tag + "/r", (1 if y_shared else B, n))).double()).float()
    return d, t, x, eps, y, mask, x0u, x0, sra, srm1


@pytest.mark.parametrize("n", [256, 576, 9000])   # one 256-thread pass; a tail; three 4096-element chunks and a tail
@pytest.mark.parametrize("y_shared", [True, False], ids=["y1", "yB"])
@pytest.mark.parametrize("m_shared", [True, False], ids=["m1", "mB"])
def test_latent_residual_matches_float64(hip, n, y_shared, m_shared):
    B = 3
    d, t, x, eps, y, mask, x0u, x0, sra, srm1 = _residual_case(n, B, y_shared, m_shared)
    outside = (x0u.abs() > 1.0)
    assert outside.any() and (~outside).any()
    assert float((x0u.abs() - 1.0).abs().min()) > 1e-5     # no element at the clamp's edge: fp32 and fp64 agree on it
    r = y.double() - mask.double() * x0
    norm = r.pow(2).sum(dim=1).sqrt()
    gref = torch.where(outside, torch.zeros_like(r), -(mask.double() * (r / norm[:, None])))
    want_de, want_gd = -gref * srm1, gref * sra

    sched = d._sched(DEV, 0.0)
    xd, ed, td, yd, md = (v.to(DEV).contiguous() for v in (x, eps, t, y, mask))
    nb, de, gd_ = torch.empty(B, device=DEV), torch.empty(B, n, device=DEV), torch.empty(B, n, device=DEV)
    nbytes = C.c_size_t()
    _lib.check(hip.cfd_dps_latent_residual_workspace_bytes(n, B, C.byref(nbytes)))
    assert nbytes.value == 8 * B * ((n + 4095) // 4096)
    ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=DEV)
    _lib.check(hip.cfd_dps_latent_residual(sched.handle, 1, _lib.ptr(xd), _lib.ptr(ed), _lib.ptr(td), _lib.ptr(yd),
                                           0 if y_shared else n, _lib.ptr(md), 0 if m_shared else n, _lib.ptr(nb),
                                           _lib.ptr(de), _lib.ptr(gd_), n, B, _lib.ptr(ws), nbytes.value,
                                           _lib.stream_of(DEV)), "cfd_dps_latent_residual")
    nb, de, gd_ = nb.cpu().double(), de.cpu().double(), gd_.cpu().double()
    print(f"n {n}: norms {norm.tolist()}, rel err {((nb - norm).abs() / norm).max():.2e}; d_eps "
          f"{(de - want_de).abs().max() / want_de.abs().max():.2e}, g_direct "
          f"{(gd_ - want_gd).abs().max() / want_gd.abs().max():.2e}")
    assert ((nb - norm).abs() <= 1e-6 * norm).all()
    assert float((de - want_de).abs().max()) <= 1e-6 * float(want_de.abs().max())
    assert float((gd_ - want_gd).abs().max()) <= 1e-6 * float(want_gd.abs().max())
    # clamped elements: exactly zero gradient
    assert (de[outside] == 0).all() and (gd_[outside] == 0).all()
    assert (de[~outside & (mask.expand(B, n) > 0)] != 0).any()

    # the x0 behind it is cfd_sched_step's pred_xstart, and the norm does not depend on B
    out, xs = torch.empty_like(xd), torch.empty_like(xd)
    _lib.check(hip.cfd_sched_step(sched.handle, 0, 1, _lib.ptr(xd), _lib.ptr(ed), _lib.ptr(td), None, 1, 0, 0,
                                  _lib.ptr(out), _lib.ptr(xs), n, B, _lib.stream_of(DEV)), "cfd_sched_step")
    assert float((xs.cpu().double() - x0).abs().max()) < 5e-7
    for b in range(B):
        n1, d1, g1 = torch.empty(1, device=DEV), torch.empty(1, n, device=DEV), torch.empty(1, n, device=DEV)
        yb = yd if y_shared else yd[b:b + 1].contiguous()
        mb = md if m_shared else md[b:b + 1].contiguous()
        _lib.check(hip.cfd_dps_latent_residual(sched.handle, 1, _lib.ptr(xd[b:b + 1].contiguous()),
                                               _lib.ptr(ed[b:b + 1].contiguous()), _lib.ptr(td[b:b + 1].contiguous()),
                                               _lib.ptr(yb), 0, _lib.ptr(mb), 0, _lib.ptr(n1), _lib.ptr(d1),
                                               _lib.ptr(g1), n, 1, _lib.ptr(ws), nbytes.value, _lib.stream_of(DEV)),
                   "cfd_dps_latent_residual")
        assert n1.cpu().double()[0] == nb[b] and torch.equal(d1.cpu().double()[0], de[b])
        assert torch.equal(g1.cpu().double()[0], gd_[b])


def test_latent_residual_argument_checks(hip):
    d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="8")
    sched = d._sched(DEV, 0.0)
    n, B = 256, 2
    z = torch.zeros(B, n, device=DEV)
    t = torch.zeros(B, dtype=torch.int64, device=DEV)
    nb = torch.zeros(B, device=DEV)
    ws = torch.zeros(B, dtype=torch.float64, device=DEV)
    de, gd_ = z.clone(), z.clone()
    call = lambda ys, ms, wb: hip.cfd_dps_latent_residual(  # noqa: E731
        sched.handle, 1, _lib.ptr(z), _lib.ptr(z), _lib.ptr(t), _lib.ptr(z), ys, _lib.ptr(z), ms, _lib.ptr(nb),
        _lib.ptr(de), _lib.ptr(gd_), n, B, _lib.ptr(ws), wb, _lib.stream_of(DEV))
    assert call(0, n, 8 * B) == 0
    assert call(3, n, 8 * B) != 0 and call(0, 2 * n, 8 * B) != 0 and call(0, 0, 8) != 0


# ---------------------------------------------------------------------------
# zero norm; chains
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddpm", "ddim"])
def test_zero_norm_step_leaves_the_sample(hip, name):
    g = golden("dps_inpaint_rows.npz")
    model = _tiny16(g)
    cond = _ps(2.0)
    sampler = _sampler(name, "8")
    x = torch.from_numpy(synth.normal(5, "zn/x", (2, 1, 16, 16))).to(DEV)
    nz = torch.from_numpy(synth.normal(5, "zn/nz", (2, 1, 16, 16)))
    zero = torch.zeros(1, 1, 16, 16)
    a = sampler.p_sample_step(model, x, 5, zero, functools.partial(cond.conditioning, mask=zero), noise=nz)
    assert (a["distance"] == 0).all() and torch.isfinite(a["sample"]).all()
    assert torch.equal(a["sample"], a["x_t"])
    ones = torch.ones(1, 1, 16, 16)
    b = sampler.p_sample_step(model, x, 5, a["pred_xstart"], functools.partial(cond.conditioning, mask=ones),
                              noise=nz)
    assert torch.equal(b["pred_xstart"], a["pred_xstart"]) and torch.equal(b["x_t"], a["x_t"])
    assert (b["distance"] == 0).all() and torch.isfinite(b["sample"]).all()
    assert torch.equal(b["sample"], b["x_t"])
    # one sample with a zero norm next to one without: only the other one moves
    y = a["pred_xstart"].clone()
    y[1] += 0.1
    c = sampler.p_sample_step(model, x, 5, y, functools.partial(cond.conditioning, mask=ones), noise=nz)
    assert float(c["distance"][0]) == 0 and float(c["distance"][1]) > 0
    assert torch.equal(c["sample"][0], c["x_t"][0]) and not torch.equal(c["sample"][1], c["x_t"][1])


@pytest.mark.parametrize("plan", [8, 1])
def test_inpaint_chains_equal_single_chains(hip, plan):
    from test_gpu_backward_edges import TOPOLOGIES, _build
    kw, _, seed, _ = TOPOLOGIES["odd24"]
    m, _ = _build(kw, seed)
    S = kw["image_size"]
    cond = _ps(0.7)
    sampler = _sampler("ddpm", "4")
    B = 3
    xs = torch.from_numpy(synth.normal(3, "inp/xs", (B, 1, S, S))).to(DEV)
    true = torch.from_numpy(synth.uniform(3, "inp/true", (B, 1, S, S), -0.9, 0.9)).to(DEV)
    mask = torch.zeros(B, 1, S, S, device=DEV)
    mask[0, :, :7] = 1.0
    mask[1, :, 5:9] = 1.0
    mask[1, :, 20, ::2] = 0.5
    mask[2, :, -3:] = 1.0
    y = mask * true
    m.set_plan_batch(plan)
    try:
        full = sampler.p_sample_loop(model=m, x_start=xs, measurement=y,
                                     measurement_cond_fn=functools.partial(cond.conditioning, mask=mask), seed=99)
        dfull = sampler.distances.clone()
        assert torch.isfinite(full).all() and (dfull > 0).all()
        for s in range(B):
            fn = functools.partial(cond.conditioning, mask=mask[s:s + 1])
            one = sampler.p_sample_loop(model=m, x_start=xs[s:s + 1], measurement=y[s:s + 1],
                                        measurement_cond_fn=fn, seed=99, sample_offset=s)
            assert torch.equal(one, full[s:s + 1]), s
            assert torch.equal(sampler.distances[:, 0], dfull[:, s]), s
    finally:
        m.set_plan_batch(0)
