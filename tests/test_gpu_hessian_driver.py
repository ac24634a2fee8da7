"""GPU: the inference driver's second-order `derived` keys (tiny shapes, the set-up of
tests/test_gpu_jacobian_driver.py): hessian, laplacian and grad_divergence saved
beside the fields match confild_amd.derived of the oracle's fp64 Hessian; the fields
and the Jacobian-derived files do not change.  The bound is the Hessian test's,
error <= K_BOUND * max(e32, 1e-7 |H64|max), with e32 the error of the same quantity
taken from the CPU fp32 double autograd's Hessian."""
import ast
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import golden
from confild_amd import derived, synth
from confild_amd.script_util import create_gaussian_diffusion, create_model
from oracle import siren as osn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# the Hessian test's bound (tests/test_gpu_siren_hessian.py): error <= K_BOUND * max(e32, 1e-7 |H64|max)
K_BOUND = 4.0


def _tiny():
    g = golden("unet_tiny16.npz")
    kw = ast.literal_eval(str(g["kwargs"]))
    m = create_model(**kw)
    sd = synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return kw, m.to(DEV), sd


def _oracle_hess(ssd, coords, lat, xmax, xmin, ymax, ymin, dtype):
    cast = lambda t: t.to(dtype)
    sdt = {k: torch.from_numpy(v).to(dtype) for k, v in ssd.items()}
    x = cast(coords)[None].expand(lat.shape[0], -1, -1).clone().requires_grad_(True)
    out = osn.denormalize(osn.forward(sdt, osn.normalize(x, cast(xmax), cast(xmin)), cast(lat)[:, None]),
                          cast(ymax), cast(ymin))
    Hs = []
    for o in range(out.shape[-1]):
        Jo = torch.autograd.grad(out[..., o].sum(), x, create_graph=True)[0]
        Hs.append(torch.stack([torch.autograd.grad(Jo[..., k].sum(), x, retain_graph=True)[0]
                               for k in range(x.shape[-1])], -2))
    return torch.stack(Hs, -3).detach()


@pytest.mark.parametrize("layout", ["lumped", "grid"])
def test_driver_saves_second_order_quantities(hip, tmp_path, layout):
    from confild_amd import inference
    kw, m, sd = _tiny()
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "ema.pt")
    if layout == "lumped":
        d, L, c, nh, H = 3, 16, 3, 2, 32
        spatial = (300,)
        yhi = torch.from_numpy(synth.uniform(5, "yhi", (1, 300, c), 0.5, 2.0))
    else:
        d, L, c, nh, H = 2, 16, 3, 2, 32
        spatial = (12, 10)
        yhi = torch.from_numpy(synth.uniform(5, "yhi", (1, c), 0.5, 2.0))
    N = int(np.prod(spatial))
    ssd = synth.siren_state_dict(5, d, L, c, nh, H)
    cnf_dir = tmp_path / "cnf"
    cnf_dir.mkdir()
    xhi, xlo = torch.full((1, d), 1.25), torch.full((1, d), -0.25)
    torch.save({"x_normalizer_params": (xhi, xlo), "y_normalizer_params": (yhi, -yhi)},
               cnf_dir / "normalizer_params.pt")
    torch.save({"epoch": 1, "model_state_dict": {k: torch.from_numpy(v) for k, v in ssd.items()}},
               cnf_dir / "checkpoint_1.pt")
    coords = synth.uniform(5, "coords", spatial + (d,), 0.0, 1.0)
    np.save(tmp_path / "coords.npy", coords)
    cnf_cfg = {"save_path": str(cnf_dir), "coor_path": str(tmp_path / "coords.npy"),
               "lumped_latent": layout == "lumped",
               "normalizer": {"method": "-11", "dim": 0}, "multiGPU": 1, "hidden_size": L, "dims": d,
               "NF": {"name": "SIRENAutodecoder_film", "out_features": c, "num_hidden_layers": nh,
                      "hidden_features": H}}
    (tmp_path / "cnf.yml").write_text(yaml.safe_dump(cnf_cfg))
    np.save(tmp_path / "max.npy", np.float32(1.5))
    np.save(tmp_path / "min.npy", np.float32(-1.5))
    cfg = {"test_batch_size": 2, "time_length": 16, "latent_length": 16, "image_size": 16,
           "num_channels": kw["num_channels"], "num_res_blocks": kw["num_res_blocks"],
           "channel_mult": kw["channel_mult"], "num_heads": kw["num_heads"],
           "num_head_channels": kw["num_head_channels"], "attention_resolutions": kw["attention_resolutions"],
           "ema_path": str(tmp_path / "ema.pt"), "steps": 1000, "noise_schedule": "cosine",
           "timestep_respacing": "8", "max_val": str(tmp_path / "max.npy"), "min_val": str(tmp_path / "min.npy"),
           "cnf_case_file_path": str(tmp_path / "cnf.yml")}

    def run(name, keys):
        folder = tmp_path / name
        folder.mkdir()
        extra = {"derived": keys} if keys is not None else {}
        (tmp_path / f"{name}.yml").write_text(yaml.safe_dump(dict(cfg, save_path=str(folder / "out.npy"), **extra)))
        return folder, inference.run(str(tmp_path / f"{name}.yml"))

    plain, _ = run("plain", None)
    vort, _ = run("vort", ["vorticity"])                       # today's names alone
    lapgd, out = run("lapgd", ["laplacian", "grad_divergence"])
    hv, _ = run("hv", ["hessian", "vorticity"])
    lap1, _ = run("lap1", ["laplacian"])                       # the diagonal form

    # no key: the fields alone; the new names add their files and change no other byte
    assert sorted(os.listdir(plain)) == ["out.npy"]
    assert sorted(os.listdir(vort)) == ["out.npy", "out_vorticity.npy"]
    assert sorted(os.listdir(lapgd)) == ["out.npy", "out_grad_divergence.npy", "out_laplacian.npy"]
    assert sorted(os.listdir(hv)) == ["out.npy", "out_hessian.npy", "out_vorticity.npy"]
    assert sorted(os.listdir(lap1)) == ["out.npy", "out_laplacian.npy"]
    for folder in (vort, lapgd, hv, lap1):
        assert (plain / "out.npy").read_bytes() == (folder / "out.npy").read_bytes()
    assert (vort / "out_vorticity.npy").read_bytes() == (hv / "out_vorticity.npy").read_bytes()
    assert np.array_equal(np.load(lapgd / "out.npy"), out) and out.shape == (32,) + spatial + (c,)
    lap, gd = np.load(lapgd / "out_laplacian.npy"), np.load(lapgd / "out_grad_divergence.npy")
    hess, lapd = np.load(hv / "out_hessian.npy"), np.load(lap1 / "out_laplacian.npy")
    assert lap.shape == (32,) + spatial + (c,) and lap.dtype == np.float32 and lapd.shape == lap.shape
    assert gd.shape == (32,) + spatial + (d,) and hess.shape == (32,) + spatial + (c, d, d)

    # the same latents by hand, then the oracle's fp64 Hessian (fp32 double autograd: the yardstick's own error)
    torch.manual_seed(42)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    diff = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="8")
    lat = diff.p_sample_loop(m, (2, 1, 16, 16), seed=seed)[:, 0]
    lat = ((lat + 1) * (1.5 + 1.5) / 2. - 1.5).reshape(32, 16).cpu()
    args = (ssd, torch.from_numpy(coords).reshape(N, d), lat, xhi, xlo, yhi, -yhi)
    H64 = _oracle_hess(*args, torch.float64)
    H32 = _oracle_hess(*args, torch.float32).double()
    floor = 1e-7 * float(H64.abs().max())
    ident = lambda h: h
    for name, got, fn in (("laplacian", lap, derived.laplacian), ("laplacian (diagonal form)", lapd, derived.laplacian),
                          ("grad_divergence", gd, derived.grad_divergence), ("hessian", hess, ident)):
        want = fn(H64).reshape(got.shape)
        e32 = (fn(H32).reshape(got.shape) - want).abs()
        err = (torch.from_numpy(got).double() - want).abs()
        r_max = float(err.max()) / max(float(e32.max()), floor)
        r_mean = float(err.mean()) / max(float(e32.mean()), floor)
        print(layout, name, "ratio max", r_max, "mean", r_mean)
        assert r_max <= K_BOUND and r_mean <= K_BOUND, (name, r_max, r_mean)
