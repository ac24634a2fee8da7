"""GPU: the inference driver's `derived_hessian_compute` key and its PDE-residual
`derived` names (tiny shapes, the set-up of tests/test_gpu_hessian_driver.py):
convective_acceleration, momentum_residual and pressure_poisson_residual saved beside the
fields match confild_amd.derived applied to the oracle's fp64 (out, J, H) at both values
of the key; the fields, the Jacobian-derived files and the f32 Laplacian do not change.

The bound is the Hessian test's form: error max and mean <= K_BOUND * max(e32, 1e-7 S),
e32 the error of the same quantity taken from the CPU fp32 double autograd and S the
largest magnitude among the quantity's own terms (convective, nu lap u, grad p / rho;
for the Poisson residual lap p and rho A:A^T), so that a residual that cancels is not
judged on its own smallness."""
import ast
import os

import numpy as np
import pytest
import torch
import yaml

import test_gpu_siren_hessian as hbase
from conftest import golden
from confild_amd import derived, synth
from confild_amd.script_util import create_gaussian_diffusion, create_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
K_BOUND = hbase.K_BOUND
NU, RHO = 0.02, 1.5
RESIDUALS = ["momentum_residual", "pressure_poisson_residual", "convective_acceleration"]


def _tiny():
    g = golden("unet_tiny16.npz")
    kw = ast.literal_eval(str(g["kwargs"]))
    m = create_model(**kw)
    sd = synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return kw, m.to(DEV), sd


def _quantities(out, J, H, pch):
    """name -> (the quantity, the largest magnitude among its terms) from (out, J, H)."""
    conv = derived.convective_acceleration(out, J)
    d = J.shape[-1]
    lap = derived.laplacian(H, diag=False)
    s_mom = max(float(conv.abs().max()), NU * float(lap[..., :d].abs().max()), float(J[..., pch, :].abs().max()) / RHO)
    A = derived.velocity_gradient(J)
    s_ppe = max(float(lap[..., pch].abs().max()), RHO * float((A * A.transpose(-1, -2)).sum((-2, -1)).abs().max()))
    return {"convective_acceleration": (conv, float(conv.abs().max())),
            "momentum_residual": (derived.momentum_residual(out, J, H, NU, pch, RHO), s_mom),
            "pressure_poisson_residual": (derived.pressure_poisson_residual(J, H, pch, RHO), s_ppe)}


@pytest.mark.parametrize("layout", ["lumped", "grid"])
def test_driver_hessian_compute_and_residuals(hip, tmp_path, layout, monkeypatch):
    from confild_amd import inference
    from confild_amd.trainer import trainer
    kw, m, sd = _tiny()
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "ema.pt")
    if layout == "lumped":
        d, L, c, nh, H = 3, 16, 4, 2, 32
        spatial = (300,)
        yhi = torch.from_numpy(synth.uniform(5, "yhi", (1, 300, c), 0.5, 2.0))
    else:
        d, L, c, nh, H = 2, 16, 3, 2, 32
        spatial = (12, 10)
        yhi = torch.from_numpy(synth.uniform(5, "yhi", (1, c), 0.5, 2.0))
    pch = c - 1
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

    calls = []
    plain_infer_hessian = trainer.infer_hessian

    def recording(self, coord, latents, diag=False, compute=None):
        calls.append((bool(diag), compute))
        return plain_infer_hessian(self, coord, latents, diag=diag, compute=compute)
    monkeypatch.setattr(trainer, "infer_hessian", recording)

    def run(name, keys, **extra):
        folder = tmp_path / name
        folder.mkdir()
        if keys is not None:
            extra["derived"] = keys
        (tmp_path / f"{name}.yml").write_text(yaml.safe_dump(dict(cfg, save_path=str(folder / "out.npy"), **extra)))
        del calls[:]
        inference.run(str(tmp_path / f"{name}.yml"))
        return folder, list(calls)

    phys = {"derived_nu": NU, "derived_rho": RHO, "derived_pressure_channel": pch}
    plain, seen = run("plain", None)
    assert seen == []
    lv0, seen = run("lv0", ["laplacian", "vorticity"])                  # no new key: today's run
    assert seen == [(True, "f32")]
    lv = {}
    for mode in ("f32", "split_f16"):
        lv[mode], seen = run("lv_" + mode, ["laplacian", "vorticity"], derived_hessian_compute=mode)
        assert seen == [(True, mode)]
    res = {}
    for mode in ("f32", "split_f16"):
        res[mode], seen = run("res_" + mode, RESIDUALS, derived_hessian_compute=mode, **phys)
        assert seen == [(True, mode)]                                   # the Laplacian is all they need

    assert sorted(os.listdir(plain)) == ["out.npy"]
    for folder in (lv0, lv["f32"], lv["split_f16"]):
        assert sorted(os.listdir(folder)) == ["out.npy", "out_laplacian.npy", "out_vorticity.npy"]
    for folder in res.values():
        assert sorted(os.listdir(folder)) == ["out.npy"] + sorted(f"out_{n}.npy" for n in RESIDUALS)
    # the fields and the Jacobian-derived file never change; f32 is today's Laplacian
    for folder in (lv0,) + tuple(lv.values()) + tuple(res.values()):
        assert (plain / "out.npy").read_bytes() == (folder / "out.npy").read_bytes()
    for folder in lv.values():
        assert (lv0 / "out_vorticity.npy").read_bytes() == (folder / "out_vorticity.npy").read_bytes()
    assert (lv0 / "out_laplacian.npy").read_bytes() == (lv["f32"] / "out_laplacian.npy").read_bytes()
    assert (lv0 / "out_laplacian.npy").read_bytes() != (lv["split_f16"] / "out_laplacian.npy").read_bytes()
    # the convective acceleration is the Jacobian launch's: not touched by the Hessian launch's key
    assert (res["f32"] / "out_convective_acceleration.npy").read_bytes() == \
        (res["split_f16"] / "out_convective_acceleration.npy").read_bytes()

    # the same latents by hand, then the oracle's fp64 (out, J, H) (fp32 double autograd: the yardstick's own error)
    torch.manual_seed(42)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    diff = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="8")
    lat = diff.p_sample_loop(m, (2, 1, 16, 16), seed=seed)[:, 0]
    lat = ((lat + 1) * (1.5 + 1.5) / 2. - 1.5).reshape(32, 16).cpu()
    args = ({k: torch.from_numpy(v) for k, v in ssd.items()}, torch.from_numpy(coords).reshape(N, d), lat, xhi, xlo,
            yhi, -yhi)
    o64 = hbase._oracle(*args, torch.float64)
    o32 = tuple(t.double() for t in hbase._oracle(*args, torch.float32))
    q64, q32, H64, H32 = _quantities(*o64, pch), _quantities(*o32, pch), o64[2], o32[2]
    q64["laplacian"] = (derived.laplacian(H64, diag=False), float(H64.abs().max()))
    q32["laplacian"] = (derived.laplacian(H32, diag=False), None)
    for mode in ("f32", "split_f16"):
        for name in RESIDUALS + ["laplacian"]:
            got = np.load((lv if name == "laplacian" else res)[mode] / f"out_{name}.npy")
            want, S = q64[name]
            shape = (32,) + spatial + tuple(want.shape[2:])
            assert got.shape == shape and got.dtype == np.float32, (name, got.shape)
            want = want.reshape(shape)
            e32 = (q32[name][0].reshape(shape) - want).abs()
            err = (torch.from_numpy(got).double() - want).abs()
            r_max = float(err.max()) / max(float(e32.max()), 1e-7 * S)
            r_mean = float(err.mean()) / max(float(e32.mean()), 1e-7 * S)
            print(layout, mode, name, "ratio max", r_max, "mean", r_mean, "S", S)
            assert r_max <= K_BOUND and r_mean <= K_BOUND, (mode, name, r_max, r_mean)
