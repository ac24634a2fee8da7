"""GPU: the inference driver's `derived_compute` key (the tiny set-up of
tests/test_gpu_jacobian_driver.py, H = 32): with split_f16 vorticity and divergence
stay within the Jacobian test's bound of the oracle's fp64 quantities and the fields
keep their bytes; without the key every file is the `derived_compute: f32` run's."""
import os

import numpy as np
import pytest
import torch
import yaml

from confild_amd import derived, synth
from confild_amd.script_util import create_gaussian_diffusion
from test_gpu_jacobian_driver import K_BOUND, _oracle_jac, _tiny

pytestmark = pytest.mark.gpu


def test_driver_derived_compute(hip, tmp_path):
    from confild_amd import inference
    kw, m, sd = _tiny()
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / "ema.pt")
    d, L, c, nh, H = 3, 16, 3, 2, 32
    N = 300
    yhi = torch.from_numpy(synth.uniform(5, "yhi", (1, N, c), 0.5, 2.0))
    ssd = synth.siren_state_dict(5, d, L, c, nh, H)
    cnf_dir = tmp_path / "cnf"
    cnf_dir.mkdir()
    xhi, xlo = torch.full((1, d), 1.25), torch.full((1, d), -0.25)
    torch.save({"x_normalizer_params": (xhi, xlo), "y_normalizer_params": (yhi, -yhi)},
               cnf_dir / "normalizer_params.pt")
    torch.save({"epoch": 1, "model_state_dict": {k: torch.from_numpy(v) for k, v in ssd.items()}},
               cnf_dir / "checkpoint_1.pt")
    coords = synth.uniform(5, "coords", (N, d), 0.0, 1.0)
    np.save(tmp_path / "coords.npy", coords)
    cnf_cfg = {"save_path": str(cnf_dir), "coor_path": str(tmp_path / "coords.npy"), "lumped_latent": True,
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
    names = ["vorticity", "divergence"]
    runs = {"plain": {}, "absent": {"derived": names}, "f32": {"derived": names, "derived_compute": "f32"},
            "split": {"derived": names, "derived_compute": "split_f16"}}
    for tag, extra in runs.items():
        (tmp_path / tag).mkdir()
        (tmp_path / f"{tag}.yml").write_text(yaml.safe_dump(dict(cfg, save_path=str(tmp_path / tag / "out.npy"),
                                                                 **extra)))
        inference.run(str(tmp_path / f"{tag}.yml"))

    files = ["out.npy", "out_divergence.npy", "out_vorticity.npy"]
    assert sorted(os.listdir(tmp_path / "plain")) == ["out.npy"]
    for tag in ("absent", "f32", "split"):
        assert sorted(os.listdir(tmp_path / tag)) == files
        # the fields never depend on `derived` or its compute
        assert (tmp_path / tag / "out.npy").read_bytes() == (tmp_path / "plain" / "out.npy").read_bytes(), tag
    for f in files:                                      # the key absent: the f32 run, byte for byte
        assert (tmp_path / "absent" / f).read_bytes() == (tmp_path / "f32" / f).read_bytes(), f
    vort, div = np.load(tmp_path / "split" / "out_vorticity.npy"), np.load(tmp_path / "split" / "out_divergence.npy")
    assert div.shape == (32, N) and div.dtype == np.float32 and vort.shape == (32, N, 3)

    # the same latents by hand, then the oracle's fp64 Jacobian (fp32 autograd: the yardstick's own error)
    torch.manual_seed(42)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    diff = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="8")
    lat = diff.p_sample_loop(m, (2, 1, 16, 16), seed=seed)[:, 0]
    lat = ((lat + 1) * (1.5 + 1.5) / 2. - 1.5).reshape(32, 16).cpu()
    args = (ssd, torch.from_numpy(coords).reshape(N, d), lat, xhi, xlo, yhi, -yhi)
    J64 = _oracle_jac(*args, torch.float64)
    J32 = _oracle_jac(*args, torch.float32).double()
    floor = 1e-7 * float(J64.abs().max())
    for name, got, fn in (("vorticity", vort, derived.vorticity), ("divergence", div, derived.divergence)):
        want = fn(J64).reshape(got.shape)
        e32 = (fn(J32).reshape(got.shape) - want).abs()
        err = (torch.from_numpy(got).double() - want).abs()
        r_max = float(err.max()) / max(float(e32.max()), floor)
        r_mean = float(err.mean()) / max(float(e32.mean()), floor)
        print("split_f16", name, "ratio max", r_max, "mean", r_mean)
        assert r_max <= K_BOUND and r_mean <= K_BOUND, (name, r_max, r_mean)
