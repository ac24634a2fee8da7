"""GPU: the rollout driver (confild_amd.rollout.extend_latents) on the tiny16 U-Net:
4 steps, 3 windows (window 0 and n_windows = 2 conditioned ones), overlap 5, both methods ('replace': known-row
replacement in the native loop; 'ps': posterior sampling with the 'inpainting'
operator).  All comparisons are bit-exact: the driver only chains calls that are
public on their own.  The inference driver's rollout_* keys are run end to end."""
import ast
import functools

import numpy as np
import pytest
import torch
import yaml

from conftest import golden
from confild_amd import inference, rollout, synth
from confild_amd.script_util import create_gaussian_diffusion, create_model
from oracle import siren as osn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T, OV, W, SEED = 16, 5, 2, 4242


@pytest.fixture(scope="module")
def tiny():
    g = golden("unet_tiny16.npz")
    kw = ast.literal_eval(str(g["kwargs"]))
    m = create_model(**kw)
    sd = synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _diffusion(method, sampler):
    if method == "replace":
        return create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="4")
    from confild_amd.guided.gaussian_diffusion import create_sampler
    return create_sampler(sampler=sampler, steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                          model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=False, timestep_respacing="4")


def _direct(tiny, method, sampler, scale, known, mask, seed, B, offset=0):
    """The conditioned call a window stands for, spelt out on the public samplers."""
    if method == "replace":
        d = _diffusion(method, sampler)
        loop = d.p_sample_loop if sampler == "ddpm" else d.ddim_sample_loop
        return loop(tiny, (B, 1, T, T), seed=seed, sample_offset=offset, known=known, known_mask=mask)
    from confild_amd.guided.condition_methods import get_conditioning_method
    from confild_amd.guided.measurements import get_noise, get_operator
    cond = get_conditioning_method("ps", get_operator("inpainting", device=DEV), get_noise("gaussian", sigma=0.0),
                                   scale=scale)
    x_T = rollout.window_noise((B, 1, T, T), seed, offset, DEV)
    return _diffusion(method, sampler).p_sample_loop(
        model=tiny, x_start=x_T, measurement=mask * known,
        measurement_cond_fn=functools.partial(cond.conditioning, mask=mask), seed=seed, sample_offset=offset)


@pytest.mark.parametrize("method,sampler", [("replace", "ddpm"), ("replace", "ddim"), ("ps", "ddpm"), ("ps", "ddim")])
def test_rollout_shape_and_stitching(hip, tiny, method, sampler):
    B, scale = 2, 0.5
    d = _diffusion(method, sampler)
    out = rollout.extend_latents(tiny, d, None, W, OV, method, scale=scale, seed=SEED, sampler=sampler, batch_size=B)
    assert out.shape == (B, 1, 38, 16) == (B, 1, T + W * (T - OV), T)
    assert torch.isfinite(out).all()
    windows = rollout.plan_windows(T, OV, W)
    # window 0: the plain loop with the same seed
    plain = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="4")
    loop = plain.p_sample_loop if sampler == "ddpm" else plain.ddim_sample_loop
    assert torch.equal(out[:, :, windows[0]], loop(tiny, (B, 1, T, T), seed=SEED))
    # later windows: a direct conditioned call on the rows before them, with seed + w
    for w in range(1, W + 1):
        sl = windows[w]
        known = torch.zeros(B, 1, T, T, device=DEV)
        known[:, :, :OV] = out[:, :, sl.start:sl.start + OV]
        mask = torch.zeros(1, 1, T, T, device=DEV)
        mask[:, :, :OV] = 1.0
        win = _direct(tiny, method, sampler, scale, known, mask, SEED + w, B)
        assert torch.equal(out[:, :, sl.start + OV:sl.stop], win[:, :, OV:]), w
        # the overlap rows are the earlier window's values
        prev = windows[w - 1]
        assert sl.start == prev.stop - OV
        if method == "replace":
            assert torch.equal(win[:, :, :OV], out[:, :, sl.start:sl.start + OV]), w
    # continuing a given first window gives the same sequence
    again = rollout.extend_latents(tiny, d, out[:, :, :T].clone(), W, OV, method, scale=scale, seed=SEED,
                                   sampler=sampler)
    assert torch.equal(again, out)
    assert not torch.equal(out[:, :, 5:16], out[:, :, 16:27]) and not torch.equal(out[:, :, 16:27], out[:, :, 27:38])


@pytest.mark.parametrize("method", ["replace", "ps"])
def test_rollout_shards_over_samples(hip, tiny, method):
    d = _diffusion(method, "ddpm")
    full = rollout.extend_latents(tiny, d, None, W, OV, method, scale=0.5, seed=SEED, batch_size=2)
    for s in range(2):
        one = rollout.extend_latents(tiny, d, None, W, OV, method, scale=0.5, seed=SEED, sample_offset=s,
                                     batch_size=1)
        assert torch.equal(one, full[s:s + 1]), s


def test_rollout_argument_errors(hip, tiny):
    d = _diffusion("replace", "ddpm")
    with pytest.raises(ValueError):
        rollout.extend_latents(tiny, d, None, 1, 16, "replace", seed=1)
    with pytest.raises(ValueError):
        rollout.extend_latents(tiny, d, None, 1, 5, "repaint", seed=1)
    with pytest.raises(TypeError):
        rollout.extend_latents(tiny, d, None, 1, 5, "ps", seed=1)


@pytest.mark.parametrize("method", ["replace", "ps"])
def test_inference_driver_rollout_keys(hip, tiny, tmp_path, method):
    """python -m confild_amd.inference with the rollout_* keys: the saved array is
    (B * T_total, N, c), the decode of extend_latents' sequence (CPU oracle decode, the
    tolerance of test_gpu_e2e.py's driver test)."""
    kw = ast.literal_eval(str(golden("unet_tiny16.npz")["kwargs"]))
    torch.save({k: v.detach().cpu() for k, v in tiny.state_dict().items()}, tmp_path / "ema.pt")
    d, L, c, nh, H, N = 3, 16, 3, 2, 32, 300
    yhi = torch.from_numpy(synth.uniform(5, "yhi", (1, N, c), 0.5, 2.0))
    ssd = synth.siren_state_dict(5, d, L, c, nh, H)
    cnf_dir = tmp_path / "cnf"
    cnf_dir.mkdir()
    torch.save({"x_normalizer_params": (torch.ones(1, d), torch.zeros(1, d)),
                "y_normalizer_params": (yhi, -yhi)}, cnf_dir / "normalizer_params.pt")
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
    B = 2
    cfg = {"test_batch_size": B, "time_length": T, "latent_length": T, "image_size": T,
           "num_channels": kw["num_channels"], "num_res_blocks": kw["num_res_blocks"],
           "channel_mult": kw["channel_mult"], "num_heads": kw["num_heads"],
           "num_head_channels": kw["num_head_channels"], "attention_resolutions": kw["attention_resolutions"],
           "ema_path": str(tmp_path / "ema.pt"), "steps": 1000, "noise_schedule": "cosine",
           "timestep_respacing": "4", "max_val": str(tmp_path / "max.npy"), "min_val": str(tmp_path / "min.npy"),
           "cnf_case_file_path": str(tmp_path / "cnf.yml"), "save_path": str(tmp_path / "out.npy"),
           "rollout_windows": W, "rollout_overlap": OV, "rollout_method": method, "rollout_scale": 0.5}
    (tmp_path / "case.yml").write_text(yaml.safe_dump(cfg))
    out = inference.run(str(tmp_path / "case.yml"))
    saved = np.load(tmp_path / "out.npy")
    total = T + W * (T - OV)
    assert saved.shape == (B * total, N, c) and np.array_equal(saved, out)

    torch.manual_seed(42)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    lat = rollout.extend_latents(tiny, _diffusion(method, "ddpm"), None, W, OV, method, scale=0.5, seed=seed,
                                 batch_size=B)[:, 0]
    lat = ((lat + 1) * (1.5 + 1.5) / 2. - 1.5).reshape(B * total, T).cpu()
    ref = osn.decode({k: torch.from_numpy(v) for k, v in ssd.items()}, torch.from_numpy(coords), lat,
                     torch.ones(1, d), torch.zeros(1, d), yhi, -yhi)
    assert np.abs(saved - ref.numpy()).max() <= 2e-5 * max(1.0, float(ref.abs().max()))
    # without the keys the driver is the plain run: window 0 of every sample
    for k in ("rollout_windows", "rollout_overlap", "rollout_method", "rollout_scale"):
        del cfg[k]
    (tmp_path / "case.yml").write_text(yaml.safe_dump(cfg))
    plain = inference.run(str(tmp_path / "case.yml"))
    assert plain.shape == (B * T, N, c)
    for b in range(B):
        assert np.abs(plain[b * T:(b + 1) * T] - saved[b * total:b * total + T]).max() <= 2e-5
