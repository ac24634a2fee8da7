"""Generate the 'inpainting' DPS golden fixtures by running the REFERENCE.

Run in the build container only (the reference tree does not exist on the GPU
box):

    python tests/golden/make_golden_dps_inpaint.py

Drives the reference's own guided samplers with its 'inpainting' operator
(C/src/guided_diffusion/measurements.py:40-56, A(x) = mask * x on the latent
image) under 'ps' (condition_methods.py:78-87), the mask handed over as
``partial(cond.conditioning, mask=mask)``: ``create_model``, ``create_sampler``
('ddpm' and 'ddim', gaussian_diffusion.py:30-52, 362-405),
``get_noise('gaussian', sigma=0)``, ``get_conditioning_method('ps', scale)`` and
``p_sample_loop`` (gaussian_diffusion.py:169-206), on the CPU, at fixture scale:
the small 16x16 U-Net of make_golden_dps.py's ``dps_tiny16`` case with the same
synthetic weights and seeds (``confild_amd.synth``).

Two cases: a row mask (the first rows of the latent sequence are known) and a
fractional mask (the row mask plus 0.5 on one further row, every third column).
The measurement is the operator applied to a "true" latent.

Every ``torch.randn_like`` draw of the loop is recorded (the p_sample noise and
the q_sample noise of the unused noisy measurement, interleaved) so the HIP
sampler can replay the same noise.  The only shim is the tensorboard stand-in
also used by make_golden.py.  Recorded per step: x0_hat, the DDPM / DDIM
sample, the conditioned image and the residual norm; arrays and settings only.
"""
from __future__ import annotations

import functools
import os
import sys

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, REF, os.path.join(REF, "ConditionalNeuralField")]

import types  # noqa: E402

# in-process stand-in for torch.utils.tensorboard (not installed; imported at
# ConditionalNeuralField/scripts/train.py:13, never used on this path)
_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = object
sys.modules["torch.utils.tensorboard"] = _tb

import numpy as np  # noqa: E402
import torch  # noqa: E402

from confild_amd import synth  # noqa: E402

torch.set_num_threads(8)

# the dps_tiny16 U-Net of make_golden_dps.py and its seed
UNET_KW = dict(image_size=16, num_channels=32, num_res_blocks=1, channel_mult="1,2", num_heads=1,
               num_head_channels=16, attention_resolutions="8")
SEED = 21
KNOWN_ROWS = 5      # rows 0-4 of 16


def row_mask(T, L):
    m = torch.zeros(1, 1, T, L)
    m[:, :, :KNOWN_ROWS] = 1.0
    return m


def frac_mask(T, L):
    m = row_mask(T, L)
    m[:, :, 9, ::3] = 0.5
    return m


CASES = {
    # name: (sampler, respacing, scale, mask)
    "dps_inpaint_rows": ("ddpm", "8", 0.5, row_mask),
    "dps_inpaint_frac": ("ddim", "6", 3.0, frac_mask),
}


def gen(case):
    from ConditionalDiffusionGeneration.src.guided_diffusion.condition_methods import get_conditioning_method
    from ConditionalDiffusionGeneration.src.guided_diffusion.gaussian_diffusion import create_sampler
    from ConditionalDiffusionGeneration.src.guided_diffusion.measurements import get_noise, get_operator
    from ConditionalDiffusionGeneration.src.guided_diffusion.unet import create_model

    name, resp, scale, mask_fn = CASES[case]
    S = UNET_KW["image_size"]
    T = L = S
    torch.manual_seed(0)
    model = create_model(**UNET_KW, model_path="")      # prints "Randomly initialize"
    sd = synth.unet_state_dict(SEED, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.eval()

    op = get_operator("inpainting", device=torch.device("cpu"))
    mask = mask_fn(T, L)
    x_true = torch.from_numpy(synth.uniform(SEED, "xtrue", (1, 1, T, L), -0.9, 0.9))
    y = op.forward(x_true, mask=mask)                   # (1, 1, T, L)
    noiser = get_noise(sigma=0.0, name="gaussian")
    cond = get_conditioning_method(operator=op, noiser=noiser, name="ps", scale=scale)
    conditioning = functools.partial(cond.conditioning, mask=mask)
    sampler = create_sampler(sampler=name, steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                             model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                             rescale_timesteps=False, timestep_respacing=resp)
    rec = {"x0": [], "sample": [], "img": [], "dist": []}

    def cond_fn(x_t, measurement, noisy_measurement, x_prev, x_0_hat):
        rec["x0"].append(x_0_hat.detach().clone())
        rec["sample"].append(x_t.detach().clone())
        img, dist = conditioning(x_t=x_t, measurement=measurement, noisy_measurement=noisy_measurement,
                                 x_prev=x_prev, x_0_hat=x_0_hat)
        rec["img"].append(img.detach().clone())
        rec["dist"].append(float(dist.detach()))
        return img, dist

    draws = []
    real = torch.randn_like

    def recording_randn_like(t, *a, **k):
        out = real(t, *a, **k)
        draws.append(out.detach().clone())
        return out

    torch.manual_seed(SEED)
    x_start = torch.randn(1, 1, T, L)
    torch.randn_like = recording_randn_like
    try:
        out = sampler.p_sample_loop(model=model, x_start=x_start, measurement=y, measurement_cond_fn=cond_fn,
                                    record=False, save_root=None)
    finally:
        torch.randn_like = real
    n = len(rec["img"])
    assert len(draws) == 2 * n, (len(draws), n)
    arrays = dict(kwargs=np.array(repr(UNET_KW)), seed=np.int64(SEED), sampler=np.array(name),
                  respacing=np.array(resp), scale=np.float64(scale), mask=mask.numpy(),
                  x_start=x_start.detach().numpy(), x_true=x_true.numpy(), measurement=y.numpy(),
                  step_noise=torch.stack(draws[0::2]).numpy(), x0=torch.stack(rec["x0"]).numpy(),
                  sample=torch.stack(rec["sample"]).numpy(), img=torch.stack(rec["img"]).numpy(),
                  dist=np.array(rec["dist"]), out=out.detach().numpy(),
                  timestep_map=np.array(sampler.timestep_map, dtype=np.int64))
    path = os.path.join(HERE, f"{case}.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB), steps {n}, dist {rec['dist'][0]:.4f} -> "
          f"{rec['dist'][-1]:.4f}")


if __name__ == "__main__":
    for case in CASES:
        gen(case)
