"""Generate the dense / masked DPS golden fixtures by running the REFERENCE.

Run in the build container only (the reference tree does not exist on the GPU
box):

    python tests/golden/make_golden_dps_dense.py

As make_golden_dps.py (the reference's own ``create_model``, ``create_sampler``,
``get_conditioning_method('ps')`` and ``DDPM.p_sample_loop``), with the
measurement operators of the data-restoration and sensor cases and the mask
passed the way the reference passes it, ``partial(cond.conditioning, mask=mask)``:

  * ``dps_dense_case2``: the reference's ``Case2Operator`` (measurements.py:58-97)
    built with ``__new__`` -- its ``__init__`` hard-codes a (2, 256, 4, 10, 256)
    SIREN and reads a checkpoint -- with a synthetic (2, 16, 4, 2, 32) SIREN, 37
    points, the reference's hard-coded Case2 normalisers, and a 0/1 mask of shape
    (16, 37, 4), about 60 % ones.  ``_unnorm`` / ``forward`` are the reference's.
  * ``dps_dense_case3gappy``: the reference's ``Case3Operator`` (:99-137, built
    with ``__new__``, 17 sensors, (2, 16, 2, 2, 32) SIREN) with the gappy (Ns, c)
    table -- channel 1 zero for the first 10 sensors, channel 0 for the rest
    (:179-180) -- passed as ``mask=``.  ``Case3Operator.forward`` drops its
    keywords and ``Case3Operator_gappy.forward`` cannot run (its arguments to
    pass_through_model_batch are in the wrong order), so the one shim here is a
    subclass whose forward is ``mask * Case3Operator.forward(data)``: the
    reference's fields with the entries of :179-180 set to zero.

Recorded as ``dps_tiny16``, plus the mask.
"""
from __future__ import annotations

import os
import sys
from functools import partial

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, REF, os.path.join(REF, "ConditionalNeuralField")]

import types  # noqa: E402

# in-process stand-in for torch.utils.tensorboard (see make_golden_dps.py)
_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = object
sys.modules["torch.utils.tensorboard"] = _tb

import numpy as np  # noqa: E402
import torch  # noqa: E402

from confild_amd import synth  # noqa: E402

torch.set_num_threads(8)

UNET = dict(image_size=16, num_channels=32, num_res_blocks=1, channel_mult="1,2", num_heads=1,
            num_head_channels=16, attention_resolutions="8")
CASES = {
    # name: (operator, siren dims (d, L, c, nh, H), points, respacing, scale, seed)
    "dps_dense_case2": ("case2", (2, 16, 4, 2, 32), 37, "6", 2.0, 31),
    "dps_dense_case3gappy": ("case3", (2, 16, 2, 2, 32), 17, "6", 2.0, 32),
}


def build(case):
    from ConditionalDiffusionGeneration.src.guided_diffusion.unet import create_model
    from ConditionalDiffusionGeneration.src.guided_diffusion import measurements as ms
    from cnf.nf_networks import SIRENAutodecoder_film
    from cnf.utils.normalize import Normalizer_ts

    kind, (d, L, c, nh, H), Ns, resp, scale, seed = CASES[case]
    S = UNET["image_size"]
    torch.manual_seed(0)
    model = create_model(**UNET, model_path="")
    sd = synth.unet_state_dict(seed, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.eval()

    nf = SIRENAutodecoder_film(d, L, c, nh, H)
    ssd = synth.siren_state_dict(seed + 100, d, L, c, nh, H)
    nf.load_state_dict({k: torch.from_numpy(v) for k, v in ssd.items()})
    nf.eval()

    if kind == "case2":
        op = ms.Case2Operator.__new__(ms.Case2Operator)
        coords = synth.uniform(seed, "points", (Ns, d), 0.0, 1.0)
        # the constants of Case2Operator.__init__ (measurements.py:70-75)
        xhi, xlo = np.array([1., 1.], dtype=np.float32), np.array([0., 0.], dtype=np.float32)
        yhi = np.array([[0.9617, 0.2666, 0.2869, 0.0290]], dtype=np.float32)
        ylo = np.array([[-0.0051, -0.2073, -0.2619, -0.0419]], dtype=np.float32)
        mask = (synth.uniform(seed, "mask", (S, Ns, c), 0.0, 1.0) < 0.6).astype(np.float32)
    else:
        class MaskedCase3(ms.Case3Operator):
            def forward(self, data, **kwargs):
                return kwargs["mask"] * ms.Case3Operator.forward(self, data)

        op = MaskedCase3.__new__(MaskedCase3)
        coords = synth.uniform(seed, "sensors", (Ns, d), -0.5, 2.0)
        xhi = synth.uniform(seed, "xhi", (1, d), 2.0, 2.5)
        xlo = synth.uniform(seed, "xlo", (1, d), -1.0, -0.5)
        yhi = synth.uniform(seed, "yhi", (c,), 0.5, 2.0)
        ylo = synth.uniform(seed, "ylo", (c,), -2.0, -0.5)
        mask = np.ones((Ns, c), dtype=np.float32)
        mask[:10, 1] = 0.
        mask[10:, 0] = 0.
    op.device = torch.device("cpu")
    op.coords = torch.tensor(coords, dtype=torch.float32)
    op.x_normalizer = Normalizer_ts(method="-11", dim=0, params=(torch.from_numpy(xhi), torch.from_numpy(xlo)))
    op.y_normalizer = Normalizer_ts(method="-11", dim=0, params=(torch.from_numpy(yhi), torch.from_numpy(ylo)))
    op.model = nf
    vmax = synth.uniform(seed, "vmax", (L,), 1.0, 2.0)
    vmin = synth.uniform(seed, "vmin", (L,), -2.0, -1.0)
    op.max_val = torch.from_numpy(vmax)
    op.min_val = torch.from_numpy(vmin)
    op.batch_size = 6
    arrays = dict(kwargs=np.array(repr(UNET)), operator=np.array(kind), seed=np.int64(seed),
                  siren_seed=np.int64(seed + 100), siren_dims=np.array([d, L, c, nh, H], dtype=np.int64),
                  coords=coords, xhi=xhi, xlo=xlo, yhi=yhi, ylo=ylo, vmax=vmax, vmin=vmin, mask=mask,
                  respacing=np.array(resp), scale=np.float64(scale), op_batch=np.int64(op.batch_size))
    return model, op, arrays, S, L, resp, scale, seed, torch.from_numpy(mask)


def gen(case):
    from ConditionalDiffusionGeneration.src.guided_diffusion.condition_methods import get_conditioning_method
    from ConditionalDiffusionGeneration.src.guided_diffusion.gaussian_diffusion import create_sampler
    from ConditionalDiffusionGeneration.src.guided_diffusion.measurements import get_noise

    model, op, arrays, S, L, resp, scale, seed, mask = build(case)
    T = S
    x_true = torch.from_numpy(synth.uniform(seed, "xtrue", (1, 1, T, L), -0.9, 0.9))
    with torch.no_grad():
        y = op.forward(x_true, mask=mask)               # (T, Ns, c), masked
    noiser = get_noise(sigma=0.0, name="gaussian")
    cond = get_conditioning_method(operator=op, noiser=noiser, name="ps", scale=scale)
    sampler = create_sampler(sampler="ddpm", steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                             model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                             rescale_timesteps=False, timestep_respacing=resp)
    rec = {"x0": [], "sample": [], "img": [], "dist": []}
    masked_fn = partial(cond.conditioning, mask=mask)

    def cond_fn(x_t, measurement, noisy_measurement, x_prev, x_0_hat):
        rec["x0"].append(x_0_hat.detach().clone())
        rec["sample"].append(x_t.detach().clone())
        img, dist = masked_fn(x_t=x_t, measurement=measurement, noisy_measurement=noisy_measurement,
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

    torch.manual_seed(seed)
    x_start = torch.randn(1, 1, T, L)
    torch.randn_like = recording_randn_like
    try:
        out = sampler.p_sample_loop(model=model, x_start=x_start, measurement=y, measurement_cond_fn=cond_fn,
                                    record=False, save_root=None)
    finally:
        torch.randn_like = real
    n = len(rec["img"])
    assert len(draws) == 2 * n, (len(draws), n)
    arrays.update(x_start=x_start.detach().numpy(), x_true=x_true.numpy(), measurement=y.numpy(),
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
