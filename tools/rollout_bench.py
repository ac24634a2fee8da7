"""Time one rollout window at config B's widths (64^2 latent, B = 8, 256 steps):

  uncond/<parent build>   the unconditioned native loop on the parent commit's library
  uncond                  the same loop on this build
  replace                 the loop with known-row replacement (cfd_sched_step_known in the graph)
  ps                      posterior sampling with the 'inpainting' operator (Python loop:
                          U-Net forward with tape, cfd_dps_latent_residual, input VJP, update)
  resample                replace with RePaint resampling jumps, resample=(10, 10)
                          (cfd_sched_step_jump in the graph; 2,506 executed steps for 256 levels)

    python tools/rollout_bench.py [--parent libconfild_hip_parent.so] [--rounds 3] [--out profiles/rollout.json]

``--mode guided`` times one window of the guided (DPS) sampler instead, at config D's
widths and chain count (bench.py: 64^2 latent, the 128-channel U-Net, SIREN (3, 64, 3, 15,
384) at 10 sensors, 256 steps, 8 chains), three child processes interleaved:

  guided/<parent build>   the guided loop without known rows on the parent commit's library
  guided                  the same loop on this build (cfd_dps_update as the step's last call)
  guided_known            the loop with known rows, the first half of the latent's rows
                          (cfd_dps_update_known as the step's last call)

Each timing is a child process (CFD_LIB selects the in-tree build), the five run
interleaved for ``--rounds`` rounds on the same device.  A child builds the
synthetic cfgB64 U-Net, runs one whole window untimed (graph capture, first
launches), then times ``--loops`` windows with a host clock around work that ends
in a device synchronise.  ms per step divides by the steps the loop executes
(``steps_run``; the resampled window runs more of them than it has levels).  The
parent library lacks this change's symbols
(_lib.load binds what a CFD_LIB build exports); its child leaves the known rows out.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESAMPLE = (10, 10)   # (jump_length, jump_n_sample) of the `resample` mode

CHILD = r"""
import ast, json, sys, time
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
mode, loops, steps, B = sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
resample = ast.literal_eval(sys.argv[6])
from confild_amd import _lib, synth
from confild_amd import gaussian_diffusion as gd
if mode == "uncond_parent":
    gd._NativeLoop.set_known = lambda self, kn, table, device: None   # the parent has no known rows to clear
from confild_amd.script_util import create_gaussian_diffusion, create_model
g = np.load(sys.argv[1] + "/tests/golden/unet_cfgB64.npz")
kw = ast.literal_eval(str(g["kwargs"]))
m = create_model(**kw)
m.load_state_dict({k: torch.from_numpy(v) for k, v in
                   synth.unet_state_dict(int(g["seed"]), {k: tuple(v.shape) for k, v in m.state_dict().items()}).items()})
dev = torch.device("cuda", 0)
m.to(dev)
S = kw["image_size"]
shape = (B, 1, S, S)
known = torch.from_numpy(synth.uniform(1, "rb/known", shape, -0.9, 0.9)).to(dev)
mask = torch.zeros(1, 1, S, S, device=dev)
mask[:, :, :S // 2] = 1.0
if mode == "ps":
    from confild_amd import rollout
    from confild_amd.guided.gaussian_diffusion import create_sampler
    d = create_sampler(sampler="ddpm", steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                       model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                       rescale_timesteps=False, timestep_respacing=steps)
    run = lambda: rollout.sample_window(m, d, shape, "ps", known=known, mask=mask, scale=0.5, seed=3)
else:
    d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing=steps)
    kwargs = dict(known=known, known_mask=mask) if mode in ("replace", "resample") else {}
    if mode == "resample":
        kwargs["resample"] = resample
    run = lambda: d.p_sample_loop(m, shape, seed=3, **kwargs)
out = run()
torch.cuda.synchronize()
assert torch.isfinite(out).all()
ts = []
for _ in range(loops):
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
n = d.num_timesteps
n_run = len(gd.resample_schedule(n, *resample)) if mode == "resample" else n
print(json.dumps({"mode": mode, "lib": _lib.LIB_PATH.rsplit("/", 1)[-1], "steps": n, "steps_run": n_run, "B": B,
                  "window_ms": [1e3 * t for t in ts], "ms_per_step": 1e3 * min(ts) / n_run}))
"""


CHILD_GUIDED = r"""
import functools, json, sys, time, warnings
import torch
sys.path.insert(0, sys.argv[1])
mode, loops, steps, B = sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
from confild_amd import _lib, rollout, synth
from confild_amd.guided.condition_methods import get_conditioning_method
from confild_amd.guided.gaussian_diffusion import create_sampler
from confild_amd.guided.measurements import Case4Operator, get_noise
from confild_amd.guided.unet import create_model
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts
dev = torch.device("cuda", 0)
S = 64
with warnings.catch_warnings():
    warnings.simplefilter("ignore")   # no model_path: the weights are set below
    m = create_model(image_size=S, num_channels=128, num_res_blocks=2, channel_mult="", num_heads=4,
                     num_head_channels=64, attention_resolutions="32,16,8")
m.load_state_dict({k: torch.from_numpy(v) for k, v in
                   synth.unet_state_dict(1234, {k: tuple(v.shape) for k, v in m.state_dict().items()}).items()})
d, L, c, nh, H = 3, 64, 3, 15, 384
nf = SIRENAutodecoder_film(d, L, c, nh, H)
nf.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(1234, d, L, c, nh, H).items()})
m.to(dev)
nf.to(dev)
coords = torch.from_numpy(synth.uniform(5, "dps/sensors", (10, d), 0.0, 1.0))
xn = Normalizer_ts(params=(torch.ones(1, d), torch.zeros(1, d)), method="-11", dim=0)
yn = Normalizer_ts(params=(torch.full((c,), 2.0), torch.full((c,), -2.0)), method="-11", dim=0)
op = Case4Operator.from_parts(dev, coords, xn, yn, nf, torch.full((L,), 1.5), torch.full((L,), -1.5), batch_size=384)
cond = get_conditioning_method(operator=op, noiser=get_noise(sigma=0.0, name="gaussian"), name="ps", scale=1.0)
smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                     model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                     rescale_timesteps=False, timestep_respacing=steps)
y = op.forward(torch.from_numpy(synth.uniform(6, "dps/xtrue", (1, 1, S, L), -0.9, 0.9)).to(dev))
shape = (B, 1, S, L)
kwargs = {}
if mode == "guided_known":
    kwargs["known"] = torch.from_numpy(synth.uniform(1, "rb/known", shape, -0.9, 0.9)).to(dev)
    kwargs["known_mask"] = torch.zeros(1, 1, S, L, device=dev)
    kwargs["known_mask"][:, :, :S // 2] = 1.0
x_T = rollout.window_noise(shape, 3, 0, dev)
fn = functools.partial(cond.conditioning)
run = lambda: smp.p_sample_loop(model=m, x_start=x_T, measurement=y, measurement_cond_fn=fn, seed=3, **kwargs)
out = run()
torch.cuda.synchronize()
assert torch.isfinite(out).all()
ts = []
for _ in range(loops):
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
n = smp.num_timesteps
print(json.dumps({"mode": mode, "lib": _lib.LIB_PATH.rsplit("/", 1)[-1], "steps": n, "steps_run": n, "B": B,
                  "window_ms": [1e3 * t for t in ts], "ms_per_step": 1e3 * min(ts) / n}))
"""


def child(mode, lib, loops, steps, B, resample):
    env = dict(os.environ)
    if lib:
        env["CFD_LIB"] = lib
    else:
        env.pop("CFD_LIB", None)
    script = CHILD_GUIDED if mode.startswith("guided") else CHILD
    p = subprocess.run([sys.executable, "-c", script, ROOT, mode, str(loops), steps, str(B), repr(resample)], env=env,
                       capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"{mode} ({lib or 'default library'}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="libconfild_hip_parent.so",
                    help="the parent commit's build under confild_amd/lib (make VARIANT=parent in its checkout)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--steps", default="256")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", choices=["rollout", "guided"], default="rollout",
                    help="guided: one window of the guided sampler at config D's widths, without and with known rows")
    a = ap.parse_args()
    runs = [("uncond_parent", a.parent), ("uncond", None), ("replace", None), ("ps", None), ("resample", None)]
    if a.mode == "guided":
        runs = [("guided_parent", a.parent), ("guided", None), ("guided_known", None)]
    resample = RESAMPLE
    res = {mode: [] for mode, _ in runs}
    for r in range(a.rounds):
        for mode, lib in runs:
            loops = 1 if mode in ("ps", "resample") else a.loops   # the two long windows: one timed each
            one = child(mode, lib, loops, a.steps, a.batch, resample)
            res[mode].append(one)
            print(f"round {r} {mode:14s} {one['ms_per_step']:.3f} ms/step, window {min(one['window_ms']):.1f} ms "
                  f"({one['steps_run']} steps)", flush=True)
    summary = {mode: {"ms_per_step": [x["ms_per_step"] for x in v], "window_ms": [min(x["window_ms"]) for x in v],
                      "steps_run": v[0]["steps_run"]} for mode, v in res.items()}
    what = ("one rollout window at config B's widths: 64^2 cfgB64 U-Net (synthetic weights), "
            f"B = {a.batch}, {a.steps} steps (resample {resample}: steps_run executed steps); "
            "ms per step = fastest timed window / steps_run")
    if a.mode == "guided":
        what = ("one window of the guided (DPS) sampler at config D's widths: 64^2 latent, 128-channel U-Net and "
                f"SIREN (3, 64, 3, 15, 384) with synthetic weights, 10 sensors, {a.batch} chains, {a.steps} steps; "
                "guided_known holds the first 32 rows; ms per step = fastest timed window / steps")
    doc = {"what": what,
           "order": f"same device, interleaved {', '.join(mode for mode, _ in runs)} for {a.rounds} rounds; each a "
                    "child process, one untimed window first",
           "summary": summary, "runs": res}
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
