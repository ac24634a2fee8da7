"""Time the fused value-Jacobian-Hessian decode (K14, cfd_siren_forward_hessian) against
the plain decode and K13, and check that the change left every existing kernel alone.

    python tools/hessian_bench.py [--parent libconfild_hip_parent.so] [--ratios FILE]
                                  [--out profiles/siren_hessian.json]

Timing (in this process): per shape (d, L, c, nh, H), the same N = 65,536 points
and 8 latent rows through
  decode/f32     SIRENAutodecoder_film.decode, exact fp32 MFMA chain
  jacobian       decode_jacobian (K13)
  hessian        decode_hessian, the full form
  hessian/diag   decode_hessian(diag=True) (d = 3: its own 8-column form)
warm runs first, then `--rounds` rounds interleaving them, each `--iters`
back-to-back calls between two device events.  The column model: a point takes RS of
the MFMA's 16 columns, so a launch costs RS x the f32 decode: K13 4 x; K14 16 x
(d = 3, full), 8 x (d = 3 diagonal, d = 2), 4 x (d = 1).

--parent, --ratios: as tools/jacobian_bench.py (libdiff and bench.py against a build
of the parent commit; the JSON lines tests/test_gpu_siren_hessian.py prints).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = [(3, 64, 3, 15, 384), (2, 256, 4, 10, 256)]
N, ROWS = 65536, 8


def time_shape(dims, rounds, iters):
    import torch

    from confild_amd import synth
    from confild_amd.nf_networks import SIRENAutodecoder_film
    from confild_amd.normalize import Normalizer_ts
    dev = torch.device("cuda", 0)
    d, L, c, nh, H = dims
    nf = SIRENAutodecoder_film(*dims)
    nf.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(7, *dims).items()})
    nf.to(dev)
    nf.set_compute("f32")
    coords = torch.from_numpy(synth.uniform(1, "hb/x", (N, d), 0.0, 1.0)).to(dev)
    lat = (torch.from_numpy(synth.normal(2, "hb/z", (ROWS, 1, L))) * 0.5).to(dev)
    xn = Normalizer_ts(params=(torch.ones(1, d), torch.zeros(1, d)), method="-11", dim=0)
    yn = Normalizer_ts(params=(torch.full((c,), 2.0), torch.full((c,), -2.0)), method="-11", dim=0)
    runs = {"decode/f32": lambda: nf.decode(coords, lat, xn, yn),
            "jacobian": lambda: nf.decode_jacobian(coords, lat, xn, yn),
            "hessian": lambda: nf.decode_hessian(coords, lat, xn, yn),
            "hessian/diag": lambda: nf.decode_hessian(coords, lat, xn, yn, diag=True)}
    for fn in runs.values():          # warm: code objects, handle, normaliser cache
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    best = {k: min(v) for k, v in ms.items()}
    model = {"jacobian": 4 if d > 1 else 2, "hessian": {1: 4, 2: 8, 3: 16}[d], "hessian/diag": {1: 4, 2: 8, 3: 8}[d]}
    over = {k: best[k] / best["decode/f32"] for k in model}
    return {"dims": list(dims), "N": N, "rows": ROWS, "ms_per_call": ms, "best_ms": best, "over_decode_f32": over,
            "model": model, "ratio_over_model": {k: over[k] / model[k] for k in model},
            # hidden-layer FLOP the MFMAs issue (all 16 columns, idle ones included)
            "hessian_mfma_tflops": 2.0 * nh * H * H * model["hessian"] * N * ROWS / (best["hessian"] * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=2)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--ratios", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siren_hessian.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/hessian_bench.py measures on the GPU; no HIP device is visible")
    doc = {"what": "decode_hessian (fused value + Jacobian + coordinate Hessian, exact fp32 MFMA chain) against "
                   f"decode and decode_jacobian; N = {N} points, {ROWS} latent rows, synthetic weights; ms per call "
                   f"from device events around {a.iters} back-to-back calls, the forms interleaved for {a.rounds} "
                   "rounds after warm runs; best_ms = fastest round",
           "timing": []}
    for dims in SHAPES:
        one = time_shape(dims, a.rounds, a.iters)
        doc["timing"].append(one)
        print(json.dumps({k: one[k] for k in ("dims", "best_ms", "over_decode_f32", "model", "ratio_over_model")}),
              flush=True)
    if a.ratios:
        rows = []
        for ln in open(a.ratios):
            if '"ratio_max"' in ln:            # pytest -v puts the test's id in front of the line
                rows.append(json.loads(ln[ln.index("{"):ln.rindex("}") + 1]))
        doc["error_ratios"] = {"what": "|hess - H64| over max(e32, 1e-7 |H64|max), max and mean; H64: double autograd "
                                       "through the CPU oracle in fp64, e32: the CPU fp32 double autograd's error "
                                       "against it; jac_ratio_*: the same call's Jacobian under K13's yardstick "
                                       "(tests/test_gpu_siren_hessian.py)", "cases": rows,
                               "largest": max([max(r["ratio_max"], r["ratio_mean"]) for r in rows], default=None),
                               "largest_jac": max([max(r["jac_ratio_max"], r["jac_ratio_mean"]) for r in rows],
                                                  default=None)}
    if a.parent:
        from jacobian_bench import untouched
        doc["existing_kernels"] = untouched(a.parent, a.bench_rounds, a.bench_steps, a.bench_warmup)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
