"""Time the fused SIREN Jacobian adjoint (K15, cfd_siren_jtape_forward / _vjp) against
the fp32 value tape (cfd_siren_tape_forward / _vjp in f32 compute) at the same (row,
sensor) pairs, and check that the change left every existing kernel alone.

    python tools/jvjp_bench.py [--parent libconfild_hip_parent.so] [--ratios FILE ...]
                               [--out profiles/siren_jvjp.json]

Timing (in this process): per shape (d, L, c, nh, H), R latent rows at Ns sensors through
  tape/fwd, tape/vjp     SIRENAutodecoder_film.tape_forward / tape_vjp, f32 compute
  jtape/fwd, jtape/vjp   jac_tape_forward / jac_tape_vjp (both gradients given)
warm runs first, then `--rounds` rounds interleaving them, each `--iters` back-to-back
calls between two device events.  The column model: a pair takes RS = 4 of the MFMA's
16 columns (d > 1) where the value tape takes one, so a K15 launch costs 4 x the value
tape's at equal matrix-pipe use.  The number is recorded, not gated.

--parent, --ratios: as tools/jacobian_bench.py (libdiff and bench.py against a build of
the parent commit; the JSON lines tests/test_gpu_siren_jvjp.py prints).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (d, L, c, nh, H), R, Ns: the Case4 widths at one step's pairs, and the Case2 widths
SHAPES = [((3, 64, 3, 15, 384), 384, 10), ((2, 256, 4, 10, 256), 384, 10)]


def time_shape(dims, R, Ns, rounds, iters):
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
    coords = torch.from_numpy(synth.uniform(1, "jb/x", (Ns, d), 0.0, 1.0)).to(dev)
    lat = (torch.from_numpy(synth.normal(2, "jb/z", (R, L))) * 0.5).to(dev)
    G0 = torch.from_numpy(synth.normal(3, "jb/g0", (R, Ns, c))).to(dev)
    G1 = torch.from_numpy(synth.normal(4, "jb/g1", (R, Ns, c, d))).to(dev)
    xn = Normalizer_ts(params=(torch.ones(1, d), torch.zeros(1, d)), method="-11", dim=0)
    yn = Normalizer_ts(params=(torch.full((c,), 2.0), torch.full((c,), -2.0)), method="-11", dim=0)
    runs = {"tape/fwd": lambda: nf.tape_forward(coords, lat, xn, yn),
            "tape/vjp": lambda: nf.tape_vjp(G0),
            "jtape/fwd": lambda: nf.jac_tape_forward(coords, lat, xn, yn),
            "jtape/vjp": lambda: nf.jac_tape_vjp(G0, G1)}
    for fn in runs.values():          # warm: code objects, handle, normaliser cache, both tapes
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
    model = 4 if d > 1 else 2
    pair = {"tape": best["tape/fwd"] + best["tape/vjp"], "jtape": best["jtape/fwd"] + best["jtape/vjp"]}
    over = {"fwd": best["jtape/fwd"] / best["tape/fwd"], "vjp": best["jtape/vjp"] / best["tape/vjp"],
            "pair": pair["jtape"] / pair["tape"]}
    return {"dims": list(dims), "rows": R, "sensors": Ns, "pairs": R * Ns, "ms_per_call": ms, "best_ms": best,
            "pair_ms": pair, "over_tape_f32": over, "model": model,
            "ratio_over_model": {k: v / model for k, v in over.items()},
            # hidden-layer FLOP the two K15 launches issue (all 16 columns, idle ones included)
            "jtape_mfma_tflops": 2.0 * 2.0 * nh * H * H * model * R * Ns / (pair["jtape"] * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=2)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--ratios", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siren_jvjp.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/jvjp_bench.py measures on the GPU; no HIP device is visible")
    doc = {"what": "jac_tape_forward / jac_tape_vjp (K15: latent gradient of a linear functional of value and "
                   "coordinate Jacobian, exact fp32 MFMA chain) against tape_forward / tape_vjp in f32 compute at the "
                   "same (row, sensor) pairs; synthetic weights; ms per call from device events around "
                   f"{a.iters} back-to-back calls, the four interleaved for {a.rounds} rounds after warm runs; "
                   "best_ms = fastest round; the Python wrapper's allocations are inside both",
           "timing": []}
    for dims, R, Ns in SHAPES:
        one = time_shape(dims, R, Ns, a.rounds, a.iters)
        doc["timing"].append(one)
        print(json.dumps({k: one[k] for k in ("dims", "pairs", "best_ms", "over_tape_f32", "model",
                                              "ratio_over_model")}), flush=True)
    rows, halves = [], []
    for path in a.ratios:
        for ln in open(path):
            if '"ratio_max"' in ln:            # pytest -v puts the test's id in front of the line
                rows.append(json.loads(ln[ln.index("{"):ln.rindex("}") + 1]))
            elif '"vs_tape_vjp_max"' in ln:
                halves.append(json.loads(ln[ln.index("{"):ln.rindex("}") + 1]))
    if rows:
        doc["error_ratios"] = {"what": "|g_z - g64| over max(e32, 1e-7 |g64|max), max and mean; g64: double autograd of "
                                       "<G0, out> + <G1, J> through the CPU oracle in fp64, e32: the CPU fp32 double "
                                       "autograd's error against it; jac_ratio_*: the forward's Jacobian under K13's "
                                       "yardstick; value_half: G1 = None against tape_vjp in f32 compute and against "
                                       "fp64 (tests/test_gpu_siren_jvjp.py)", "cases": rows, "value_half": halves,
                               "largest": max(max(r["ratio_max"], r["ratio_mean"]) for r in rows),
                               "largest_jac": max(max(r["jac_ratio_max"], r["jac_ratio_mean"]) for r in rows)}
    if a.parent:
        from jacobian_bench import untouched
        doc["existing_kernels"] = untouched(a.parent, a.bench_rounds, a.bench_steps, a.bench_warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
