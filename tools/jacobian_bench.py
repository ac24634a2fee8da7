"""Time the fused value-and-Jacobian decodes (K13, cfd_siren_forward_jacobian; K13s,
cfd_siren_forward_jacobian_split) against the plain decode, and check that the change
left every existing kernel alone.

    python tools/jacobian_bench.py [--parent libconfild_hip_parent.so] [--ratios FILE]
                                   [--out profiles/siren_jacobian_split.json]

Timing (in this process): per shape (d, L, c, nh, H), the same N = 65,536 points
and 8 latent rows through
  decode/f32        SIRENAutodecoder_film.decode, exact fp32 MFMA chain
  decode/split_f16  the same decode in the default split-f16 mode (context)
  jacobian          decode_jacobian (the exact fp32 chain, K13)
  jacobian/split_f16  decode_jacobian(compute="split_f16") (K13s)
warm runs first, then `--rounds` rounds interleaving the four, each `--iters`
back-to-back calls between two device events.  The model is (1 + d) x the f32
decode (the chains of a point share an MFMA; 4 x with the idle column at d = 2);
for the split form, the RS = 4 MFMA columns a point takes against the split decode's
one.  (profiles/siren_jacobian.json is the three-form record of K13's own change.)

--parent: a build of the parent commit under confild_amd/lib.  Runs tools/libdiff.py
(every case's output hash, parent against this build) and `python bench.py`
alternating between the two libraries (CFD_LIB), `--bench-rounds` runs each.
--ratios: the JSON lines tests/test_gpu_siren_jacobian.py or
tests/test_gpu_siren_jacobian_split.py print (pytest -s), kept as the measured error
ratios.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(3, 384, 3, 15, 384), (2, 256, 4, 10, 256)]
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
    coords = torch.from_numpy(synth.uniform(1, "jb/x", (N, d), 0.0, 1.0)).to(dev)
    lat = (torch.from_numpy(synth.normal(2, "jb/z", (ROWS, 1, L))) * 0.5).to(dev)
    xn = Normalizer_ts(params=(torch.ones(1, d), torch.zeros(1, d)), method="-11", dim=0)
    yn = Normalizer_ts(params=(torch.full((c,), 2.0), torch.full((c,), -2.0)), method="-11", dim=0)

    def decode(mode):
        nf.set_compute(mode)
        return nf.decode(coords, lat, xn, yn)

    runs = {"decode/f32": lambda: decode("f32"), "decode/split_f16": lambda: decode("split_f16"),
            "jacobian": lambda: nf.decode_jacobian(coords, lat, xn, yn),
            "jacobian/split_f16": lambda: nf.decode_jacobian(coords, lat, xn, yn, compute="split_f16")}
    for fn in runs.values():          # warm: code objects, handle, normaliser cache
        for _ in range(3):
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
    model = 1 + d if d != 2 else 4
    ratio = best["jacobian"] / best["decode/f32"]
    # hidden-layer FLOP of the launch as the algorithm needs them: (1 + d) chains
    flops = 2.0 * nh * H * H * (1 + d) * N * ROWS
    split = "jacobian/split_f16"
    columns = 2 if d == 1 else 4        # MFMA columns per point (RS) against the split decode's one
    return {"dims": list(dims), "N": N, "rows": ROWS, "ms_per_call": ms, "best_ms": best,
            "jacobian_over_decode_f32": ratio, "model": model, "ratio_over_model": ratio / model,
            "jacobian_over_decode_split_f16": best["jacobian"] / best["decode/split_f16"],
            "jacobian_hidden_tflops": flops / (best["jacobian"] * 1e-3) / 1e12,
            "split_slowest_ms": max(ms[split]), "jacobian_fastest_ms": best["jacobian"],
            "split_slowest_below_jacobian_fastest": max(ms[split]) < best["jacobian"],
            "jacobian_over_split": best["jacobian"] / best[split],
            "split_over_decode_split_f16": best[split] / best["decode/split_f16"], "column_model": columns,
            "split_ratio_over_column_model": best[split] / best["decode/split_f16"] / columns,
            "split_hidden_tflops": flops / (best[split] * 1e-3) / 1e12}


def bench_headline(lib, steps, warmup):
    env = dict(os.environ)
    if lib:
        env["CFD_LIB"] = lib
    else:
        env.pop("CFD_LIB", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"bench.py ({lib or 'this build'}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"value"' in ln][-1])
    return rec["value"]


def untouched(parent, rounds, steps, warmup):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import libdiff                      # one child process per build, as `python tools/libdiff.py a b`
    ra = libdiff.run(parent)
    print("libdiff:", len(ra), "cases on", parent, flush=True)
    rb = libdiff.run("libconfild_hip.so")
    diff = {"a": parent, "b": "libconfild_hip.so", "cases": len(ra), "differ": [k for k in ra if ra[k] != rb.get(k)]}
    print("libdiff:", json.dumps(diff), flush=True)
    vals = {"parent": [], "this": []}
    for _ in range(rounds):
        vals["parent"].append(bench_headline(parent, steps, warmup))
        vals["this"].append(bench_headline(None, steps, warmup))
        print("bench.py fields/s: parent", vals["parent"][-1], "this", vals["this"][-1], flush=True)
    lo, hi = min(vals["parent"]), max(vals["parent"])
    return {"libdiff": diff,
            "bench": {"command": f"python bench.py --gpus 1 --steps {steps} --warmup {warmup}", "unit": "fields/s",
                      "order": "parent, this build, alternating; one process each", "values": vals,
                      "parent_range": [lo, hi],
                      "this_inside_parent_range": [lo <= v <= hi for v in vals["this"]]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=2)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--ratios", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siren_jacobian_split.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/jacobian_bench.py measures on the GPU; no HIP device is visible")
    doc = {"what": "decode_jacobian (fused value + coordinate Jacobian) on the exact fp32 MFMA chain and on the "
                   f"split-f16 chain, against decode; N = {N} points, {ROWS} latent rows, synthetic weights; ms per "
                   f"call from device events around {a.iters} back-to-back calls, the four interleaved for "
                   f"{a.rounds} rounds after warm runs; best_ms = fastest round",
           "timing": []}
    for dims in SHAPES:
        one = time_shape(dims, a.rounds, a.iters)
        doc["timing"].append(one)
        print(json.dumps({k: one[k] for k in ("dims", "ms_per_call", "jacobian_over_decode_f32", "model",
                                              "ratio_over_model", "jacobian_over_split",
                                              "split_slowest_below_jacobian_fastest",
                                              "split_over_decode_split_f16")}), flush=True)
    if a.ratios:
        rows = []
        for ln in open(a.ratios):
            if '"ratio_max"' in ln:            # pytest -v puts the test's id in front of the line
                rows.append(json.loads(ln[ln.index("{"):].strip()))
        doc["error_ratios"] = {"what": "|jac - J64| over max(e32, 1e-7 |J64|max), max and mean; J64: autograd through "
                                       "the CPU oracle in fp64, e32: the CPU fp32 autograd's error against it "
                                       "(the Jacobian tests)", "cases": rows,
                               "largest": max([max(r["ratio_max"], r["ratio_mean"]) for r in rows], default=None)}
    if a.parent:
        doc["existing_kernels"] = untouched(a.parent, a.bench_rounds, a.bench_steps, a.bench_warmup)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
