"""Time the fused value-Jacobian-Hessian decode (K14, cfd_siren_forward_hessian) against
the plain decode and K13, and check that the change left every existing kernel alone.

    python tools/hessian_bench.py [--parent libconfild_hip_parent.so] [--ratios FILE]
                                  [--out profiles/siren_hessian.json]
    python tools/hessian_bench.py --split [--resources FILE] [--parent ...] [--ratios FILE]
                                  [--out profiles/siren_hessian_split.json]

Timing (in this process): per shape (d, L, c, nh, H), the same N = 65,536 points
and 8 latent rows through
  decode/f32     SIRENAutodecoder_film.decode, exact fp32 MFMA chain
  jacobian       decode_jacobian (K13)
  hessian        decode_hessian, the full form
  hessian/diag   decode_hessian(diag=True) (d = 3: its own 8-column form)
and with --split also through the split-f16 forms (K14s, cfd_siren_forward_hessian_split)
  decode/split_f16          decode on the split-f16 chain
  jacobian/split_f16        decode_jacobian(compute="split_f16") (K13s)
  hessian/split_f16         decode_hessian(compute="split_f16")
  hessian/diag/split_f16    decode_hessian(diag=True, compute="split_f16")
warm runs first, then `--rounds` rounds interleaving them, each `--iters`
back-to-back calls between two device events.  The column model: a point takes RS of
the MFMA's 16 columns, so a launch costs RS x the f32 decode: K13 4 x; K14 16 x
(d = 3, full), 8 x (d = 3 diagonal, d = 2), 4 x (d = 1).

With --split the record says whether K14s's slowest round is below K14's fastest, and
gives K14s against RS / 4 x K13s and against RS x the split decode (the column model).

--parent, --ratios: as tools/jacobian_bench.py (libdiff and bench.py against a build
of the parent commit; the JSON lines tests/test_gpu_siren_hessian.py or, with --split,
tests/test_gpu_siren_hessian_split.py print).  --resources: a JSON file with the
compiler's register / LDS / scratch report of every instantiation, copied into the record.
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


def time_shape(dims, rounds, iters, split=False):
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
    S = "split_f16"
    if split:
        # the split decode is the handle's split_f16 mode: a second module on the same weights,
        # so no timed call switches a mode (K13s and K14s take compute= and ignore the mode)
        nfs = SIRENAutodecoder_film(*dims)
        nfs.load_state_dict(nf.state_dict())
        nfs.to(dev)
        nfs.set_compute(S)
        runs.update({"decode/" + S: lambda: nfs.decode(coords, lat, xn, yn),
                     "jacobian/" + S: lambda: nf.decode_jacobian(coords, lat, xn, yn, compute=S),
                     "hessian/" + S: lambda: nf.decode_hessian(coords, lat, xn, yn, compute=S),
                     "hessian/diag/" + S: lambda: nf.decode_hessian(coords, lat, xn, yn, diag=True, compute=S)})
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
    rec = {"dims": list(dims), "N": N, "rows": ROWS, "ms_per_call": ms, "best_ms": best, "over_decode_f32": over,
           "model": model, "ratio_over_model": {k: over[k] / model[k] for k in model},
           # hidden-layer FLOP the MFMAs issue (all 16 columns, idle ones included)
           "hessian_mfma_tflops": 2.0 * nh * H * H * model["hessian"] * N * ROWS / (best["hessian"] * 1e-3) / 1e12}
    if split:
        k13s_rs = 2 if d == 1 else 4    # K13s's columns per point
        rec["split"] = {}
        for form in ("hessian", "hessian/diag"):
            k, rs = form + "/" + S, model[form]
            rec["split"][form] = {
                "slowest_ms": max(ms[k]), "f32_fastest_ms": best[form],
                "slowest_below_f32_fastest": max(ms[k]) < best[form], "f32_over_split": best[form] / best[k],
                "columns": rs, "over_k13s": best[k] / best["jacobian/" + S],
                "over_k13s_column_model": best[k] / best["jacobian/" + S] / (rs / k13s_rs),
                "over_decode_split_f16": best[k] / best["decode/" + S],
                "over_decode_column_model": best[k] / best["decode/" + S] / rs,
                "mfma_tflops": 2.0 * nh * H * H * rs * N * ROWS / (best[k] * 1e-3) / 1e12}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=2)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--ratios", default=None)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "siren_hessian_split.json" if a.split else "siren_hessian.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/hessian_bench.py measures on the GPU; no HIP device is visible")
    doc = {"what": "decode_hessian (fused value + Jacobian + coordinate Hessian, exact fp32 MFMA chain) against "
                   f"decode and decode_jacobian; N = {N} points, {ROWS} latent rows, synthetic weights; ms per call "
                   f"from device events around {a.iters} back-to-back calls, the forms interleaved for {a.rounds} "
                   "rounds after warm runs; best_ms = fastest round",
           "timing": []}
    if a.split:
        doc["what"] += ("; with the split-f16 forms (K14s, K13s, the split decode) in the same rounds: split.* compares "
                        "K14s's slowest round with K14's fastest and gives it against RS / 4 x K13s and RS x the "
                        "split decode (the column model)")
    if a.resources:
        doc["resources"] = json.load(open(a.resources))
    for dims in SHAPES:
        one = time_shape(dims, a.rounds, a.iters, a.split)
        doc["timing"].append(one)
        print(json.dumps({k: one[k] for k in ("dims", "best_ms", "over_decode_f32", "model", "ratio_over_model",
                                              "split") if k in one}), flush=True)
    if a.ratios:
        rows = []
        for ln in open(a.ratios):
            if '"ratio_max"' in ln:            # pytest -v puts the test's id in front of the line
                rows.append(json.loads(ln[ln.index("{"):ln.rindex("}") + 1]))
        if a.split:                            # the log may hold the fp32 test's lines as well
            rows = [r for r in rows if r.get("compute") == "split_f16"]
        doc["error_ratios"] = {"what": "|hess - H64| over max(e32, 1e-7 |H64|max), max and mean; H64: double autograd "
                                       "through the CPU oracle in fp64, e32: the CPU fp32 double autograd's error "
                                       "against it; jac_ratio_*: the same call's Jacobian under K13's yardstick "
                                       "(tests/test_gpu_siren_hessian.py, with --split "
                                       "tests/test_gpu_siren_hessian_split.py)", "cases": rows,
                               "largest": max([max(r["ratio_max"], r["ratio_mean"]) for r in rows], default=None),
                               "largest_jac": max([max(r["jac_ratio_max"], r["jac_ratio_mean"]) for r in rows],
                                                  default=None)}
    if a.ratios and a.split:
        import re
        pat = re.compile(r"(lumped|grid) (f32|split_f16) (\w+) ratio max (\S+) mean (\S+) S (\S+)")
        doc["driver_ratios"] = {"what": "tests/test_gpu_hessian_split_driver.py: the driver's saved quantity against "
                                        "confild_amd.derived of the oracle's fp64 (out, J, H), error over "
                                        "max(e32, 1e-7 S), at both values of derived_hessian_compute",
                                "cases": [{"layout": m[1], "derived_hessian_compute": m[2], "quantity": m[3],
                                           "ratio_max": float(m[4]), "ratio_mean": float(m[5]), "S": float(m[6])}
                                          for m in pat.finditer(open(a.ratios).read())]}
    if a.parent:
        from jacobian_bench import untouched
        doc["existing_kernels"] = untouched(a.parent, a.bench_rounds, a.bench_steps, a.bench_warmup)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
