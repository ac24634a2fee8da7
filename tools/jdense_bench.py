"""Time the dense Jacobian adjoint (K16, cfd_siren_jdense_grad) at the Case2 widths,
one sample of T = 256 rows x N = 16384 points in a 1 GB budget, against
  dense_f32   K12's fp32 sum form (cfd_siren_dense_grad, set_dense_form("sum", "f32")) at
              the same shape: the column model says RS = 4 x (a pair takes 4 of the
              MFMA's 16 columns where the value chain takes one);
  jtape       the whole-tape K15 path (jac_tape_forward + cfd_dps_residual_linear +
              jac_tape_vjp) at the largest N whose tape fits in the free memory (and
              under --jtape-cap points, 47 GB of tape by default: the GPU may be
              shared), compared per (row, point) pair;
and check that the change left every existing kernel alone.

    python tools/jdense_bench.py [--parent libconfild_hip_parent.so] [--ratios FILE ...]
                                 [--out profiles/dense_stencil.json]

Each form runs in a child process of its own per round (warm calls, then `--iters`
calls between two device events); the rounds interleave the forms.  best_ms is the
fastest round.  Numbers are recorded, not gated.

--parent: an in-tree build of the parent commit (confild_amd/lib/<name>): tools/libdiff.py
against it, and bench.py --gpus 1 alternating with it.  --ratios: logs with the JSON
lines tests/test_gpu_siren_jdense.py prints.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (2, 256, 4, 10, 256)      # the Case2 widths
ROWS, POINTS, BUDGET = 256, 16384, 1 << 30
FORMS = ("jdense", "dense_f32", "jtape")

CHILD = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1])
form, iters, N = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
from confild_amd import synth
from confild_amd.guided import stencils
from confild_amd.guided.measurements import SensorStencilOperator
from confild_amd.nf_networks import SIRENAutodecoder_film
from confild_amd.normalize import Normalizer_ts
dims, R, budget = tuple(json.loads(sys.argv[5])), int(sys.argv[6]), int(sys.argv[7])
d, L, c, nh, H = dims
dev = torch.device("cuda", 0)
nf = SIRENAutodecoder_film(*dims)
nf.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(7, *dims).items()})
nf.to(dev)
nf.set_compute("f32")
pair_bytes = 4 * (2 + d) * (nh + 1) * H
if form == "jtape" and N == 0:      # the largest whole number of slabs whose tape fits in 80 % of the free memory
    free = torch.cuda.mem_get_info(dev)[0]
    N = min(int(sys.argv[8]), int(0.8 * free / (pair_bytes * R)) // 64 * 64)
coords = torch.from_numpy(synth.uniform(1, "jdb/x", (N, d), 0.0, 1.0)).to(dev)
lat = (torch.from_numpy(synth.normal(2, "jdb/z", (R, L))) * 0.5).to(dev)
xn = Normalizer_ts(params=(torch.ones(1, d), torch.zeros(1, d)), method="-11", dim=0)
yn = Normalizer_ts(params=(torch.full((c,), 2.0), torch.full((c,), -2.0)), method="-11", dim=0)
wv, wj = stencils.stack([stencils.vorticity_z(c, d), stencils.divergence(d, c)], c, d)   # M = 2, derivative readings
M = 2
y = torch.from_numpy(synth.normal(3, "jdb/y", (R, N, M))).to(dev)
if form == "jdense":
    wjd = torch.as_tensor(wj).to(dev)
    run = lambda: nf.jac_dense_grad(coords, lat, R, y, None, wjd, None, xn, yn, budget)
elif form == "dense_f32":
    yv = torch.from_numpy(synth.normal(3, "jdb/yv", (R, N, c))).to(dev)
    nf.set_dense_form("sum", "f32")
    run = lambda: nf.dense_grad(coords, lat, R, yv, None, xn, yn, budget)
else:
    op = SensorStencilOperator.from_parts(dev, coords, xn, yn, nf, torch.ones(L), -torch.ones(L), value_weights=wv,
                                          jac_weights=wj)
    def run():
        out, jac = nf.jac_tape_forward(coords, lat, xn, yn)
        _, g_out, g_jac, _ = op.residual(out, jac, y, 1)
        return nf.jac_tape_vjp(g_out, g_jac)
run()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(iters):
    run()
e1.record()
e1.synchronize()
print(json.dumps({"form": form, "N": N, "ms": e0.elapsed_time(e1) / iters,
                  "workspace_bytes": getattr(nf, "dense_workspace_bytes", None) if form != "jtape" else pair_bytes * R * N,
                  "peak_bytes": torch.cuda.max_memory_allocated(dev)}))
"""


def child(form, iters, N, cap):
    env = dict(os.environ)
    env.pop("CFD_LIB", None)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, form, str(iters), str(N), json.dumps(DIMS), str(ROWS),
                        str(BUDGET), str(cap)], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"{form} failed with {p.returncode}:\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def bench_headline(lib, steps, warmup):
    env = dict(os.environ)
    env.pop("CFD_LIB", None)
    if lib:
        env["CFD_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f"bench.py ({lib or 'this build'}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"value"' in ln][-1])["value"]


def untouched(parent, rounds, steps, warmup, libdiff):
    res = {}
    if libdiff:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "libdiff.py"), parent, "libconfild_hip.so"],
                           capture_output=True, text=True, timeout=1800)
        if not p.stdout.strip():
            raise SystemExit(f"libdiff failed with {p.returncode}:\n{p.stderr[-2000:]}")
        res["libdiff"] = dict(json.loads(p.stdout.strip().splitlines()[-1]), exit_code=p.returncode)
        print("libdiff:", json.dumps(res["libdiff"]), flush=True)
    vals = {"parent": [], "this": []}
    for _ in range(rounds):
        vals["parent"].append(bench_headline(parent, steps, warmup))
        vals["this"].append(bench_headline(None, steps, warmup))
        print("bench.py: parent", vals["parent"][-1], "this", vals["this"][-1], flush=True)
    lo, hi = min(vals["parent"]), max(vals["parent"])
    res["bench"] = {"command": f"python bench.py --gpus 1 --steps {steps} --warmup {warmup}",
                    "order": "parent, this build, alternating; one process each", "values": vals,
                    "parent_range": [lo, hi], "this_inside_parent_range": [lo <= v <= hi for v in vals["this"]]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--jtape-points", type=int, default=0, help="N of the whole-tape form (0: what fits in memory)")
    ap.add_argument("--jtape-cap", type=int, default=4096, help="most points the whole-tape form may take")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--no-libdiff", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--ratios", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_stencil.json"))
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    d, L, c, nh, H = DIMS
    if not a.no_timing:
        runs = {f: [] for f in FORMS}
        for _ in range(a.rounds):
            for f in FORMS:
                runs[f].append(child(f, a.iters, a.jtape_points if f == "jtape" else POINTS, a.jtape_cap))
                print(json.dumps(runs[f][-1]), flush=True)
        best = {f: min(r["ms"] for r in runs[f]) for f in FORMS}
        nj = runs["jtape"][0]["N"]
        per_pair = {f: best[f] * 1e3 / (ROWS * (nj if f == "jtape" else POINTS)) for f in FORMS}   # us per pair
        doc["timing"] = {
            "what": f"one call at the Case2 widths {list(DIMS)}, {ROWS} rows of one sample, f32 compute; jdense and "
                    f"dense_f32 at N = {POINTS} in a budget of {BUDGET} bytes, jtape at N = {nj} (the whole tape in "
                    f"memory); ms per call from device events around {a.iters} calls after a warm one, one child "
                    f"process per form and round, {a.rounds} rounds interleaved; best_ms = fastest round",
            "runs": runs, "best_ms": best, "us_per_pair": per_pair,
            "jdense_over_dense_f32": best["jdense"] / best["dense_f32"], "model": 4,
            "ratio_over_model": best["jdense"] / best["dense_f32"] / 4,
            "jdense_over_jtape_per_pair": per_pair["jdense"] / per_pair["jtape"],
            "whole_tape_bytes_at_full_shape": 4 * (2 + d) * (nh + 1) * H * ROWS * POINTS,
            # hidden-layer FLOP the two chain launches issue (4 columns per pair)
            "jdense_mfma_tflops": 2.0 * 2.0 * nh * H * H * 4 * ROWS * POINTS / (best["jdense"] * 1e-3) / 1e12}
    rows, k15 = [], []
    for path in a.ratios:
        for ln in open(path):
            if '"ratio_max"' in ln:
                rows.append(json.loads(ln[ln.index("{"):ln.rindex("}") + 1]))
            elif '"vs_k15_max"' in ln:
                k15.append(json.loads(ln[ln.index("{"):ln.rindex("}") + 1]))
    if rows:
        doc["error_ratios"] = {
            "what": "|g_z - g64| over max(e32, 1e-7 |g64|max), max and mean; g64: double autograd of the per-sample "
                    "norms through the CPU oracle in fp64, e32: the CPU fp32 double autograd's error against it; "
                    "norm_rel: the norms' relative error; vs_k15: the difference to jac_tape_forward + "
                    "cfd_dps_residual_linear + jac_tape_vjp under the same yardstick "
                    "(tests/test_gpu_siren_jdense.py)",
            "cases": rows, "vs_k15": k15, "largest": max(max(r["ratio_max"], r["ratio_mean"]) for r in rows),
            "largest_norm_rel": max(r["norm_rel"] for r in rows),
            "largest_vs_k15": max([max(r["vs_k15_max"], r["vs_k15_mean"]) for r in k15], default=None)}
    if a.parent:
        doc["existing_kernels"] = untouched(a.parent, a.bench_rounds, a.bench_steps, a.bench_warmup, not a.no_libdiff)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
