"""Time the dense DPS operator adjoint alone (cfd_siren_dense_grad)
at the Case2 widths: SIREN (2, 256, 4, 10, 256), T = 256 rows, B = 1, N points in
{1024, 4096, 16384}.  Writes profiles/dense_dps.json.

    python tools/dense_dps_bench.py [--reps 20] [--sizes 1024,4096,16384] [--out profiles/dense_dps.json]

Variants, alternated inside every repeat (one call each, device events around it):
  tape              the present route, tape_forward + cfd_dps_residual + tape_vjp (whole
                    tape in memory: 5.9 GB at N = 1024, 23.6 GB at 4096; not run above)
  sum/f32           tile sums on chip, fp32 MFMA chain           (default budget)
  delta/f32         delta tape per chunk + column sums, fp32 chain
  sum/split_f16     tile sums on chip, K9t split-f16 tape kernels
  delta/split_f16   delta tape per chunk + column sums, K9t
  <form>@<budget>   sum/f32 and sum/split_f16 at 256 MiB (Infinity Cache) and 4 GiB (1 GiB above)
Workspaces come from torch's caching allocator, kept warm: the warm-up rounds allocate,
the timed rounds reuse the blocks (no hipMalloc inside a timed region).
Per (size, variant): median ms, the spread (min, max, inter-quartile range) over the
repeats, the algorithmic FLOP -- per (row, point) pair 2 * 2 * nh * H^2 for the hidden
layers forward and backward, 2 * d * H the first layer, 2 * 2 * H * c the last layer and
its input gradient -- and the share of the peak that applies: the fp32 MFMA peak for
the fp32 chain, the f16 MFMA peak / 3 for the three-product split.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from confild_amd import _lib, synth  # noqa: E402
from confild_amd.nf_networks import SIRENAutodecoder_film  # noqa: E402
from confild_amd.normalize import Normalizer_ts  # noqa: E402

DIMS = (2, 256, 4, 10, 256)
T = 256
PEAK_F32_MFMA = 157.3e12          # MI355X, v_mfma_f32_16x16x4_f32
PEAK_F16_MFMA = 16 * 157.3e12     # v_mfma_f32_16x16x32_f16
MiB, GiB = 1 << 20, 1 << 30


def flop(N):
    d, L, c, nh, H = DIMS
    return T * N * (2 * 2 * nh * H * H + 2 * d * H + 2 * 2 * H * c)


DEFAULT = "sum/split_f16"   # what cfd_siren_dense_grad runs for a handle in split_f16 compute (the default)


def summarise(result):
    """The shipped defaults and what the measurements say about them."""
    result["default"] = {
        "budget_bytes": GiB,
        "split_f16_compute": {"compute": "split_f16 (K9t tape kernels)", "backward": "sum", "variant": DEFAULT},
        "f32_compute": {"compute": "f32", "backward": "sum", "variant": "sum/f32"},
        "allocation": "torch caching allocator kept warm; no allocation inside a timed region",
        "note": "verdict[N] names the fastest variant, the losing variants' times and, per form, the times at "
                "256 MiB, 1 GiB and 4 GiB (budget_ms).  1 GiB is the shipped default budget.",
    }
    verdict = {}
    for N, rec in result["sizes"].items():
        v = {"fastest": min(rec, key=lambda k: rec[k]["ms"]), "default_ms": rec[DEFAULT]["ms"],
             "default_workspace_bytes": rec[DEFAULT]["workspace_bytes"],
             "losing_ms": {k: r["ms"] for k, r in rec.items() if k != DEFAULT}}
        v["budget_ms"] = {form: {tag: rec[form + ("" if tag == "1GiB" else "@" + tag)]["ms"]
                                 for tag in ("256MiB", "1GiB", "4GiB")
                                 if form + ("" if tag == "1GiB" else "@" + tag) in rec}
                          for form in (DEFAULT, "sum/f32")}
        if "tape" in rec:
            spread = max(rec[DEFAULT]["iqr_ms"], rec["tape"]["iqr_ms"])
            v.update(tape_ms=rec["tape"]["ms"], spread_ms=spread,
                     default_not_slower_than_tape=bool(rec[DEFAULT]["ms"] <= rec["tape"]["ms"] + spread),
                     f32_default_not_slower_than_tape=bool(rec["sum/f32"]["ms"] <= rec["tape"]["ms"] + spread))
        else:
            v["tape"] = ("not run: the whole tape is 2 R N (nh+1) H floats = %.1f GB" %
                         (2 * T * int(N) * 11 * 256 * 4 / 1e9))
        verdict[N] = v
    result["verdict"] = verdict
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resummarise", help="recompute the default / verdict sections of an existing record (no GPU)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--tape-max", type=int, default=4096, help="largest N the whole-tape route is run at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_dps.json"))
    a = ap.parse_args()
    if a.resummarise:
        with open(a.resummarise) as f:
            result = summarise(json.load(f))
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
        print("wrote", a.out)
        return
    dev = torch.device("cuda", 0)
    d, L, c, nh, H = DIMS
    sd = synth.siren_state_dict(61, d, L, c, nh, H)

    def module(compute, form):
        nf = SIRENAutodecoder_film(d, L, c, nh, H)
        nf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return nf.to(dev).set_compute(compute).set_dense_form(*form).prepare(dev)

    mods = {"sum/f32": module("split_f16", ("sum", "f32")), "delta/f32": module("split_f16", ("delta", "f32")),
            "sum/split_f16": module("split_f16", ("sum", "auto")),
            "delta/split_f16": module("split_f16", ("delta", "auto"))}
    xn = Normalizer_ts(method="-11", dim=0, params=[torch.tensor([1., 1.]), torch.tensor([0., 0.])])
    yn = Normalizer_ts(method="-11", dim=0, params=[torch.tensor([[0.9617, 0.2666, 0.2869, 0.0290]]),
                                                    torch.tensor([[-0.0051, -0.2073, -0.2619, -0.0419]])])
    z = (torch.from_numpy(synth.normal(61, "z", (T, L))) * 0.5).to(dev)
    lib = _lib.lib()
    st = _lib.stream_of(dev)
    result = {"siren": list(DIMS), "rows_per_sample": T, "batch": 1, "reps": a.reps, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "peak_f32_mfma_tflops": PEAK_F32_MFMA / 1e12,
              "peak_f16_mfma_over_3_tflops": PEAK_F16_MFMA / 3 / 1e12, "sizes": {}}
    for N in (int(s) for s in a.sizes.split(",")):
        coords = torch.from_numpy(synth.uniform(61, f"c{N}", (N, d), 0.0, 1.0)).to(dev)
        y = torch.from_numpy(synth.normal(61, f"y{N}", (T, N, c))).to(dev)
        mask = torch.from_numpy((synth.uniform(61, f"m{N}", (T, N, c), 0., 1.) < 0.6).astype(np.float32)).to(dev)
        variants = {}

        def dense(name, budget=None):
            nf = mods[name]
            return lambda: nf.dense_grad(coords, z, T, y, mask, xn, yn, budget)

        if N <= a.tape_max:
            tp = mods["sum/f32"]      # the handle in its default (split_f16) compute, as the sampler has it
            ym = y                    # the present route has no mask: the unmasked residual, same FLOP

            def tape():
                A = tp.tape_forward(coords, z, xn, yn)
                gA = torch.empty_like(A)
                dist = torch.empty(1, device=dev)
                _lib.check(lib.cfd_dps_residual(_lib.ptr(ym), 0, _lib.ptr(A), _lib.ptr(gA), _lib.ptr(dist),
                                                A.numel(), 1, st), "cfd_dps_residual")
                return tp.tape_vjp(gA), dist
            variants["tape"] = (tape, "f32")   # P >= 32768 pairs: launch_tape sends both modes to the fp32 chain
        variants["sum/f32"] = (dense("sum/f32"), "f32")
        variants["delta/f32"] = (dense("delta/f32"), "f32")
        variants["sum/split_f16"] = (dense("sum/split_f16"), "split_f16")
        variants["delta/split_f16"] = (dense("delta/split_f16"), "split_f16")
        for b, tag in ((256 * MiB, "256MiB"), (4 * GiB, "4GiB")):
            variants[f"sum/f32@{tag}"] = (dense("sum/f32", b), "f32")
            variants[f"{DEFAULT}@{tag}"] = (dense(DEFAULT, b), "split_f16")
        times = {k: [] for k in variants}
        ws = {}
        for rep in range(a.warmup + a.reps):
            for name, (fn, _) in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                e1.synchronize()
                del out
                if rep >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
                if name != "tape":
                    ws[name] = mods[name.split("@")[0]].dense_workspace_bytes
        rec = {}
        for name, (_, comp) in variants.items():
            t = np.array(times[name])
            med = float(np.median(t))
            peak = PEAK_F32_MFMA if comp == "f32" else PEAK_F16_MFMA / 3
            rec[name] = {"ms": med, "min_ms": float(t.min()), "max_ms": float(t.max()),
                         "iqr_ms": float(np.percentile(t, 75) - np.percentile(t, 25)), "flop": flop(N),
                         "tflops": flop(N) / med / 1e9, "compute": comp,
                         "share_of_peak": flop(N) / (med * 1e-3) / peak}
            if name in ws:
                rec[name]["workspace_bytes"] = ws[name]
            else:
                n = C.c_size_t()
                _lib.check(lib.cfd_siren_vjp_workspace_bytes(tp._handle(dev), N, T, C.byref(n)), "vjp workspace")
                rec[name]["workspace_bytes"] = n.value
            print(f"N={N:6d} {name:18s} {med:9.3f} ms  (min {t.min():.3f}, max {t.max():.3f})  "
                  f"{rec[name]['tflops']:7.1f} TFLOP/s  {100 * rec[name]['share_of_peak']:5.1f} % of peak  "
                  f"ws {rec[name]['workspace_bytes'] / MiB:9.1f} MiB", flush=True)
        result["sizes"][str(N)] = rec
        del coords, y, mask
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summarise(result), f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
