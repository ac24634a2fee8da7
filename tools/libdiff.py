"""Bit-identity check of two in-tree builds of the library (development tool):
runs a fixed set of HIP-path computations in a child process per build
(CFD_LIB selects the build) and compares the outputs' hashes.

    python tools/libdiff.py libconfild_hip_pre.so libconfild_hip.so

The cases named "up/..." run split-f16 Upsample convolutions (every multi-level
split-f16 U-Net, and cfd_upsample_conv where both builds have it): a build with
another form of that convolution (the phase form against the 9-tap form) differs
there at fp32 rounding level, which is reported as max |a - b| / max |a| per case.
Such a case may differ by at most UP_TOL (1e-5: rounding level of the fp32-accurate
forward and its adjoint; a wrong kernel is orders above it) and fails the run beyond
it.  The "up/" cases whose values are not kept for the comparison (parameter
gradients, the 384^2 model) are listed under `unbounded`.

The cases named "k1h/..." are the remaining ones that contain a forward K1h launch
(the single-level split-f16 U-Nets: a 3x3 convolution of 128 or more output channels
on 256-pixel halo tiles; the multi-level ones and the halo-tiled cfd_upsample_conv
shapes are "up/" cases already): a build with K1h on another MFMA shape (16x16x32
against 32x32x16, make VARIANT=k1h32 VFLAGS=-DCFD_K1H_MFMA32) is expected to differ
there at rounding level, in the forward and in what is computed from its tape, and
is held to the same tolerance.  Every other case must be bit-identical.

The cases named "deriv/..." are the SIREN derivative kernels (K13, K13s, K14, K14s,
K15, K16), every output hashed, with and without the normalisers; `--deriv` runs only
these (a few seconds):

    python tools/libdiff.py libconfild_hip_pre.so libconfild_hip.so --deriv
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP_TOL = 1e-5   # max |a - b| / max |a| an "up/" or "k1h/" case may differ by
ROUNDING = ("up/", "k1h/")   # the cases expected to differ at rounding level

CHILD = r"""
import hashlib, json, sys, torch, numpy as np
sys.path.insert(0, sys.argv[1])
vals = {}
from confild_amd import synth
from confild_amd.script_util import create_model
from confild_amd.nf_networks import SIRENAutodecoder_film
out = {}
def h(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
DERIV_ONLY = len(sys.argv) > 3 and sys.argv[3] == "deriv"
def emit():
    np.savez(sys.argv[2], **{k.replace("/", "|"): v for k, v in vals.items()})
    print(json.dumps(out))
# The SIREN derivative kernels, 77 points and 2 latent rows, each network the smallest
# that reaches a distinct instantiation; every case with both normalisers and with neither.
from confild_amd.normalize import Normalizer_ts
def siren(dims):
    nf = SIRENAutodecoder_film(*dims)
    nf.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(5, *dims).items()})
    return nf.to("cuda")
def normalisers(dims, N, tag):
    d, c = dims[0], dims[2]
    xn = Normalizer_ts(params=(torch.from_numpy(synth.uniform(6, tag + "/xmax", (1, d), 1.5, 2.0)),
                               torch.from_numpy(synth.uniform(6, tag + "/xmin", (1, d), -0.5, -0.2))), method="-11", dim=0)
    yn = Normalizer_ts(params=(torch.from_numpy(synth.uniform(6, tag + "/ymax", (1, N, c), 0.5, 2.0)),
                               torch.from_numpy(synth.uniform(6, tag + "/ymin", (1, N, c), -2.0, -0.5))), method="-11", dim=0)
    return {"norm": (xn, yn), "raw": (None, None)}
F32 = ((1, 8, 1, 2, 16), (2, 8, 2, 3, 48), (3, 8, 3, 2, 512), (3, 64, 3, 15, 384))
SPLIT = ((1, 8, 1, 1, 32), (2, 8, 4, 1, 32), (2, 128, 2, 17, 256), (3, 64, 3, 15, 384))
for dims in sorted(set(F32 + SPLIT)):
    nf = siren(dims)
    g = torch.Generator().manual_seed(3)
    coords = torch.rand(77, dims[0], generator=g).cuda()
    lat = (torch.randn(2, 1, dims[1], generator=g) * 0.5).cuda()
    for nk, (xn, yn) in normalisers(dims, 77, "ld/deriv").items():
        if dims in F32:   # K13
            o, j = nf.decode_jacobian(coords, lat, xn, yn)
            out[f"deriv/jacobian/{dims}/{nk}"] = h(o) + h(j)
        if dims in F32 or dims == (2, 128, 2, 17, 256):   # K14: full and diagonal form
            for diag in (False, True):
                o, j, hs = nf.decode_hessian(coords, lat, xn, yn, diag=diag)
                out[f"deriv/hessian/{dims}/{'diag' if diag else 'full'}/{nk}"] = h(o) + h(j) + h(hs)
        if dims in SPLIT:   # K13s, K14s
            o, j = nf.decode_jacobian(coords, lat, xn, yn, compute="split_f16")
            out[f"deriv/jacobian_split/{dims}/{nk}"] = h(o) + h(j)
            for diag in (False, True):
                o, j, hs = nf.decode_hessian(coords, lat, xn, yn, diag=diag, compute="split_f16")
                out[f"deriv/hessian_split/{dims}/{'diag' if diag else 'full'}/{nk}"] = h(o) + h(j) + h(hs)
    if dims in F32:   # K15: 5 sensors, 3 rows
        sens = torch.rand(5, dims[0], generator=g).cuda()
        rows = (torch.randn(3, dims[1], generator=g) * 0.5).cuda()
        for nk, (xn, yn) in normalisers(dims, 5, "ld/jvjp").items():
            o, j = nf.jac_tape_forward(sens, rows, xn, yn)
            gz = nf.jac_tape_vjp(torch.randn(o.shape, generator=g).cuda(), torch.randn(j.shape, generator=g).cuda())
            out[f"deriv/jvjp/{dims}/{nk}"] = h(o) + h(j) + h(gz)
# K16: two 64-point slabs with a short last one (the shapes of tests/test_gpu_siren_jdense.py);
# the first has no hidden layer, so the second adds the weight ring
for dims, N, R, T in (((3, 16, 1, 0, 64), 65, 2, 1), ((2, 128, 2, 2, 256), 70, 3, 3)):
    nf = siren(dims)
    d, c = dims[0], dims[2]
    g = torch.Generator().manual_seed(4)
    coords = torch.rand(N, d, generator=g).cuda()
    lat = (torch.randn(R, dims[1], generator=g) * 0.5).cuda()
    y, wv, wj = torch.randn(T, N, 3, generator=g).cuda(), torch.randn(N, 3, c, generator=g).cuda(), (torch.randn(3, c, d, generator=g) * 0.3).cuda()
    for nk, (xn, yn) in normalisers(dims, N, "ld/jdense").items():
        gz, norms = nf.jac_dense_grad(coords, lat, T, y, wv, wj, None, xn, yn)
        out[f"deriv/jdense/{dims}/N{N}/{nk}"] = h(gz) + h(norms)
if DERIV_ONLY:
    emit()
    sys.exit(0)
cases = [(16, "2", "split_f16", (3,)), (32, "3", "split_f16", (1,)), (32, "1,2,3,4", "split_f16", (1, 3)), (64, "", "split_f16", (1, 2, 8)), (128, "", "bf16", (2,)),
         (64, "", "fp32", (2,)), (128, "", "split_f16", (1,)), (384, "1,1,2,2,4,4", "split_f16", (1,))]
for S, mult, comp, Bs in cases:
    m = create_model(image_size=S, num_channels=128, num_res_blocks=2, channel_mult=mult, num_heads=4,
                     num_head_channels=64, attention_resolutions="32,16,8")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in
                       synth.unet_state_dict(7, {k: tuple(v.shape) for k, v in m.state_dict().items()}).items()})
    m.to("cuda").set_compute(comp)
    for pb in ((0, 1, 2) if S == 64 else (0,)):
        m.set_plan_batch(pb)
        for B in Bs:
            x = torch.from_numpy(synth.normal(3, f"ld/x{S}", (B, 1, S, S))).cuda()
            t = torch.tensor([999, 500, 3, 250, 700, 10, 900, 60][:B], dtype=torch.int64).cuda()
            # "up/": the forward runs split-f16 Upsample convolutions
            # "k1h/": no Upsample convolution, but 3x3 convolutions on K1h's halo tiles
            # (128 or more output channels and an image that 256-pixel blocks of 16 or
            # more columns tile: plan_conv's K1h condition; else the case must be identical)
            k1h = 128 * min(m.channel_mult) >= 128 and S % 16 == 0
            up = "" if comp != "split_f16" else "up/" if len(m.channel_mult) > 1 else "k1h/" if k1h else ""
            tag = f"{S}/{mult or 'default'}/{comp}/pb{pb}/B{B}"
            eps = m(x, t)
            out[f"{up}fwd/{tag}"] = h(eps)
            if up and S <= 128:
                vals[f"{up}fwd/{tag}"] = eps.cpu().numpy()
            if comp != "bf16" and S <= 128:
                m.forward_tape(x, t)
                d = torch.from_numpy(synth.normal(4, f"ld/d{S}", (B, 1, S, S))).cuda()
                g = m.input_vjp(d)
                out[f"{up}vjp/{tag}"] = h(g)
                if up:
                    vals[f"{up}vjp/{tag}"] = g.cpu().numpy()
                if S <= 64 and B <= 2:
                    m.forward_tape(x, t, for_param_grad=True)
                    out[f"{up}pgrad/{tag}"] = h(m.param_grad(d))
    m.set_plan_batch(0)
for dims in ((3, 64, 3, 15, 384), (2, 32, 3, 10, 128), (2, 128, 2, 17, 256), (3, 48, 3, 5, 96)):
    nf = SIRENAutodecoder_film(*dims)
    nf.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(5, *dims).items()})
    nf.to("cuda")
    g = torch.Generator().manual_seed(1)
    coords = torch.rand(20000, dims[0], generator=g).cuda()
    lat = (torch.randn(6, 1, dims[1], generator=g) * 0.5).cuda()
    out[f"siren/{dims}"] = h(nf(coords, lat))
# the ring shapes of tests/test_gpu_siren_ring.py: fewer blocks than ring slots, the
# ring wrapping over layer boundaries, config E; a short last tile (385 points)
for dims in ((3, 8, 3, 1, 64), (3, 16, 3, 1, 128), (2, 16, 2, 1, 256), (3, 16, 3, 1, 384), (2, 8, 2, 2, 64),
             (2, 16, 4, 3, 128), (3, 16, 3, 2, 256), (3, 64, 3, 15, 384), (2, 128, 2, 17, 256)):
    nf = SIRENAutodecoder_film(*dims)
    nf.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(5, *dims).items()})
    nf.to("cuda")
    g = torch.Generator().manual_seed(2)
    coords = torch.rand(385, dims[0], generator=g).cuda()
    lat = (torch.randn(3, 1, dims[1], generator=g) * 0.5).cuda()
    out[f"siren_ring/{dims}"] = h(nf(coords, lat))
# one Upsample convolution on its own (builds that have the entry point)
from confild_amd import _lib
import ctypes as C
if hasattr(_lib.lib(), "cfd_upsample_conv"):
    for (B, H, W, Ci, Co) in ((8, 8, 8, 512, 512), (8, 16, 16, 384, 384), (2, 32, 32, 256, 256), (3, 4, 4, 96, 96)):
        x = torch.from_numpy(synth.normal(5, f"ld/ux{H}", (B, H, W, Ci))).cuda()
        w = torch.from_numpy(synth.normal(5, f"ld/uw{H}", (Co, Ci, 3, 3))) * 0.05
        b = torch.from_numpy(synth.normal(5, f"ld/ub{H}", (Co,)))
        o = torch.empty((B, 2 * H, 2 * W, Co), device="cuda")
        kx = C.c_int(0)
        _lib.check(_lib.lib().cfd_upsample_conv(_lib.ptr(x), C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()),
                                                _lib.ptr(o), B, H, W, Ci, Co, 0, 0, C.byref(kx), None), "upconv")
        out[f"up/conv/{B}x{H}x{W}x{Ci}"] = h(o)
        vals[f"up/conv/{B}x{H}x{W}x{Ci}"] = o.cpu().numpy()
emit()
"""


def run(lib, tmp, only):
    env = dict(os.environ, CFD_LIB=lib)
    vals = os.path.join(tmp, os.path.basename(lib) + ".npz")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, vals, only], capture_output=True, text=True, env=env,
                       timeout=900)
    if r.returncode != 0:
        print(r.stderr[-3000:])
        raise SystemExit(1)
    return json.loads(r.stdout.strip().splitlines()[-1]), vals


if __name__ == "__main__":
    import tempfile

    import numpy as np

    a, b = sys.argv[1], sys.argv[2]
    only = "deriv" if "--deriv" in sys.argv[3:] else "all"
    with tempfile.TemporaryDirectory() as tmp:
        (ra, va), (rb, vb) = run(a, tmp, only), run(b, tmp, only)
        both = [k for k in ra if k in rb]
        diff = [k for k in both if ra[k] != rb[k]]
        za, zb = np.load(va), np.load(vb)
        rel = {}
        for k in diff:
            f = k.replace("/", "|")
            if k.startswith(ROUNDING) and f in za.files and f in zb.files:
                rel[k] = float(np.abs(za[f].astype(np.float64) - zb[f]).max() / np.abs(za[f]).max())
    bad = [k for k in diff if not k.startswith(ROUNDING)]
    beyond = [k for k, v in rel.items() if not v <= UP_TOL]
    print(json.dumps({"a": a, "b": b, "cases": len(both), "deriv_cases": len([k for k in both if k.startswith("deriv/")]), "only_in_one": sorted(set(ra) ^ set(rb)),
                      "differ_upsample": {k: rel.get(k) for k in diff if k.startswith("up/")},
                      "differ_k1h": {k: rel.get(k) for k in diff if k.startswith("k1h/")},
                      "unbounded": [k for k in diff if k.startswith(ROUNDING) and k not in rel],
                      "up_tol": UP_TOL, "differ_upsample_beyond_tol": beyond, "differ_other": bad}))
    sys.exit(1 if bad or beyond else 0)
