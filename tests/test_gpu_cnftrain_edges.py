"""GPU: the CNF training backward (K10, cfd_siren_train_grad through
SIRENAutodecoder_film.train_grad) at every kernel form it can take, against fp64
autograd through the CPU oracle (oracle/siren.py::forward), in both compute modes.

tests/test_gpu_cnftrain.py pins K10 to the reference's own run at one shape
((3, 16, 3, 3, 64), 1,200 pairs: siren_tape_*_ks<4, 4>, gemm_tn_kernel<., 64>).
The cases here run the forms a training run at other widths and pair counts takes:

* the tape: siren_tape_*<NB, 1 / 2 / 4>, siren_tape_*_ks<NB, 4> and K9t (the split-f16
  tape, split compute at H = 128 / 256 / 384 below 32,768 pairs) as the source of
  the weight gradients;
* gemm_tn_kernel<., 128> (M, N >= 128) and <., 64>, 128- and 64-tile edges, K tails
  that are no multiple of 16, K < 16, k-spans above 256, all 64 slices;
* mse_grad_kernel's grid-stride loop, colsum_part_kernel's direct write into D,
  its span above 256 and its 4-unrolled tail, nh = 0, d = 1 / 2, c = 1 / 2 / 4,
  L = 4 ... 128, unsorted and one-row batches.

Rule (DESIGN.md section 5, K13 / K14's with the same k = 4): per parameter tensor,
for the latent-table gradient and with e32 the CPU fp32 autograd's own error against
fp64 on the same inputs,
  f32 handle:    max|got - g64| <= 4 max(e32, 1e-7 max|g64|), loss 1e-5 relative;
  split handle:  max|got - g64| <= 2 x the f32 handle's error + 1e-7 max|g64|, and the
                 f32 handle's bits wherever the tape is not K9t.

The split rule is relative to the f32 handle, so a defect both handles share (the
weight-gradient products are fp32 in both) is the f32 test's to catch.

The rest: a repeat, accumulation into pre-filled sums (bit-exact), coordinate
chunks against the whole call; every refusal with the caller's sums untouched;
train_autodecoder at a K9t width with uneven chunks against a float64 restatement
of _single_trainer with torch.optim.Adam; the bounds-checked build.

Measured on an MI355X, the worst tensor per case: the f32 handle's error over
max(e32, 1e-7 max|g64|) (bound 4); the split handle's over 2 x the f32 handle's
error + 1e-7 max|g64| (bound 1; "bits": the f32 handle's bits, so 0.47 ... 0.49);
and the split handle's on the f32 handle's scale, over max(e32, 1e-7 max|g64|):

  case               f32     split   split / max(e32, floor)
  w4_h16_stride      2.39    bits    2.39
  w4_h128            1.57    bits    1.57
  k9t_h128_tail      1.36    0.60    1.60
  h192_edge          2.06    bits    2.06
  k9t_h384           1.25    0.82    1.39
  k9t_h256_L128      1.89    0.53    1.32
  nh0_h48            2.35    bits    2.35
  w2_h96             1.48    bits    1.48
  h512               2.14    bits    2.14
  k9t_h128_tail_r1   1.13    0.81    1.09
  nh0_h48_r1         1.67    bits    1.67
  chunks, k9t_h128_tail at 37:   f32 1.32, split 0.59 (1.60 on the f32 scale)
  chunks, w2_h96 at 1234:        f32 1.38, split 0.49 (1.38)

The loss was within 1.3e-7 relative in every case.  The loop: losses within 5.4e-7
(f32) / 6.8e-7 (split) relative; parameters at most 2.9e-5 / 3.5e-5 off, 0.006 % of
the elements beyond 1e-5 (cap 4e-4: first Adam steps of gradients within rounding
of zero); the table within 1.3e-6 / 1.6e-6.  No case needed a restated e32.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

from confild_amd import _lib, synth
from confild_amd.cnf_train import train_autodecoder
from confild_amd.nf_networks import SIRENAutodecoder_film
from oracle import siren as osn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_SO = os.path.join(ROOT, "confild_amd", "lib", "libconfild_hip_debug.so")

N_TABLE = 7          # latent-table rows; rows[i] = (3 i + 5) % 7 leaves some out
K_BOUND = 4.0
MODES = ("f32", "split_f16")

# id: (d, L, c, nh, H), R, N
CASES = {
    "w4_h16_stride": ((1, 4, 4, 1, 16), 3, 21847),
    "w4_h128": ((3, 16, 3, 2, 128), 4, 8193),
    "k9t_h128_tail": ((3, 16, 3, 2, 128), 3, 111),
    "h192_edge": ((2, 8, 2, 1, 192), 2, 45),
    "k9t_h384": ((3, 64, 3, 2, 384), 3, 50),
    "k9t_h256_L128": ((2, 128, 2, 1, 256), 6, 21),
    "nh0_h48": ((3, 12, 4, 0, 48), 5, 33),
    "w2_h96": ((2, 8, 3, 3, 96), 2, 4101),
    "h512": ((2, 4, 1, 1, 512), 2, 19),
}
# the one-row batches (rows = [6]) of two of them
ONE_ROW = {"k9t_h128_tail_r1": "k9t_h128_tail", "nh0_h48_r1": "nh0_h48"}
ALL = list(CASES) + list(ONE_ROW)


def _spec(name):
    """dims, rows, N of a case (or of its one-row batch)."""
    if name in ONE_ROW:
        dims, _, N = CASES[ONE_ROW[name]]
        return dims, [6], N
    dims, R, N = CASES[name]
    return dims, [(3 * i + 5) % N_TABLE for i in range(R)], N


def _is_k9t(name):
    """Whether a split-compute handle runs K9t on this case (include/confild.h)."""
    (d, L, c, nh, H), rows, N = _spec(name)
    return H in (128, 256, 384) and nh >= 1 and len(rows) * N < 32768


@functools.lru_cache(maxsize=None)
def _inputs(name):
    dims, rows, N = _spec(name)
    d, L, c, nh, H = dims
    seed, tag = 101 + ALL.index(name), "cnfedge/" + name
    sd = {k: torch.from_numpy(v) for k, v in synth.siren_state_dict(seed, *dims).items()}
    coords = torch.from_numpy(synth.uniform(seed, tag + "/x", (N, d), -1.0, 1.0))
    Z = torch.from_numpy(synth.normal(seed, tag + "/z", (N_TABLE, L))) * 0.5
    tgt = torch.from_numpy(synth.normal(seed, tag + "/y", (len(rows), N, c))) * 0.3
    return dims, rows, N, sd, coords, Z, tgt


def _autograd(sd, coords, Z, rows, tgt, dtype):
    """loss, {key: gradient}, table gradient of the MSE loss through the oracle in `dtype`."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    z = Z.to(dtype).clone().requires_grad_(True)
    out = osn.forward(p, coords.to(dtype)[None], z[rows][:, None])
    loss = ((out - tgt.to(dtype)) ** 2).mean()
    keys = sorted(p)
    gs = torch.autograd.grad(loss, [p[k] for k in keys] + [z])
    return float(loss.detach()), dict(zip(keys, gs[:-1])), gs[-1]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """fp64 loss and gradients ("latents": the table's), and e32 per tensor: the CPU
    fp32 evaluation's error against them.  Computed once per case, never modified."""
    dims, rows, N, sd, coords, Z, tgt = _inputs(name)
    loss64, g64, z64 = _autograd(sd, coords, Z, rows, tgt, torch.float64)
    _, g32, z32 = _autograd(sd, coords, Z, rows, tgt, torch.float32)
    g64["latents"], g32["latents"] = z64, z32
    e32 = {k: float((g32[k].double() - g64[k]).abs().max()) for k in g64}
    return loss64, g64, e32


_LAYOUT = {}   # case -> [(key, shape)] of the flat gradient, param_keys() order


def _net(name, mode):
    dims, rows, N, sd, coords, Z, tgt = _inputs(name)
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict(sd)
    net.to(DEV).set_compute(mode)
    named = dict(net.named_parameters())
    _LAYOUT[name] = [(k, tuple(named[k].shape)) for k in net.param_keys()]
    return net


def _run(name, mode, init=None, split_at=None):
    """grad, grad_latents, sse of one backward (or of two over coords[:k], coords[k:]),
    accumulated into zeros or into clones of `init`."""
    dims, rows, N, sd, coords, Z, tgt = _inputs(name)
    net = _net(name, mode)
    n_par = net.flat_params().numel()
    if init is None:
        grad = torch.zeros(n_par, device=DEV)
        gz = torch.zeros(N_TABLE, dims[1], device=DEV)
        sse = torch.zeros(1, device=DEV)
    else:
        grad, gz, sse = (t.clone() for t in init)
    scale = 2.0 / (len(rows) * N * dims[2])
    rows_t = torch.tensor(rows, dtype=torch.int64, device=DEV)
    cd, Zd, td = coords.to(DEV), Z.to(DEV).contiguous(), tgt.to(DEV)
    for a, b in ([(0, N)] if split_at is None else [(0, split_at), (split_at, N)]):
        net.train_grad(cd[a:b], Zd, rows_t, td[:, a:b], scale, grad, gz, sse)
    torch.cuda.synchronize()
    return grad, gz, sse


@functools.lru_cache(maxsize=None)
def _whole(name, mode):
    """The zero-initialised whole call, shared by the tests that compare against it."""
    return _run(name, mode)


def _errors(name, got):
    """{tensor: max|got - g64|} per parameter tensor (sliced out of the flat gradient in
    param_keys() order) and for the table gradient, and the loss's relative error."""
    dims, rows, N, sd, coords, Z, tgt = _inputs(name)
    loss64, g64, _ = _reference(name)
    grad, gz, sse = got
    layout = _LAYOUT[name]
    assert sorted(k for k, _ in layout) == sorted(sd)
    err, o = {}, 0
    gc = grad.cpu().double()
    for k, shape in layout:
        n = g64[k].numel()
        err[k] = float((gc[o:o + n].reshape(shape) - g64[k]).abs().max())
        o += n
    assert o == grad.numel()
    err["latents"] = float((gz.cpu().double() - g64["latents"]).abs().max())
    loss = float(sse) / (len(rows) * N * dims[2])
    return err, abs(loss - loss64) / loss64


def _check_rule(name, mode, got, f32_err, what):
    """Part 1's rule on `got`; f32_err: the f32 handle's errors on the same problem
    (the split handle's yardstick).  Prints the ratios, returns the errors."""
    loss64, g64, e32 = _reference(name)
    err, loss_rel = _errors(name, got)
    ratios = {}
    for k in err:
        gmax = float(g64[k].abs().max())
        assert gmax > 0, k                       # no reference tensor is identically zero
        floor = 1e-7 * gmax
        ratios[k] = err[k] / max(e32[k], floor) if mode == "f32" else err[k] / (2 * f32_err[k] + floor)
    rec = {"case": name, "mode": mode, "what": what, "k9t": mode != "f32" and _is_k9t(name),
           "worst": max(ratios.values()), "worst_tensor": max(ratios, key=ratios.get), "loss_rel": loss_rel,
           "bound": K_BOUND if mode == "f32" else 1.0, "ratios": {k: round(v, 3) for k, v in ratios.items()}}
    if mode != "f32":   # the split handle's error on the f32 handle's scale too
        rec["vs_e32"] = max(err[k] / max(e32[k], 1e-7 * float(g64[k].abs().max())) for k in err)
    print(json.dumps(rec))
    for k, r in ratios.items():
        assert r <= rec["bound"], (name, mode, what, k, r)
    assert loss_rel <= 1e-5, (name, mode, loss_rel)
    return err


def _rows_left_out(name):
    rows = _spec(name)[1]
    return [r for r in range(N_TABLE) if r not in rows]


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ALL)
def test_f32_gradients_against_fp64_autograd(hip, name):
    got = _whole(name, "f32")
    _check_rule(name, "f32", got, None, "whole")
    out = _rows_left_out(name)
    assert out and not got[1][out].any()         # table rows outside the batch stay exactly 0


@pytest.mark.parametrize("name", ALL)
def test_split_gradients_against_fp64_autograd(hip, name):
    f32 = _whole(name, "f32")
    got = _whole(name, "split_f16")
    f32_err, _ = _errors(name, f32)
    _check_rule(name, "split_f16", got, f32_err, "whole")
    assert not got[1][_rows_left_out(name)].any()
    if not _is_k9t(name):                        # the fp32 chain in both modes: the same bits
        assert all(torch.equal(a, b) for a, b in zip(got, f32)), name
    else:
        assert not torch.equal(got[0], f32[0]), name   # K9t did run


# --------------------------------------------------------------------------- 2
BIT_CASES = ("k9t_h128_tail", "w2_h96")
CHUNK_AT = {"k9t_h128_tail": 37, "w2_h96": 1234}   # no multiple of 16


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", BIT_CASES)
def test_repeat_and_accumulation_are_bit_exact(hip, name, mode):
    g, gz, sse = _whole(name, mode)
    again = _run(name, mode)
    assert all(torch.equal(a, b) for a, b in zip(again, (g, gz, sse)))
    tag = f"cnfedge/acc/{name}"
    g0 = torch.from_numpy(synth.normal(7, tag + "/g", tuple(g.shape))).to(DEV)
    z0 = torch.from_numpy(synth.normal(8, tag + "/z", tuple(gz.shape))).to(DEV)
    s0 = torch.from_numpy(synth.normal(9, tag + "/s", (1,))).to(DEV)
    g1, z1, s1 = _run(name, mode, init=(g0, z0, s0))
    # the kernels form G + s in fp32 with the s of the zero-initialised call
    assert torch.equal(g1, g0 + g) and torch.equal(z1, z0 + gz) and torch.equal(s1, s0 + sse)
    out = _rows_left_out(name)
    assert torch.equal(z1[out], z0[out])


@pytest.mark.parametrize("name", BIT_CASES)
def test_coordinate_chunks_add_up(hip, name):
    """coords[:k] and coords[k:] with the full-count scale: part 1's rule (the split
    handle against the f32 handle's error on the same two calls)."""
    k = CHUNK_AT[name]
    assert k % 16 != 0 and 0 < k < _spec(name)[2]
    f32 = _run(name, "f32", split_at=k)
    f32_err = _check_rule(name, "f32", f32, None, f"chunks at {k}")
    _check_rule(name, "split_f16", _run(name, "split_f16", split_at=k), f32_err, f"chunks at {k}")


# --------------------------------------------------------------------------- 3
def _abi_problem(dims, R=3, N=40):
    """Device arrays of a small problem, pre-filled sums, and the raw call."""
    d, L, c, nh, H = dims
    net = SIRENAutodecoder_film(*dims)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.siren_state_dict(77, *dims).items()})
    net.to(DEV)
    tag = "cnfedge/abi"
    coords = torch.from_numpy(synth.uniform(1, tag + "/x", (N, d), -1.0, 1.0)).to(DEV)
    Z = (torch.from_numpy(synth.normal(2, tag + "/z", (N_TABLE, L))) * 0.5).to(DEV)
    tgt = (torch.from_numpy(synth.normal(3, tag + "/y", (R, N, c))) * 0.3).to(DEV)
    rows = torch.tensor([5, 1, 4][:R], dtype=torch.int64, device=DEV)
    n_par = sum(p.numel() for p in net.parameters())
    sums = (torch.from_numpy(synth.normal(4, tag + "/g", (n_par,))).to(DEV),
            torch.from_numpy(synth.normal(5, tag + "/gz", (N_TABLE, L))).to(DEV),
            torch.from_numpy(synth.normal(6, tag + "/s", (1,))).to(DEV))
    h = net._handle(DEV)

    def call(ws_ptr, ws_bytes, n=N, r=R):
        return _lib.load().cfd_siren_train_grad(h, _lib.ptr(coords), n, _lib.ptr(Z), _lib.ptr(rows), r, _lib.ptr(tgt),
                                                2.0 / (R * N * c), _lib.ptr(sums[0]), _lib.ptr(sums[1]),
                                                _lib.ptr(sums[2]), C.c_void_p(ws_ptr), ws_bytes,
                                                _lib.stream_of(DEV))
    return net, h, call, sums, (coords, Z, rows, tgt)


def _untouched(sums, before):
    torch.cuda.synchronize()
    return all(torch.equal(a, b) for a, b in zip(sums, before))


def test_unsupported_latent_width_is_a_shape_error(hip):
    net, h, call, sums, _ = _abi_problem((3, 6, 3, 1, 64))
    before = tuple(t.clone() for t in sums)
    n = C.c_size_t(12345)
    assert hip.cfd_siren_train_workspace_bytes(h, 40, 3, C.byref(n)) == 4      # CFD_ESHAPE
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    assert call(ws.data_ptr(), ws.numel()) == 4
    assert _untouched(sums, before)


def test_bad_workspace_and_counts_are_refused_before_any_launch(hip):
    net, h, call, sums, _ = _abi_problem((3, 16, 3, 2, 128))
    before = tuple(t.clone() for t in sums)
    n = C.c_size_t()
    assert hip.cfd_siren_train_workspace_bytes(h, 40, 3, C.byref(n)) == 0 and n.value > 0
    ws = torch.zeros(n.value + 16, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    assert call(ws.data_ptr(), n.value - 1) == 1                # CFD_EARG: one byte short
    assert call(ws.data_ptr() + 4, n.value) == 1                # 4 bytes off 16-byte alignment
    assert call(ws.data_ptr(), n.value, n=(1 << 20) + 1) == 1   # the count alone: no array is that long
    assert call(ws.data_ptr(), n.value, r=0) == 1
    assert _untouched(sums, before)
    assert call(ws.data_ptr(), n.value) == 0                    # and the same arguments, whole, run
    torch.cuda.synchronize()
    assert not torch.equal(sums[0], before[0]) and not torch.equal(sums[2], before[2])


def test_driver_refuses_duplicate_rows_and_cpu_tables(hip):
    net, h, call, sums, (coords, Z, rows, tgt) = _abi_problem((3, 16, 3, 2, 128))
    before = tuple(t.clone() for t in sums)
    with pytest.raises(ValueError):
        net.train_grad(coords, Z, torch.tensor([5, 1, 5], device=DEV), tgt, 1e-3, *sums)
    with pytest.raises(_lib.CfdError):
        net.train_grad(coords, Z.cpu(), rows, tgt, 1e-3, *sums)
    assert _untouched(sums, before)


# --------------------------------------------------------------------------- 4
LOOP = dict(dims=(3, 16, 3, 2, 128), samples=5, N=203, batch=2, epochs=3, lr_nf=1e-4, lr_lat=1e-3, chunk=150)


@functools.lru_cache(maxsize=None)
def _loop_problem():
    d, L, c, nh, H = LOOP["dims"]
    sd = {k: torch.from_numpy(v) for k, v in synth.siren_state_dict(55, *LOOP["dims"]).items()}
    coords = torch.from_numpy(synth.uniform(56, "cnfedge/loop/x", (LOOP["N"], d), -1.0, 1.0))
    Z = torch.from_numpy(synth.normal(57, "cnfedge/loop/z", (LOOP["samples"], L))) * 0.5
    fois = torch.from_numpy(synth.normal(58, "cnfedge/loop/y", (LOOP["samples"], LOOP["N"], c))) * 0.3
    return sd, coords, Z, fois


@functools.lru_cache(maxsize=None)
def _loop_reference():
    """_single_trainer's order in float64 with torch.optim.Adam: the net steps at the
    start of every epoch but the first, on the gradient accumulated over the previous
    epoch's batches; the latent table steps after every batch."""
    sd, coords, Z, fois = _loop_problem()
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    z = Z.double().clone().requires_grad_(True)
    opt_net = torch.optim.Adam(list(p.values()), lr=LOOP["lr_nf"])
    opt_lat = torch.optim.Adam([z], lr=LOOP["lr_lat"])
    idxs = [list(range(s, min(s + LOOP["batch"], LOOP["samples"]))) for s in range(0, LOOP["samples"], LOOP["batch"])]
    losses = []
    for ep in range(LOOP["epochs"]):
        if ep != 0:
            opt_net.step()
            opt_net.zero_grad()
        for idx in idxs:
            opt_lat.zero_grad()
            loss = ((osn.forward(p, coords.double()[None], z[idx][:, None]) - fois[idx].double()) ** 2).mean()
            loss.backward()
            opt_lat.step()
            losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in p.items()}, z.detach()


@pytest.mark.parametrize("mode", MODES)
def test_training_loop_at_a_k9t_width_with_uneven_chunks(hip, mode):
    sd, coords, Z0, fois = _loop_problem()
    ref_losses, ref_p, ref_z = _loop_reference()
    net = SIRENAutodecoder_film(*LOOP["dims"])
    net.load_state_dict(sd)
    net.to(DEV).set_compute(mode)
    Z = Z0.to(DEV).contiguous()
    # 75 coordinates per call at R = 2, 150 at R = 1: every batch ends on a chunk of 53
    assert LOOP["N"] % (LOOP["chunk"] // 2) == 53 and LOOP["N"] % LOOP["chunk"] == 53
    losses = []
    train_autodecoder(net, Z, coords, fois, LOOP["epochs"], LOOP["batch"],
                      {"nf": LOOP["lr_nf"], "latents": LOOP["lr_lat"]}, shuffle=False, coord_chunk=LOOP["chunk"],
                      on_batch=lambda i, idx, loss: losses.append(loss))
    torch.cuda.synchronize()
    assert len(losses) == len(ref_losses) == 9
    rel = max(abs(a - b) / b for a, b in zip(losses, ref_losses))
    n_net_steps, n_lat_steps = LOOP["epochs"] - 1, len(losses)
    worst, frac = 0.0, 0.0
    for k, p in net.named_parameters():
        dlt = (p.detach().cpu().double() - ref_p[k]).abs()
        worst, frac = max(worst, float(dlt.max())), max(frac, float((dlt > 1e-5).double().mean()))
        assert float((dlt > 1e-5).double().mean()) <= 1e-3 and float(dlt.max()) <= 2 * LOOP["lr_nf"] * n_net_steps, k
    dz = (Z.cpu().double() - ref_z).abs()
    print(json.dumps({"loop": mode, "loss_rel": rel, "param_max": worst, "param_frac_gt_1e-5": frac,
                      "latent_max": float(dz.max()), "latent_frac_gt_1e-5": float((dz > 1e-5).double().mean())}))
    assert rel <= 1e-5
    assert float((dz > 1e-5).double().mean()) <= 1e-3 and float(dz.max()) <= 2 * LOOP["lr_lat"] * n_lat_steps


# --------------------------------------------------------------------------- 5
DEBUG_CASES = ("k9t_h128_tail", "nh0_h48", "h192_edge")


def _bits(ts):
    return [hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for t in ts]


def _debug_bits():
    return {f"{name}-{mode}": _bits(_whole(name, mode)) for name in DEBUG_CASES for mode in MODES}


def _child_main():
    print(json.dumps(_debug_bits()))


def test_bounds_checked_build_gives_the_same_bits(hip):
    """The debug library (device-side CFD_DASSERT checks live), loaded with CFD_LIB in a
    child process: K9t and the fp32 tapes feeding both gemm_tn tiles; same bits as
    the shipped library, no device assertion."""
    if not os.path.exists(DEBUG_SO):
        pytest.skip("debug build absent (make -C confild_amd/csrc DEBUG=1)")
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; "
            "import test_gpu_cnftrain_edges as t; t._child_main()")
    env = dict(os.environ, CFD_LIB="libconfild_hip_debug.so")
    r = subprocess.run([sys.executable, "-c", code, ROOT, os.path.join(ROOT, "tests")], capture_output=True,
                       text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == _debug_bits()
