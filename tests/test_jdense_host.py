"""CPU: the host side of the dense derivative measurements (K16): the workspace
planner cfd_siren_jdense_plan (no device needed) and the 'dense_stencil' operator's
registry entry, constructor and weight checks."""
import ctypes as C
import inspect

import pytest
import torch

from confild_amd import _lib
from confild_amd.guided import measurements as ms
from confild_amd.nf_networks import SIRENAutodecoder_film

GiB = 1 << 30


def _plan(cfg, N, R, M, budget):
    b, pts, rows = C.c_size_t(), C.c_int64(), C.c_int()
    rc = _lib.load().cfd_siren_jdense_plan(C.byref(cfg), N, R, M, budget, C.byref(b), C.byref(pts), C.byref(rows))
    return rc, b.value, pts.value, rows.value


def test_planner_is_bounded_by_the_budget_not_by_n():
    cfg = _lib.SirenCfg(2, 256, 4, 10, 256, 30.0)      # the Case2 widths
    R = 64
    rc, b, pts, rows = _plan(cfg, 16384, R, 1, GiB)
    assert rc == 0 and 0 < b <= GiB and rows == R and pts > 64 and pts % 64 == 0
    # K15's whole tape would be (2 + d) R N (nh+1) H floats = 47 GB (189 GB at 256 rows)
    assert 4 * R * 16384 * 11 * 256 * 4 > 40 * GiB
    rc2, b2, pts2, rows2 = _plan(cfg, 1 << 20, R, 1, GiB)
    assert rc2 == 0 and (b2, pts2, rows2) == (b, pts, rows)      # does not grow with N
    rc3, b3, pts3, _ = _plan(cfg, 100, R, 3, GiB)
    assert rc3 == 0 and b3 <= b and pts3 == 128                  # capped at N's own slabs
    assert _plan(cfg, 16384, R, 1, 0) == (0, b, pts, rows)       # budget 0: the library's 1 GiB
    # a larger budget plans a larger chunk, a smaller one a smaller chunk, each within itself
    for budget in (GiB // 4, 4 * GiB):
        rcb, bb, ptsb, rowsb = _plan(cfg, 1 << 20, R, 1, budget)
        assert rcb == 0 and bb <= budget and ptsb % 64 == 0 and rowsb == R
        assert (ptsb > pts) == (budget > GiB) and ptsb != pts


def test_planner_blocks_rows_when_one_slab_of_all_rows_does_not_fit():
    cfg = _lib.SirenCfg(2, 256, 4, 10, 256, 30.0)
    # one slab of one row: 64 points x 3 x 11 x 256 floats of tape = 2.2 MB
    budget = 64 * GiB // 1024                                     # 64 MiB
    rc, b, pts, rows = _plan(cfg, 16384, 256, 2, budget)
    assert rc == 0 and b <= budget and pts == 64 and 1 <= rows < 256
    rc1, b1, pts1, rows1 = _plan(cfg, 16384, 256, 2, budget // 2)
    assert rc1 == 0 and b1 <= budget // 2 and pts1 == 64 and rows1 <= rows


def test_planner_errors():
    cfg = _lib.SirenCfg(2, 256, 4, 10, 256, 30.0)
    rc, *_ = _plan(cfg, 16384, 256, 1, 1 << 20)                  # below one slab of one row
    assert rc == 1 and b"too small" in _lib.load().cfd_last_error()
    assert _plan(cfg, 16384, 256, 0, GiB)[0] == 1                # M < 1
    assert _plan(cfg, 0, 256, 1, GiB)[0] == 1
    assert _plan(cfg, 16384, 0, 1, GiB)[0] == 1
    cfg4 = _lib.SirenCfg(4, 256, 4, 10, 256, 30.0)               # d > 3
    assert _plan(cfg4, 16384, 256, 1, GiB)[0] == 1 and b"in_coord_features" in _lib.load().cfd_last_error()


@pytest.mark.parametrize("dims,tile", [((1, 8, 1, 2, 16), 64), ((2, 8, 2, 3, 48), 32), ((3, 8, 3, 2, 512), 16),
                                       ((1, 8, 1, 2, 512), 32)])
def test_planner_counts_the_tile_partials(dims, tile):
    """The tile partials are (64 / tile) (nh+1) H floats per (row, slab): more of them
    in the forms with smaller tiles, within the same budget."""
    d, L, c, nh, H = dims
    cfg = _lib.SirenCfg(d, L, c, nh, H, 30.0)
    rc, b, pts, rows = _plan(cfg, 640, 4, 1, 1 << 26)
    assert rc == 0 and pts == 640 and rows == 4
    nf = (nh + 1) * H
    slab_sums = 10 * nf if tile < 64 else 0                      # a 64-pair tile's partial is the slab's
    need = 4 * (640 * (1 + d) * nf + 10 * (64 // tile) * nf + slab_sums + 640 * c * (1 + d))
    assert 4 * need <= b <= 4 * need + (1 << 16)                 # plus the fixed part and padding


def test_operator_is_registered_with_the_sensor_stencil_constructor():
    assert ms.__OPERATOR__["dense_stencil"] is ms.DenseStencilOperator
    assert not issubclass(ms.DenseStencilOperator, ms.SensorStencilOperator)   # the sampler's K15 branch must not catch it
    want = list(inspect.signature(ms.SensorStencilOperator.__init__).parameters)
    assert list(inspect.signature(ms.DenseStencilOperator.__init__).parameters) == want
    assert want[-2:] == ["value_weights", "jac_weights"]
    fp = list(inspect.signature(ms.DenseStencilOperator.from_parts).parameters)
    assert fp == list(inspect.signature(ms.SensorStencilOperator.from_parts).parameters)
    assert hasattr(ms.DenseStencilOperator, "dense_grad")
    assert not hasattr(ms.DenseStencilOperator, "forward_tape") and not hasattr(ms.DenseStencilOperator, "vjp")
    assert "mask" in inspect.signature(ms.DenseStencilOperator.forward).parameters


def test_operator_weight_shape_errors():
    d, L, c, nh, H = 2, 8, 3, 1, 32
    net = SIRENAutodecoder_film(d, L, c, nh, H)
    N = 7
    coords = torch.rand(N, d)

    def make(**kw):
        return ms.DenseStencilOperator.from_parts("cpu", coords, None, None, net, torch.ones(L), -torch.ones(L), **kw)

    with pytest.raises(ValueError, match="needs value_weights"):
        make()
    op = make(value_weights=torch.ones(2, c), jac_weights=torch.ones(N, 2, c, d))      # shared and per point
    assert op.readings == 2 and not op.wv_per_sensor and op.wj_per_sensor
    assert make(jac_weights=torch.ones(5, c, d)).readings == 5
    with pytest.raises(ValueError, match="neither"):
        make(value_weights=torch.ones(2, c + 1))
    with pytest.raises(ValueError, match="neither"):
        make(jac_weights=torch.ones(2, c, d + 1))
    with pytest.raises(ValueError, match="neither"):
        make(value_weights=torch.ones(N + 1, 2, c))                                   # per point, wrong N
    with pytest.raises(ValueError, match="readings"):
        make(value_weights=torch.ones(2, c), jac_weights=torch.ones(3, c, d))
    with pytest.raises(ValueError, match="readings"):
        make(value_weights=torch.ones(0, c))
    with pytest.raises(_lib.CfdError):                                                # no CPU path
        op.dense_grad(torch.zeros(1, 1, 2, L), torch.zeros(2, N, 2))
