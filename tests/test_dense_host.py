"""Host side of the dense / masked DPS operators (case2, case3, case3_gappy): no GPU.

* the CPU oracle's unchanged ``dps_step`` replays the reference's recorded masked
  runs (tests/golden/dps_dense_*.npz, make_golden_dps_dense.py) with
  ``operator = lambda x0: mask * case4_forward(...)``;
* the operator registry, constructor parameter names and the gappy mask table;
* ``_method_of`` collects the ``mask`` keyword of a partial chain and refuses others;
* the dense adjoint's planner stays within its budget and does not grow with N.
"""
import ast
import ctypes as C
import functools
import inspect

import numpy as np
import pytest
import torch

from conftest import golden
from confild_amd import _lib, synth
from oracle import diffusion as od
from oracle import dps as odps
from oracle import unet as ou

FIXTURES = ["dps_dense_case2", "dps_dense_case3gappy"]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_replays_masked_reference_run(name):
    g = golden(f"{name}.npz")
    kw = ast.literal_eval(str(g["kwargs"]))
    cfg = ou.Config(**kw)
    sd = {k: torch.from_numpy(v) for k, v in synth.unet_state_dict(int(g["seed"]), ou.param_shapes(cfg)).items()}
    d, L, c, nh, H = (int(v) for v in g["siren_dims"])
    ssd = {k: torch.from_numpy(v) for k, v in synth.siren_state_dict(int(g["siren_seed"]), d, L, c, nh, H).items()}
    tb = od.Tables(1000, "cosine", str(g["respacing"]))
    T = lambda k: torch.from_numpy(g[k])  # noqa: E731
    mask = T("mask")
    assert mask.shape == ((16, 37, 4) if name == "dps_dense_case2" else (17, 2))
    assert set(np.unique(g["mask"])) == {0.0, 1.0}
    operator = lambda x0: mask * odps.case4_forward(ssd, T("coords"), T("xhi"), T("xlo"), T("yhi"), T("ylo"),  # noqa: E731
                                                    T("vmax"), T("vmin"), x0, batch=int(g["op_batch"]))
    unet = lambda x, t: ou.forward(sd, cfg, x, t)  # noqa: E731
    assert np.array_equal(tb.timestep_map, g["timestep_map"])
    with torch.no_grad():
        assert np.array_equal(operator(T("x_true")).numpy(), g["measurement"])
    _, traj = odps.dps_loop(tb, unet, operator, T("x_start"), T("measurement"), T("step_noise"), float(g["scale"]))
    assert len(traj) == len(g["img"]) == 6
    for k, (img, x0, sample, norm) in enumerate(traj):
        assert np.array_equal(x0.numpy(), g["x0"][k]), k
        assert np.array_equal(sample.numpy(), g["sample"][k]), k
        assert np.array_equal(img.numpy(), g["img"][k]), k
        assert float(norm) == np.float32(g["dist"][k]), k
    assert np.array_equal(traj[-1][0].numpy(), g["out"])


def test_operators_are_registered_with_the_reference_parameters():
    from confild_amd.guided import measurements as ms
    want = {
        "case2": ["device", "ckpt_path", "max_val", "min_val", "coords", "batch_size"],
        "case3": ["device", "coords", "batch_size", "max_val", "min_val", "normalizer_params_path", "ckpt_path"],
        "case3_gappy": ["device", "coords", "batch_size", "max_val", "min_val", "normalizer_params_path",
                        "ckpt_path"],
        "case4": ["device", "coords_path", "batch_size", "max_val_path", "min_val_path", "normalizer_params_path",
                  "ckpt_path"],
    }
    classes = {"case2": ms.Case2Operator, "case3": ms.Case3Operator, "case3_gappy": ms.Case3Operator_gappy,
               "case4": ms.Case4Operator}
    for name, params in want.items():
        cls = ms.__OPERATOR__[name]
        assert cls is classes[name]
        assert list(inspect.signature(cls.__init__).parameters)[1:] == params, name
        assert callable(getattr(cls, "from_parts"))
    with pytest.raises(NameError):
        ms.get_operator("case5")
    # get_operator resolves the names: the constructors run up to their first file read
    for name in ("case3", "case3_gappy"):
        with pytest.raises(FileNotFoundError):
            ms.get_operator(name, device="cpu", coords=np.zeros((3, 2), np.float32), batch_size=4,
                            max_val=np.ones(4, np.float32), min_val=-np.ones(4, np.float32),
                            normalizer_params_path="/nonexistent/params.pt", ckpt_path="/nonexistent/ckpt.pt")
    with pytest.raises(FileNotFoundError):
        ms.get_operator("case2", device="cpu", ckpt_path="/nonexistent/ckpt.pt", max_val=np.ones(4, np.float32),
                        min_val=-np.ones(4, np.float32), coords=np.zeros((3, 2), np.float32), batch_size=4)


def test_case2_constants_and_gappy_mask_table():
    from confild_amd.guided import measurements as ms
    from confild_amd.nf_networks import SIRENAutodecoder_film
    from confild_amd.normalize import Normalizer_ts
    src = inspect.getsource(ms.Case2Operator.__init__)
    for lit in ("[1., 1.]", "[0., 0.]", "[[0.9617, 0.2666, 0.2869, 0.0290]]", "[[-0.0051, -0.2073, -0.2619, -0.0419]]"):
        assert lit in src, lit
    nf = SIRENAutodecoder_film(2, 16, 2, 2, 32)
    xn = Normalizer_ts(params=(torch.ones(1, 2), torch.zeros(1, 2)), method="-11", dim=0)
    yn = Normalizer_ts(params=(torch.ones(2), -torch.ones(2)), method="-11", dim=0)
    op = ms.Case3Operator_gappy.from_parts("cpu", np.zeros((17, 2), np.float32), xn, yn, nf, np.ones(16, np.float32),
                                           -np.ones(16, np.float32))
    m = op.default_mask()
    assert m.shape == (17, 2)
    want = np.ones((17, 2), np.float32)
    want[:10, 1] = 0.
    want[10:, 0] = 0.
    assert np.array_equal(m.numpy(), want)
    assert ms.Case3Operator.from_parts("cpu", np.zeros((17, 2), np.float32), xn, yn, nf, np.ones(16, np.float32),
                                       -np.ones(16, np.float32)).default_mask() is None


def test_method_of_collects_the_mask_keyword():
    from confild_amd.guided.condition_methods import get_conditioning_method
    from confild_amd.guided.gaussian_diffusion import _method_of
    from confild_amd.guided.measurements import get_noise
    cond = get_conditioning_method(operator=object(), noiser=get_noise(sigma=0.0, name="gaussian"), name="ps",
                                   scale=2.0)
    mask, other = torch.ones(3), torch.zeros(3)
    method, kw = _method_of(functools.partial(cond.conditioning))
    assert method is cond and kw == {}
    method, kw = _method_of(functools.partial(functools.partial(cond.conditioning, mask=mask)))
    assert method is cond and list(kw) == ["mask"] and kw["mask"] is mask
    # the outer partial's keyword wins, as it does when the partial is called
    inner = functools.partial(cond.conditioning, mask=other)
    _, kw = _method_of(functools.partial(inner, mask=mask))
    assert kw["mask"] is mask
    with pytest.raises(NotImplementedError, match="foo"):
        _method_of(functools.partial(cond.conditioning, foo=1))
    with pytest.raises(NotImplementedError, match="foo"):
        _method_of(functools.partial(functools.partial(cond.conditioning, foo=1), mask=mask))
    with pytest.raises(NotImplementedError):
        _method_of(lambda **k: None)


def _plan(cfg, N, R, budget, form=(0, 0)):
    """form: (backward 0 sum / 1 delta, compute 0 auto (K9t at this width) / 1 fp32)."""
    lib = _lib.load()
    b, pts, rows = C.c_size_t(), C.c_int64(), C.c_int()
    rc = lib.cfd_siren_dense_plan(C.byref(cfg), N, R, budget, form[0], form[1], C.byref(b), C.byref(pts),
                                  C.byref(rows))
    return rc, b.value, pts.value, rows.value


def test_dense_planner_is_bounded_by_the_budget_not_by_n():
    cfg = _lib.SirenCfg(2, 256, 4, 10, 256, 30.0)      # the Case2 widths
    GiB = 1 << 30
    for form in ((0, 0), (1, 0), (0, 1), (1, 1)):
        rc, b, pts, rows = _plan(cfg, 65536, 256, GiB, form)
        assert rc == 0 and 0 < b <= GiB and rows == 256 and pts >= 64 and pts % 64 == 0
        # the tape of the whole field would be 2 R N (nh+1) H floats = 378 GB
        assert 2 * 256 * 65536 * 11 * 256 * 4 > 300 * GiB
        rc2, b2, pts2, _ = _plan(cfg, 1 << 20, 256, GiB, form)
        assert rc2 == 0 and (b2, pts2) == (b, pts)              # does not grow with N
        rc3, b3, pts3, _ = _plan(cfg, 100, 256, GiB, form)
        assert rc3 == 0 and b3 <= b and pts3 == 128             # capped at N's own slabs
    # the default budget (0) is the library's 1 GiB
    assert _plan(cfg, 65536, 256, 0)[1:] == _plan(cfg, 65536, 256, GiB)[1:]
    # one slab of all rows does not fit: blocks of rows, one slab each
    rc, b, pts, rows = _plan(cfg, 65536, 2048, 256 << 20)
    assert rc == 0 and b <= 256 << 20 and pts == 64 and 1 <= rows < 2048
    # too small for one slab of one row: an argument error, with a message
    rc, *_ = _plan(cfg, 65536, 256, 1 << 20)
    assert rc == 1 and b"budget" in _lib.load().cfd_last_error()
