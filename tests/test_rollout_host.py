"""CPU tests of the conditioning-on-known-rows feature: the window plan of
confild_amd.rollout, the 'inpainting' operator (plain torch) and the
self-consistency of the reference-made fixtures.  No GPU calls."""
import inspect

import numpy as np
import pytest
import torch

from conftest import golden
from confild_amd.rollout import plan_windows
from confild_amd.script_util import create_gaussian_diffusion


def test_plan_windows_slices_and_coverage():
    T, ov, W = 16, 5, 2             # three windows: window 0 and two conditioned ones
    sl = plan_windows(T, ov, W)
    assert sl == [slice(0, 16), slice(11, 27), slice(22, 38)]
    total = T + W * (T - ov)
    assert sl[-1].stop == total == 38
    cover = np.zeros(total, dtype=np.int64)
    for s in sl:
        assert s.stop - s.start == T
        cover[s] += 1
    # every row once, apart from the overlaps (twice), which are the first `ov` rows of windows 1..W
    twice = np.zeros(total, dtype=bool)
    for s in sl[1:]:
        twice[s.start:s.start + ov] = True
    assert np.array_equal(cover, 1 + twice.astype(np.int64))
    assert plan_windows(16, 15, 2) == [slice(0, 16), slice(1, 17), slice(2, 18)]
    assert plan_windows(16, 5, 0) == [slice(0, 16)]


@pytest.mark.parametrize("T,ov,W", [(16, 0, 1), (16, 16, 1), (16, 17, 1), (16, -1, 1), (1, 1, 1), (16, 5, -1)])
def test_plan_windows_errors(T, ov, W):
    with pytest.raises(ValueError):
        plan_windows(T, ov, W)


def test_inpainting_operator_registered_and_values():
    from confild_amd.guided import measurements as ms
    cls = ms.__OPERATOR__["inpainting"]
    assert list(inspect.signature(cls.__init__).parameters)[1:] == ["device"]
    op = ms.get_operator("inpainting", device=torch.device("cpu"))
    assert isinstance(op, ms.LinearOperator)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 4, 6, generator=g)
    m = torch.zeros(1, 1, 4, 6)
    m[:, :, :2] = 1.0
    m[:, :, 3, ::3] = 0.5
    assert torch.equal(op.forward(x, mask=m), x * m)
    assert torch.equal(op.ortho_project(x, mask=m), x - x * m)
    assert op.transpose(x) is x
    with pytest.raises(ValueError, match="Require mask"):
        op.forward(x)
    with pytest.raises(ValueError, match="Require mask"):
        op.ortho_project(x)
    with pytest.raises(ValueError, match="Require mask"):
        op.forward(x, mask=None)
    # still not built: the reference's `project` cannot run on any of its own operators
    from confild_amd.guided.condition_methods import get_conditioning_method
    with pytest.raises(NotImplementedError):
        get_conditioning_method("projection", op, ms.get_noise("gaussian", sigma=0.0))


@pytest.mark.parametrize("name,sampler,steps,scale", [("dps_inpaint_rows", "ddpm", 8, 0.5),
                                                      ("dps_inpaint_frac", "ddim", 6, 3.0)])
def test_inpaint_fixture_is_self_consistent(name, sampler, steps, scale):
    g = golden(f"{name}.npz")
    assert str(g["sampler"]) == sampler and float(g["scale"]) == scale
    assert len(g["img"]) == len(g["x0"]) == len(g["sample"]) == len(g["dist"]) == len(g["step_noise"]) == steps
    m = g["mask"].astype(np.float64)
    assert m.shape == (1, 1, 16, 16)
    want = np.zeros((16, 16))
    want[:5] = 1.0
    if name.endswith("frac"):
        want[9, ::3] = 0.5
    assert np.array_equal(m[0, 0], want)
    y = g["measurement"].astype(np.float64)
    assert np.array_equal(g["measurement"], g["mask"] * g["x_true"])
    for k in range(steps):
        d = np.sqrt(((y - m * g["x0"][k].astype(np.float64)) ** 2).sum())
        assert abs(d - g["dist"][k]) <= 1e-5 * d, (k, d, g["dist"][k])
    assert np.array_equal(g["out"], g["img"][-1])
    d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing=str(g["respacing"]))
    assert np.array_equal(np.array(d.timestep_map), g["timestep_map"])


def test_known_table_levels():
    """(a_i, b_i) = (sqrt(abar_prev), sqrt(1 - abar_prev)): float64 tables cast to fp32;
    the last step (i = 0) carries the known rows themselves."""
    d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="8")
    tab = d.known_table()
    assert tab.shape == (8, 2) and tab.dtype == torch.float32
    assert tab[0, 0].item() == 1.0 and tab[0, 1].item() == 0.0
    assert torch.equal(tab[:, 0], torch.from_numpy(np.sqrt(d.alphas_cumprod_prev)).float())
    assert torch.equal(tab[:, 1], torch.from_numpy(np.sqrt(1.0 - d.alphas_cumprod_prev)).float())
    assert d.coef_table().shape == (8, 8)
