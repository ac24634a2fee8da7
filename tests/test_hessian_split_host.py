"""CPU: the width rule of the split-f16 Hessian as Python states it
(nf_networks.hessian_split_supported), the driver's `derived_hessian_compute` key, which
is checked against the CNF case file before anything is loaded, and the keys of the
PDE-residual `derived` names."""
import pytest
import yaml

from confild_amd import inference
from confild_amd.nf_networks import (HESSIAN_COMPUTE, JACOBIAN_SPLIT_WIDTHS, hessian_split_refusal,
                                     hessian_split_supported)
from confild_amd.read_input import basic_input


def test_width_rule():
    assert HESSIAN_COMPUTE == ("f32", "split_f16")
    for H in range(16, 513, 16):
        for d in (1, 2, 3):
            assert hessian_split_supported(d, 2, H) == (H in JACOBIAN_SPLIT_WIDTHS), (d, H)
    assert hessian_split_supported(3, 15, 384) and hessian_split_supported(2, 17, 256)
    for (d, nh, H), reason in (((2, 2, 48), "multiple of 32"), ((2, 2, 512), "512"), ((2, 2, 160), "160"),
                               ((2, 0, 64), "num_hidden_layers"), ((4, 1, 32), "in_coord_features"),
                               ((0, 1, 32), "in_coord_features")):
        assert not hessian_split_supported(d, nh, H)
        assert reason in hessian_split_refusal(d, nh, H), (d, nh, H)
    # LDS staging: 2 blocks of H x 16 weights (hi + lo f16) + (nh + 1) FiLM rows + the first layer, 160 KiB
    lds = lambda nh, H: 4 * (2 * (H // 16) * 256 + (nh + 1) * H + 4 * H)
    for H in (32, 384):
        nh = next(n for n in range(1, 10000) if lds(n, H) > 160 * 1024)
        assert hessian_split_supported(3, nh - 1, H) and not hessian_split_supported(3, nh, H)
        assert "LDS" in hessian_split_refusal(3, nh, H)


def _driver_yaml(tmp_path, H, derived=("laplacian",), c=3, **extra):
    cnf = {"save_path": str(tmp_path / "cnf"), "hidden_size": 16, "dims": 2,
           "NF": {"name": "SIRENAutodecoder_film", "out_features": c, "num_hidden_layers": 2, "hidden_features": H}}
    (tmp_path / "cnf.yml").write_text(yaml.safe_dump(cnf))
    # no ema_path, checkpoint or bounds exist: a run that got as far as loading one would fail differently
    cfg = dict({"cnf_case_file_path": str(tmp_path / "cnf.yml"), "ema_path": str(tmp_path / "absent.pt"),
                "derived": list(derived)}, **extra)
    (tmp_path / "run.yml").write_text(yaml.safe_dump(cfg))
    return basic_input(str(tmp_path / "run.yml"))


def test_driver_reads_derived_hessian_compute(tmp_path):
    assert inference.derived_hessian_compute(_driver_yaml(tmp_path, 48)) == "f32"          # default; any width
    assert inference.derived_hessian_compute(_driver_yaml(tmp_path, 48, derived_hessian_compute="f32")) == "f32"
    inp = _driver_yaml(tmp_path, 64, derived_hessian_compute="split_f16")
    assert inference.derived_hessian_compute(inp) == "split_f16"
    assert inference.derived_compute(inp) == "f32"                # the Jacobian launch's key is its own
    inp = _driver_yaml(tmp_path, 64, derived_compute="split_f16")
    assert inference.derived_hessian_compute(inp) == "f32" and inference.derived_compute(inp) == "split_f16"


@pytest.mark.parametrize("value", ["f16", "bf16", "split", 1])
def test_driver_rejects_unknown_derived_hessian_compute(tmp_path, value):
    with pytest.raises(ValueError, match="derived_hessian_compute"):
        inference.derived_hessian_compute(_driver_yaml(tmp_path, 64, derived_hessian_compute=value))


def test_driver_rejects_split_at_refused_width_before_loading(tmp_path):
    inp = _driver_yaml(tmp_path, 48, derived_hessian_compute="split_f16")
    with pytest.raises(ValueError, match="multiple of 32"):
        inference.derived_hessian_compute(inp)
    # in run() the keys are read right after the YAML, before create_model / load_state_dict
    src = open(inference.__file__).read()
    body = src[src.index("def run("):]
    assert 0 < body.index("derived_hessian_compute(inp)") < body.index("create_model(")
    assert 0 < body.index("derived_physics(inp)") < body.index("create_model(")


def test_residual_names_and_keys(tmp_path):
    names = ["momentum_residual", "pressure_poisson_residual", "convective_acceleration"]
    for n in names:
        assert n in inference.DERIVED
    assert "convective_acceleration" not in inference.HESSIAN_DERIVED           # the Jacobian launch
    assert set(inference.RESIDUAL_DERIVED) <= set(inference.HESSIAN_DERIVED)
    inp = _driver_yaml(tmp_path, 32, names, derived_nu=0.01, derived_pressure_channel=2)
    assert inference.derived_names(inp) == names
    assert inference.derived_physics(inp) == {"nu": 0.01, "rho": 1.0, "pressure_channel": 2}
    inp = _driver_yaml(tmp_path, 32, names, derived_nu=1, derived_rho=2.5, derived_pressure_channel=0,
                       derived_velocity_channels=[1, 2])
    assert inference.derived_physics(inp) == {"nu": 1.0, "rho": 2.5, "pressure_channel": 0}
    # the momentum residual alone may drop its pressure term; no residual name: no key is required
    inp = _driver_yaml(tmp_path, 32, ["momentum_residual"], derived_nu=0.5)
    assert inference.derived_physics(inp) == {"nu": 0.5, "rho": 1.0, "pressure_channel": None}
    assert inference.derived_physics(_driver_yaml(tmp_path, 32, ["laplacian", "convective_acceleration"])) == \
        {"nu": None, "rho": 1.0, "pressure_channel": None}


def test_residual_keys_are_validated(tmp_path):
    with pytest.raises(ValueError, match="derived_nu"):
        inference.derived_physics(_driver_yaml(tmp_path, 32, ["momentum_residual"], derived_pressure_channel=2))
    with pytest.raises(ValueError, match="derived_pressure_channel"):
        inference.derived_physics(_driver_yaml(tmp_path, 32, ["pressure_poisson_residual"], derived_nu=0.1))
    for bad in (3, -1):                                                          # out_features = 3
        with pytest.raises(ValueError, match="out of range"):
            inference.derived_physics(_driver_yaml(tmp_path, 32, ["pressure_poisson_residual"],
                                                   derived_pressure_channel=bad))
    with pytest.raises(ValueError, match="derived_pressure_channel"):
        inference.derived_physics(_driver_yaml(tmp_path, 32, ["momentum_residual"], derived_nu=0.1,
                                               derived_pressure_channel="p"))
    # the pressure is not a velocity component (the first d = 2 channels, or derived_velocity_channels)
    for pch, extra in ((0, {}), (1, {}), (2, {"derived_velocity_channels": [0, 2]})):
        with pytest.raises(ValueError, match="velocity channels"):
            inference.derived_physics(_driver_yaml(tmp_path, 32, ["pressure_poisson_residual"],
                                                   derived_pressure_channel=pch, **extra))
    for d, reason in ((4, "16 MFMA columns"), (0, "in_coord_features")):
        assert reason in hessian_split_refusal(d, 1, 32)
    for key in ("derived_nu", "derived_rho"):
        with pytest.raises(ValueError, match=key):
            inference.derived_physics(_driver_yaml(tmp_path, 32, ["momentum_residual"],
                                                   **dict({"derived_nu": 0.1}, **{key: "x"})))
    with pytest.raises(ValueError, match="derived_rho"):
        inference.derived_physics(_driver_yaml(tmp_path, 32, ["momentum_residual"], derived_nu=0.1, derived_rho=0))
    with pytest.raises(ValueError, match="derived"):
        inference.derived_names(_driver_yaml(tmp_path, 32, ["momentum"]))
