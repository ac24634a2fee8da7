"""CPU: the width rule of the split-f16 Jacobian as Python states it
(nf_networks.jacobian_split_supported) and the driver's `derived_compute` key, which is
checked against the CNF case file before anything is loaded."""
import pytest
import yaml

from confild_amd import inference
from confild_amd.nf_networks import (JACOBIAN_SPLIT_WIDTHS, jacobian_split_refusal, jacobian_split_supported)
from confild_amd.read_input import basic_input


def test_width_rule():
    assert JACOBIAN_SPLIT_WIDTHS == (32, 64, 96, 128, 192, 256, 384)
    for H in range(16, 513, 16):
        for d in (1, 2, 3):
            assert jacobian_split_supported(d, 2, H) == (H in JACOBIAN_SPLIT_WIDTHS), (d, H)
    assert jacobian_split_supported(3, 15, 384) and jacobian_split_supported(2, 17, 256)
    for (d, nh, H), reason in (((2, 2, 48), "multiple of 32"), ((2, 2, 512), "512"), ((2, 2, 160), "160"),
                               ((2, 0, 64), "num_hidden_layers"), ((4, 1, 32), "in_coord_features"),
                               ((0, 1, 32), "in_coord_features")):
        assert not jacobian_split_supported(d, nh, H)
        assert reason in jacobian_split_refusal(d, nh, H), (d, nh, H)
    # LDS staging: 2 blocks of H x 16 weights (hi + lo f16) + (nh + 1) FiLM rows + the first layer, 160 KiB
    assert jacobian_split_supported(3, 60, 384) and not jacobian_split_supported(3, 80, 384)
    assert "LDS" in jacobian_split_refusal(3, 80, 384)
    lds = lambda nh, H: 4 * (2 * (H // 16) * 256 + (nh + 1) * H + 4 * H)
    nh = next(n for n in range(1, 10000) if lds(n, 32) > 160 * 1024)
    assert jacobian_split_supported(1, nh - 1, 32) and not jacobian_split_supported(1, nh, 32)


def _driver_yaml(tmp_path, H, **extra):
    cnf = {"save_path": str(tmp_path / "cnf"), "hidden_size": 16, "dims": 2,
           "NF": {"name": "SIRENAutodecoder_film", "out_features": 2, "num_hidden_layers": 2, "hidden_features": H}}
    (tmp_path / "cnf.yml").write_text(yaml.safe_dump(cnf))
    # no ema_path, checkpoint or bounds exist: a run that got as far as loading one would fail differently
    cfg = dict({"cnf_case_file_path": str(tmp_path / "cnf.yml"), "ema_path": str(tmp_path / "absent.pt"),
                "derived": ["vorticity"]}, **extra)
    (tmp_path / "run.yml").write_text(yaml.safe_dump(cfg))
    return basic_input(str(tmp_path / "run.yml"))


def test_driver_reads_derived_compute(tmp_path):
    assert inference.derived_compute(_driver_yaml(tmp_path, 48)) == "f32"          # default; any width
    assert inference.derived_compute(_driver_yaml(tmp_path, 48, derived_compute="f32")) == "f32"
    assert inference.derived_compute(_driver_yaml(tmp_path, 64, derived_compute="split_f16")) == "split_f16"


@pytest.mark.parametrize("value", ["f16", "bf16", "split", 1])
def test_driver_rejects_unknown_derived_compute(tmp_path, value):
    with pytest.raises(ValueError, match="derived_compute"):
        inference.derived_compute(_driver_yaml(tmp_path, 64, derived_compute=value))


def test_driver_rejects_split_at_refused_width_before_loading(tmp_path):
    inp = _driver_yaml(tmp_path, 48, derived_compute="split_f16")
    with pytest.raises(ValueError, match="multiple of 32"):
        inference.derived_compute(inp)
    # in run() the key is read right after the YAML, before create_model / load_state_dict
    src = open(inference.__file__).read()
    body = src[src.index("def run("):]
    assert 0 < body.index("derived_compute(inp)") < body.index("create_model(")
