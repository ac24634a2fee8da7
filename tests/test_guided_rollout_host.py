"""CPU tests of the sensor-guided rollout's host side: the 'guided' method of
confild_amd.rollout and window_measurement, which cuts one window's rows out of a
measurement record and out of a mask that has a row dimension.  T = 16, overlap 5,
W = 2: windows [0, 16), [11, 27), [22, 38) of a record of 38 rows.  No GPU calls."""
import pytest
import torch

from confild_amd import rollout

T, OV, W, B, NS, C = 16, 5, 2, 2, 7, 3
TOTAL = T + W * (T - OV)


def _record(*lead):
    n = 1
    for v in lead + (NS, C):
        n *= v
    return torch.arange(n, dtype=torch.float32).reshape(lead + (NS, C))


def test_guided_is_a_rollout_method():
    assert "guided" in rollout.METHODS and rollout.METHODS[:2] == ("replace", "ps")


@pytest.mark.parametrize("w", [0, 1, 2])
def test_window_measurement_slices_record_and_mask(w):
    sl = rollout.plan_windows(T, OV, W)[w]
    assert TOTAL == 38 and sl == slice(w * 11, w * 11 + 16)
    shared, per = _record(TOTAL), _record(B, TOTAL)
    m2 = (_record() % 2)                                # (Ns, c)
    m3, m4 = (_record(TOTAL) % 3) / 2, (_record(B, TOTAL) % 5) / 4
    # the two measurement forms, no mask
    y, m = rollout.window_measurement(shared, None, sl, B, TOTAL)
    assert m is None and y.shape == (T, NS, C) and torch.equal(y, shared[sl.start:sl.stop])
    y, m = rollout.window_measurement(per, None, sl, B, TOTAL)
    assert m is None and y.shape == (B * T, NS, C)
    assert torch.equal(y, torch.cat([per[b, sl.start:sl.stop] for b in range(B)]))
    # the four mask forms, with either measurement form
    for rec in (shared, per):
        y0 = rollout.window_measurement(rec, None, sl, B, TOTAL)[0]
        y, m = rollout.window_measurement(rec, m2, sl, B, TOTAL)
        assert torch.equal(y, y0) and m.shape == (NS, C) and torch.equal(m, m2)
        y, m = rollout.window_measurement(rec, m3, sl, B, TOTAL)
        assert torch.equal(y, y0) and m.shape == (T, NS, C) and torch.equal(m, m3[sl.start:sl.stop])
        y, m = rollout.window_measurement(rec, m4, sl, B, TOTAL)
        assert torch.equal(y, y0) and m.shape == (B * T, NS, C)
        assert torch.equal(m, torch.cat([m4[b, sl.start:sl.stop] for b in range(B)]))
    # one sample of a per-sample record is that sample's rows
    y, _ = rollout.window_measurement(per[1:2], None, sl, 1, TOTAL)
    assert torch.equal(y, per[1, sl.start:sl.stop])


def test_window_measurement_errors():
    sl = rollout.plan_windows(T, OV, W)[1]
    good = _record(TOTAL)
    for bad in (_record(TOTAL - 1), _record(T), _record(B, TOTAL + 1), _record(B + 1, TOTAL), _record(),
                _record(1, B, TOTAL)):
        with pytest.raises(ValueError, match="measurement of shape"):
            rollout.window_measurement(bad, None, sl, B, TOTAL)
    for bad in (_record(1, B, TOTAL), _record(TOTAL - 1), _record(B, T), _record(B + 1, TOTAL),
                torch.ones(C)):
        with pytest.raises(ValueError, match="mask of shape"):
            rollout.window_measurement(good, bad, sl, B, TOTAL)


def test_guided_argument_errors_need_no_gpu():
    """The checks that come before any launch: an unknown method, resample with 'guided',
    'guided' on a non-guided diffusion or without cond_fn / measurement."""
    from confild_amd.guided.gaussian_diffusion import create_sampler
    from confild_amd.script_util import create_gaussian_diffusion
    plain = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="4")
    guided = create_sampler(sampler="ddpm", steps=1000, noise_schedule="cosine", model_mean_type="epsilon",
                            model_var_type="fixed_large", dynamic_threshold=False, clip_denoised=True,
                            rescale_timesteps=False, timestep_respacing="4")
    first = torch.zeros(B, 1, T, T)
    with pytest.raises(ValueError):
        rollout.extend_latents(None, guided, first, W, OV, "guided", seed=1, resample=(2, 2), cond_fn=len,
                               measurement=_record(TOTAL))
    with pytest.raises(TypeError):
        rollout.extend_latents(None, plain, first, W, OV, "guided", seed=1, cond_fn=len, measurement=_record(TOTAL))
    with pytest.raises(TypeError):
        rollout.extend_latents(None, guided, first, W, OV, "guided", seed=1)
    with pytest.raises(TypeError):
        rollout.sample_window(None, guided, (B, 1, T, T), "guided", seed=1, measurement=_record(T))
    with pytest.raises(ValueError):
        rollout.sample_window(None, guided, (B, 1, T, T), "guided", seed=1, resample=(2, 2))
