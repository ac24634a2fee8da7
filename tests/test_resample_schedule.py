"""Host: RePaint's resampling schedule (gaussian_diffusion.resample_schedule) and the
merged forward step of a jump (GaussianDiffusion.jump_coefs).  No GPU."""
import os
import re

import numpy as np
import pytest

from confild_amd import _lib
from confild_amd.gaussian_diffusion import resample_schedule
from confild_amd.script_util import create_gaussian_diffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(8, 2, 2), (8, 3, 3), (8, 2, 3), (8, 1, 2), (8, 7, 2), (8, 8, 4), (8, 4, 1), (50, 5, 3), (256, 10, 10)]


@pytest.mark.parametrize("n,J,r", CASES)
def test_schedule_properties(n, J, r):
    s = resample_schedule(n, J, r)
    P = len(range(0, n - J, J))
    assert len(s) == n + P * (r - 1) * J
    assert s[-1] == (0, None)
    for i, to in s:
        assert 0 <= i <= n - 1
        if to is not None:
            assert to == i - 1 + J <= n - 1 and i >= 1
    if r == 1 or J >= n:
        assert s == [(i, None) for i in range(n - 1, -1, -1)]
    else:
        assert sum(to is not None for _, to in s) == P * (r - 1)
    # the walk is connected: each step runs the level the one before it left the state at
    level = n - 1
    for i, to in s:
        assert i == level
        level = i - 1 if to is None else to
    assert level == -1
    # table indices 1 .. P * J lie under a jump and run r times, the others once
    visits = np.bincount([i for i, _ in s], minlength=n)
    for lv in range(n):
        assert visits[lv] == (r if 1 <= lv <= P * J else 1), (lv, visits[lv])


def test_schedule_examples():
    N = None
    assert resample_schedule(8, 2, 2) == [(7, N), (6, N), (5, 6), (6, N), (5, N), (4, N), (3, 4), (4, N), (3, N),
                                          (2, N), (1, 2), (2, N), (1, N), (0, N)]
    assert len(resample_schedule(8, 3, 3)) == 20
    assert len(resample_schedule(256, 10, 10)) == 2506


def test_schedule_argument_errors():
    with pytest.raises(ValueError):
        resample_schedule(8, 0, 2)
    with pytest.raises(ValueError):
        resample_schedule(8, -1, 2)
    with pytest.raises(ValueError):
        resample_schedule(8, 2, 0)


@pytest.mark.parametrize("respacing,J,r", [("8", 2, 2), ("8", 3, 3), ("8", 1, 2), ("256", 10, 10)])
def test_jump_coefs_are_the_composed_forward_steps(respacing, J, r):
    """rho = abar[L + J] / abar[L] is the product of the J single forward steps'
    (1 - beta), from the object's own (respaced) tables; (a, b) are its roots in fp32."""
    d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing=respacing)
    n = d.num_timesteps
    assert n == int(respacing)
    jumps = [(i, to) for i, to in resample_schedule(n, J, r) if to is not None]
    assert jumps
    ulp = float(np.spacing(np.float32(1.0)))
    for i, to in jumps:
        a, b = d.jump_coefs(i, to)
        L = i - 1
        rho = d.alphas_cumprod[to] / d.alphas_cumprod[L]
        assert a == float(np.float32(np.sqrt(rho))) and b == float(np.float32(np.sqrt(1.0 - rho)))
        assert 0.0 < b <= 1.0 and 0.0 <= a < 1.0
        a32, b32 = np.float32(a), np.float32(b)
        assert abs(float(a32 * a32 + b32 * b32) - 1.0) <= 2 * ulp
        prod = np.prod(1.0 - d.betas[L + 1:to + 1])
        assert to - L == J and abs(rho - prod) <= 1e-12 * prod


def test_jump_coefs_argument_errors():
    d = create_gaussian_diffusion(steps=1000, noise_schedule="cosine", timestep_respacing="8")
    for i, to in ((0, 1), (3, 8), (4, 2)):
        with pytest.raises(ValueError):
            d.jump_coefs(i, to)


def test_header_declares_the_jump_entries():
    hdr = open(os.path.join(ROOT, "include", "confild.h")).read()
    declared = set(re.findall(r"\b(cfd_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ("cfd_sched_step_jump", "cfd_sampler_set_jumps"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
