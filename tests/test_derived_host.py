"""confild_amd.derived on analytic flows (CPU, fp64): the quantities read off a
Jacobian whose last two axes are (component, coordinate)."""
import pytest
import torch

from confild_amd import derived

F64 = torch.float64


def _taylor_green(n=257):
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(n, generator=g, dtype=F64) - 0.5) * 12.0
    y = (torch.rand(n, generator=g, dtype=F64) - 0.5) * 12.0
    sx, cx, sy, cy = torch.sin(x), torch.cos(x), torch.sin(y), torch.cos(y)
    # u = sin x cos y, v = -cos x sin y
    jac = torch.stack((torch.stack((cx * cy, -sx * sy), -1), torch.stack((sx * sy, -cx * cy), -1)), -2)
    return x, y, jac


def _abc(n=193, A=1.0, B=0.7, Cc=0.4):
    g = torch.Generator().manual_seed(4)
    x, y, z = ((torch.rand(n, generator=g, dtype=F64) - 0.5) * 10.0 for _ in range(3))
    # u = A sin z + C cos y, v = B sin x + A cos z, w = C sin y + B cos x
    vel = torch.stack((A * torch.sin(z) + Cc * torch.cos(y), B * torch.sin(x) + A * torch.cos(z),
                       Cc * torch.sin(y) + B * torch.cos(x)), -1)
    o = torch.zeros_like(x)
    jac = torch.stack((torch.stack((o, -Cc * torch.sin(y), A * torch.cos(z)), -1),
                       torch.stack((B * torch.cos(x), o, -A * torch.sin(z)), -1),
                       torch.stack((-B * torch.sin(x), Cc * torch.cos(y), o), -1)), -2)
    return vel, jac


def test_taylor_green_2d():
    x, y, jac = _taylor_green()
    assert jac.shape == (257, 2, 2)
    eps = 8 * torch.finfo(F64).eps
    assert derived.divergence(jac).abs().max() <= eps
    w = derived.vorticity(jac)
    assert w.shape == (257,)
    assert (w - 2 * torch.sin(x) * torch.sin(y)).abs().max() <= eps
    S = derived.strain_rate(jac)
    assert torch.equal(S, S.transpose(-1, -2)) and (S - 0.5 * (jac + jac.transpose(-1, -2))).abs().max() <= eps
    A = derived.velocity_gradient(jac)
    assert torch.equal(A, jac)
    q = derived.q_criterion(jac)
    assert (q + 0.5 * torch.einsum("nij,nji->n", A, A)).abs().max() <= eps


def test_abc_flow_3d():
    vel, jac = _abc()
    eps = 16 * torch.finfo(F64).eps
    curl = derived.vorticity(jac)
    assert curl.shape == (193, 3)
    assert (curl - vel).abs().max() <= eps                      # Beltrami: curl u = u
    assert derived.divergence(jac).abs().max() <= eps
    q = derived.q_criterion(jac)
    assert (q + 0.5 * torch.einsum("nij,nji->n", jac, jac)).abs().max() <= eps   # Q = -tr(A^2) / 2, div-free A


def test_leading_axes_are_kept():
    _, _, jac = _taylor_green(6 * 5 * 4)
    grid = jac.reshape(6, 5, 4, 2, 2)
    assert derived.vorticity(grid).shape == (6, 5, 4)
    assert derived.divergence(grid).shape == (6, 5, 4)
    assert derived.q_criterion(grid).shape == (6, 5, 4)
    assert derived.strain_rate(grid).shape == (6, 5, 4, 2, 2)
    assert torch.equal(derived.vorticity(grid).reshape(-1), derived.vorticity(jac))


def test_velocity_channels_on_c4_field():
    """A c = 4 field (p, v, T, u) in 2-D: the velocity is channels (3, 1)."""
    x, y, tg = _taylor_green(64)
    g = torch.Generator().manual_seed(9)
    jac = torch.randn(64, 4, 2, generator=g, dtype=F64)
    jac[:, 3] = tg[:, 0]
    jac[:, 1] = tg[:, 1]
    A = derived.velocity_gradient(jac, velocity_channels=(3, 1))
    assert torch.equal(A, tg)
    assert torch.equal(derived.vorticity(jac, (3, 1)), derived.vorticity(tg))
    assert torch.equal(derived.divergence(jac, [3, 1]), derived.divergence(tg))
    assert torch.equal(derived.q_criterion(jac, velocity_channels=(3, 1)), derived.q_criterion(tg))
    assert torch.equal(derived.strain_rate(jac, (3, 1)), derived.strain_rate(tg))
    # the default is the first d channels
    assert torch.equal(derived.velocity_gradient(jac), jac[:, :2])
    assert not torch.equal(derived.vorticity(jac), derived.vorticity(jac, (3, 1)))


@pytest.mark.parametrize("fn", [derived.velocity_gradient, derived.vorticity, derived.divergence,
                                derived.strain_rate, derived.q_criterion])
def test_shape_mismatches_raise(fn):
    with pytest.raises(ValueError):
        fn(torch.zeros(5))                        # no (component, coordinate) axes
    with pytest.raises(ValueError):
        fn(torch.zeros(5, 3, 1))                  # one coordinate: no velocity gradient
    with pytest.raises(ValueError):
        fn(torch.zeros(5, 4, 4))                  # four coordinates
    with pytest.raises(ValueError):
        fn(torch.zeros(5, 2, 3))                  # fewer components than coordinates
    with pytest.raises(ValueError):
        fn(torch.zeros(5, 4, 2), (0, 1, 2))       # three channels for two coordinates
    with pytest.raises(ValueError):
        fn(torch.zeros(5, 4, 2), (0, 4))          # channel out of range
