"""confild_amd.derived's second-order functions on analytic flows (CPU, fp64): the
quantities read off a Hessian whose last three axes are (component, coordinate,
coordinate), or its diagonal form (component, coordinate)."""
import math

import pytest
import torch

from confild_amd import derived

F64 = torch.float64
EPS = 64 * torch.finfo(F64).eps       # a few dozen fp64 roundings of O(1) terms


def _taylor_green(n=257, nu=0.1, t=0.3, rho=1.3):
    """Fields (u, v, p) of the decaying 2-D Taylor-Green vortex, their Jacobian (n, 3, 2),
    Hessian (n, 3, 2, 2) and du/dt (n, 2)."""
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(n, generator=g, dtype=F64) - 0.5) * 12.0
    y = (torch.rand(n, generator=g, dtype=F64) - 0.5) * 12.0
    sx, cx, sy, cy = torch.sin(x), torch.cos(x), torch.sin(y), torch.cos(y)
    F = math.exp(-2.0 * nu * t)
    u, v = sx * cy * F, -cx * sy * F
    p = rho / 4.0 * (torch.cos(2 * x) + torch.cos(2 * y)) * F * F
    o = torch.zeros_like(x)
    pair = lambda a, b: torch.stack((a, b), -1)
    jac = torch.stack((pair(cx * cy * F, -sx * sy * F), pair(sx * sy * F, -cx * cy * F),
                       pair(-rho / 2.0 * torch.sin(2 * x) * F * F, -rho / 2.0 * torch.sin(2 * y) * F * F)), -2)
    hess = torch.stack((torch.stack((pair(-u, -cx * sy * F), pair(-cx * sy * F, -u)), -2),
                        torch.stack((pair(-v, sx * cy * F), pair(sx * cy * F, -v)), -2),
                        torch.stack((pair(-rho * torch.cos(2 * x) * F * F, o),
                                     pair(o, -rho * torch.cos(2 * y) * F * F)), -2)), -3)
    fields = torch.stack((u, v, p), -1)
    return fields, jac, hess, -2.0 * nu * fields[:, :2], nu, rho


def _abc(n=193, A=1.0, B=0.7, Cc=0.4):
    """Fields (u, v, w, p) of an ABC (Beltrami) flow with p = -|u|^2 / 2, their Jacobian
    (n, 4, 3) and Hessian (n, 4, 3, 3)."""
    g = torch.Generator().manual_seed(4)
    x, y, z = ((torch.rand(n, generator=g, dtype=F64) - 0.5) * 10.0 for _ in range(3))
    # u = A sin z + C cos y, v = B sin x + A cos z, w = C sin y + B cos x
    vel = torch.stack((A * torch.sin(z) + Cc * torch.cos(y), B * torch.sin(x) + A * torch.cos(z),
                       Cc * torch.sin(y) + B * torch.cos(x)), -1)
    o = torch.zeros_like(x)
    J = torch.stack((torch.stack((o, -Cc * torch.sin(y), A * torch.cos(z)), -1),
                     torch.stack((B * torch.cos(x), o, -A * torch.sin(z)), -1),
                     torch.stack((-B * torch.sin(x), Cc * torch.cos(y), o), -1)), -2)
    Hv = torch.zeros(n, 3, 3, 3, dtype=F64)       # no mixed derivatives
    Hv[:, 0, 1, 1], Hv[:, 0, 2, 2] = -Cc * torch.cos(y), -A * torch.sin(z)
    Hv[:, 1, 0, 0], Hv[:, 1, 2, 2] = -B * torch.sin(x), -A * torch.cos(z)
    Hv[:, 2, 0, 0], Hv[:, 2, 1, 1] = -B * torch.cos(x), -Cc * torch.sin(y)
    # p = -u_i u_i / 2: d_k p = -u_i d_k u_i, d_k d_l p = -(d_l u_i d_k u_i + u_i d_k d_l u_i)
    p = -0.5 * (vel * vel).sum(-1)
    Jp = -torch.einsum("ni,nik->nk", vel, J)
    Hp = -(torch.einsum("nil,nik->nkl", J, J) + torch.einsum("ni,nikl->nkl", vel, Hv))
    fields = torch.cat((vel, p[:, None]), -1)
    return fields, torch.cat((J, Jp[:, None]), -2), torch.cat((Hv, Hp[:, None]), -3)


def test_taylor_green_2d():
    f, jac, hess, dudt, nu, rho = _taylor_green()
    assert jac.shape == (257, 3, 2) and hess.shape == (257, 3, 2, 2)
    lap = derived.laplacian(hess)
    assert lap.shape == (257, 3)
    assert (lap[:, :2] + 2 * f[:, :2]).abs().max() <= EPS                       # lap(u) = -2 u
    gd = derived.grad_divergence(hess)
    assert gd.shape == (257, 2) and gd.abs().max() <= EPS
    conv = derived.convective_acceleration(f, jac)
    assert conv.shape == (257, 2)
    assert (conv - torch.einsum("nk,nik->ni", f[:, :2], jac[:, :2])).abs().max() <= EPS
    R = derived.momentum_residual(f, jac, hess, nu, pressure_channel=2, rho=rho, dudt=dudt)
    assert R.shape == (257, 2) and R.abs().max() <= EPS
    pp = derived.pressure_poisson_residual(jac, hess, 2, rho=rho)
    assert pp.shape == (257,) and pp.abs().max() <= EPS
    # the pieces are really there: without dudt, or without the pressure, the residual is not zero
    assert derived.momentum_residual(f, jac, hess, nu, pressure_channel=2, rho=rho).abs().max() > 1e-3
    assert derived.momentum_residual(f, jac, hess, nu, rho=rho, dudt=dudt).abs().max() > 1e-3
    assert (derived.momentum_residual(f, jac, hess, nu, rho=rho, dudt=dudt)
            - (R - jac[:, 2] / rho)).abs().max() <= EPS


def test_abc_flow_3d():
    f, jac, hess = _abc()
    assert jac.shape == (193, 4, 3) and hess.shape == (193, 4, 3, 3)
    lap = derived.laplacian(hess)
    assert (lap[:, :3] + f[:, :3]).abs().max() <= EPS                           # lap(u) = -u
    assert derived.grad_divergence(hess).abs().max() <= EPS
    R = derived.momentum_residual(f, jac, hess, 0.0, pressure_channel=3)        # steady Euler
    assert R.shape == (193, 3) and R.abs().max() <= EPS
    assert derived.pressure_poisson_residual(jac, hess, 3).abs().max() <= 4 * EPS
    # viscous: lap(u) = -u leaves nu * u
    Rv = derived.momentum_residual(f, jac, hess, 0.25, pressure_channel=3)
    assert (Rv - 0.25 * f[:, :3]).abs().max() <= EPS


def test_diagonal_form_matches_the_full_form():
    f, jac, hess = _abc(60)
    dg = torch.diagonal(hess, dim1=-2, dim2=-1).contiguous()                    # (n, 4, 3)
    assert torch.equal(derived.laplacian(dg, diag=True), derived.laplacian(hess))
    assert torch.equal(derived.laplacian(dg[:, :2]), derived.laplacian(hess)[:, :2])   # (n, 2, 3): inferred
    assert torch.equal(derived.laplacian(dg[0, :2]), derived.laplacian(hess)[0, :2])   # (2, 3), no leading axis
    assert torch.equal(derived.momentum_residual(f, jac, dg, 0.25, pressure_channel=3),
                       derived.momentum_residual(f, jac, hess, 0.25, pressure_channel=3))
    assert torch.equal(derived.pressure_poisson_residual(jac, dg, 3), derived.pressure_poisson_residual(jac, hess, 3))
    # c == d behind a leading axis looks like a full Hessian: diag=True says otherwise
    sq = dg[:, :3]
    assert torch.equal(derived.laplacian(sq, diag=True), derived.laplacian(hess)[:, :3])
    assert derived.laplacian(sq).shape == (60,)
    # leading axes are kept
    grid = hess.reshape(6, 10, 4, 3, 3)
    assert derived.laplacian(grid).shape == (6, 10, 4) and derived.grad_divergence(grid).shape == (6, 10, 3)
    assert torch.equal(derived.laplacian(grid).reshape(60, 4), derived.laplacian(hess))


def test_channel_selection():
    """A c = 4 field (p, v, T, u) in 2-D: the velocity is channels (3, 1), the pressure 0."""
    f, jac, hess, dudt, nu, rho = _taylor_green(64)
    g = torch.Generator().manual_seed(9)
    f4 = torch.randn(64, 4, generator=g, dtype=F64)
    j4 = torch.randn(64, 4, 2, generator=g, dtype=F64)
    h4 = torch.randn(64, 4, 2, 2, generator=g, dtype=F64)
    for src, dst in ((0, 3), (1, 1), (2, 0)):
        f4[:, dst], j4[:, dst], h4[:, dst] = f[:, src], jac[:, src], hess[:, src]
    vc = (3, 1)
    assert torch.equal(derived.grad_divergence(h4, vc), derived.grad_divergence(hess))
    assert torch.equal(derived.convective_acceleration(f4, j4, vc), derived.convective_acceleration(f, jac))
    assert torch.equal(derived.momentum_residual(f4, j4, h4, nu, 0, rho, dudt, vc),
                       derived.momentum_residual(f, jac, hess, nu, 2, rho, dudt))
    assert torch.equal(derived.pressure_poisson_residual(j4, h4, 0, rho, vc),
                       derived.pressure_poisson_residual(jac, hess, 2, rho))
    assert torch.equal(derived.laplacian(h4)[:, [3, 1, 0]], derived.laplacian(hess))
    # the default is the first d channels
    assert not torch.equal(derived.grad_divergence(h4), derived.grad_divergence(h4, vc))


def test_shape_errors_raise():
    z = torch.zeros
    for bad in (z(5), 3.0):
        with pytest.raises(ValueError):
            derived.laplacian(bad)
    with pytest.raises(ValueError):
        derived.laplacian(z(5, 3, 2), diag=False)          # not (c, d, d)
    with pytest.raises(ValueError):
        derived.laplacian(z(3, 2), diag=False)
    for bad, vc in ((z(5, 3), None), (z(5, 3, 2), None),   # no, or unequal, coordinate axes
                    (z(5, 3, 1, 1), None), (z(5, 4, 4, 4), None),   # one and four coordinates
                    (z(5, 2, 3, 3), None),                  # fewer components than coordinates
                    (z(5, 4, 2, 2), (0, 1, 2)), (z(5, 4, 2, 2), (0, 4))):
        with pytest.raises(ValueError):
            derived.grad_divergence(bad, vc)
    u, jac, hess = z(5, 3), z(5, 3, 2), z(5, 3, 2, 2)
    with pytest.raises(ValueError):
        derived.convective_acceleration(z(5, 2), jac)       # u is not the Jacobian's fields
    with pytest.raises(ValueError):
        derived.convective_acceleration(u, z(5, 3, 4))      # four coordinates
    with pytest.raises(ValueError):
        derived.convective_acceleration(u, jac, (0, 3))
    with pytest.raises(ValueError):
        derived.momentum_residual(u, jac, z(5, 3, 3, 3), 0.1)       # a Hessian of another d
    with pytest.raises(ValueError):
        derived.momentum_residual(u, jac, z(4, 3, 2, 2), 0.1)       # of another point count
    with pytest.raises(ValueError):
        derived.momentum_residual(u, jac, hess, 0.1, pressure_channel=3)
    with pytest.raises(ValueError):
        derived.momentum_residual(u, jac, hess, 0.1, dudt=z(5, 3))
    with pytest.raises(ValueError):
        derived.momentum_residual(z(5, 2), jac, hess, 0.1)
    with pytest.raises(ValueError):
        derived.pressure_poisson_residual(jac, hess, None)
    with pytest.raises(ValueError):
        derived.pressure_poisson_residual(jac, hess, -1)
    with pytest.raises(ValueError):
        derived.pressure_poisson_residual(jac, z(5, 3, 2, 3), 2)
    with pytest.raises(ValueError):
        derived.pressure_poisson_residual(z(5, 3, 2)[..., :1], z(5, 3, 1, 1), 2)   # one coordinate
