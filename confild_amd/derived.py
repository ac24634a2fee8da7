"""Flow quantities derived from a field's spatial Jacobian (pure torch, any device,
no kernel): the read-outs of ``SIRENAutodecoder_film.decode_jacobian`` /
``trainer.infer_jacobian``.

Every function takes a Jacobian whose last two axes are (component, coordinate),
``jac[..., o, k] = d field_o / d x_k`` with d = 2 or 3 coordinates, and
``velocity_channels``: which d components are the velocity (u, v[, w]), in the
coordinates' order (default: the first d).  Leading axes are kept.

The second-order functions read the Hessian of ``decode_hessian`` /
``trainer.infer_hessian``: ``hess[..., o, k, l] = d2 field_o / d x_k d x_l``, last
three axes (component, coordinate, coordinate), or its diagonal form
``hess[..., o, k] = d2 field_o / d x_k^2``, last two axes (component, coordinate).
"""
from __future__ import annotations

import torch

__all__ = ["velocity_gradient", "vorticity", "divergence", "strain_rate", "q_criterion", "laplacian",
           "grad_divergence", "convective_acceleration", "momentum_residual", "pressure_poisson_residual"]


def velocity_gradient(jac: torch.Tensor, velocity_channels=None) -> torch.Tensor:
    """A (..., d, d), A[..., i, k] = d u_i / d x_k."""
    if not isinstance(jac, torch.Tensor) or jac.dim() < 2:
        raise ValueError("jac must be a tensor whose last two axes are (component, coordinate)")
    c, d = jac.shape[-2], jac.shape[-1]
    if d not in (2, 3):
        raise ValueError(f"a velocity gradient needs 2 or 3 coordinates, the Jacobian has {d}")
    if velocity_channels is None:
        if c < d:
            raise ValueError(f"the Jacobian has {c} components, fewer than its {d} coordinates: no velocity in it")
        return jac[..., :d, :]
    ch = [int(v) for v in velocity_channels]
    if len(ch) != d:
        raise ValueError(f"velocity_channels {ch} must name {d} components, one per coordinate")
    if any(v < 0 or v >= c for v in ch):
        raise ValueError(f"velocity_channels {ch} out of range for {c} components")
    return jac[..., ch, :]


def vorticity(jac: torch.Tensor, velocity_channels=None) -> torch.Tensor:
    """2-D: the scalar dv/dx - du/dy (...); 3-D: the curl vector (..., 3)."""
    A = velocity_gradient(jac, velocity_channels)
    if A.shape[-1] == 2:
        return A[..., 1, 0] - A[..., 0, 1]
    return torch.stack((A[..., 2, 1] - A[..., 1, 2], A[..., 0, 2] - A[..., 2, 0], A[..., 1, 0] - A[..., 0, 1]), -1)


def divergence(jac: torch.Tensor, velocity_channels=None) -> torch.Tensor:
    """trace A (...): zero for an incompressible flow."""
    return torch.diagonal(velocity_gradient(jac, velocity_channels), dim1=-2, dim2=-1).sum(-1)


def strain_rate(jac: torch.Tensor, velocity_channels=None) -> torch.Tensor:
    """S = (A + A^T) / 2 (..., d, d)."""
    A = velocity_gradient(jac, velocity_channels)
    return 0.5 * (A + A.transpose(-1, -2))


def q_criterion(jac: torch.Tensor, velocity_channels=None) -> torch.Tensor:
    """Q = (||Omega||^2 - ||S||^2) / 2 (...), Omega = (A - A^T) / 2, Frobenius norms."""
    A = velocity_gradient(jac, velocity_channels)
    S = 0.5 * (A + A.transpose(-1, -2))
    Om = 0.5 * (A - A.transpose(-1, -2))
    return 0.5 * ((Om * Om).sum((-2, -1)) - (S * S).sum((-2, -1)))


def _velocity_channels(c: int, d: int, velocity_channels) -> list:
    """The d velocity components out of c, as velocity_gradient picks them."""
    if velocity_channels is None:
        if c < d:
            raise ValueError(f"{c} components, fewer than the {d} coordinates: no velocity in them")
        return list(range(d))
    ch = [int(v) for v in velocity_channels]
    if len(ch) != d:
        raise ValueError(f"velocity_channels {ch} must name {d} components, one per coordinate")
    if any(v < 0 or v >= c for v in ch):
        raise ValueError(f"velocity_channels {ch} out of range for {c} components")
    return ch


def _channel(c: int, channel, what: str) -> int:
    ch = int(channel)
    if ch < 0 or ch >= c:
        raise ValueError(f"{what} {ch} out of range for {c} components")
    return ch


def laplacian(hess: torch.Tensor, diag=None) -> torch.Tensor:
    """sum_k d2 field_o / d x_k^2 (..., c) of a full Hessian (..., c, d, d) (its trace) or
    of the diagonal form (..., c, d).  ``diag`` says which one ``hess`` is; None takes a
    tensor of three or more axes whose last two are equal for a full Hessian, so a
    diagonal form with c == d behind a leading axis needs ``diag=True``."""
    if not isinstance(hess, torch.Tensor) or hess.dim() < 2:
        raise ValueError("hess must be a tensor (..., c, d, d), or (..., c, d) in the diagonal form")
    if diag is None:
        diag = not (hess.dim() >= 3 and hess.shape[-1] == hess.shape[-2])
    if diag:
        return hess.sum(-1)
    if hess.dim() < 3 or hess.shape[-1] != hess.shape[-2]:
        raise ValueError(f"a full Hessian ends in (c, d, d), got {tuple(hess.shape)}")
    return torch.diagonal(hess, dim1=-2, dim2=-1).sum(-1)


def _full_hessian(hess, what: str):
    if not isinstance(hess, torch.Tensor) or hess.dim() < 3 or hess.shape[-1] != hess.shape[-2]:
        raise ValueError(f"{what} needs the full Hessian (..., c, d, d)")
    if hess.shape[-1] not in (2, 3):
        raise ValueError(f"{what} needs 2 or 3 coordinates, the Hessian has {hess.shape[-1]}")
    return hess


def grad_divergence(hess: torch.Tensor, velocity_channels=None) -> torch.Tensor:
    """grad(div u) (..., d): out[..., i] = d_i d_k u_k, from the full Hessian."""
    hess = _full_hessian(hess, "grad_divergence")
    c, d = hess.shape[-3], hess.shape[-1]
    ch = _velocity_channels(c, d, velocity_channels)
    return sum(hess[..., ch[k], :, k] for k in range(d))


def convective_acceleration(u: torch.Tensor, jac: torch.Tensor, velocity_channels=None) -> torch.Tensor:
    """(u . grad) u (..., d): out[..., i] = u_k d_k u_i, u the fields (..., c) of the Jacobian."""
    A = velocity_gradient(jac, velocity_channels)
    if not isinstance(u, torch.Tensor) or tuple(u.shape) != tuple(jac.shape[:-1]):
        raise ValueError(f"u must be the fields (..., c) of the Jacobian: {tuple(jac.shape[:-1])}, got "
                         f"{tuple(u.shape) if isinstance(u, torch.Tensor) else type(u).__name__}")
    ch = _velocity_channels(jac.shape[-2], jac.shape[-1], velocity_channels)
    return (A * u[..., ch][..., None, :]).sum(-1)


def _laplacian_like(jac, hess, what: str):
    """The Laplacian (..., c) of a Hessian that goes with ``jac``: full (jac's shape and
    one more coordinate axis) or diagonal (jac's shape)."""
    if not isinstance(jac, torch.Tensor) or jac.dim() < 2 or not isinstance(hess, torch.Tensor):
        raise ValueError(f"{what}: jac must be (..., c, d) and hess (..., c, d, d) or (..., c, d)")
    if tuple(hess.shape) == tuple(jac.shape):
        return laplacian(hess, diag=True)
    if tuple(hess.shape) == tuple(jac.shape) + (jac.shape[-1],):
        return laplacian(hess, diag=False)
    raise ValueError(f"{what}: a Hessian of shape {tuple(hess.shape)} goes with no Jacobian of shape "
                     f"{tuple(jac.shape)}")


def momentum_residual(u: torch.Tensor, jac: torch.Tensor, hess: torch.Tensor, nu, pressure_channel=None, rho=1.0,
                      dudt=None, velocity_channels=None) -> torch.Tensor:
    """Residual of the incompressible momentum equation (..., d):
    R_i = dudt_i + u_k d_k u_i + (1 / rho) d_i p - nu lap(u_i).  ``hess`` is the full or the
    diagonal Hessian; ``dudt`` (..., d) the velocity's time derivative (None: steady);
    the pressure term is dropped when ``pressure_channel`` is None."""
    R = convective_acceleration(u, jac, velocity_channels)
    c, d = jac.shape[-2], jac.shape[-1]
    ch = _velocity_channels(c, d, velocity_channels)
    R = R - nu * _laplacian_like(jac, hess, "momentum_residual")[..., ch]
    if pressure_channel is not None:
        R = R + jac[..., _channel(c, pressure_channel, "pressure_channel"), :] / rho
    if dudt is not None:
        if not isinstance(dudt, torch.Tensor) or tuple(dudt.shape) != tuple(R.shape):
            raise ValueError(f"dudt must be the velocity's time derivative of shape {tuple(R.shape)}")
        R = R + dudt
    return R


def pressure_poisson_residual(jac: torch.Tensor, hess: torch.Tensor, pressure_channel, rho=1.0,
                              velocity_channels=None) -> torch.Tensor:
    """lap(p) + rho d_i u_k d_k u_i (...): zero for an incompressible Navier-Stokes flow."""
    A = velocity_gradient(jac, velocity_channels)
    lap = _laplacian_like(jac, hess, "pressure_poisson_residual")
    if pressure_channel is None:
        raise ValueError("pressure_poisson_residual needs a pressure_channel")
    p = _channel(jac.shape[-2], pressure_channel, "pressure_channel")
    return lap[..., p] + rho * (A * A.transpose(-1, -2)).sum((-2, -1))
