"""Flow quantities derived from a field's spatial Jacobian (pure torch, any device,
no kernel): the read-outs of ``SIRENAutodecoder_film.decode_jacobian`` /
``trainer.infer_jacobian``.

Every function takes a Jacobian whose last two axes are (component, coordinate),
``jac[..., o, k] = d field_o / d x_k`` with d = 2 or 3 coordinates, and
``velocity_channels``: which d components are the velocity (u, v[, w]), in the
coordinates' order (default: the first d).  Leading axes are kept.
"""
from __future__ import annotations

import torch

__all__ = ["velocity_gradient", "vorticity", "divergence", "strain_rate", "q_criterion"]


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
