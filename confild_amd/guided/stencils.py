"""Weight builders for the 'sensor_stencil' measurement operator
(confild_amd.guided.measurements.SensorStencilOperator): each returns
``(value_weights, jac_weights)`` as float32 arrays, (M, c) / (M, c, d) or per sensor
(Ns, M, c) / (Ns, M, c, d), an unused set as None.  A reading is

    A[m] = sum_o value_weights[m, o] out[o] + sum_{o,k} jac_weights[m, o, k] d out[o] / d x_k

``stack`` joins the readings of several stencils.
"""
from __future__ import annotations

import numpy as np


def divergence(d, c):
    """One reading: sum_k d u_k / d x_k over the first d output channels (the trace)."""
    if not 1 <= d <= c:
        raise ValueError(f"divergence of {d} coordinates needs at least {d} output channels, got {c}")
    w = np.zeros((1, c, d), dtype=np.float32)
    for k in range(d):
        w[0, k, k] = 1.0
    return None, w


def vorticity_z(c, d=2):
    """One reading: d v / d x - d u / d y, (u, v) the first two channels, (x, y) the
    first two coordinates."""
    if c < 2 or d < 2:
        raise ValueError("vorticity_z needs two velocity channels and two coordinates")
    w = np.zeros((1, c, d), dtype=np.float32)
    w[0, 1, 0] = 1.0
    w[0, 0, 1] = -1.0
    return None, w


def directional(normals, channel, c):
    """Per sensor, one reading: the derivative of output ``channel`` along the sensor's
    own direction ``normals`` (Ns, d), e.g. wall shear d u_t / d n."""
    n = np.asarray(normals, dtype=np.float32)
    if n.ndim != 2:
        raise ValueError(f"normals must be (Ns, d), got {n.shape}")
    if not 0 <= channel < c:
        raise ValueError(f"channel {channel} is not one of {c} outputs")
    w = np.zeros((n.shape[0], 1, c, n.shape[1]), dtype=np.float32)
    w[:, 0, channel, :] = n
    return None, w


def values(c, d=None):
    """c readings: the outputs themselves (Case4's operator in this form)."""
    return np.eye(c, dtype=np.float32), None


def stack(stencils, c, d):
    """The readings of several (value_weights, jac_weights) pairs, one after the other.
    Shared and per-sensor weights mix: shared ones are repeated over the sensors."""
    ns = {w.shape[0] for wv, wj in stencils for w, nd in ((wv, 3), (wj, 4)) if w is not None and w.ndim == nd}
    if len(ns) > 1:
        raise ValueError(f"per-sensor stencils disagree on the sensor count: {sorted(ns)}")
    Ns = ns.pop() if ns else None

    def per_sensor(w, nd, m, tail):
        if w is None:
            w = np.zeros((m,) + tail, dtype=np.float32)
        w = np.asarray(w, dtype=np.float32)
        if Ns is not None and w.ndim == nd - 1:
            w = np.broadcast_to(w, (Ns,) + w.shape)
        return w

    wvs, wjs = [], []
    for wv, wj in stencils:
        ref = wv if wv is not None else wj
        if ref is None:
            raise ValueError("a stencil needs at least one weight set")
        m = ref.shape[-2] if ref is wv else ref.shape[-3]
        wvs.append(per_sensor(wv, 3, m, (c,)))
        wjs.append(per_sensor(wj, 4, m, (c, d)))
    any_v = any(wv is not None for wv, _ in stencils)
    any_j = any(wj is not None for _, wj in stencils)
    axis = 0 if Ns is None else 1
    return (np.ascontiguousarray(np.concatenate(wvs, axis=axis)) if any_v else None,
            np.ascontiguousarray(np.concatenate(wjs, axis=axis)) if any_j else None)
