"""Measurement operators and noises (C/src/guided_diffusion/measurements.py).

The CoNFiLD operators case2, case3, case3_gappy and case4 (SURVEY.md section 8
a17).  Their forward is the fused HIP SIREN decode at the measured coordinates.
The DPS sampler additionally uses ``forward_tape`` / ``vjp`` (Case4's 10-sensor
latent gradient, the whole tape in memory) or ``dense_grad`` (a dense or masked
measurement: residual norm and latent gradient in bounded memory).
"""
from __future__ import annotations

from abc import ABC, abstractmethod

import numpy as np
import torch

from .. import _lib
from ..inference import latent_denorm
from ..nf_networks import SIRENAutodecoder_film
from ..normalize import Normalizer_ts

__OPERATOR__ = {}


def register_operator(name: str):
    def wrapper(cls):
        if __OPERATOR__.get(name, None):
            raise NameError(f"Name {name} is already registered!")
        __OPERATOR__[name] = cls
        return cls
    return wrapper


def get_operator(name: str, **kwargs):
    """measurements.py:30-33."""
    if __OPERATOR__.get(name, None) is None:
        raise NameError(f"Name {name} is not defined.")
    return __OPERATOR__[name](**kwargs)


class LinearOperator(ABC):
    @abstractmethod
    def forward(self, data, **kwargs):
        pass


class NonLinearOperator(ABC):
    @abstractmethod
    def forward(self, data, **kwargs):
        pass

    def project(self, data, measurement, **kwargs):
        return data + measurement - self.forward(data)


@register_operator(name="inpainting")
class InpaintingOperator(LinearOperator):
    """measurements.py:40-56: A(x) = mask * x on the latent image itself (known rows
    of a latent sequence, gaps, end states).  Plain torch, CPU tensors included;
    under 'ps' the guided sampler runs its adjoint as one cfd_dps_latent_residual."""

    def __init__(self, device):
        self.device = device

    def forward(self, data, **kwargs):
        """mask * data on the operator's device; without a usable ``mask`` keyword the
        reference's ValueError("Require mask")."""
        mask = kwargs.get("mask")
        if not torch.is_tensor(mask):
            raise ValueError("Require mask")
        try:
            return mask.to(self.device) * data.to(self.device)
        except RuntimeError as e:
            raise ValueError("Require mask") from e

    def transpose(self, data, **kwargs):
        """A^T applied to a measurement: the identity, as in the reference (:52-53)."""
        return data

    def ortho_project(self, data, **kwargs):
        """(I - A) data, the part of the image the mask hides (:55-56)."""
        return data - self.forward(data, **kwargs)


def _siren_dims(sd):
    n1 = sorted(int(k.split(".")[1]) for k in sd if k.startswith("net1.") and k.endswith(".weight"))
    first, last = sd["net1.0.weight"], sd[f"net1.{n1[-1]}.weight"]
    return first.shape[1], sd["net2.0.weight"].shape[1], last.shape[0], len(n1) - 2, first.shape[0]


class _SirenFieldOperator(NonLinearOperator):
    """What the SIREN-decoding operators share: latents (s, 1, t, l) in [-1, 1] are
    un-normalised with max_val / min_val, flattened to rows and decoded at
    ``coords`` through the '-11' x / y normalisers."""

    _name = "SIREN"

    @classmethod
    def from_parts(cls, device, coords, x_normalizer, y_normalizer, model, max_val, min_val, batch_size=384):
        """An operator from in-memory pieces (what a test or a synthetic run needs)."""
        op = cls.__new__(cls)
        op.device = device
        op.coords = torch.as_tensor(coords, dtype=torch.float32).to(device)
        op.x_normalizer, op.y_normalizer, op.model = x_normalizer, y_normalizer, model.to(device)
        op.max_val = torch.as_tensor(max_val).to(device)
        op.min_val = torch.as_tensor(min_val).to(device)
        op.batch_size = batch_size
        return op

    def _load_model(self, ckpt_path, cin_size, cout_size, device):
        ckpt = torch.load(ckpt_path, weights_only=True, map_location="cpu")
        sd = ckpt["model_state_dict"]
        d, L, c, nh, H = _siren_dims(sd)
        if d != cin_size or c != cout_size:
            raise ValueError(f"{self._name} SIREN must map {cin_size} coordinates to {cout_size} outputs, "
                             f"checkpoint has {d} -> {c}")
        self.model = SIRENAutodecoder_film(d, L, c, nh, H)
        self.model.load_state_dict(sd)
        self.model.eval()
        self.model.to(device)

    def _unnorm(self, norm_data):
        return ((norm_data[:, 0, ...] + 1) * (self.max_val - self.min_val) / 2 + self.min_val)[:, None, ...]

    def _bounds(self):
        vmax = self.max_val.to(device=self.coords.device, dtype=torch.float32).reshape(-1).contiguous()
        vmin = self.min_val.to(device=self.coords.device, dtype=torch.float32).reshape(-1).contiguous()
        return vmax, vmin

    def _rows(self, data):
        """_unnorm + rearrange "s c t l -> (s c t) l" on the GPU (cfd_latent_denorm)."""
        if data.dim() != 4 or data.shape[1] != 1:
            raise ValueError(f"{self._name} latents must be (s, 1, t, l), got {tuple(data.shape)}")
        vmax, vmin = self._bounds()
        z = latent_denorm(data.detach().to(torch.float32).contiguous(), vmax, vmin)
        return z.reshape(-1, data.shape[-1])

    def _fields(self, data):
        with torch.no_grad():
            return self.model.decode(self.coords, self._rows(data)[:, None], self.x_normalizer, self.y_normalizer)

    def default_mask(self):
        """The mask the operator itself applies ((Ns, c) table), or None."""
        return None

    def forward(self, data, **kwargs):
        """(s, 1, t, l) latents in [-1, 1] -> (s*t, Ns, c) measurements (one fused launch;
        pass_through_model_batch's row chunking does not change values)."""
        return self._fields(data)

    # -- adjoint used by the DPS sampler ----------------------------------------
    def dense_grad(self, data, measurement, mask=None, budget=None):
        """(g_z (s*t, l), norms (s)): the masked residual norm ||y - mask * forward(data)||
        per sample and its gradient w.r.t. the un-normalised latent rows, in bounded
        memory (SIRENAutodecoder_film.dense_grad)."""
        return self.model.dense_grad(self.coords, self._rows(data), data.shape[2], measurement, mask,
                                     self.x_normalizer, self.y_normalizer, budget)


@register_operator(name="case2")
class Case2Operator(_SirenFieldOperator):
    """measurements.py:58-97: a full 2-D field (2 coordinates -> 4 outputs) times a
    ``mask`` keyword.  The reference hard-codes SIRENAutodecoder_film(2, 256, 4, 10,
    256); here the dimensions are read from the checkpoint.  The normalisers are the
    reference's constants."""

    _name = "Case2"

    def __init__(self, device, ckpt_path, max_val, min_val, coords, batch_size):
        self.device = device
        self.coords = torch.tensor(coords, dtype=torch.float32, device=device)
        self.x_normalizer = Normalizer_ts(method="-11", dim=0,
                                          params=[torch.tensor([1., 1.], device=device),
                                                  torch.tensor([0., 0.], device=device)])
        self.y_normalizer = Normalizer_ts(method="-11", dim=0,
                                          params=[torch.tensor([[0.9617, 0.2666, 0.2869, 0.0290]], device=device),
                                                  torch.tensor([[-0.0051, -0.2073, -0.2619, -0.0419]], device=device)])
        self._load_model(ckpt_path, 2, 4, device)
        self.max_val = torch.from_numpy(max_val).to(device)
        self.min_val = torch.from_numpy(min_val).to(device)
        self.batch_size = batch_size

    def forward(self, data, mask=None, **kwargs):
        """mask * fields; without a mask the fields themselves (the reference fails on
        ``None * fields``)."""
        out = self._fields(data)
        return out if mask is None else torch.as_tensor(mask).to(device=out.device, dtype=out.dtype) * out


@register_operator(name="case3")
class Case3Operator(_SirenFieldOperator):
    """measurements.py:99-137: sensors on the periodic hill (2 -> 2)."""

    _name = "Case3"

    def __init__(self, device, coords, batch_size, max_val, min_val, normalizer_params_path, ckpt_path) -> None:
        self.device = device
        self.coords = torch.tensor(coords, dtype=torch.float32, device=device)
        params = torch.load(normalizer_params_path, weights_only=True, map_location="cpu")
        x_ub, x_lb = params["x_normalizer_params"]
        y_ub, y_lb = params["y_normalizer_params"]
        cin_size, cout_size = 2, 2
        self.x_normalizer = Normalizer_ts(method="-11", dim=0, params=(x_ub, x_lb))
        self.y_normalizer = Normalizer_ts(method="-11", dim=0, params=(y_ub[:cout_size], y_lb[:cout_size]))
        self._load_model(ckpt_path, cin_size, cout_size, device)
        self.max_val = torch.from_numpy(max_val).to(device)
        self.min_val = torch.from_numpy(min_val).to(device)
        self.batch_size = batch_size

    def forward(self, data, mask=None, **kwargs):
        out = self._fields(data)
        return out if mask is None else torch.as_tensor(mask).to(device=out.device, dtype=out.dtype) * out


@register_operator(name="case3_gappy")
class Case3Operator_gappy(Case3Operator):
    """measurements.py:139-181: Case3 with one velocity component blanked per sensor
    group -- channel 1 for the first 10 sensors, channel 0 for the rest (:179-180),
    kept here as a (Ns, c) 0/1 table.  The reference's forward hands its arguments
    to pass_through_model_batch in the wrong order (batch_size where the x normaliser
    belongs) and cannot run; this builds its evident intent: Case3's fields with
    those entries set to zero."""

    _name = "Case3 (gappy)"
    GAP = 10   # sensors whose channel 1 is blanked

    def default_mask(self):
        m = torch.ones(self.coords.shape[0], self.model.out_features, dtype=torch.float32, device=self.coords.device)
        m[:self.GAP, 1] = 0.
        m[self.GAP:, 0] = 0.
        return m

    def forward(self, data, mask=None, **kwargs):
        out = self._fields(data) * self.default_mask()
        return out if mask is None else torch.as_tensor(mask).to(device=out.device, dtype=out.dtype) * out


@register_operator(name="case4")
class Case4Operator(_SirenFieldOperator):
    """measurements.py:184-226.  The reference hard-codes SIRENAutodecoder_film(3,
    384, 3, 15, 384); here the dimensions are read from the checkpoint (identical
    for the reference's checkpoint, and usable for others)."""

    _name = "Case4"

    def __init__(self, device, coords_path, batch_size, max_val_path, min_val_path, normalizer_params_path,
                 ckpt_path) -> None:
        self.device = device
        coords = np.load(coords_path)
        self.coords = torch.tensor(coords, dtype=torch.float32, device=device)
        params = torch.load(normalizer_params_path, weights_only=True, map_location="cpu")
        x_uub, x_llb = params["x_normalizer_params"]
        y_uub, _ = params["y_normalizer0u_params"]
        _, y_llb = params["y_normalizer0l_params"]
        cin_size, cout_size = 3, 3
        self.x_normalizer = Normalizer_ts(method="-11", dim=0, params=(x_uub, x_llb))
        self.y_normalizer = Normalizer_ts(method="-11", dim=0, params=(y_uub[:cout_size], y_llb[:cout_size]))
        self._load_model(ckpt_path, cin_size, cout_size, device)
        self.max_val = torch.from_numpy(np.load(max_val_path)).to(device)
        self.min_val = torch.from_numpy(np.load(min_val_path)).to(device)
        self.batch_size = batch_size

    # the 10-sensor adjoint: the whole tape in memory (cfd_siren_tape_forward / _vjp)
    def forward_tape(self, data):
        return self.model.tape_forward(self.coords, self._rows(data), self.x_normalizer, self.y_normalizer)

    def vjp(self, g_out):
        """gradient w.r.t. the un-normalised latent rows of the last forward_tape."""
        return self.model.tape_vjp(g_out)


@register_operator(name="sensor_stencil")
class SensorStencilOperator(_SirenFieldOperator):
    """Linear stencils on the decoded value and its exact coordinate Jacobian at Ns
    sensors (no reference counterpart): M readings per sensor,

        A[r, s, m] = sum_o wv[s, m, o] out[r, s, o] + sum_{o,k} wj[s, m, o, k] jac[r, s, o, k]

    with ``value_weights`` (M, c) or per sensor (Ns, M, c) and ``jac_weights`` (M, c, d)
    or (Ns, M, c, d); at least one of the two (confild_amd.guided.stencils builds
    divergence, vorticity, directional-derivative and plain-value weights).  out and
    jac are decode_jacobian's, in physical units.  The DPS sampler runs its adjoint
    through the Jacobian tape (cfd_siren_jtape_forward / _vjp, cfd_dps_residual_linear).
    A sensor or reading is switched off with a zero weight row; a ``mask`` keyword
    is refused."""

    _name = "SensorStencil"

    def __init__(self, device, coords_path, batch_size, max_val_path, min_val_path, normalizer_params_path,
                 ckpt_path, value_weights=None, jac_weights=None) -> None:
        """Case4Operator's files (the SIREN's dimensions come from the checkpoint) and the
        two weight arrays."""
        self.device = device
        self.coords = torch.tensor(np.load(coords_path), dtype=torch.float32, device=device)
        params = torch.load(normalizer_params_path, weights_only=True, map_location="cpu")
        x_uub, x_llb = params["x_normalizer_params"]
        y_uub, _ = params["y_normalizer0u_params"]
        _, y_llb = params["y_normalizer0l_params"]
        sd = torch.load(ckpt_path, weights_only=True, map_location="cpu")["model_state_dict"]
        cin_size, _, cout_size, _, _ = _siren_dims(sd)
        self.x_normalizer = Normalizer_ts(method="-11", dim=0, params=(x_uub, x_llb))
        self.y_normalizer = Normalizer_ts(method="-11", dim=0, params=(y_uub[:cout_size], y_llb[:cout_size]))
        self._load_model(ckpt_path, cin_size, cout_size, device)
        self.max_val = torch.from_numpy(np.load(max_val_path)).to(device)
        self.min_val = torch.from_numpy(np.load(min_val_path)).to(device)
        self.batch_size = batch_size
        self._set_weights(value_weights, jac_weights)

    @classmethod
    def from_parts(cls, device, coords, x_normalizer, y_normalizer, model, max_val, min_val, batch_size=384,
                   value_weights=None, jac_weights=None):
        op = super().from_parts(device, coords, x_normalizer, y_normalizer, model, max_val, min_val, batch_size)
        op._set_weights(value_weights, jac_weights)
        return op

    def _set_weights(self, value_weights, jac_weights):
        if value_weights is None and jac_weights is None:
            raise ValueError("SensorStencil needs value_weights, jac_weights or both")
        Ns, c, d = self.coords.shape[0], self.model.out_features, self.model.in_coord_features
        self.wv = self.wj = None
        self.wv_per_sensor = self.wj_per_sensor = False
        M = None
        for name, w, tail in (("value_weights", value_weights, (c,)), ("jac_weights", jac_weights, (c, d))):
            if w is None:
                continue
            w = torch.as_tensor(w, dtype=torch.float32)
            shared, per = ("M",) + tail, (Ns, "M") + tail
            if w.dim() == len(shared) and tuple(w.shape[1:]) == tail:
                per_sensor, m = False, w.shape[0]
            elif w.dim() == len(per) and w.shape[0] == Ns and tuple(w.shape[2:]) == tail:
                per_sensor, m = True, w.shape[1]
            else:
                raise ValueError(f"{name} of shape {tuple(w.shape)} is neither {shared} nor {per}")
            if m < 1 or (M is not None and m != M):
                raise ValueError(f"{name} has {m} readings per sensor, expected {M if M is not None else 'at least 1'}")
            M = m
            w = w.to(self.coords.device).contiguous()
            if name == "value_weights":
                self.wv, self.wv_per_sensor = w, per_sensor
            else:
                self.wj, self.wj_per_sensor = w, per_sensor
        self.readings = M

    def residual(self, out, jac, y, B, norm_out=None, want_A=False):
        """cfd_dps_residual_linear on (out (R, Ns, c), jac (R, Ns, c, d)): the B per-sample
        norms ||y - A||, g_out and g_jac (None without the weight set), and A (R, Ns, M)
        when asked for.  y: one sample's (T, Ns, M) readings or the batch's (R, Ns, M)."""
        _require_gpu(out)
        R, Ns, c = out.shape
        d, M = self.model.in_coord_features, self.readings
        if R % B:
            raise ValueError(f"{R} rows do not split into {B} samples")
        per = (R // B) * Ns * M
        if y.numel() not in (per, per * B):
            raise ValueError(f"measurement of {y.numel()} values matches neither one sample ({per}) "
                             f"nor the batch ({per * B})")
        y = y.to(device=out.device, dtype=torch.float32).contiguous()
        g_out = torch.empty_like(out) if self.wv is not None else None
        g_jac = torch.empty_like(jac) if self.wj is not None else None
        norm = norm_out if norm_out is not None else torch.empty(B, dtype=torch.float32, device=out.device)
        A = torch.empty((R, Ns, M), dtype=torch.float32, device=out.device) if want_A else None
        _lib.check(_lib.lib().cfd_dps_residual_linear(
            _lib.ptr(y), int(y.numel() == per * B and B > 1), _lib.ptr(out), _lib.ptr(jac), _lib.ptr(self.wv),
            int(self.wv_per_sensor), _lib.ptr(self.wj), int(self.wj_per_sensor), _lib.ptr(g_out), _lib.ptr(g_jac),
            _lib.ptr(norm), _lib.ptr(A), Ns, M, c, d, R // B, B, _lib.stream_of(out.device)),
            "cfd_dps_residual_linear")
        return norm, g_out, g_jac, A

    def forward(self, data, **kwargs):
        """(s, 1, t, l) latents in [-1, 1] -> (s*t, Ns, M) readings: decode_jacobian at the
        sensors and the stencil contraction (cfd_dps_residual_linear's A)."""
        if kwargs.get("mask") is not None:
            raise NotImplementedError(_STENCIL_MASK)
        with torch.no_grad():
            out, jac = self.model.decode_jacobian(self.coords, self._rows(data)[:, None], self.x_normalizer,
                                                  self.y_normalizer)
        R = out.shape[0]
        zero = torch.zeros((R, self.coords.shape[0], self.readings), dtype=torch.float32, device=out.device)
        return self.residual(out.contiguous(), jac.contiguous(), zero, 1, want_A=True)[3]

    # the adjoint: the whole Jacobian tape in memory (cfd_siren_jtape_forward / _vjp)
    def forward_tape(self, data):
        return self.model.jac_tape_forward(self.coords, self._rows(data), self.x_normalizer, self.y_normalizer)

    def vjp(self, g_out=None, g_jac=None):
        """gradient w.r.t. the un-normalised latent rows of the last forward_tape."""
        return self.model.jac_tape_vjp(g_out, g_jac)


class _StencilReadings:
    """A (R, n, M) of cfd_dps_residual_linear for point batches [n0, n1) of an operator's
    stencils.  The call also wants a target and writes the residual's gradients: a
    zero target and two scratch buffers, allocated once for the largest batch."""

    def __init__(self, op, R, step):
        c, d, dev = op.model.out_features, op.model.in_coord_features, op.coords.device
        self.op, self.R, self.M, self.c, self.d = op, R, op.readings, c, d
        self.zero = torch.zeros(R * step * self.M, dtype=torch.float32, device=dev)
        self.A = torch.empty(R * step * self.M, dtype=torch.float32, device=dev)
        self.g_out = torch.empty(R * step * c, dtype=torch.float32, device=dev) if op.wv is not None else None
        self.g_jac = torch.empty(R * step * c * d, dtype=torch.float32, device=dev) if op.wj is not None else None
        self.norm = torch.empty(1, dtype=torch.float32, device=dev)

    def __call__(self, out, jac, n0, n1):
        op, n = self.op, n1 - n0
        wv = op.wv[n0:n1].contiguous() if op.wv_per_sensor else op.wv
        wj = op.wj[n0:n1].contiguous() if op.wj_per_sensor else op.wj
        out, jac = out.contiguous(), jac.contiguous()
        _lib.check(_lib.lib().cfd_dps_residual_linear(
            _lib.ptr(self.zero), 0, _lib.ptr(out), _lib.ptr(jac), _lib.ptr(wv), int(op.wv_per_sensor), _lib.ptr(wj),
            int(op.wj_per_sensor), _lib.ptr(self.g_out), _lib.ptr(self.g_jac), _lib.ptr(self.norm), _lib.ptr(self.A),
            n, self.M, self.c, self.d, self.R, 1, _lib.stream_of(out.device)), "cfd_dps_residual_linear")
        return self.A[:self.R * n * self.M].reshape(self.R, n, self.M)


_STENCIL_MASK = ("the 'sensor_stencil' operator takes no mask keyword: switch a sensor or a reading off with a "
                 "zero weight row")


@register_operator(name="dense_stencil")
class DenseStencilOperator(_SirenFieldOperator):
    """SensorStencilOperator's readings at every point of a whole field (no reference
    counterpart): M linear stencils per point on the decoded value and its exact
    coordinate Jacobian,

        A[r, n, m] = sum_o wv[n, m, o] out[r, n, o] + sum_{o,k} wj[n, m, o, k] jac[r, n, o, k]

    with ``value_weights`` (M, c) or per point (N, M, c) and ``jac_weights`` (M, c, d) or
    (N, M, c, d).  Where 'sensor_stencil' keeps the whole Jacobian tape in memory, the DPS
    sampler runs this operator's adjoint in bounded memory (``dense_grad``:
    cfd_siren_jdense_grad), so N may be the whole mesh: a measured
    vorticity field, divergence-free guidance at every collocation point (a zero
    measurement), or, with per-point weights, value sensors at a few points and a
    derivative reading at all of them.  A ``mask`` keyword (tables of (N, M)) works as
    for case2 / case3.  It has no forward_tape / vjp."""

    _name = "DenseStencil"

    # SensorStencilOperator's constructor files, weight arrays and weight checks
    __init__ = SensorStencilOperator.__init__
    _set_weights = SensorStencilOperator._set_weights

    @classmethod
    def from_parts(cls, device, coords, x_normalizer, y_normalizer, model, max_val, min_val, batch_size=384,
                   value_weights=None, jac_weights=None):
        op = super().from_parts(device, coords, x_normalizer, y_normalizer, model, max_val, min_val, batch_size)
        op._set_weights(value_weights, jac_weights)
        return op

    def _y_normalizer_at(self, n0, n1):
        """The y normaliser of points [n0, n1): a per-point (N, c) table is sliced."""
        yn, N, c = self.y_normalizer, self.coords.shape[0], self.model.out_features
        if yn is None or yn.method != "-11" or yn.params[0].numel() != N * c or N == 1:
            return yn
        return Normalizer_ts(method="-11", dim=0, params=tuple(p.reshape(N, c)[n0:n1] for p in yn.params[:2]))

    def forward(self, data, mask=None, **kwargs):
        """(s, 1, t, l) latents in [-1, 1] -> (s*t, N, M) readings (times ``mask``):
        decode_jacobian and the stencil contraction (cfd_dps_residual_linear's A) in
        batches of ``batch_size`` points, so the Jacobian of the whole field is never
        held at once."""
        _require_gpu(data)
        rows = self._rows(data)
        R, N, M = rows.shape[0], self.coords.shape[0], self.readings
        A = torch.empty((R, N, M), dtype=torch.float32, device=rows.device)
        step = max(1, min(N, int(self.batch_size)))
        readings = _StencilReadings(self, R, step)
        for n0 in range(0, N, step):
            n1 = min(N, n0 + step)
            with torch.no_grad():
                out, jac = self.model.decode_jacobian(self.coords[n0:n1], rows[:, None], self.x_normalizer,
                                                      self._y_normalizer_at(n0, n1))
            A[:, n0:n1] = readings(out, jac, n0, n1)
        return A if mask is None else torch.as_tensor(mask).to(device=A.device, dtype=A.dtype) * A

    # -- adjoint used by the DPS sampler ----------------------------------------
    def dense_grad(self, data, measurement, mask=None, budget=None):
        """(g_z (s*t, l), norms (s)): ||y - mask * forward(data)|| per sample and its gradient
        w.r.t. the un-normalised latent rows, in bounded memory
        (SIRENAutodecoder_film.jac_dense_grad).  ``measurement`` None: a zero target."""
        _require_gpu(data)
        return self.model.jac_dense_grad(self.coords, self._rows(data), data.shape[2], measurement, self.wv, self.wj,
                                         mask, self.x_normalizer, self.y_normalizer, budget)


# =============
# Noise classes
# =============
__NOISE__ = {}


def register_noise(name: str):
    def wrapper(cls):
        if __NOISE__.get(name, None):
            raise NameError(f"Name {name} is already defined!")
        __NOISE__[name] = cls
        return cls
    return wrapper


def get_noise(name: str, **kwargs):
    """measurements.py:242-247."""
    if __NOISE__.get(name, None) is None:
        raise NameError(f"Name {name} is not defined.")
    noiser = __NOISE__[name](**kwargs)
    noiser.__name__ = name
    return noiser


class Noise(ABC):
    def __call__(self, data):
        return self.forward(data)

    @abstractmethod
    def forward(self, data):
        pass


@register_noise(name="clean")
class Clean(Noise):
    def forward(self, data):
        return data


@register_noise(name="gaussian")
class GaussianNoise(Noise):
    def __init__(self, sigma):
        self.sigma = sigma

    def forward(self, data):
        return data + torch.randn_like(data, device=data.device) * self.sigma


def _require_gpu(t):
    if t.device.type != "cuda":
        raise _lib.CfdError("the DPS path runs on the GPU only")
