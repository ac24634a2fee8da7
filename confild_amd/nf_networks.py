"""SIRENAutodecoder_film drop-in (N/cnf/nf_networks.py:443-495) on the fused HIP kernel.

Parameter tree and state_dict keys are the reference's (``net1.{i}.weight``,
``net1.{i}.bias``, ``net2.{i}.weight``), so ``checkpoint_*.pt["model_state_dict"]``
loads unchanged.  ``forward(coords, latents)`` keeps the reference signature and
broadcasting; ``decode(...)`` additionally fuses the coordinate normaliser and the
output de-normaliser (Normalizer_ts '-11') into the same launch.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib

DEFAULT_W0 = 30.0  # N/cnf/initialization.py:5


class BatchLinear(nn.Linear):
    """Parameter holder with the reference layout (components.py:55-76).  Its
    arithmetic runs inside the fused SIREN kernel, never here."""

    def forward(self, input, params=None):
        raise _lib.CfdError("BatchLinear is evaluated inside the fused HIP SIREN kernel; call the network instead")


def _sine_init(m, w0=DEFAULT_W0):
    with torch.no_grad():
        n = m.weight.size(-1)
        m.weight.uniform_(-math.sqrt(6 / n) / w0, math.sqrt(6 / n) / w0)   # initialization.py:117-125


def _first_layer_sine_init(m):
    with torch.no_grad():
        n = m.weight.size(-1)
        m.weight.uniform_(-1 / n, 1 / n)                                     # initialization.py:127-132


def latent_grad_flops(d, L, c, nh, H, rows, points):
    """FLOPs of the DPS operator's SIREN part as FlopCounterMode counts the
    reference (measurements.py:219-226 under condition_methods.py:31-47): the
    forward at ``rows`` latent rows x ``points`` sensor coordinates -- the FiLM
    products (nh + 1) x (L -> H) per row, the first coordinate layer once per
    point (the reference broadcasts it over the rows), 2(nh H^2 + Hc) per (row,
    point) pair -- and autograd's backward to the latents only: every hidden and the
    output layer's input-gradient per pair, and the FiLM products' latent gradient
    per row.  Returns {"forward", "backward"}.  Pinned against FlopCounterMode on
    the CPU oracle (tests/test_host.py)."""
    film = 2 * (nh + 1) * H * L * rows
    fwd = 2 * d * H * points + 2 * (nh * H * H + H * c) * rows * points + film
    bwd = 2 * (nh * H * H + H * c) * rows * points + film
    return {"forward": fwd, "backward": bwd}


JACOBIAN_COMPUTE = ("f32", "split_f16")                 # decode_jacobian(compute=...)
JACOBIAN_SPLIT_WIDTHS = tuple(32 * k for k in (1, 2, 3, 4, 6, 8, 12))


def jacobian_split_refusal(d, nh, H):
    """Why decode_jacobian(compute="split_f16") refuses a network of ``d`` coordinate
    features, ``nh`` hidden layers of width ``H`` (the rule of
    cfd_siren_forward_jacobian_split, no library call), or None when it runs."""
    if not 1 <= d <= 3:
        return f"in_coord_features must be 1..3, got {d} (the 1 + d chains of a point share 4 MFMA columns)"
    if nh < 1:
        return f"num_hidden_layers must be >= 1, got {nh} (no hidden product to run on f16 MFMA)"
    if H % 32:
        return f"hidden_features must be a multiple of 32, got {H} (32-feature K-chunks of the f16 MFMA)"
    if H not in JACOBIAN_SPLIT_WIDTHS:
        return f"hidden_features must be one of {list(JACOBIAN_SPLIT_WIDTHS)}, got {H}"
    if 4 * (2 * (H // 16) * 256 + (nh + 1) * H + 4 * H) > 160 * 1024:
        return f"{nh} hidden layers of width {H} are too deep for the LDS staging (160 KiB)"
    return None


def jacobian_split_supported(d, nh, H):
    """True when decode_jacobian(compute="split_f16") takes these widths."""
    return jacobian_split_refusal(d, nh, H) is None


HESSIAN_COMPUTE = JACOBIAN_COMPUTE                      # decode_hessian(compute=...)


def hessian_split_refusal(d, nh, H):
    """Why decode_hessian(compute="split_f16") refuses a network of ``d`` coordinate
    features, ``nh`` hidden layers of width ``H`` (the rule of
    cfd_siren_forward_hessian_split, no library call), or None when it runs.  K14s
    takes K13s's widths with K13s's LDS staging, so this is jacobian_split_refusal's
    rule (the value, tangent and second-order chains of a point share 16 MFMA columns)."""
    if not 1 <= d <= 3:
        return (f"in_coord_features must be 1..3, got {d} (the value, tangent and second-order chains of a point "
                "share 16 MFMA columns)")
    return jacobian_split_refusal(d, nh, H)


def hessian_split_supported(d, nh, H):
    """True when decode_hessian(compute="split_f16") takes these widths."""
    return hessian_split_refusal(d, nh, H) is None


class SIRENAutodecoder_film(nn.Module):
    """Constructor as nf_networks.py:447-478 (sine nonlinearity, no premap)."""

    def __init__(self, in_coord_features, in_latent_features, out_features, num_hidden_layers, hidden_features,
                 outermost_linear=False, nonlinearity="sine", weight_init=None, bias_init=None, premap_mode=None,
                 **kwargs):
        super().__init__()
        if nonlinearity != "sine":
            raise NotImplementedError(f"nonlinearity {nonlinearity!r}: the fused kernel implements sine only")
        if premap_mode is not None:
            raise NotImplementedError("premap_mode (FeatureMapping) is not used by any CoNFiLD recipe")
        self.in_coord_features = in_coord_features
        self.in_latent_features = in_latent_features
        self.out_features = out_features
        self.num_hidden_layers = num_hidden_layers
        self.hidden_features = hidden_features
        self.w0 = DEFAULT_W0
        self.net1 = nn.ModuleList([BatchLinear(in_coord_features, hidden_features)]
                                  + [BatchLinear(hidden_features, hidden_features) for _ in range(num_hidden_layers)]
                                  + [BatchLinear(hidden_features, out_features)])
        self.net2 = nn.ModuleList([BatchLinear(in_latent_features, hidden_features, bias=False)
                                   for _ in range(num_hidden_layers + 1)])
        init = weight_init or _sine_init
        self.net1.apply(lambda m: init(m) if isinstance(m, BatchLinear) else None)
        self.net2.apply(lambda m: init(m) if isinstance(m, BatchLinear) else None)
        _first_layer_sine_init(self.net1[0])
        _first_layer_sine_init(self.net2[0])
        if bias_init is not None:
            self.net2.apply(bias_init)
        self._handles = {}
        self._compute = None  # None: the library default (CFD_SIREN_SPLIT_F16 where H % 32 == 0)

    COMPUTE_MODES = {"f32": 0, "split_f16": 1}

    def set_compute(self, mode: str):
        """Hidden-layer arithmetic of the fused decoder: "split_f16" (3 f16 MFMAs on
        two-term splits, fp32-level error; the default) or "f32" (exact fp32 MFMA)."""
        if mode not in self.COMPUTE_MODES:
            raise ValueError(f"compute mode {mode!r} not in {sorted(self.COMPUTE_MODES)}")
        self._compute = mode
        return self

    def compute_mode(self, device) -> str:
        """The mode a decode on `device` actually runs (split_f16 falls back to f32
        when H % 32 != 0 or there is no hidden layer)."""
        v = C.c_int()
        _lib.check(_lib.load().cfd_siren_get_compute(self._handle(device), C.byref(v)), "cfd_siren_get_compute")
        return {v_: k for k, v_ in self.COMPUTE_MODES.items()}[v.value]

    # -- device handle --------------------------------------------------------
    def prepare(self, device=None):
        """Upload and pack the parameters into the device handle now (the first
        decode does it otherwise).  Returns self."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.CfdError("SIRENAutodecoder_film.prepare needs a GPU device")
        self._handle(dev)
        return self

    def _signature(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _handle(self, device):
        lib = _lib.lib()
        dev = device.index if device.index is not None else torch.cuda.current_device()
        entry = self._handles.get(dev)
        if entry is None:
            cfg = _lib.SirenCfg(self.in_coord_features, self.in_latent_features, self.out_features,
                                self.num_hidden_layers, self.hidden_features, self.w0)
            h = C.c_void_p()
            _lib.check(lib.cfd_siren_create(C.byref(cfg), dev, C.byref(h)), "cfd_siren_create")
            entry = [h, None]
            self._handles[dev] = entry
        sig = self._signature()
        if entry[1] != sig:
            for k, p in self.named_parameters():
                host = p.detach().to("cpu", torch.float32).contiguous()
                _lib.check(lib.cfd_siren_set_param(entry[0], k.encode(), C.c_void_p(host.data_ptr()), host.numel()),
                           f"siren set_param {k}")
            _lib.check(lib.cfd_siren_ready(entry[0]), "cfd_siren_ready")
            entry[1] = sig
        if self._compute is not None:
            _lib.check(lib.cfd_siren_set_compute(entry[0], self.COMPUTE_MODES[self._compute]), "cfd_siren_set_compute")
        return entry[0]

    # -- forward ----------------------------------------------------------------
    @staticmethod
    def _flatten(coords, latents, d, L):
        if coords.shape[-1] != d:
            raise ValueError(f"coords last dim {coords.shape[-1]} != in_coord_features {d}")
        if latents.shape[-1] != L:
            raise ValueError(f"latents last dim {latents.shape[-1]} != in_latent_features {L}")
        spatial = tuple(coords.shape[:-1])
        # reference broadcasting: coords (1, N, d) x latents (b, 1, L) -> (b, N, c);
        # coords (h, w, d) x latents (b, 1, 1, L) -> (b, h, w, c)
        if latents.dim() >= 2 and any(s != 1 for s in latents.shape[1:-1]):
            raise NotImplementedError("latents must be (b, 1, ..., 1, L): one latent per output field")
        if len(spatial) == latents.dim() - 1 and len(spatial) > 1 and spatial[0] == 1:
            spatial = spatial[1:]
        b = latents.shape[0] if latents.dim() >= 2 else 1
        return coords.reshape(-1, d), latents.reshape(b, L), spatial

    def _dev_param(self, t, dev):
        """fp32 device copy of a (usually host) normaliser parameter, cached while the
        source tensor is unchanged: a host-to-device copy from pageable memory waits for
        the stream, which in the DPS step would idle the GPU between the U-Net forward
        and the SIREN tape (4 such copies per step before the cache)."""
        if t.device == dev and t.dtype == torch.float32:
            return t
        cache = self.__dict__.setdefault("_norm_dev_cache", {})
        key = (id(t), dev)
        hit = cache.get(key)
        if hit is not None and hit[0] is t and hit[1] == t._version:
            return hit[2]
        v = t.to(device=dev, dtype=torch.float32)
        cache.pop(key, None)
        cache[key] = (t, t._version, v)
        while len(cache) > self._NORM_CACHE_MAX:   # bounded: callers may build new normalisers per call
            cache.pop(next(iter(cache)))
        return v

    _NORM_CACHE_MAX = 8   # (max, min) of the coordinate and output normalisers, two devices

    def _norm_args(self, cf, N, dev, x_normalizer, y_normalizer):
        """Fusable '-11' normaliser bounds -> (coords, xmax, xmin, ymax, ymin, ystride, post)."""
        d, c = self.in_coord_features, self.out_features
        xmax = xmin = ymax = ymin = None
        ystride = 0
        if x_normalizer is not None:
            if x_normalizer.method != "-11":
                cf = x_normalizer.normalize(cf).contiguous()
            else:
                xmax = self._dev_param(x_normalizer.params[0], dev).reshape(-1).contiguous()
                xmin = self._dev_param(x_normalizer.params[1], dev).reshape(-1).contiguous()
                if xmax.numel() != d:
                    raise ValueError("coordinate normaliser must have one (max, min) per coordinate feature")
        post = None
        if y_normalizer is not None:
            if y_normalizer.method != "-11":
                post = y_normalizer
            else:
                ymax = self._dev_param(y_normalizer.params[0], dev)
                ymin = self._dev_param(y_normalizer.params[1], dev)
                if ymax.numel() == c:
                    ystride = 0
                elif ymax.numel() == N * c:
                    ystride = c
                else:
                    raise ValueError(f"output normaliser params of {ymax.numel()} values match neither (c) nor (N, c)")
                ymax = ymax.reshape(-1).contiguous()
                ymin = ymin.reshape(-1).contiguous()
        return cf, xmax, xmin, ymax, ymin, ystride, post

    def decode(self, coords, latents, x_normalizer=None, y_normalizer=None, out=None):
        """denorm(NF(norm(coords), latents)) in one fused launch (trainer.infer,
        N/scripts/train.py:265-279; pass_through_model_batch, inference_function.py:22-48).
        ``out``: a contiguous fp32 (b, N, c) tensor the fields are written into (e.g.
        a row slice of a larger batch; fused '-11' output normalisers only)."""
        d, L, c = self.in_coord_features, self.in_latent_features, self.out_features
        dev = latents.device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN decode needs GPU tensors (the HIP path has no CPU fallback)")
        if latents.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("torch autograd does not run through the HIP SIREN: use tape_forward + "
                                      "tape_vjp (the DPS sampler in confild_amd.guided does)")
        cf, lat, spatial = self._flatten(coords, latents, d, L)
        cf = cf.to(device=dev, dtype=torch.float32).contiguous()
        lat = lat.detach().to(torch.float32).contiguous()
        N = cf.shape[0]
        cf, xmax, xmin, ymax, ymin, ystride, post = self._norm_args(cf, N, dev, x_normalizer, y_normalizer)
        h = self._handle(dev)
        b = lat.shape[0]
        nbytes = C.c_size_t()
        lib = _lib.load()
        _lib.check(lib.cfd_siren_workspace_bytes(h, b, C.byref(nbytes)), "siren workspace")
        ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty((b, N, c), dtype=torch.float32, device=dev)
        elif (tuple(out.shape) != (b, N, c) or out.dtype != torch.float32 or not out.is_contiguous()
              or out.device != dev or post is not None):
            raise ValueError(f"out must be a contiguous fp32 ({b}, {N}, {c}) tensor on {dev} (fused '-11' output "
                             f"normaliser only)")
        _lib.check(lib.cfd_siren_forward(h, _lib.ptr(cf), N, _lib.ptr(lat), b, _lib.ptr(xmax), _lib.ptr(xmin),
                                         _lib.ptr(ymax), _lib.ptr(ymin), ystride, _lib.ptr(out), _lib.ptr(ws),
                                         ws.numel(), _lib.stream_of(dev)), "cfd_siren_forward")
        if post is not None:
            out = post.denormalize(out)
        return out.reshape((b,) + spatial + (c,))

    # -- value and coordinate Jacobian (K13: cfd_siren_forward_jacobian) ------------
    def decode_jacobian(self, coords, latents, x_normalizer=None, y_normalizer=None, compute=None):
        """decode() together with its exact spatial derivatives, one fused launch:
        returns (out (b, *spatial, c), jac (b, *spatial, c, d)) with jac[..., o, k] =
        d out[..., o] / d coords[..., k], both in physical units (the chain rule through
        the normalisers is applied).  Broadcasting as decode().  Only '-11' normalisers
        (fused).  ``compute``: None or "f32", the exact fp32 chain (K13), whatever
        set_compute chose; "split_f16", the same chain on the f16 matrix pipes with
        fp32-level accuracy (K13s, cfd_siren_forward_jacobian_split), for the widths
        jacobian_split_supported() names -- any other width is a CfdError, never a
        fall-back."""
        if compute not in (None,) + JACOBIAN_COMPUTE:
            raise ValueError(f"compute must be None or one of {list(JACOBIAN_COMPUTE)}, got {compute!r}")
        d, L, c = self.in_coord_features, self.in_latent_features, self.out_features
        dev = latents.device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN decode_jacobian needs GPU tensors (the HIP path has no CPU fallback)")
        cf, lat, spatial = self._flatten(coords, latents, d, L)
        cf = cf.to(device=dev, dtype=torch.float32).contiguous()
        lat = lat.detach().to(torch.float32).contiguous()
        N, b = cf.shape[0], lat.shape[0]
        cf, xmax, xmin, ymax, ymin, ystride, post = self._norm_args(cf, N, dev, x_normalizer, y_normalizer)
        if post is not None or (x_normalizer is not None and xmax is None):
            raise NotImplementedError("the SIREN coordinate Jacobian fuses '-11' normalisers only")
        h, lib = self._handle(dev), _lib.load()
        nbytes = C.c_size_t()
        _lib.check(lib.cfd_siren_jacobian_workspace_bytes(h, b, C.byref(nbytes)), "siren jacobian workspace")
        ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dev)
        out = torch.empty((b, N, c), dtype=torch.float32, device=dev)
        jac = torch.empty((b, N, c, d), dtype=torch.float32, device=dev)
        name = "cfd_siren_forward_jacobian_split" if compute == "split_f16" else "cfd_siren_forward_jacobian"
        _lib.check(getattr(lib, name)(h, _lib.ptr(cf), N, _lib.ptr(lat), b, _lib.ptr(xmax), _lib.ptr(xmin),
                                      _lib.ptr(ymax), _lib.ptr(ymin), ystride, _lib.ptr(out), _lib.ptr(jac),
                                      _lib.ptr(ws), ws.numel(), _lib.stream_of(dev)), name)
        return out.reshape((b,) + spatial + (c,)), jac.reshape((b,) + spatial + (c, d))

    # -- value, Jacobian and coordinate Hessian (K14: cfd_siren_forward_hessian) ------
    def decode_hessian(self, coords, latents, x_normalizer=None, y_normalizer=None, diag=False, compute=None):
        """decode_jacobian() together with the exact second spatial derivatives, one
        fused launch: returns (out, jac, hess) with hess (b, *spatial, c, d, d),
        hess[..., o, k, l] = d2 out[..., o] / d coords[..., k] d coords[..., l] in
        physical units, symmetric to the bit; ``diag=True`` returns (b, *spatial, c, d),
        the unmixed derivatives alone (all a Laplacian needs: half the columns at d = 3).
        Broadcasting and normalisers as decode_jacobian().  ``compute``: None or "f32",
        the exact fp32 chain (K14), whatever set_compute chose; "split_f16", the same
        chain on the f16 matrix pipes with fp32-level accuracy (K14s,
        cfd_siren_forward_hessian_split; the handle's compute mode is left alone), for
        the widths hessian_split_supported() names -- any other width is a CfdError,
        never a fall-back."""
        if compute not in (None,) + HESSIAN_COMPUTE:
            raise ValueError(f"compute must be None or one of {list(HESSIAN_COMPUTE)}, got {compute!r}")
        d, L, c = self.in_coord_features, self.in_latent_features, self.out_features
        dev = latents.device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN decode_hessian needs GPU tensors (the HIP path has no CPU fallback)")
        cf, lat, spatial = self._flatten(coords, latents, d, L)
        cf = cf.to(device=dev, dtype=torch.float32).contiguous()
        lat = lat.detach().to(torch.float32).contiguous()
        N, b = cf.shape[0], lat.shape[0]
        cf, xmax, xmin, ymax, ymin, ystride, post = self._norm_args(cf, N, dev, x_normalizer, y_normalizer)
        if post is not None or (x_normalizer is not None and xmax is None):
            raise NotImplementedError("the SIREN coordinate Hessian fuses '-11' normalisers only")
        h, lib = self._handle(dev), _lib.load()
        nbytes = C.c_size_t()
        _lib.check(lib.cfd_siren_hessian_workspace_bytes(h, b, C.byref(nbytes)), "siren hessian workspace")
        ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dev)
        hshape = (c, d) if diag else (c, d, d)
        out = torch.empty((b, N, c), dtype=torch.float32, device=dev)
        jac = torch.empty((b, N, c, d), dtype=torch.float32, device=dev)
        hess = torch.empty((b, N) + hshape, dtype=torch.float32, device=dev)
        name = "cfd_siren_forward_hessian_split" if compute == "split_f16" else "cfd_siren_forward_hessian"
        _lib.check(getattr(lib, name)(h, _lib.ptr(cf), N, _lib.ptr(lat), b, _lib.ptr(xmax), _lib.ptr(xmin),
                                      _lib.ptr(ymax), _lib.ptr(ymin), ystride, _lib.ptr(out), _lib.ptr(jac),
                                      _lib.ptr(hess), int(bool(diag)), _lib.ptr(ws), ws.numel(),
                                      _lib.stream_of(dev)), name)
        return (out.reshape((b,) + spatial + (c,)), jac.reshape((b,) + spatial + (c, d)),
                hess.reshape((b,) + spatial + hshape))

    # -- latent gradient at a few query points (DPS measurement operator) ---------
    def tape_forward(self, coords, latents, x_normalizer=None, y_normalizer=None):
        """decode() of R latent rows (R, L) at Ns points (Ns, d) -> (R, Ns, c), keeping the
        per-layer pre-activations for tape_vjp.  Only '-11' normalisers (fused)."""
        d, L, c = self.in_coord_features, self.in_latent_features, self.out_features
        dev = latents.device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN tape_forward needs GPU tensors (the HIP path has no CPU fallback)")
        cf = coords.reshape(-1, d).to(device=dev, dtype=torch.float32).contiguous()
        lat = latents.detach().reshape(-1, L).to(torch.float32).contiguous()
        Ns, R = cf.shape[0], lat.shape[0]
        cf, xmax, xmin, ymax, ymin, ystride, post = self._norm_args(cf, Ns, dev, x_normalizer, y_normalizer)
        if post is not None or (x_normalizer is not None and xmax is None):
            raise NotImplementedError("the SIREN latent gradient fuses '-11' normalisers only")
        h = self._handle(dev)
        lib = _lib.load()
        n = C.c_size_t()
        _lib.check(lib.cfd_siren_vjp_workspace_bytes(h, Ns, R, C.byref(n)), "siren vjp workspace")
        ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=dev)
        out = torch.empty((R, Ns, c), dtype=torch.float32, device=dev)
        _lib.check(lib.cfd_siren_tape_forward(h, _lib.ptr(cf), Ns, _lib.ptr(lat), R, _lib.ptr(xmax), _lib.ptr(xmin),
                                              _lib.ptr(ymax), _lib.ptr(ymin), ystride, _lib.ptr(out), _lib.ptr(ws),
                                              ws.numel(), _lib.stream_of(dev)), "cfd_siren_tape_forward")
        # keep every buffer the kernels read until tape_vjp
        self._vjp_tape = (ws, Ns, R, ymax, ymin, ystride, cf, lat, xmax, xmin, self._signature())
        return out

    def tape_vjp(self, g_out):
        """d<g_out, tape_forward(...)>/d latents -> (R, L), for the last tape_forward."""
        tape = getattr(self, "_vjp_tape", None)
        if tape is None:
            raise RuntimeError("tape_vjp needs a preceding tape_forward")
        ws, Ns, R, ymax, ymin, ystride, _, _, _, _, sig = tape
        if sig != self._signature():
            raise RuntimeError("parameters changed since tape_forward")
        if tuple(g_out.shape) != (R, Ns, self.out_features) or g_out.device != ws.device:
            raise ValueError("g_out must match the output of the last tape_forward")
        g = g_out.detach().to(torch.float32).contiguous()
        gz = torch.empty((R, self.in_latent_features), dtype=torch.float32, device=ws.device)
        h = self._handle(ws.device)
        _lib.check(_lib.load().cfd_siren_tape_vjp(h, _lib.ptr(g), Ns, R, _lib.ptr(ymax), _lib.ptr(ymin), ystride,
                                                  _lib.ptr(gz), _lib.ptr(ws), ws.numel(), _lib.stream_of(ws.device)),
                   "cfd_siren_tape_vjp")
        return gz

    # -- latent gradient of value and Jacobian functionals (K15: cfd_siren_jtape_*) ----
    def jac_tape_forward(self, coords, latents, x_normalizer=None, y_normalizer=None):
        """decode_jacobian() of R latent rows (R, L) at Ns points (Ns, d) -> (out (R, Ns, c),
        jac (R, Ns, c, d)), keeping every layer's value and tangent accumulators for
        jac_tape_vjp.  Always the exact fp32 chain; only '-11' normalisers (fused)."""
        d, L, c = self.in_coord_features, self.in_latent_features, self.out_features
        dev = latents.device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN jac_tape_forward needs GPU tensors (the HIP path has no CPU fallback)")
        cf = coords.reshape(-1, d).to(device=dev, dtype=torch.float32).contiguous()
        lat = latents.detach().reshape(-1, L).to(torch.float32).contiguous()
        Ns, R = cf.shape[0], lat.shape[0]
        cf, xmax, xmin, ymax, ymin, ystride, post = self._norm_args(cf, Ns, dev, x_normalizer, y_normalizer)
        if post is not None or (x_normalizer is not None and xmax is None):
            raise NotImplementedError("the SIREN Jacobian adjoint fuses '-11' normalisers only")
        h = self._handle(dev)
        lib = _lib.load()
        n = C.c_size_t()
        _lib.check(lib.cfd_siren_jtape_workspace_bytes(h, Ns, R, C.byref(n)), "siren jtape workspace")
        ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=dev)
        out = torch.empty((R, Ns, c), dtype=torch.float32, device=dev)
        jac = torch.empty((R, Ns, c, d), dtype=torch.float32, device=dev)
        _lib.check(lib.cfd_siren_jtape_forward(h, _lib.ptr(cf), Ns, _lib.ptr(lat), R, _lib.ptr(xmax), _lib.ptr(xmin),
                                               _lib.ptr(ymax), _lib.ptr(ymin), ystride, _lib.ptr(out), _lib.ptr(jac),
                                               _lib.ptr(ws), ws.numel(), _lib.stream_of(dev)),
                   "cfd_siren_jtape_forward")
        # keep every buffer the kernels read until jac_tape_vjp
        self._jvjp_tape = (ws, Ns, R, ymax, ymin, ystride, cf, lat, xmax, xmin, self._signature())
        return out, jac

    def jac_tape_vjp(self, g_out=None, g_jac=None):
        """d(<g_out, out> + <g_jac, jac>)/d latents -> (R, L), for the last
        jac_tape_forward; a gradient left None is zero."""
        tape = getattr(self, "_jvjp_tape", None)
        if tape is None:
            raise RuntimeError("jac_tape_vjp needs a preceding jac_tape_forward")
        ws, Ns, R, ymax, ymin, ystride, _, _, _, _, sig = tape
        if sig != self._signature():
            raise RuntimeError("parameters changed since jac_tape_forward")
        c, d = self.out_features, self.in_coord_features
        for name, g, shape in (("g_out", g_out, (R, Ns, c)), ("g_jac", g_jac, (R, Ns, c, d))):
            if g is not None and (tuple(g.shape) != shape or g.device != ws.device):
                raise ValueError(f"{name} must match the output of the last jac_tape_forward")
        g0 = None if g_out is None else g_out.detach().to(torch.float32).contiguous()
        g1 = None if g_jac is None else g_jac.detach().to(torch.float32).contiguous()
        gz = torch.empty((R, self.in_latent_features), dtype=torch.float32, device=ws.device)
        h = self._handle(ws.device)
        _lib.check(_lib.load().cfd_siren_jtape_vjp(h, _lib.ptr(g0), _lib.ptr(g1), Ns, R, _lib.ptr(ymax),
                                                   _lib.ptr(ymin), ystride, _lib.ptr(gz), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_of(ws.device)), "cfd_siren_jtape_vjp")
        return gz

    # -- dense masked DPS adjoint (K12: cfd_siren_dense_grad) ------------------------
    DENSE_BACKWARD = {"sum": 0, "delta": 1}
    DENSE_COMPUTE = {"auto": 0, "f32": 1}

    def set_dense_form(self, backward="sum", compute="auto"):
        """Forms of dense_grad (development: tools/dense_dps_bench.py and the tests; the
        defaults are the shipped choice).  compute: "auto" -- the K9t split-f16 tape
        kernels in split_f16 compute where they take the width, else the fp32 chain --
        or "f32"; set_compute("f32") always keeps exact fp32.  backward: "sum" (tile
        sums on chip) or "delta" (delta tape per chunk + column sums)."""
        if backward not in self.DENSE_BACKWARD or compute not in self.DENSE_COMPUTE:
            raise ValueError(f"dense form ({backward!r}, {compute!r}) not in {sorted(self.DENSE_BACKWARD)} x "
                             f"{sorted(self.DENSE_COMPUTE)}")
        self._dense_form = (backward, compute)
        return self

    def dense_grad(self, coords, latents, rows_per_sample, y, mask=None, x_normalizer=None, y_normalizer=None,
                   budget=None):
        """Masked residual norm of a dense measurement and its latent gradient, in
        bounded memory: for R latent rows (R, L) at N points (N, d), sample b owning
        rows [b T, (b+1) T) (T = rows_per_sample),
            norms[b] = || y - mask * decode(coords, latents) ||_2,   g_z = d norms / d latents.
        y: (T, N, c) shared by the samples or (R, N, c); mask: None, (N, c), (T, N, c) or
        (R, N, c).  budget: bytes of workspace the call may plan for (None: the library
        default); the result's bits do not depend on it.  Only '-11' normalisers (fused).
        Returns (g_z (R, L), norms (R / T))."""
        d, L, c = self.in_coord_features, self.in_latent_features, self.out_features
        dev = latents.device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN dense_grad needs GPU tensors (the HIP path has no CPU fallback)")
        cf = coords.reshape(-1, d).to(device=dev, dtype=torch.float32).contiguous()
        lat = latents.detach().reshape(-1, L).to(torch.float32).contiguous()
        N, R, T = cf.shape[0], lat.shape[0], int(rows_per_sample)
        if T < 1 or R % T:
            raise ValueError(f"rows_per_sample {T} does not divide the {R} latent rows")
        cf, xmax, xmin, ymax, ymin, ystride, post = self._norm_args(cf, N, dev, x_normalizer, y_normalizer)
        if post is not None or (x_normalizer is not None and xmax is None):
            raise NotImplementedError("the SIREN latent gradient fuses '-11' normalisers only")
        yv = y.detach().to(device=dev, dtype=torch.float32).contiguous()
        if yv.numel() not in (T * N * c, R * N * c):
            raise ValueError(f"measurement of {yv.numel()} values matches neither one sample ({T * N * c}) nor the "
                             f"batch ({R * N * c})")
        y_rows = yv.numel() // (N * c)
        mv, mask_rows = None, 0
        if mask is not None:
            mv = mask.detach().to(device=dev, dtype=torch.float32).contiguous()
            mask_rows = mv.numel() // (N * c)
            if mv.numel() != mask_rows * N * c or mask_rows not in (1, T, R):
                raise ValueError(f"mask of {mv.numel()} values is not 1, {T} or {R} tables of ({N}, {c})")
        h, lib = self._handle(dev), _lib.load()
        bwd, comp = getattr(self, "_dense_form", ("sum", "auto"))
        _lib.check(lib.cfd_siren_dense_set_form(h, self.DENSE_BACKWARD[bwd], self.DENSE_COMPUTE[comp]),
                   "cfd_siren_dense_set_form")
        budget = 0 if budget is None else int(budget)
        n = C.c_size_t()
        _lib.check(lib.cfd_siren_dense_workspace_bytes(h, N, R, budget, C.byref(n)), "siren dense workspace")
        ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=dev)
        self.dense_workspace_bytes = n.value   # what the last call allocated
        gz = torch.empty((R, L), dtype=torch.float32, device=dev)
        norms = torch.empty((R // T,), dtype=torch.float32, device=dev)
        _lib.check(lib.cfd_siren_dense_grad(h, _lib.ptr(cf), N, _lib.ptr(lat), R, T, _lib.ptr(xmax), _lib.ptr(xmin),
                                            _lib.ptr(ymax), _lib.ptr(ymin), ystride, _lib.ptr(yv), y_rows,
                                            _lib.ptr(mv), mask_rows, _lib.ptr(gz), _lib.ptr(norms), _lib.ptr(ws),
                                            ws.numel(), budget, _lib.stream_of(dev)), "cfd_siren_dense_grad")
        return gz, norms

    # -- dense derivative measurements (K16: cfd_siren_jdense_grad) ----------------------
    def jac_dense_grad(self, coords, latents, rows_per_sample, y, value_weights=None, jac_weights=None, mask=None,
                       x_normalizer=None, y_normalizer=None, budget=None):
        """dense_grad() for linear stencils on the value and the exact coordinate
        Jacobian at every point: with (out, jac) = decode_jacobian(coords, latents) and
            A[r, n, m] = sum_o wv[n, m, o] out[r, n, o] + sum_{o,k} wj[n, m, o, k] jac[r, n, o, k],
            norms[b] = || y - mask * A ||_2,   g_z = d norms / d latents
        in bounded memory.  value_weights: (M, c) or per point (N, M, c); jac_weights:
        (M, c, d) or (N, M, c, d); at least one.  y: None (a zero target), (T, N, M) shared
        by the samples or (R, N, M); mask: None, (N, M), (T, N, M) or (R, N, M).  budget,
        normalisers and the result as dense_grad; always the exact fp32 chain.
        Returns (g_z (R, L), norms (R / T))."""
        d, L, c = self.in_coord_features, self.in_latent_features, self.out_features
        dev = latents.device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN jac_dense_grad needs GPU tensors (the HIP path has no CPU fallback)")
        cf = coords.reshape(-1, d).to(device=dev, dtype=torch.float32).contiguous()
        lat = latents.detach().reshape(-1, L).to(torch.float32).contiguous()
        N, R, T = cf.shape[0], lat.shape[0], int(rows_per_sample)
        if T < 1 or R % T:
            raise ValueError(f"rows_per_sample {T} does not divide the {R} latent rows")
        cf, xmax, xmin, ymax, ymin, ystride, post = self._norm_args(cf, N, dev, x_normalizer, y_normalizer)
        if post is not None or (x_normalizer is not None and xmax is None):
            raise NotImplementedError("the SIREN Jacobian adjoint fuses '-11' normalisers only")
        if value_weights is None and jac_weights is None:
            raise ValueError("jac_dense_grad needs value_weights, jac_weights or both")
        M, w, per_point = None, [None, None], [0, 0]
        for i, (name, t, tail) in enumerate((("value_weights", value_weights, (c,)),
                                             ("jac_weights", jac_weights, (c, d)))):
            if t is None:
                continue
            t = torch.as_tensor(t).detach().to(device=dev, dtype=torch.float32).contiguous()
            if t.dim() == 1 + len(tail) and tuple(t.shape[1:]) == tail:
                m = t.shape[0]
            elif t.dim() == 2 + len(tail) and t.shape[0] == N and tuple(t.shape[2:]) == tail:
                m, per_point[i] = t.shape[1], 1
            else:
                raise ValueError(f"{name} of shape {tuple(t.shape)} is neither {('M',) + tail} nor "
                                 f"{(N, 'M') + tail}")
            if m < 1 or (M is not None and m != M):
                raise ValueError(f"{name} has {m} readings per point, expected {M if M is not None else 'at least 1'}")
            M, w[i] = m, t
        yv, y_rows = None, 0
        if y is not None:
            yv = y.detach().to(device=dev, dtype=torch.float32).contiguous()
            if yv.numel() not in (T * N * M, R * N * M):
                raise ValueError(f"measurement of {yv.numel()} values matches neither one sample ({T * N * M}) nor "
                                 f"the batch ({R * N * M})")
            y_rows = yv.numel() // (N * M)
        mv, mask_rows = None, 0
        if mask is not None:
            mv = mask.detach().to(device=dev, dtype=torch.float32).contiguous()
            mask_rows = mv.numel() // (N * M)
            if mv.numel() != mask_rows * N * M or mask_rows not in (1, T, R):
                raise ValueError(f"mask of {mv.numel()} values is not 1, {T} or {R} tables of ({N}, {M})")
        h, lib = self._handle(dev), _lib.load()
        budget = 0 if budget is None else int(budget)
        n = C.c_size_t()
        _lib.check(lib.cfd_siren_jdense_workspace_bytes(h, N, R, M, budget, C.byref(n)), "siren jdense workspace")
        ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=dev)
        self.dense_workspace_bytes = n.value   # what the last call allocated
        gz = torch.empty((R, L), dtype=torch.float32, device=dev)
        norms = torch.empty((R // T,), dtype=torch.float32, device=dev)
        _lib.check(lib.cfd_siren_jdense_grad(h, _lib.ptr(cf), N, _lib.ptr(lat), R, T, _lib.ptr(xmax), _lib.ptr(xmin),
                                             _lib.ptr(ymax), _lib.ptr(ymin), ystride, _lib.ptr(w[0]), per_point[0],
                                             _lib.ptr(w[1]), per_point[1], M, _lib.ptr(yv), y_rows, _lib.ptr(mv),
                                             mask_rows, _lib.ptr(gz), _lib.ptr(norms), _lib.ptr(ws), ws.numel(),
                                             budget, _lib.stream_of(dev)), "cfd_siren_jdense_grad")
        return gz, norms

    # -- training (K10: cfd_siren_train_grad; the loop is confild_amd.cnf_train) ----
    def param_keys(self):
        """Parameter keys in the library's flat-gradient order (cfd_siren_param_info)."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN training needs the parameters on a GPU")
        h, lib = self._handle(dev), _lib.load()
        n = C.c_int()
        _lib.check(lib.cfd_siren_num_params(h, C.byref(n)), "cfd_siren_num_params")
        keys = []
        for i in range(n.value):
            k, nd, shp = C.c_char_p(), C.c_int(), (C.c_int64 * 4)()
            _lib.check(lib.cfd_siren_param_info(h, i, C.byref(k), C.byref(nd), shp), "cfd_siren_param_info")
            keys.append(k.value.decode())
        return keys

    def flat_params(self):
        """(n,) fp32 device copy of every parameter, in param_keys() order."""
        named = dict(self.named_parameters())
        return torch.cat([named[k].detach().reshape(-1).to(torch.float32) for k in self.param_keys()]).contiguous()

    def load_flat(self, flat):
        """Copy a flat_params()-ordered buffer back into the parameters (the handle
        re-packs its weight images on the next call)."""
        named = dict(self.named_parameters())
        o = 0
        with torch.no_grad():
            for k in self.param_keys():
                p = named[k]
                p.copy_(flat[o:o + p.numel()].reshape(p.shape))
                o += p.numel()
        if o != flat.numel():
            raise ValueError(f"flat buffer has {flat.numel()} values, the parameters {o}")

    def train_grad(self, coords, latents, rows, target, scale, grad, grad_latents, sse):
        """One backward of MSELoss for the latent rows `rows` of the (N_samples, L)
        table `latents` at raw coordinates (N, d) against target (R, N, c); adds
        into grad (flat, param_keys() order), grad_latents (N_samples, L) and sse (1)."""
        dev = latents.device
        if dev.type != "cuda":
            raise _lib.CfdError("SIREN training needs GPU tensors (the HIP path has no CPU fallback)")
        d, L, c = self.in_coord_features, self.in_latent_features, self.out_features
        cf = coords.reshape(-1, d).to(device=dev, dtype=torch.float32).contiguous()
        N = cf.shape[0]
        rows = rows.to(device=dev, dtype=torch.int64).contiguous()
        R = rows.numel()
        if torch.unique(rows).numel() != R:
            raise ValueError("batch latent rows must be distinct")
        tgt = target.to(device=dev, dtype=torch.float32).reshape(R, N, c).contiguous()
        for t, name in ((latents, "latents"), (grad, "grad"), (grad_latents, "grad_latents"), (sse, "sse")):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{name} must be a contiguous fp32 tensor on {dev}")
        if latents.shape[-1] != L or grad_latents.shape != latents.shape:
            raise ValueError("latents / grad_latents must be (N_samples, in_latent_features)")
        h, lib = self._handle(dev), _lib.load()
        n = C.c_size_t()
        _lib.check(lib.cfd_siren_train_workspace_bytes(h, N, R, C.byref(n)), "siren train workspace")
        ws = torch.empty(max(n.value, 16), dtype=torch.uint8, device=dev)
        _lib.check(lib.cfd_siren_train_grad(h, _lib.ptr(cf), N, _lib.ptr(latents), _lib.ptr(rows), R, _lib.ptr(tgt),
                                            float(scale), _lib.ptr(grad), _lib.ptr(grad_latents), _lib.ptr(sse),
                                            _lib.ptr(ws), ws.numel(), _lib.stream_of(dev)), "cfd_siren_train_grad")

    def forward(self, coords, latents):
        """nf_networks.py:480-495 (raw, un-normalised in and out)."""
        return self.decode(coords, latents)

    def disable_gradient(self):
        for p in self.parameters():
            p.requires_grad = False

    def __del__(self):
        try:
            lib = _lib.load()
            for h, _ in self._handles.values():
                lib.cfd_siren_destroy(h)
        except Exception:
            pass
