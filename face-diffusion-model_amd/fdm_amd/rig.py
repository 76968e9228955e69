"""Rig hand-off: decoded vertex offsets -> blendshape coefficients per frame at the consumer's frame rate, a ridge-regularised,
box-constrained least-squares fit onto a basis, on the device (include/fdm_hip.h, fdm_rig_*; kernels csrc/rig_out.hpp; DESIGN.md
section 2 item 19 is the definition).  With smooth > 0 the frames of a clip are fitted together under a penalty on the change from one
output frame to the next (fdm_rig_set_temporal; item 21)."""
import contextlib
import ctypes as C
import hashlib
from collections import namedtuple

import numpy as np
import torch

from ._lib import FdmError, check, lib
from .handoff import HandoffPlan, fps_pair, frames_list, frames_out_max, offsets_batch

# weights [B, L_out_max, K] fp32 (rows at or past frames[b] are zeros), frames = L_out per clip, names = the K coefficient names or None
RigFrames = namedtuple("RigFrames", "weights frames names")

SWEEPS = 16      # projected Gauss-Seidel sweeps by default (what an ill-conditioned artist rig needs is unmeasured, and strong smoothing needs more: DESIGN.md items 19, 21)


def _host(x, shape, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    if a.shape != shape:
        raise FdmError(f"{what} must have shape {shape}, got {a.shape}")
    return a


def basis_array(basis):
    """basis as a contiguous float32 [K, 3 V] numpy array (host); [K, V, 3] is accepted."""
    if isinstance(basis, torch.Tensor):
        basis = basis.detach().cpu().numpy()
    e = np.asarray(basis, dtype=np.float32)
    if e.ndim == 3 and e.shape[2] == 3:
        e = e.reshape(e.shape[0], -1)
    if e.ndim != 2 or e.shape[0] < 1 or e.shape[1] < 3 or e.shape[1] % 3:
        raise FdmError(f"basis must be [K, 3 V] (or [K, V, 3]), got {e.shape}")
    return np.ascontiguousarray(e)


def gram(basis, weights=None, ridge=0.0):
    """(G [K, K] float64, L [K, K] float32) of fdm_rig_gram_host: G = E diag(w) E^T + ridge I and its Cholesky factor, rounded."""
    e = basis_array(basis)
    K, V = e.shape[0], e.shape[1] // 3
    w = None if weights is None else _host(weights, (V,), "weights")
    g, l = np.zeros((K, K), dtype=np.float64), np.zeros((K, K), dtype=np.float32)
    check(lib().fdm_rig_gram_host(e.ctypes.data, None if w is None else w.ctypes.data, K, V, float(ridge), g.ctypes.data, l.ctypes.data))
    return g, l


def temporal_tables(gram, smooth, weights=None):
    """(lam [K] float64 ascending, Q [K, K] float64) of fdm_rig_temporal_tables_host for G = gram [K, K], M = smooth diag(weights):
    Q^T G Q = diag(lam) and Q^T M Q = I.  Host only."""
    g = np.ascontiguousarray(np.asarray(gram, dtype=np.float64))
    if g.ndim != 2 or g.shape[0] != g.shape[1] or g.shape[0] < 1:
        raise FdmError(f"gram must be [K, K], got {g.shape}")
    K = int(g.shape[0])
    m = None if weights is None else _host(weights, (K,), "smooth_weights")
    lam, q = np.zeros(K, dtype=np.float64), np.zeros((K, K), dtype=np.float64)
    check(lib().fdm_rig_temporal_tables_host(g.ctypes.data, K, float(smooth), None if m is None else m.ctypes.data, lam.ctypes.data, q.ctypes.data))
    return lam, q


def _arguments(basis, weights, ridge, bounds, sweeps, names, smooth=0.0, smooth_weights=None):
    """RigPlan's arguments as host arrays: (basis [K, 3 V], weights [V] | None, ridge, lo [K] | None, hi [K] | None, sweeps, names,
    smooth, smooth_weights [K] | None)."""
    e = basis_array(basis)
    K, V = int(e.shape[0]), int(e.shape[1]) // 3
    w = None if weights is None else _host(weights, (V,), "weights")
    lo = hi = None
    if bounds is not None:
        lo, hi = (_host(np.broadcast_to(np.asarray(b, dtype=np.float32), (K,)), (K,), "bounds") for b in bounds)
    names = None if names is None else [str(n) for n in names]
    if names is not None and len(names) != K:
        raise FdmError(f"{len(names)} names for {K} coefficients")
    m = None if smooth_weights is None else _host(smooth_weights, (K,), "smooth_weights")
    return e, w, float(ridge), lo, hi, int(sweeps), names, float(smooth), m


def _key(a):
    e, w, ridge, lo, hi, sweeps, names, smooth, m = a
    d = hashlib.sha1(e.tobytes())
    for x in (w, lo, hi):
        d.update(b"-" if x is None else x.tobytes())
    d.update(repr((ridge, sweeps, names)).encode())
    if smooth != 0.0 or m is not None:        # (a per-frame rig keeps the digest it had before there was a temporal fit)
        d.update(repr(smooth).encode() + (b"-" if m is None else m.tobytes()))
    return (int(e.shape[0]), int(e.shape[1]) // 3, d.hexdigest())


def identity(basis, weights=None, ridge=0.0, bounds=None, sweeps=SWEEPS, names=None, smooth=0.0, smooth_weights=None):
    """RigPlan(...).key without making the plan: (K, V, digest of every argument)."""
    return _key(_arguments(basis, weights, ridge, bounds, sweeps, names, smooth, smooth_weights))


class RigPlan(HandoffPlan):
    """Thin binding of fdm_rig_create / fdm_rig_forward for one rig: the fp64 Gram matrix and its Cholesky factor are formed and
    uploaded here, forward() only passes pointers.  basis [K, 3 V] blendshape deltas, weights [V] >= 0 or None, ridge >= 0, bounds =
    (lo, hi) (scalars or [K]) or None, sweeps of projected Gauss-Seidel, names of the K coefficients.  A plan holds one scratch: it
    serves one stream at a time (pipeline.to_rig keeps them per (device, stream, rig)).  Without a visible device the plan still
    validates its arguments and forward() raises.  smooth = mu > 0 fits a clip's frames together under 1/2 (c_f - c_{f-1})^T M (c_f -
    c_{f-1}), M = mu diag(smooth_weights) (weights [K] > 0 or None: all 1), on OUTPUT frames: at another output rate the same mu
    smooths over a different time span.  mu is in the units of G: tr(G) / K is the scale at which it starts to matter (gram())."""

    _destroy = "fdm_rig_destroy"

    def __init__(self, basis, weights=None, ridge=0.0, bounds=None, sweeps=SWEEPS, names=None, device="cuda:0", smooth=0.0, smooth_weights=None):
        super().__init__(device)
        a = _arguments(basis, weights, ridge, bounds, sweeps, names, smooth, smooth_weights)
        self.basis, self.weights, self.ridge, self.lo, self.hi, self.sweeps, self.names, self.smooth, self.smooth_weights = a
        self.K, self.V = int(self.basis.shape[0]), int(self.basis.shape[1]) // 3
        self.key = _key(a)            # the rig's identity: what pipeline.to_rig caches plans by
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        self._create("fdm_rig_create", self.basis.ctypes.data, self.K, self.V, ptr(self.weights), self.ridge, ptr(self.lo), ptr(self.hi), self.sweeps)
        if self.smooth != 0.0 or self.smooth_weights is not None:
            self._set_temporal()

    def _set_temporal(self):
        m = self.smooth_weights
        with torch.cuda.device(self.device) if torch.cuda.is_available() else contextlib.nullcontext():
            check(lib().fdm_rig_set_temporal(self.h, self.smooth, None if m is None else m.ctypes.data))

    def set_temporal(self, smooth, smooth_weights=None):
        """Change the smoothing strength of this plan (fdm_rig_set_temporal: new tables, waits for the device); 0 returns it to the
        per-frame fit.  The plan's key changes with it: do this to a plan of your own, not to one pipeline.to_rig has cached."""
        m = None if smooth_weights is None else _host(smooth_weights, (self.K,), "smooth_weights")
        old = self.smooth, self.smooth_weights
        self.smooth, self.smooth_weights = float(smooth), m
        try:
            self._set_temporal()
        except FdmError:
            self.smooth, self.smooth_weights = old          # (a refused call leaves the object as it was)
            raise
        self.key = _key(_arguments(**self.arguments()))

    def arguments(self):
        """The arguments that make this plan again (on another device or stream)."""
        return dict(basis=self.basis, weights=self.weights, ridge=self.ridge, bounds=None if self.lo is None else (self.lo, self.hi),
                    sweeps=self.sweeps, names=self.names, smooth=self.smooth, smooth_weights=self.smooth_weights)

    def forward(self, offsets, frames=None, fps=None, proj=False, out=None):
        """offsets [B, L_max, 3 V] (or [L, 3 V]) fp32 on the plan's device: the decoder's output BEFORE the template is added; frames:
        L per clip (None: L_max); fps = (fps_in, fps_out) or None -> RigFrames, or (RigFrames, proj [B, L_out_max, K]) with proj=True
        (the projections the solve consumed).  out: a weights tensor to write instead of a new one (its second dimension is
        L_out_max).  New outputs are L_out_max = max(frames out) long."""
        dv = self.device
        x = offsets_batch(offsets, self.V, dv)
        B, L_max = int(x.shape[0]), int(x.shape[1])
        fr, (fi, fo) = frames_list(frames, B, L_max), fps_pair(fps)
        if out is None:
            Lo = frames_out_max(fr, fi, fo)
            coef = torch.empty(B, Lo, self.K, dtype=torch.float32, device=dv)
        else:
            coef = out
            Lo = int(coef.shape[1]) if coef.dim() == 3 else 0
            if coef.dtype != torch.float32 or coef.device != dv or tuple(coef.shape) != (B, Lo, self.K) or not coef.is_contiguous():
                raise FdmError(f"out must be a contiguous float32 [{B}, L_out_max, {self.K}] tensor on {dv}, got {coef.dtype} {tuple(coef.shape)} on {coef.device}")
        pj = torch.empty(B, Lo, self.K, dtype=torch.float32, device=dv) if proj else None
        fa, got = (C.c_int * B)(*fr), (C.c_int * B)()
        with torch.cuda.device(dv):
            check(lib().fdm_rig_forward(self.h, x.data_ptr(), fa, B, L_max, fi, fo, coef.data_ptr(), None if pj is None else pj.data_ptr(), Lo,
                                        got, torch.cuda.current_stream(dv).cuda_stream))
        self._keep = x                # read asynchronously on this stream
        rf = RigFrames(coef, list(got), self.names)
        return (rf, pj) if proj else rf
