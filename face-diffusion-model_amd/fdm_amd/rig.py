"""Rig hand-off: decoded vertex offsets -> blendshape coefficients per frame at the consumer's frame rate, a ridge-regularised,
box-constrained least-squares fit onto a basis, on the device (include/fdm_hip.h, fdm_rig_*; kernels csrc/rig_out.hpp; DESIGN.md
section 2 item 19 is the definition)."""
import ctypes as C
import hashlib
from collections import namedtuple

import numpy as np
import torch

from ._lib import FdmError, check, lib
from .handoff import HandoffPlan, fps_pair, frames_list, frames_out_max, offsets_batch

# weights [B, L_out_max, K] fp32 (rows at or past frames[b] are zeros), frames = L_out per clip, names = the K coefficient names or None
RigFrames = namedtuple("RigFrames", "weights frames names")

SWEEPS = 16      # projected Gauss-Seidel sweeps by default (what an ill-conditioned artist rig needs is unmeasured: DESIGN.md)


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


def _arguments(basis, weights, ridge, bounds, sweeps, names):
    """RigPlan's arguments as host arrays: (basis [K, 3 V], weights [V] | None, ridge, lo [K] | None, hi [K] | None, sweeps, names)."""
    e = basis_array(basis)
    K, V = int(e.shape[0]), int(e.shape[1]) // 3
    w = None if weights is None else _host(weights, (V,), "weights")
    lo = hi = None
    if bounds is not None:
        lo, hi = (_host(np.broadcast_to(np.asarray(b, dtype=np.float32), (K,)), (K,), "bounds") for b in bounds)
    names = None if names is None else [str(n) for n in names]
    if names is not None and len(names) != K:
        raise FdmError(f"{len(names)} names for {K} coefficients")
    return e, w, float(ridge), lo, hi, int(sweeps), names


def _key(a):
    e, w, ridge, lo, hi, sweeps, names = a
    d = hashlib.sha1(e.tobytes())
    for x in (w, lo, hi):
        d.update(b"-" if x is None else x.tobytes())
    d.update(repr((ridge, sweeps, names)).encode())
    return (int(e.shape[0]), int(e.shape[1]) // 3, d.hexdigest())


def identity(basis, weights=None, ridge=0.0, bounds=None, sweeps=SWEEPS, names=None):
    """RigPlan(...).key without making the plan: (K, V, digest of every argument)."""
    return _key(_arguments(basis, weights, ridge, bounds, sweeps, names))


class RigPlan(HandoffPlan):
    """Thin binding of fdm_rig_create / fdm_rig_forward for one rig: the fp64 Gram matrix and its Cholesky factor are formed and
    uploaded here, forward() only passes pointers.  basis [K, 3 V] blendshape deltas, weights [V] >= 0 or None, ridge >= 0, bounds =
    (lo, hi) (scalars or [K]) or None, sweeps of projected Gauss-Seidel, names of the K coefficients.  A plan holds one scratch: it
    serves one stream at a time (pipeline.to_rig keeps them per (device, stream, rig)).  Without a visible device the plan still
    validates its arguments and forward() raises."""

    _destroy = "fdm_rig_destroy"

    def __init__(self, basis, weights=None, ridge=0.0, bounds=None, sweeps=SWEEPS, names=None, device="cuda:0"):
        super().__init__(device)
        a = _arguments(basis, weights, ridge, bounds, sweeps, names)
        self.basis, self.weights, self.ridge, self.lo, self.hi, self.sweeps, self.names = a
        self.K, self.V = int(self.basis.shape[0]), int(self.basis.shape[1]) // 3
        self.key = _key(a)            # the rig's identity: what pipeline.to_rig caches plans by
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        self._create("fdm_rig_create", self.basis.ctypes.data, self.K, self.V, ptr(self.weights), self.ridge, ptr(self.lo), ptr(self.hi), self.sweeps)

    def arguments(self):
        """The arguments that make this plan again (on another device or stream)."""
        return dict(basis=self.basis, weights=self.weights, ridge=self.ridge, bounds=None if self.lo is None else (self.lo, self.hi),
                    sweeps=self.sweeps, names=self.names)

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
