"""Time filter hand-off: a zero-phase FIR filter of the decoded offsets along time, per clip at its own length, on the device
(include/fdm_hip.h, fdm_tfilter_*; kernel csrc/tfilter.hpp; DESIGN.md section 2 item 27 is the definition).  It stands at the head of
the output chain (pipeline._Outputs), so the mesh, wrap, render, rig and head hand-offs all read the filtered offsets.  What a given
filter does to perceptual quality or to lip-sync metrics is unmeasured: there are no trained checkpoints here.  Off unless asked for."""
import ctypes as C
import hashlib
import math

import numpy as np
import torch

from . import _lib
from ._lib import FdmError, check, lib
from .handoff import HandoffPlan, frames_list, offsets_batch

RADIUS_MAX = 32      # csrc/tfilter.hpp, TF_RMAX
FRAME_TILE, COLUMN_CHUNK = 128, 96      # TF_TILE, TF_CHUNK: nothing depends on them but the tests' sizes
EDGES = {"mirror": _lib.TFILTER_MIRROR, "nearest": _lib.TFILTER_NEAREST}


def taps_host(kind, radius, param):
    """The R + 1 half-taps of fdm_tfilter_taps_host as float64 (host only): kind "gaussian" with param = sigma, "savgol" with
    param = the polynomial order."""
    code = {"gaussian": _lib.TFILTER_GAUSSIAN, "savgol": _lib.TFILTER_SAVGOL}.get(kind)
    if code is None:
        raise ValueError(f"time filter kind {kind!r} (gaussian | savgol)")
    radius = int(radius)
    h = np.zeros(max(radius, 0) + 1, dtype=np.float64)
    check(lib().fdm_tfilter_taps_host(code, radius, float(param), h.ctypes.data))
    return h


def gaussian(sigma, radius=None):
    """Half-taps of a Gaussian of `sigma` frames, cut at `radius` (default min(32, ceil(3 sigma))) and normalised to sum 1."""
    if radius is None:
        radius = min(RADIUS_MAX, int(math.ceil(3.0 * float(sigma))))
    return taps_host("gaussian", radius, sigma)


def savgol(radius, order):
    """Half-taps of the Savitzky-Golay smoothing filter of window 2 radius + 1 and polynomial `order` (2 .. 5)."""
    return taps_host("savgol", radius, order)


def strength_from_region(V, idx, inside, outside=1.0):
    """strength [V]: `inside` on the vertices idx, `outside` elsewhere (the lips keep their closures with inside = 0)."""
    s = np.full(int(V), float(outside), dtype=np.float32)
    s[np.asarray(idx, dtype=np.int64).reshape(-1)] = float(inside)
    return s


def _arguments(V, taps=None, kind="gaussian", sigma=None, order=None, radius=None, edge="mirror", strength=None):
    """(V, taps [R + 1] float32, edge name, strength [V] float32 or None): what the C object is made from"""
    if taps is None:
        if kind == "gaussian":
            if sigma is None:
                raise ValueError("a gaussian time filter needs sigma= (frames) or taps=")
            taps = gaussian(sigma, radius)
        elif kind == "savgol":
            if radius is None or order is None:
                raise ValueError("a savgol time filter needs radius= and order=")
            taps = savgol(radius, order)
        else:
            raise ValueError(f"time filter kind {kind!r} (gaussian | savgol)")
    if isinstance(taps, torch.Tensor):
        taps = taps.detach().cpu().numpy()
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1).astype(np.float32))      # rounded to fp32 HERE
    if edge not in EDGES:
        raise ValueError(f"time filter edge {edge!r} (mirror | nearest)")
    if strength is not None:
        if isinstance(strength, torch.Tensor):
            strength = strength.detach().cpu().numpy()
        strength = np.ascontiguousarray(np.asarray(strength, dtype=np.float32).reshape(-1))
        if len(strength) != int(V):
            raise FdmError(f"{len(strength)} strengths for {int(V)} vertices")
    return int(V), taps, edge, strength


def _key(a):
    d = hashlib.sha1()
    for x in (a[1], a[3]):
        d.update(b"-" if x is None else x.tobytes())
    return (a[0], len(a[1]) - 1, a[2], d.hexdigest())


def identity(V, **kw):
    """TimeFilterPlan(V, **kw).key without making the plan: (V, R, edge, digest of taps and strength)."""
    return _key(_arguments(V, **kw))


class TimeFilterPlan(HandoffPlan):
    """Thin binding of fdm_tfilter_create / fdm_tfilter_forward for V vertices.  taps: the half-taps h[0..R] (R <= 32; rounded to
    float32 here), or kind="gaussian" with sigma= frames (radius= default min(32, ceil(3 sigma))), or kind="savgol" with radius= and
    order=.  edge: "mirror" (the end sample not repeated) | "nearest".  strength [V] in [0, 1]: how much of the filter each vertex
    takes (0: its input bits).  The object is bound to the stream current at creation (pipeline keeps plans per (device, stream,
    filter)); without a visible device the plan still validates and forward() raises."""

    _destroy = "fdm_tfilter_destroy"

    def __init__(self, V, taps=None, kind="gaussian", sigma=None, order=None, radius=None, edge="mirror", strength=None, device="cuda:0"):
        super().__init__(device)
        a = _arguments(V, taps, kind, sigma, order, radius, edge, strength)
        self.V, self.taps, self.edge, self.strength = a
        self.radius = len(self.taps) - 1
        self.key = _key(a)
        stream = None
        if torch.cuda.is_available():
            stream = torch.cuda.current_stream(self.device).cuda_stream
        self._create("fdm_tfilter_create", self.V, self.radius, self.taps.ctypes.data, None if self.strength is None else self.strength.ctypes.data,
                     EDGES[self.edge], stream)
        self.stream = stream

    def arguments(self):
        """The arguments that make this plan again (on another device or stream)."""
        return dict(V=self.V, taps=self.taps, edge=self.edge, strength=self.strength)

    def forward(self, x, frames=None, out=None):
        """x [B, L_max, 3 V] (or [L, 3 V]) fp32 on the plan's device, frames: L per clip (None: L_max) -> y of the same shape: each
        clip filtered along its own frames, rows at or past them zeros.  out: a tensor to write instead (it may not overlap x)."""
        dv = self.device
        x = offsets_batch(x, self.V, dv)
        B, L_max = int(x.shape[0]), int(x.shape[1])
        fr = frames_list(frames, B, L_max)
        if out is None:
            out = torch.empty_like(x)
        elif out.dtype != torch.float32 or out.device != dv or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
            raise FdmError(f"out must be a contiguous float32 {tuple(x.shape)} tensor on {dv}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        fa = (C.c_int * B)(*fr)
        with torch.cuda.device(dv):
            if torch.cuda.current_stream(dv).cuda_stream != self.stream:
                raise FdmError("this TimeFilterPlan was made on another stream (a plan serves one stream: make one per stream)")
            check(lib().fdm_tfilter_forward(self.h, x.data_ptr(), fa, B, L_max, out.data_ptr()))
        self._keep = x                # read asynchronously on this stream
        return out
