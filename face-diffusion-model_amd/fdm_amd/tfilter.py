"""Time filter hand-off: a zero-phase FIR filter of the decoded offsets along time, per clip at its own length, on the device
(include/fdm_hip.h, fdm_tfilter_*; kernel csrc/tfilter.hpp; DESIGN.md section 2 item 27 is the definition), or a recurrence -- a
one-pole low-pass ("ema") or the One Euro filter ("one_euro": its cutoff rises with the vertex's smoothed speed), causal with a state
carried from call to call or zero-phase (kernel csrc/trecur.hpp).  It stands at the head of
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
RECUR_KINDS = {"ema": _lib.TFILTER_EMA, "one_euro": _lib.TFILTER_ONE_EURO}
DIRECTIONS = {"causal": _lib.TFILTER_CAUSAL, "zero_phase": _lib.TFILTER_ZERO_PHASE}
RECUR_VERTS = 64      # csrc/trecur.hpp, TR_VERTS: vertices per workgroup; nothing depends on it but the tests' sizes
PREFETCH_DEPTHS, PREFETCH_DEFAULT = (1, 4, 8, 16), 16      # fdm_tfilter_set_prefetch; TR_DEPTH


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


def recur_coeffs(kind, fps, cutoff=None, min_cutoff=None, beta=None, d_cutoff=1.0):
    """The constants of fdm_tfilter_recur_coeffs_host as float32 [8] = (k, c0, be, cd, fr, ad, a0, 0) (host only).  kind "ema" with
    cutoff= Hz; "one_euro" with min_cutoff= Hz, beta= (>= 0, in Hz per (mesh unit per second): a sensible value depends on the mesh's
    scale) and d_cutoff= Hz (1.0).  fps: the frame rate of the frames that are filtered."""
    code = RECUR_KINDS.get(kind)
    if code is None:
        raise ValueError(f"time filter kind {kind!r} (ema | one_euro)")
    if fps is None:
        raise ValueError(f"a {kind} time filter needs fps= (the frame rate of the frames)")
    if kind == "ema":
        if cutoff is None or min_cutoff is not None or beta is not None:
            raise ValueError("an ema time filter takes cutoff= (Hz) and neither min_cutoff= nor beta=")
        c, be, cd = cutoff, 0.0, 1.0
    else:
        if min_cutoff is None or beta is None or cutoff is not None:
            raise ValueError("a one_euro time filter takes min_cutoff= (Hz) and beta=, not cutoff=")
        c, be, cd = min_cutoff, beta, 1.0 if d_cutoff is None else d_cutoff
    q = np.zeros(_lib.TFILTER_NCOEFF, dtype=np.float32)
    check(lib().fdm_tfilter_recur_coeffs_host(code, float(fps), float(c), float(be), float(cd), q.ctypes.data))
    return q


def strength_from_region(V, idx, inside, outside=1.0):
    """strength [V]: `inside` on the vertices idx, `outside` elsewhere (the lips keep their closures with inside = 0)."""
    s = np.full(int(V), float(outside), dtype=np.float32)
    s[np.asarray(idx, dtype=np.int64).reshape(-1)] = float(inside)
    return s


def _strength(V, strength):
    if strength is None:
        return None
    if isinstance(strength, torch.Tensor):
        strength = strength.detach().cpu().numpy()
    strength = np.ascontiguousarray(np.asarray(strength, dtype=np.float32).reshape(-1))
    if len(strength) != int(V):
        raise FdmError(f"{len(strength)} strengths for {int(V)} vertices")
    return strength


def _arguments(V, taps=None, kind="gaussian", sigma=None, order=None, radius=None, edge="mirror", strength=None, fps=None, cutoff=None,
               min_cutoff=None, beta=None, d_cutoff=None, direction=None, coeffs=None):
    """What the C object is made from.  An FIR filter: (V, taps [R + 1] float32, edge name, strength [V] float32 or None).  A
    recurrence: (V, coeffs [8] float32, (kind, direction), strength)."""
    if kind in RECUR_KINDS:
        if taps is not None or sigma is not None or order is not None or radius is not None or edge not in (None, "mirror"):
            raise ValueError(f"a {kind} time filter has no taps=, sigma=, order=, radius= or edge=")
        direction = "zero_phase" if direction is None else direction
        if direction not in DIRECTIONS:
            raise ValueError(f"time filter direction {direction!r} (zero_phase | causal)")
        if coeffs is None:
            coeffs = recur_coeffs(kind, fps, cutoff, min_cutoff, beta, d_cutoff)
        coeffs = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float32).reshape(-1))
        if len(coeffs) != _lib.TFILTER_NCOEFF:
            raise FdmError(f"{len(coeffs)} coefficients, a recurrence has {_lib.TFILTER_NCOEFF}")
        return int(V), coeffs, (kind, direction), _strength(V, strength)
    if any(v is not None for v in (fps, cutoff, min_cutoff, beta, d_cutoff, direction, coeffs)):
        raise ValueError("fps=, cutoff=, min_cutoff=, beta=, d_cutoff= and direction= belong to kind=\"ema\" | \"one_euro\"")
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
            raise ValueError(f"time filter kind {kind!r} (gaussian | savgol | ema | one_euro)")
    if isinstance(taps, torch.Tensor):
        taps = taps.detach().cpu().numpy()
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1).astype(np.float32))      # rounded to fp32 HERE
    if edge not in EDGES:
        raise ValueError(f"time filter edge {edge!r} (mirror | nearest)")
    return int(V), taps, edge, _strength(V, strength)


def _key(a):
    d = hashlib.sha1()
    for x in (a[1], a[3]):
        d.update(b"-" if x is None else x.tobytes())
    if isinstance(a[2], tuple):      # a recurrence: (V, kind, direction, digest of coefficients and strength)
        return (a[0],) + a[2] + (d.hexdigest(),)
    return (a[0], len(a[1]) - 1, a[2], d.hexdigest())


def identity(V, **kw):
    """TimeFilterPlan(V, **kw).key without making the plan: (V, R, edge, digest of taps and strength), or for a recurrence (V, kind,
    direction, digest of coefficients and strength)."""
    return _key(_arguments(V, **kw))


class RecurState:
    """The carried state of a causal recurrence for B clips, on the device: seen [B] int32 (frames consumed so far, 0 = fresh) and
    st [B, 3, 3 V] float32 (y_prev, x_prev, dh).  TimeFilterPlan.new_state(B) makes one; forward(..., state=) reads and advances it."""

    def __init__(self, B, V, device):
        self.B, self.V = int(B), int(V)
        self.seen = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.st = torch.zeros(self.B, 3, 3 * self.V, dtype=torch.float32, device=device)

    def reset(self, clips=None):
        """Start afresh: every clip, or the clips listed."""
        if clips is None:
            self.seen.zero_()
            self.st.zero_()
        else:
            idx = torch.as_tensor(list(clips), dtype=torch.long, device=self.seen.device)
            self.seen[idx] = 0
            self.st[idx] = 0


class TimeFilterPlan(HandoffPlan):
    """Thin binding of fdm_tfilter_create / fdm_tfilter_create_recur / fdm_tfilter_forward for V vertices.  An FIR filter -- taps: the
    half-taps h[0..R] (R <= 32; rounded to float32 here), or kind="gaussian" with sigma= frames (radius= default min(32, ceil(3 sigma))),
    or kind="savgol" with radius= and order=; edge: "mirror" (the end sample not repeated) | "nearest".  A recurrence -- kind="ema" with
    fps= and cutoff= (Hz), or kind="one_euro" with fps=, min_cutoff= (Hz), beta= (>= 0, in Hz per (mesh unit per second): it depends on
    the mesh's scale) and d_cutoff= (Hz, 1.0); direction: "zero_phase" (the default: forward, then backward over the result) | "causal"
    (it lags; forward(..., state=) carries it from call to call).  These settings are not measurements: what they do to perceptual
    quality or lip-sync metrics is unmeasured.  strength [V] in [0, 1]: how much of the filter each vertex takes (0: its input bits).
    The object is bound to the stream current at creation (pipeline keeps plans per (device, stream, filter)); without a visible device
    the plan still validates and forward() raises."""

    _destroy = "fdm_tfilter_destroy"

    def __init__(self, V, taps=None, kind="gaussian", sigma=None, order=None, radius=None, edge="mirror", strength=None, device="cuda:0", fps=None,
                 cutoff=None, min_cutoff=None, beta=None, d_cutoff=None, direction=None, coeffs=None):
        super().__init__(device)
        a = _arguments(V, taps, kind, sigma, order, radius, edge, strength, fps, cutoff, min_cutoff, beta, d_cutoff, direction, coeffs)
        self.key = _key(a)
        self.V, self.strength = a[0], a[3]
        self.recurrence = isinstance(a[2], tuple)
        stream = None
        if torch.cuda.is_available():
            stream = torch.cuda.current_stream(self.device).cuda_stream
        sp = None if self.strength is None else self.strength.ctypes.data
        if self.recurrence:
            self.coeffs, (self.kind, self.direction) = a[1], a[2]
            self.taps = self.edge = self.radius = None
            self._create("fdm_tfilter_create_recur", self.V, RECUR_KINDS[self.kind], self.coeffs.ctypes.data, sp, DIRECTIONS[self.direction], stream)
        else:
            self.taps, self.edge = a[1], a[2]
            self.radius = len(self.taps) - 1
            self._create("fdm_tfilter_create", self.V, self.radius, self.taps.ctypes.data, sp, EDGES[self.edge], stream)
        self.stream = stream

    def arguments(self):
        """The arguments that make this plan again (on another device or stream)."""
        if self.recurrence:
            return dict(V=self.V, kind=self.kind, coeffs=self.coeffs, direction=self.direction, strength=self.strength)
        return dict(V=self.V, taps=self.taps, edge=self.edge, strength=self.strength)

    def new_state(self, B):
        """A fresh RecurState for B clips on the plan's device (a causal recurrence only)."""
        if not self.recurrence or self.direction != "causal":
            raise FdmError("only a causal ema / one_euro filter carries a state (an FIR filter and a zero-phase one see the whole clip)")
        return RecurState(B, self.V, self.device)

    def set_prefetch(self, depth):
        """How many frames the recurrence kernel loads ahead of its walk (PREFETCH_DEPTHS): a tuning knob, no bit depends on it."""
        check(lib().fdm_tfilter_set_prefetch(self.h, int(depth)))

    def forward(self, x, frames=None, out=None, state=None):
        """x [B, L_max, 3 V] (or [L, 3 V]) fp32 on the plan's device, frames: L per clip (None: L_max) -> y of the same shape: each
        clip filtered along its own frames, rows at or past them zeros.  out: a tensor to write instead (it may not overlap x).
        state: a RecurState of B clips (a causal recurrence only): every clip continues where its earlier frames ended, exactly as if
        they had been contiguous, and the state advances; a clip with 0 frames in this call is left as it is."""
        dv = self.device
        x = offsets_batch(x, self.V, dv)
        B, L_max = int(x.shape[0]), int(x.shape[1])
        fr = frames_list(frames, B, L_max)
        if state is not None:
            if not isinstance(state, RecurState) or state.B != B or state.V != self.V or state.st.device != dv:
                raise FdmError(f"state= takes the plan's new_state({B}) (a RecurState of {B} clips of {self.V} vertices on {dv})")
        if out is None:
            out = torch.empty_like(x)
        elif out.dtype != torch.float32 or out.device != dv or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
            raise FdmError(f"out must be a contiguous float32 {tuple(x.shape)} tensor on {dv}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        fa = (C.c_int * B)(*fr)
        with torch.cuda.device(dv):
            if torch.cuda.current_stream(dv).cuda_stream != self.stream:
                raise FdmError("this TimeFilterPlan was made on another stream (a plan serves one stream: make one per stream)")
            if state is None:
                check(lib().fdm_tfilter_forward(self.h, x.data_ptr(), fa, B, L_max, out.data_ptr()))
            else:
                check(lib().fdm_tfilter_forward_state(self.h, x.data_ptr(), fa, B, L_max, state.st.data_ptr(), state.seen.data_ptr(), out.data_ptr()))
        self._keep = x                # read asynchronously on this stream
        return out
