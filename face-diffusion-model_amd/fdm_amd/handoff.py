"""What mesh.MeshOutPlan, rig.RigPlan and flame.FlamePlan share: the C handle's life, forward()'s arguments, pipeline.py's plan cache."""
import contextlib
import ctypes as C

import torch

from ._lib import FdmError, check, lib


class HandoffPlan:
    """A C object made on one device and destroyed with the plan: a subclass names its destroy symbol and calls _create().  self.stream
    is the stream current at creation (None without a visible device: the plan has validated its arguments and forward() raises)."""
    _destroy = None      # the fdm_*_destroy symbol

    def __init__(self, device):
        self.h = self.stream = None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise FdmError(f"{type(self).__name__} runs on the HIP path only (no CPU fallback)")

    def _create(self, symbol, *args):
        h = C.c_void_p()
        with torch.cuda.device(self.device) if torch.cuda.is_available() else contextlib.nullcontext():
            check(getattr(lib(), symbol)(*args, C.byref(h)))
            if torch.cuda.is_available():
                self.stream = torch.cuda.current_stream(self.device).cuda_stream
        self.h = h

    def __del__(self):
        try:
            if self.h:
                getattr(lib(), self._destroy)(self.h)
                self.h = None
        except Exception:
            pass


def offsets_batch(offsets, V, device):
    """offsets [B, L_max, 3 V] (or [L, 3 V]) -> the contiguous float32 batch on `device`, refused otherwise"""
    x = offsets.detach()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.device != device or x.dtype != torch.float32 or x.dim() != 3 or x.shape[2] != 3 * V:
        raise FdmError(f"offsets must be float32 [B, L, {3 * V}] on {device}, got {x.dtype} {tuple(x.shape)} on {x.device}")
    return x.contiguous()


def frames_list(frames, B, L_max):
    """L per clip as a list of B ints (None: L_max each)"""
    fr = [L_max] * B if frames is None else [int(f) for f in frames]
    if len(fr) != B:
        raise FdmError(f"{len(fr)} frame counts for {B} clips")
    return fr


def fps_pair(fps):
    """fps = (fps_in, fps_out) or None -> two floats, 0 where no rate is given"""
    return (0.0, 0.0) if fps is None else (float(fps[0] or 0), float(fps[1] or 0))


def frames_out(frames_in, fps_in, fps_out):
    """L_out of a clip of frames_in frames (fdm_mesh_frames; host only)."""
    n = C.c_int(0)
    check(lib().fdm_mesh_frames(int(frames_in), float(fps_in or 0), float(fps_out or 0), C.byref(n)))
    return n.value


def frames_out_max(fr, fi, fo):
    """L_out_max of new outputs: the longest clip's L_out, at least 1"""
    return max([frames_out(f, fi, fo) for f in fr] + [1])


_PLANS = {}      # (device, stream, kind, identity) -> the plan


def cached_plan(at, kind, identity, make, given=None):
    """The plan of `kind` and `identity` at `at` = (device name, stream): a plan serves one stream at a time.  A miss takes `given` --
    a plan the caller holds -- as it is where it was made for this device and stream, and calls make() otherwise."""
    key = tuple(at) + (kind, identity)
    plan = _PLANS.get(key)
    if plan is None:
        mine = given is not None and str(given.device) == at[0] and given.stream == at[1]
        _PLANS[key] = plan = given if mine else make()
    return plan
