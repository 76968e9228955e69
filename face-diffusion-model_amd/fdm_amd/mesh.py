"""Mesh hand-off: decoded vertex offsets -> positions (+ template) at the consumer's frame rate and area-weighted vertex normals, on
the device (include/fdm_hip.h, fdm_mesh_*; kernels csrc/mesh_out.hpp; DESIGN.md section 2 item 18 is the definition)."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import FdmError, check, lib

# positions [B, L_out_max, V, 3] (interleaved: [B, L_out_max, V, 6] = position then normal, and normals is None), normals the same
# shape as planar positions or None, frames = L_out per clip (rows at or past it are zeros)
MeshFrames = namedtuple("MeshFrames", "positions normals frames")


def faces_array(faces):
    """faces as a contiguous int32 [F, 3] numpy array (host)."""
    if isinstance(faces, torch.Tensor):
        faces = faces.detach().cpu().numpy()
    f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
    return f


def adjacency(faces, V):
    """(offsets [V + 1], items [3 F]) of fdm_mesh_adjacency_host: the faces incident to each vertex, ascending, one per corner."""
    f = faces_array(faces)
    off, items = np.zeros(int(V) + 1 if V > 0 else 1, dtype=np.int32), np.zeros(max(3 * len(f), 1), dtype=np.int32)
    check(lib().fdm_mesh_adjacency_host(f.ctypes.data, len(f), int(V), off.ctypes.data, items.ctypes.data))
    return off, items[:3 * len(f)]


def frames_out(frames_in, fps_in, fps_out):
    """L_out of a clip of frames_in frames (fdm_mesh_frames; host only)."""
    n = C.c_int(0)
    check(lib().fdm_mesh_frames(int(frames_in), float(fps_in or 0), float(fps_out or 0), C.byref(n)))
    return n.value


class MeshOutPlan:
    """Thin binding of fdm_mesh_create / fdm_mesh_forward for one topology: the incident-face lists are built and uploaded here,
    forward() only passes pointers.  A plan holds one scratch: it serves one stream at a time (one plan per stream for concurrent
    calls; pipeline.to_mesh keeps them per (device, stream, topology))."""

    def __init__(self, faces, V, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise FdmError("MeshOutPlan runs on the HIP path only (no CPU fallback)")
        self.faces, self.V = faces_array(faces), int(V)
        self.h = None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().fdm_mesh_create(self.faces.ctypes.data, len(self.faces), self.V, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h:
                lib().fdm_mesh_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def forward(self, offsets, frames=None, template=None, fps=None, normals=True, interleaved=False, half=False, out=None):
        """offsets [B, L_max, 3 V] (or [L, 3 V]) fp32 on the plan's device, frames: L per clip (None: L_max), template [1 or B, 3 V],
        fps = (fps_in, fps_out) or None -> MeshFrames.  out: (positions, normals) tensors to write instead of new ones (normals
        None where the call writes none); their second dimension is L_out_max.  New outputs are L_out_max = max(frames out) long."""
        dv = self.device
        x = offsets.detach()
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.device != dv or x.dtype != torch.float32 or x.dim() != 3 or x.shape[2] != 3 * self.V:
            raise FdmError(f"offsets must be float32 [B, L, {3 * self.V}] on {dv}, got {x.dtype} {tuple(x.shape)} on {x.device}")
        x = x.contiguous()
        B, L_max = int(x.shape[0]), int(x.shape[1])
        fr = [L_max] * B if frames is None else [int(f) for f in frames]
        if len(fr) != B:
            raise FdmError(f"{len(fr)} frame counts for {B} clips")
        fi, fo = (0.0, 0.0) if fps is None else (float(fps[0] or 0), float(fps[1] or 0))
        tp, rows = None, 0
        if template is not None:
            tp = torch.as_tensor(template, dtype=torch.float32).to(dv).reshape(-1, 3 * self.V).contiguous()
            rows = int(tp.shape[0])
        flags = (_lib.MESH_INTERLEAVED if interleaved else 0) | (_lib.MESH_F16 if half else 0) | (_lib.MESH_NORMALS if normals else 0)
        dt = torch.float16 if half else torch.float32
        if out is None:
            Lo = max([frames_out(f, fi, fo) for f in fr] + [1])
            pos = torch.empty(B, Lo, self.V, 6 if interleaved else 3, dtype=dt, device=dv)
            nrm = torch.empty(B, Lo, self.V, 3, dtype=dt, device=dv) if normals and not interleaved else None
        else:
            pos, nrm = out
            Lo = int(pos.shape[1]) if pos.dim() == 4 else 0
            for t, w in ((pos, 6 if interleaved else 3), (nrm, 3)):
                if t is not None and (t.dtype != dt or t.device != dv or tuple(t.shape) != (B, Lo, self.V, w) or not t.is_contiguous()):
                    raise FdmError(f"out must be contiguous {dt} [{B}, L_out_max, {self.V}, {w}] tensors on {dv}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        fa, got = (C.c_int * B)(*fr), (C.c_int * B)()
        with torch.cuda.device(dv):
            check(lib().fdm_mesh_forward(self.h, x.data_ptr(), fa, B, L_max, None if tp is None else tp.data_ptr(), rows, fi, fo, flags,
                                         pos.data_ptr(), None if nrm is None or not normals or interleaved else nrm.data_ptr(), Lo, got,
                                         torch.cuda.current_stream(dv).cuda_stream))
        self._keep = (x, tp)          # read asynchronously on this stream
        return MeshFrames(pos, nrm if normals and not interleaved else None, list(got))
