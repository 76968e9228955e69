"""Mesh hand-off: decoded vertex offsets -> positions (+ template) at the consumer's frame rate and area-weighted vertex normals, on
the device (include/fdm_hip.h, fdm_mesh_*; kernels csrc/mesh_out.hpp; DESIGN.md section 2 item 18 is the definition)."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import FdmError, check, lib
from .handoff import HandoffPlan, fps_pair, frames_list, frames_out, frames_out_max, offsets_batch  # noqa: F401  (frames_out: fdm_mesh_frames, public here)

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


class MeshOutPlan(HandoffPlan):
    """Thin binding of fdm_mesh_create / fdm_mesh_forward for one topology: the incident-face lists are built and uploaded here,
    forward() only passes pointers.  A plan holds one scratch: it serves one stream at a time (one plan per stream for concurrent
    calls; pipeline.to_mesh keeps them per (device, stream, topology))."""

    _destroy = "fdm_mesh_destroy"

    def __init__(self, faces, V, device="cuda:0"):
        super().__init__(device)
        self.faces, self.V = faces_array(faces), int(V)
        self._create("fdm_mesh_create", self.faces.ctypes.data, len(self.faces), self.V)

    def forward(self, offsets, frames=None, template=None, fps=None, normals=True, interleaved=False, half=False, out=None):
        """offsets [B, L_max, 3 V] (or [L, 3 V]) fp32 on the plan's device, frames: L per clip (None: L_max), template [1 or B, 3 V],
        fps = (fps_in, fps_out) or None -> MeshFrames.  out: (positions, normals) tensors to write instead of new ones (normals
        None where the call writes none); their second dimension is L_out_max.  New outputs are L_out_max = max(frames out) long."""
        dv = self.device
        x = offsets_batch(offsets, self.V, dv)
        B, L_max = int(x.shape[0]), int(x.shape[1])
        fr, (fi, fo) = frames_list(frames, B, L_max), fps_pair(fps)
        tp, rows = None, 0
        if template is not None:
            tp = torch.as_tensor(template, dtype=torch.float32).to(dv).reshape(-1, 3 * self.V).contiguous()
            rows = int(tp.shape[0])
        flags = (_lib.MESH_INTERLEAVED if interleaved else 0) | (_lib.MESH_F16 if half else 0) | (_lib.MESH_NORMALS if normals else 0)
        dt = torch.float16 if half else torch.float32
        if out is None:
            Lo = frames_out_max(fr, fi, fo)
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
