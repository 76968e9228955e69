"""Wrap hand-off: a mesh of another topology follows the animated face through a surface binding, on the device (include/fdm_hip.h,
fdm_wrap_*; kernels csrc/wrap_out.hpp; DESIGN.md section 2 item 22 is the definition).  Every target vertex is bound once to a triangle
of the source's rest surface and follows it in every frame.  There is no frame-rate step here: the wrapped frames have the layout
to_mesh and to_rig read, and resampling, normals on the target's triangles, fp16 and a rig fit on the target's own blendshapes are
those calls, AFTER this one."""
import ctypes as C
import hashlib

import numpy as np
import torch

from . import _lib
from ._lib import FdmError, check, lib
from .handoff import HandoffPlan, frames_list, offsets_batch
from .mesh import faces_array

FACE_TILE = 256      # faces per LDS tile of the nearest-face search (csrc/wrap_out.hpp, WRAP_FT): nothing depends on it but the tests' sizes


def _rest(x, what):
    """vertices as a contiguous float32 [n, 3] numpy array (host)"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, 3))
    if not len(x):
        raise FdmError(f"{what}: no vertices")
    return x


def _arguments(src_rest, faces, dst_rest, face_idx=None, weights=None):
    s, f, t = _rest(src_rest, "src_rest"), faces_array(faces), _rest(dst_rest, "dst_rest")
    fi = w = None
    if face_idx is not None:
        fi = np.ascontiguousarray(np.asarray(face_idx).reshape(-1), dtype=np.int32)
        if len(fi) != len(t):
            raise FdmError(f"{len(fi)} face indices for {len(t)} target vertices")
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights.detach().cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float32).reshape(-1))
        if len(w) != len(t):
            raise FdmError(f"{len(w)} weights for {len(t)} target vertices")
    return s, f, t, fi, w


def _key(a):
    d = hashlib.sha1()
    for x in a:
        d.update(b"-" if x is None else x.tobytes())
    return (len(a[0]), len(a[2]), d.hexdigest())


def identity(src_rest, faces, dst_rest, face_idx=None, weights=None):
    """WrapPlan(...).key without making the plan: (V, Vt, digest of every argument)."""
    return _key(_arguments(src_rest, faces, dst_rest, face_idx, weights))


def coords(src_rest, faces, dst_rest, face_idx):
    """(uvh [Vt, 3], dist [Vt]) of fdm_wrap_coords_host for a given binding: fp64 on the host, rounded once; no device needed."""
    s, f, t, fi, _ = _arguments(src_rest, faces, dst_rest, face_idx)
    uvh, dist = np.zeros((len(t), 3), dtype=np.float32), np.zeros(len(t), dtype=np.float32)
    check(lib().fdm_wrap_coords_host(s.ctypes.data, f.ctypes.data, len(f), len(s), t.ctypes.data, len(t), fi.ctypes.data, uvh.ctypes.data, dist.ctypes.data))
    return uvh, dist


def falloff_weights(dist, r0, r1):
    """Weights [Vt] from the binding's distances: 1 inside r0, 0 beyond r1, smoothstep between (host numpy).  For a body mesh of which
    only the face should move: the vertices far from the source surface keep their rest position."""
    if not (0 <= r0 <= r1):
        raise ValueError(f"falloff radii {r0}, {r1}: 0 <= r0 <= r1")
    d = np.asarray(dist, dtype=np.float64)
    x = np.clip((r1 - d) / (r1 - r0), 0.0, 1.0) if r1 > r0 else (d <= r0).astype(np.float64)
    return (x * x * (3.0 - 2.0 * x)).astype(np.float32)


class WrapPlan(HandoffPlan):
    """Thin binding of fdm_wrap_create / fdm_wrap_forward for one pair of meshes: src_rest [V, 3] and faces [F, 3] are the model's rest
    surface, dst_rest [Vt, 3] the target's rest vertices in the same space.  face_idx [Vt] is a binding brought from elsewhere (None: the
    nearest-face search runs on the device, here), weights [Vt] in [0, 1] scale each vertex's displacement from its rest position
    (falloff_weights).  The binding is made and uploaded here; forward() only passes pointers.  A plan serves one stream at a time
    (pipeline.to_wrap keeps them per (device, stream, binding)).  With face_idx given and no visible device the plan still validates
    and forward() raises."""

    _destroy = "fdm_wrap_destroy"

    def __init__(self, src_rest, faces, dst_rest, face_idx=None, weights=None, device="cuda:0"):
        super().__init__(device)
        a = _arguments(src_rest, faces, dst_rest, face_idx, weights)
        self.src_rest, self.faces, self.dst_rest, self.face_idx, self.weights = a
        self.V, self.Vt = len(self.src_rest), len(self.dst_rest)
        self.key = _key(a)            # the binding's identity: what pipeline.to_wrap caches plans by
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        self._create("fdm_wrap_create", self.src_rest.ctypes.data, self.faces.ctypes.data, len(self.faces), self.V, self.dst_rest.ctypes.data,
                     self.Vt, ptr(self.face_idx), ptr(self.weights))

    def arguments(self):
        """The arguments that make this plan again (on another device or stream): the binding found here goes along, so the search
        does not run twice."""
        return dict(src_rest=self.src_rest, faces=self.faces, dst_rest=self.dst_rest, face_idx=self.binding()[0], weights=self.weights)

    def binding(self):
        """(face_idx [Vt] int32, uvh [Vt, 3], dist [Vt]) as numpy: the face each target vertex follows, its coordinates
        q = a + u e1 + v e2 + h nh on it, and its distance to it (what falloff_weights reads)."""
        fi, uvh, dist = np.zeros(self.Vt, dtype=np.int32), np.zeros((self.Vt, 3), dtype=np.float32), np.zeros(self.Vt, dtype=np.float32)
        check(lib().fdm_wrap_binding(self.h, fi.ctypes.data, uvh.ctypes.data, dist.ctypes.data))
        return fi, uvh, dist

    def forward(self, offsets, frames=None, template=None, offsets_out=False, out=None):
        """offsets [B, L_max, 3 V] (or [L, 3 V]) fp32 on the plan's device, frames: L per clip (None: L_max), template [1 or B, 3 V] of the
        SOURCE -> wrapped vertices [B, L_max, 3 Vt] fp32 (rows at or past a clip's frames are zeros); offsets_out: displacements from
        the target's rest position instead (what a rig fit on the target topology reads).  out: a tensor to write instead."""
        dv = self.device
        x = offsets_batch(offsets, self.V, dv)
        B, L_max = int(x.shape[0]), int(x.shape[1])
        fr = frames_list(frames, B, L_max)
        tp, rows = None, 0
        if template is not None:
            tp = torch.as_tensor(template, dtype=torch.float32).to(dv).reshape(-1, 3 * self.V).contiguous()
            rows = int(tp.shape[0])
        if out is None:
            out = torch.empty(B, L_max, 3 * self.Vt, dtype=torch.float32, device=dv)
        elif out.dtype != torch.float32 or out.device != dv or tuple(out.shape) != (B, L_max, 3 * self.Vt) or not out.is_contiguous():
            raise FdmError(f"out must be a contiguous float32 [{B}, {L_max}, {3 * self.Vt}] tensor on {dv}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        fa = (C.c_int * B)(*fr)
        with torch.cuda.device(dv):
            check(lib().fdm_wrap_forward(self.h, x.data_ptr(), fa, B, L_max, None if tp is None else tp.data_ptr(), rows,
                                         _lib.WRAP_OFFSETS if offsets_out else 0, out.data_ptr(), torch.cuda.current_stream(dv).cuda_stream))
        self._keep = (x, tp)          # read asynchronously on this stream
        return out
