"""Render hand-off: the animated mesh -> shaded image frames, a depth image and a face-id image, on the device (include/fdm_hip.h,
fdm_render_*; kernels csrc/render_out.hpp; DESIGN.md section 2 item 23 is the definition).  The definition is this project's own -- a
pinhole camera, exact integer coverage, a maximum of 1 / depth per pixel, a Lambert sum over directional lights: the reference's camera
numbers and light directions are the defaults here, its metallic-roughness material is not reproduced."""
import ctypes as C
import hashlib
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from ._lib import FdmError, RenderMaterial, RenderPlanes, check, lib
from .handoff import HandoffPlan, fps_pair, frames_list, frames_out_max, offsets_batch
from .mesh import faces_array

# images [B, L_out_max, H, W, 3] uint8, depth [B, L_out_max, H, W] float32 or None (0 where no surface), face_ids [B, L_out_max, H, W] int32
# or None (-1 where no surface), frames = L_out per clip (rows at or past it are zeros)
# alpha [B, L_out_max, H, W] uint8 or None (coverage: 255 n / S rounded, n of the pixel's S samples covered), yuv [B, L_out_max, 3 W H / 2]
# uint8 or None (each frame's Y'CbCr 4:2:0 planes, I420 or NV12, as ffmpeg's rawvideo reads them)
ImageFrames = namedtuple("ImageFrames", "images depth face_ids frames alpha yuv", defaults=(None, None))

MAX_LIGHTS = 8
REFERENCE_F = 4754.97941935      # render/render.py: the focal length at 800 x 800 is this over 2 (vocaset, MEAD) or over 8 (BIWI)
LIGHT_INTENSITY = 0.5            # this project's choice: a normal facing the camera under the five default lights gives
#                                  k = 0.2 + 0.5 (1 + 4 cos(pi / 6)) = 2.43 and a channel of 0.3 k = 0.73, below saturation


class Camera:
    """A pinhole camera: fx, fy, cx, cy in pixels of a width x height image, near / far in scene units, world-to-camera rotation R [3, 3]
    and translation t [3] (pc = R p + t; the camera looks down its -z axis, x to the right, y up).  The default stands 1 unit in front
    of the origin, as the reference's does."""

    def __init__(self, fx, fy, cx, cy, width, height, near=0.01, far=3.0, R=None, t=(0.0, 0.0, -1.0)):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.width, self.height, self.near, self.far = int(width), int(height), float(near), float(far)
        self.R = np.eye(3, dtype=np.float32) if R is None else np.ascontiguousarray(np.asarray(R, dtype=np.float32).reshape(3, 3))
        self.t = np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(3))

    @classmethod
    def preset(cls, name):
        """The reference's cameras (render/render.py, render_mead.py): 800 x 800, principal point (400, 400), near 0.01, far 3."""
        div = {"vocaset": 2.0, "biwi": 8.0, "mead": 2.0}.get(str(name).lower())
        if div is None:
            raise ValueError(f"camera preset {name!r}: vocaset, biwi or mead")
        return cls(REFERENCE_F / div, REFERENCE_F / div, 400.0, 400.0, 800, 800)

    def resized(self, width, height):
        """The same view on a width x height image: the intrinsics scale with the image."""
        sx, sy = width / self.width, height / self.height
        return Camera(self.fx * sx, self.fy * sy, self.cx * sx, self.cy * sy, width, height, self.near, self.far, self.R, self.t)

    def with_pose(self, R=None, t=None):
        return Camera(self.fx, self.fy, self.cx, self.cy, self.width, self.height, self.near, self.far, self.R if R is None else R,
                      self.t if t is None else t)

    def numbers(self):
        """camera [6] float32 = {fx, fy, cx, cy, near, far} as fdm_render_create reads it"""
        return np.array([self.fx, self.fy, self.cx, self.cy, self.near, self.far], dtype=np.float32)


def reference_lights():
    """dict(lights [5, 4], ambient, base): the reference's five directions -- towards the camera, and that direction turned by +-pi/6
    about x and about y -- as unit vectors towards the light in camera space, each with LIGHT_INTENSITY; ambient 0.2 and base colour
    0.3 are the reference's."""
    a = math.pi / 6.0
    s, c = math.sin(a), math.cos(a)
    d = [(0.0, 0.0, 1.0), (0.0, -s, c), (0.0, s, c), (-s, 0.0, c), (s, 0.0, c)]
    return dict(lights=np.array([x + (LIGHT_INTENSITY,) for x in d], dtype=np.float32), ambient=0.2, base=(0.3, 0.3, 0.3))


SAMPLE_COUNTS = (1, 4, 16)          # coverage samples per pixel (fdm_render_set "samples")


def sample_pattern(n):
    """The offsets of the n = 1, 4 or 16 coverage samples of a pixel, int32 [n, 2] = (x, y) in 1/256 pixel from the pixel's corner
    (fdm_render_sample_pattern_host; no device needed)."""
    xy = np.zeros((max(int(n), 0), 2), dtype=np.int32)
    check(lib().fdm_render_sample_pattern_host(int(n), xy.ctypes.data))
    return xy


YUV_RANGES = {"limited": 0, "full": 1}          # fdm_render_set "yuv_range"
YUV_LAYOUTS = {"i420": 0, "nv12": 1}            # fdm_render_set "yuv_layout"


def yuv_coeffs(matrix, full_range):
    """int32 [10] = {yr, yg, yb, ur, ug, ub, vr, vg, vb, y0}: the 16-bit fixed-point numbers of the RGB -> Y'CbCr conversion for matrix
    601 or 709, limited or full range (fdm_render_yuv_coeffs_host; no device needed)."""
    k = np.zeros(10, dtype=np.int32)
    check(lib().fdm_render_yuv_coeffs_host(int(matrix), int(bool(full_range)), k.ctypes.data))
    return k


def write_y4m(path, yuv, frames, width, height, fps, full_range=False):
    """One clip's I420 frames as a YUV4MPEG2 file (which ffmpeg, mpv and the encoders' own command lines read): yuv uint8
    [L_out_max, 3 W H / 2] or [1, L_out_max, 3 W H / 2], a tensor or an array; frames: how many of them are live (an int, or the
    ImageFrames.frames of one clip); fps: a number or (num, den); full_range: what the plan's yuv_range was.  The header is
    `YUV4MPEG2 W.. H.. F<num>:<den> Ip A1:1 C420jpeg XCOLORRANGE=FULL|LIMITED`, then `FRAME` and the frame's bytes per live frame.
    NV12 has no Y4M form: save those bytes raw.  Returns the file's size in bytes."""
    a = yuv.detach().cpu().numpy() if isinstance(yuv, torch.Tensor) else np.asarray(yuv)
    W, H = int(width), int(height)
    n = 3 * W * H // 2
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    L = int(frames[0] if isinstance(frames, (list, tuple)) else frames)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != n or W % 2 or H % 2 or not 0 <= L <= a.shape[0]:
        raise FdmError(f"write_y4m takes one clip's uint8 [L_out_max >= {L}, {n}] I420 frames of an even {W} x {H}, got {a.dtype} {a.shape}")
    num, den = (int(fps[0]), int(fps[1])) if isinstance(fps, (list, tuple)) else Fraction(fps).limit_denominator(1001).as_integer_ratio()
    head = f"YUV4MPEG2 W{W} H{H} F{num}:{den} Ip A1:1 C420jpeg XCOLORRANGE={'FULL' if full_range else 'LIMITED'}\n".encode()
    with open(path, "wb") as f:
        f.write(head)
        for t in range(L):
            f.write(b"FRAME\n")
            f.write(np.ascontiguousarray(a[t]).tobytes())
    return len(head) + L * (6 + n)


# ---- materials (include/fdm_hip.h, fdm_render_set_material)
FILTERS = {"nearest": 0, "bilinear": 1}
# this project's own control points (position in [0, 1], (r, g, b)); "monotone": no channel ever falls along the table
COLORMAPS = {
    "grey": (((0.0, (0.0, 0.0, 0.0)), (1.0, (1.0, 1.0, 1.0))), True),
    "heat": (((0.0, (0.0, 0.0, 0.0)), (0.375, (1.0, 0.0, 0.0)), (0.75, (1.0, 1.0, 0.0)), (1.0, (1.0, 1.0, 1.0))), True),
    "jet": (((0.0, (0.0, 0.0, 0.5)), (0.125, (0.0, 0.0, 1.0)), (0.375, (0.0, 1.0, 1.0)), (0.625, (1.0, 1.0, 0.0)), (0.875, (1.0, 0.0, 0.0)),
             (1.0, (0.5, 0.0, 0.0))), False),
}


def colormap(name, n=256):
    """float32 [n, 3], 2 <= n <= 1024: the table `name` ("heat", "jet" or "grey") from COLORMAPS' control points, piecewise linear in
    fp64 at i / (n - 1), rounded to fp32.  The end points are the first and the last control point exactly."""
    if name not in COLORMAPS:
        raise ValueError(f"colormap {name!r}: {', '.join(sorted(COLORMAPS))}")
    if not 2 <= int(n) <= 1024:
        raise ValueError(f"colormap: n = {n} (2 .. 1024)")
    pts = COLORMAPS[name][0]
    at = np.array([p[0] for p in pts], dtype=np.float64)
    t = np.arange(int(n), dtype=np.float64) / float(int(n) - 1)
    return np.stack([np.interp(t, at, np.array([p[1][c] for p in pts], dtype=np.float64)) for c in range(3)], axis=1).astype(np.float32)


def uv_corners(vt, ft):
    """A UV set with a face list of its own (FLAME's vt [T, 2] and ft [F, 3]) -> float32 [F, 3, 2], one (u, v) per face corner: what
    Material.texture takes.  A vertex on a seam has one vt per side, so nothing is split."""
    vt, ft = np.asarray(vt, dtype=np.float32), np.asarray(ft)
    if vt.ndim != 2 or vt.shape[1] != 2 or ft.ndim != 2 or ft.shape[1] != 3 or not np.issubdtype(ft.dtype, np.integer):
        raise ValueError(f"uv_corners takes vt [T, 2] and integer ft [F, 3], got {vt.shape} and {ft.dtype} {ft.shape}")
    if len(ft) and (ft.min() < 0 or ft.max() >= len(vt)):
        raise ValueError(f"uv_corners: ft names entries {int(ft.min())} .. {int(ft.max())} of {len(vt)}")
    return np.ascontiguousarray(vt[ft])


class Material:
    """What stands where the base colour stands in the shade (fdm_render_set_material): state of a RenderPlan.  Made by
    Material.vertex_colors(c [V, 3] >= 0), Material.scalar_map(a table [N, 3] or a colormap's name, lo, hi) -- the call then brings
    scalars [B, L, V], mapped lo -> the table's first row, hi -> its last, NaN -> its first -- or Material.texture(image [Ht, Wt, 3]
    uint8 with row 0 at the top, uv [F, 3, 2] per face corner (uv_corners), filter "bilinear" or "nearest"; no mip levels: a minified
    texture aliases, samples=16 is the remedy), each with unlit=True for k = 1 in place of the Lambert sum; Material.base(unlit=) is
    the base colour.  What is wrong with the arrays themselves is a ValueError here, before any plan.  `token` names the material to the
    plan caches; the arrays are copied and kept read-only, so it cannot go stale."""

    def __init__(self, kind, unlit=False, colors=None, lut=None, lo=0.0, hi=1.0, uv=None, image=None, filter="bilinear"):  # noqa: A002
        self.kind, self.unlit = int(kind), bool(unlit)
        self.colors = self.lut = self.uv = self.image = None
        self.lo, self.hi, self.filter = np.float32(lo), np.float32(hi), str(filter).lower()
        bad = lambda a: not np.isfinite(a).all() or (a < 0).any()  # noqa: E731
        if self.kind == 1:
            self.colors = np.array(colors, dtype=np.float32, order="C")
            if self.colors.ndim != 2 or self.colors.shape[1] != 3 or bad(self.colors):
                raise ValueError(f"vertex colours are [V, 3], finite and >= 0, got {self.colors.shape}")
        elif self.kind == 2:
            self.lut = colormap(lut) if isinstance(lut, str) else np.array(lut, dtype=np.float32, order="C")
            if self.lut.ndim != 2 or self.lut.shape[1] != 3 or not 2 <= len(self.lut) <= 1024 or bad(self.lut):
                raise ValueError(f"a colour table is [N, 3] with 2 <= N <= 1024, finite and >= 0, got {self.lut.shape}")
            with np.errstate(all="ignore"):
                span = self.hi - self.lo
            if not (np.isfinite(self.lo) and np.isfinite(self.hi) and self.lo < self.hi and np.isfinite(span)):
                raise ValueError(f"a scalar map's range is finite with lo < hi, got lo = {lo}, hi = {hi}")
        elif self.kind == 3:
            img = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or not (1 <= img.shape[0] <= 8192 and 1 <= img.shape[1] <= 8192):
                raise ValueError(f"a texture is uint8 [Ht, Wt, 3] with 1 <= Wt, Ht <= 8192, got {img.dtype} {img.shape}")
            self.image, self.uv = np.array(img, order="C"), np.array(uv, dtype=np.float32, order="C")
            if self.uv.ndim != 3 or self.uv.shape[1:] != (3, 2):
                raise ValueError(f"uv is [F, 3, 2], one pair per face corner (uv_corners makes it from vt and ft), got {self.uv.shape}")
            if self.filter not in FILTERS:
                raise ValueError(f"filter = {filter!r}: nearest or bilinear")
        elif self.kind != 0:
            raise ValueError(f"material kind {kind}: 0 base, 1 vertex colours, 2 scalar map, 3 texture")
        d = hashlib.sha1()
        for a in (self.colors, self.lut, self.uv, self.image):      # the material's own copies, read-only: the token stays true
            if a is not None:
                a.flags.writeable = False
                d.update(repr(a.shape).encode() + a.tobytes())
        self.token = (self.kind, self.unlit, float(self.lo), float(self.hi), self.filter if self.kind == 3 else "", d.hexdigest())

    @classmethod
    def base(cls, unlit=False):
        return cls(0, unlit)

    @classmethod
    def vertex_colors(cls, c, unlit=False):
        return cls(1, unlit, colors=c)

    @classmethod
    def scalar_map(cls, lut_or_name, lo, hi, unlit=False):
        return cls(2, unlit, lut=lut_or_name, lo=lo, hi=hi)

    @classmethod
    def texture(cls, image, uv, filter="bilinear", unlit=False):  # noqa: A002
        return cls(3, unlit, uv=uv, image=image, filter=filter)

    def descriptor(self, V, F):
        """The fdm_render_material of this material for a mesh of V vertices and F faces (it points into this object's arrays)."""
        if self.kind == 1 and len(self.colors) != V:
            raise ValueError(f"the material has {len(self.colors)} vertex colours, the mesh {V} vertices")
        if self.kind == 3 and len(self.uv) != F:
            raise ValueError(f"the material has uv for {len(self.uv)} faces, the mesh {F} faces")
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        h, w = self.image.shape[:2] if self.kind == 3 else (0, 0)
        return RenderMaterial(self.kind, int(self.unlit), ptr(self.colors), ptr(self.lut), 0 if self.lut is None else len(self.lut), float(self.lo),
                              float(self.hi), ptr(self.uv), ptr(self.image), int(w), int(h), FILTERS.get(self.filter, 0))


def vertex_error(pred, gt):
    """Per-vertex distance |pred - gt| on the device (fdm_op_vertex_dist): pred and gt float32 device tensors of one shape, [..., 3 V] (at
    most three dimensions) or [B, L, V, 3] -> [..., V] float32: the scalars of an error heat map (Material.scalar_map)."""
    if not (isinstance(pred, torch.Tensor) and isinstance(gt, torch.Tensor)) or not pred.is_cuda or pred.dtype != torch.float32:
        raise FdmError("vertex_error runs on float32 device tensors (no CPU fallback)")
    if gt.shape != pred.shape or gt.dtype != pred.dtype or gt.device != pred.device:
        raise ValueError(f"vertex_error: pred is {pred.dtype} {tuple(pred.shape)} on {pred.device}, gt {gt.dtype} {tuple(gt.shape)} on {gt.device}")
    if pred.dim() < 1 or pred.dim() > 4 or (pred.dim() == 4 and pred.shape[-1] != 3) or (pred.dim() < 4 and pred.shape[-1] % 3) or not pred.numel():
        raise ValueError(f"vertex_error takes [..., 3 V] or [B, L, V, 3], got {tuple(pred.shape)}")
    lead = tuple(pred.shape[:-2]) + (int(pred.shape[-2]),) if pred.dim() == 4 else tuple(pred.shape[:-1]) + (int(pred.shape[-1]) // 3,)
    a, b = pred.detach().contiguous(), gt.detach().contiguous()
    V = lead[-1]
    out = torch.empty(lead, dtype=torch.float32, device=pred.device)
    with torch.cuda.device(pred.device):
        check(lib().fdm_op_vertex_dist(a.data_ptr(), b.data_ptr(), out.data_ptr(), out.numel() // V, V, torch.cuda.current_stream(pred.device).cuda_stream))
    return out


def _arguments(camera, lights=None, ambient=None, base=None, background=(1.0, 1.0, 1.0), chunk_frames=0, samples=1, yuv_matrix=709,
               yuv_range="limited", yuv_layout="i420", material=None):
    if material is not None and not isinstance(material, Material):
        raise ValueError(f"material= takes a render.Material, got {type(material).__name__}")
    ref = reference_lights()
    if isinstance(camera, str):
        camera = Camera.preset(camera)
    lt = ref["lights"] if lights is None else np.asarray(lights, dtype=np.float32).reshape(-1, 4)
    three = lambda x: np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float32), (3,)))  # noqa: E731
    rng, lay = str(yuv_range).lower(), str(yuv_layout).lower()
    if int(yuv_matrix) not in (601, 709) or rng not in YUV_RANGES or lay not in YUV_LAYOUTS:
        raise FdmError(f"yuv_matrix = {yuv_matrix!r} (601 or 709), yuv_range = {yuv_range!r} (limited or full), yuv_layout = {yuv_layout!r} (i420 or nv12)")
    return dict(camera=camera, lights=np.ascontiguousarray(lt), ambient=float(ref["ambient"] if ambient is None else ambient),
                base=three(ref["base"] if base is None else base), background=three(background), chunk_frames=int(chunk_frames),
                samples=int(samples), yuv_matrix=int(yuv_matrix), yuv_range=rng, yuv_layout=lay, material=material)


def _view_key(a):
    d = hashlib.sha1()
    cam = a["camera"]
    for x in (cam.numbers(), cam.R, cam.t, a["lights"], a["base"], a["background"]):
        d.update(x.tobytes())
    key = (cam.width, cam.height, a["ambient"], a["chunk_frames"], a["samples"], a["yuv_matrix"], a["yuv_range"], a["yuv_layout"], d.hexdigest())
    return key if a.get("material") is None else key + (a["material"].token,)      # (no material: the key it always was)


def identity(faces, V, camera, lights=None, ambient=None, base=None, background=(1.0, 1.0, 1.0), chunk_frames=0, samples=1, yuv_matrix=709,
             yuv_range="limited", yuv_layout="i420", material=None):
    """RenderPlan(...).key without making the plan: (V, digest of the faces, the view, the sample count and the yuv settings among it,
    and with a material its token)."""
    return (int(V), hashlib.sha1(faces_array(faces).tobytes()).hexdigest()) + _view_key(_arguments(camera, lights, ambient, base, background, chunk_frames,
                                                                                                    samples, yuv_matrix, yuv_range, yuv_layout, material))


class RenderPlan(HandoffPlan):
    """Thin binding of fdm_render_create / fdm_render_forward for one topology and one view: faces [F, 3] over V vertices, camera (a
    Camera or a preset's name), lights [n <= 8, 4] = unit direction towards the light in camera space and intensity (None: the
    reference's five), ambient, base colour [3], background [3] in [0, 1] (white, as the reference's default), chunk_frames (0: scratch
    under 256 MB), samples (1, 4 or 16 coverage samples per pixel: anti-aliased frames; the scratch holds 8 W H
    samples bytes per frame), yuv_matrix (601 or 709), yuv_range ("limited" or "full") and yuv_layout ("i420" or "nv12") of the 4:2:0
    planes that forward(yuv=True) writes.  The faces are checked and uploaded here; forward() only passes pointers.  A plan holds one scratch: it serves one
    stream at a time (pipeline.to_images keeps them per (device, stream, topology, view)).  Without a visible device the plan still
    validates and forward() raises."""

    _destroy = "fdm_render_destroy"
    _PLANES = ("rgb", "depth", "face_ids", "alpha", "yuv")

    def __init__(self, faces, V, camera, lights=None, ambient=None, base=None, background=(1.0, 1.0, 1.0), chunk_frames=0, samples=1,
                 yuv_matrix=709, yuv_range="limited", yuv_layout="i420", material=None, device="cuda:0"):
        super().__init__(device)
        self.faces, self.V = faces_array(faces), int(V)
        self.view = _arguments(camera, lights, ambient, base, background, chunk_frames, samples, yuv_matrix, yuv_range, yuv_layout, material)
        if material is not None:
            material.descriptor(self.V, len(self.faces))      # (a material that does not fit the mesh: before the object is made)
        a = self.view
        cam = a["camera"]
        self.W, self.H = cam.width, cam.height
        self._create("fdm_render_create", self.faces.ctypes.data, len(self.faces), self.V, self.W, self.H, cam.numbers().ctypes.data, cam.R.ctypes.data,
                     cam.t.ctypes.data, a["lights"].ctypes.data if len(a["lights"]) else None, len(a["lights"]), a["ambient"], a["base"].ctypes.data,
                     a["background"].ctypes.data)
        if a["chunk_frames"]:
            self.set_chunk_frames(a["chunk_frames"])
        if a["samples"] != 1:
            self.set_samples(a["samples"])
        if (a["yuv_matrix"], a["yuv_range"], a["yuv_layout"]) != (709, "limited", "i420"):
            self.set_yuv(a["yuv_matrix"], a["yuv_range"], a["yuv_layout"])
        if material is not None:
            self.set_material(material)
        self.key = identity(self.faces, self.V, **a)

    def arguments(self):
        """The arguments that make this plan again (on another device or stream)."""
        return dict(faces=self.faces, V=self.V, **self.view)

    def set_view(self, camera=None, lights=None, ambient=None):
        """Another camera pose / intrinsics (same image size), other lights or ambient term, without a new plan (fdm_render_set_view)."""
        a = self.view
        cam = a["camera"] if camera is None else camera
        if (cam.width, cam.height) != (self.W, self.H):
            raise FdmError(f"set_view keeps the image size {self.W} x {self.H}, got {cam.width} x {cam.height}")
        lt = a["lights"] if lights is None else np.ascontiguousarray(np.asarray(lights, dtype=np.float32).reshape(-1, 4))
        amb = a["ambient"] if ambient is None else float(ambient)
        check(lib().fdm_render_set_view(self.h, cam.numbers().ctypes.data, cam.R.ctypes.data, cam.t.ctypes.data, lt.ctypes.data if len(lt) else None,
                                        len(lt), amb))
        self.view = dict(a, camera=cam, lights=lt, ambient=amb)
        self.key = identity(self.faces, self.V, **self.view)

    def set_chunk_frames(self, n):
        """Frames per chunk of scratch (0: the default).  The pixels do not depend on it."""
        check(lib().fdm_render_set(self.h, b"chunk_frames", int(n)))
        self.view = dict(self.view, chunk_frames=int(n))

    def set_samples(self, n):
        """Coverage samples per pixel: 1, 4 or 16 (fdm_render_set "samples").  The plan's key follows: plans of different sample counts
        are different plans to pipeline's cache."""
        check(lib().fdm_render_set(self.h, b"samples", int(n)))
        self.view = dict(self.view, samples=int(n))
        self.key = identity(self.faces, self.V, **self.view)

    def set_material(self, material):
        """The plan's material (a Material, or None: the base colour again; fdm_render_set_material).  The plan's key follows, as with
        set_samples.  A scalar map makes forward() take scalars=."""
        if material is not None and not isinstance(material, Material):
            raise ValueError(f"set_material takes a render.Material or None, got {type(material).__name__}")
        desc = None if material is None else material.descriptor(self.V, len(self.faces))
        check(lib().fdm_render_set_material(self.h, None if desc is None else C.byref(desc)))
        self.view = dict(self.view, material=material)
        self.key = identity(self.faces, self.V, **self.view)

    def set_yuv(self, matrix=None, range=None, layout=None):  # noqa: A002 (the C key is "yuv_range")
        """The 4:2:0 planes of forward(yuv=True): matrix 601 or 709, range "limited" or "full", layout "i420" or "nv12" (None: as it is;
        fdm_render_set "yuv_matrix" / "yuv_range" / "yuv_layout").  The plan's key follows, as with set_samples."""
        a = self.view
        new = _arguments(a["camera"], yuv_matrix=a["yuv_matrix"] if matrix is None else matrix, yuv_range=a["yuv_range"] if range is None else range,
                         yuv_layout=a["yuv_layout"] if layout is None else layout)
        check(lib().fdm_render_set(self.h, b"yuv_matrix", new["yuv_matrix"]))
        check(lib().fdm_render_set(self.h, b"yuv_range", YUV_RANGES[new["yuv_range"]]))
        check(lib().fdm_render_set(self.h, b"yuv_layout", YUV_LAYOUTS[new["yuv_layout"]]))
        self.view = dict(a, yuv_matrix=new["yuv_matrix"], yuv_range=new["yuv_range"], yuv_layout=new["yuv_layout"])
        self.key = identity(self.faces, self.V, **self.view)

    def forward(self, positions, frames=None, template=None, fps=None, normals=None, depth=False, face_ids=False, out=None, rgb=True,
                alpha=False, yuv=False, scalars=None):
        """positions [B, L_max, 3 V] (or [L, 3 V]) fp32 on the plan's device -- vertices, or offsets with template [1 or B, 3 V] --, frames:
        L per clip (None: L_max), fps = (fps_in, fps_out) or None, normals [B, L_out_max, V, 3] fp32 (what to_mesh returns for the same
        frames; None: computed here by the same kernel) -> ImageFrames.  out: (images, depth, face_ids) tensors to write instead of
        new ones (None where the call writes none); their second dimension is L_out_max.
        rgb=False, alpha=True or yuv=True choose the planes form (fdm_render_forward_planes): images only with rgb, alpha
        [B, L_out_max, H, W] uint8 coverage, yuv [B, L_out_max, 3 W H / 2] uint8 in the plan's matrix, range and layout (W and H even).
        out may also be a dict keyed rgb / depth / face_ids / alpha / yuv: the call then writes exactly its tensors, whatever the flags
        say.  A call that makes rgb and neither alpha nor yuv, without a dict, is fdm_render_forward as before.
        scalars [B, L_max, V] fp32 (or [L, V]): the field a scalar-map material draws, on the INPUT frames (resampled with the positions);
        required with such a material, refused without one (ValueError)."""
        want = dict(rgb=rgb, depth=depth, face_ids=face_ids, alpha=alpha, yuv=yuv)
        dv = self.device
        x = offsets_batch(positions, self.V, dv)
        B, L_max = int(x.shape[0]), int(x.shape[1])
        mat, sc = self.view.get("material"), None
        if (mat is not None and mat.kind == 2) != (scalars is not None):
            raise ValueError("scalars= goes with a scalar-map material (Material.scalar_map) and with no other: the plan has " +
                             ("none" if mat is None else f"kind {mat.kind}") + (" and the call no scalars" if scalars is None else ""))
        if scalars is not None:
            sc = torch.as_tensor(scalars, dtype=torch.float32).to(dv)
            if sc.numel() != B * L_max * self.V:
                raise ValueError(f"scalars must be [{B}, {L_max}, {self.V}] (one per input frame and vertex), got {tuple(sc.shape)}")
            sc = sc.reshape(B, L_max, self.V).contiguous()
        fr, (fi, fo) = frames_list(frames, B, L_max), fps_pair(fps)
        tp, rows = None, 0
        if template is not None:
            tp = torch.as_tensor(template, dtype=torch.float32).to(dv).reshape(-1, 3 * self.V).contiguous()
            rows = int(tp.shape[0])
        H, W = self.H, self.W
        spec = dict(rgb=(torch.uint8, (H, W, 3)), depth=(torch.float32, (H, W)), face_ids=(torch.int32, (H, W)), alpha=(torch.uint8, (H, W)),
                    yuv=(torch.uint8, (3 * W * H // 2,)))
        if isinstance(out, dict):
            if set(out) - set(self._PLANES):
                raise FdmError(f"out has the keys {sorted(out)}: the outputs are {', '.join(self._PLANES)}")
            given = {k: t for k, t in out.items() if t is not None}
            names = [k for k in self._PLANES if k in given]
        else:
            given = {} if out is None else {k: t for k, t in zip(self._PLANES, out) if t is not None}
            names = [k for k in self._PLANES if want[k] or k in given]
        if not names:
            raise FdmError("the call makes no output: every one of rgb, depth, face_ids, alpha and yuv is off")
        first = next(iter(given.values()), None)
        Lo = frames_out_max(fr, fi, fo) if first is None else (int(first.shape[1]) if first.dim() >= 2 else 0)
        t = {}
        for k in names:
            dt, shp = spec[k]
            shp = (B, Lo) + shp
            t[k] = given.get(k)
            if t[k] is None:
                t[k] = torch.empty(shp, dtype=dt, device=dv)
            elif t[k].dtype != dt or t[k].device != dv or tuple(t[k].shape) != shp or not t[k].is_contiguous():
                raise FdmError(f"out[{k!r}] must be a contiguous {dt} {list(shp)} tensor on {dv}, got {t[k].dtype} {tuple(t[k].shape)} on {t[k].device}")
        nr = None
        if normals is not None:
            nr = normals.detach()
            if nr.dtype != torch.float32 or nr.device != dv or nr.numel() != B * Lo * 3 * self.V or nr.shape[0] != B:
                raise FdmError(f"normals must be float32 [{B}, {Lo}, {self.V}, 3] on {dv}, got {nr.dtype} {tuple(nr.shape)} on {nr.device}")
            nr = nr.contiguous()
        fa, got = (C.c_int * B)(*fr), (C.c_int * B)()
        ptr = lambda a: None if a is None else a.data_ptr()  # noqa: E731
        p = [ptr(t.get(k)) for k in self._PLANES]
        head = (self.h, x.data_ptr(), fa, B, L_max, ptr(tp), rows, fi, fo, ptr(nr))
        with torch.cuda.device(dv):
            tail = (Lo, got, torch.cuda.current_stream(dv).cuda_stream)
            if sc is not None:
                check(lib().fdm_render_forward_material(*head, C.byref(RenderPlanes(*p)), *tail, sc.data_ptr()))
            elif not isinstance(out, dict) and "rgb" in t and "alpha" not in t and "yuv" not in t:
                check(lib().fdm_render_forward(*head, *p[:3], *tail))
            else:
                check(lib().fdm_render_forward_planes(*head, C.byref(RenderPlanes(*p)), *tail))
        self._keep = (x, tp, nr, sc)      # read asynchronously on this stream
        return ImageFrames(t.get("rgb"), t.get("depth"), t.get("face_ids"), list(got), t.get("alpha"), t.get("yuv"))
