"""End-to-end clip pipeline: wav -> processor normalisation -> HuBERT -> T-step sampling -> quant ->
decode (+ template) -> [B, L, V3] vertices, as wired by the reference's coherent callers
(samples/sample_diffusion_vocaset.py:59-88, samples/sample_diffusion_mead.py:67-86) and intended by
demo/demo_*.py:77-106 (flags + I/O layout kept; the demos' undefined names are re-wired per samples/)."""
import os

import numpy as np
import torch

from . import presets, schedule
from ._lib import SLOT_FINISHED, FdmError
from .handoff import cached_plan
from .modules import (FDM, ClassifierFreeSampleModel, FDMBiwi, FDMMead, GaussianDiffusion, VQAutoEncoder)

EMOTIONS = ["angry", "contempt", "disgusted", "fear", "happy", "sad", "surprised"]     # demo/demo_3d_mead.py:118


def load_wav(path, sr=16000):
    """16 kHz mono float32 (librosa.load(sr=16000) of the demos; scipy-based, no librosa here)."""
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    rate, x = wavfile.read(path)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    if x.ndim > 1:
        x = x.mean(axis=1)
    if rate != sr:
        g = np.gcd(int(rate), sr)
        x = resample_poly(x, sr // g, int(rate) // g).astype(np.float32)
    return x


def processor_normalize(x, pad_seconds=1.0, sr=16000):
    """Wav2Vec2Processor default: zero mean / unit variance ((x - mu)/sqrt(var + 1e-7)), then the demo's
    1 s of trailing zeros (demo/demo_vocaset.py:84-90)."""
    x = np.asarray(x, dtype=np.float32)
    x = (x - x.mean()) / np.sqrt(x.var() + 1e-7)
    if pad_seconds:
        x = np.concatenate([x, np.zeros(int(pad_seconds * sr), dtype=np.float32)])
    return x.astype(np.float32)


def load_pcm(path):
    """(samples, rate) of a WAV file as stored: int16 / int32 / uint8 / float32, [frames] or [frames, C].  No arithmetic: conversion,
    downmix, resampling and normalisation are prepare_audio()'s, on the device."""
    from scipy.io import wavfile
    rate, x = wavfile.read(path)
    if x.dtype not in (np.int16, np.int32, np.uint8, np.float32):
        raise ValueError(f"{path}: sample type {x.dtype} (int16, int32, uint8 or float32)")
    return x, int(rate)


def _on_stream(device):
    """(torch.device, (its name, the current stream on it)): what every plan cache below starts its key with."""
    dv = torch.device(device)
    return dv, (str(dv), torch.cuda.current_stream(dv).cuda_stream)


_FRONTENDS = {}      # (device, stream) -> hubert.FrontendPlan holding every rate seen there so far


def _frontend(rates, device):
    """The front-end plan of `device` and the current stream (a plan serves one stream at a time).  ONE plan per (device, stream): a
    rate it has not seen replaces it by a plan for the union (16 kHz needs no table), so what the process keeps is bounded by the
    distinct rates it meets, not by their combinations."""
    from .hubert import FrontendPlan
    key = _on_stream(device)[1]
    want = {int(r) for r in rates} - {16000}
    plan = _FRONTENDS.get(key)
    if plan is None or not want <= set(plan.rates):
        _FRONTENDS[key] = plan = FrontendPlan(want | set(plan.rates if plan else ()), device)
    return plan


def _pcm_tensor(pcm, device):
    """A raw PCM array or tensor on `device`, dtype kept.  A CPU TENSOR is refused as everywhere on the HIP path (the caller's numpy
    array is the host input and is uploaded as it is: no arithmetic happens on the host)."""
    if torch.device(device).type != "cuda":
        raise FdmError("prepare_audio runs on the HIP path only (no CPU fallback)")
    if isinstance(pcm, torch.Tensor):
        if not pcm.is_cuda:
            raise FdmError("prepare_audio needs device tensors or numpy arrays (no CPU fallback on the product path)")
        return pcm.to(device)
    return torch.from_numpy(np.ascontiguousarray(pcm)).to(device)


def prepare_audio_many(pcms, rates, pad_seconds=1.0, device="cuda:0", normalize=True):
    """Raw PCM clips (int16 / int32 / uint8 / float32, [frames] or [frames, C], numpy or device tensors) at rates[b] Hz (or one rate
    for all) -> (wav [B, n_max] fp32 on `device`, lens): load_wav's conversion, downmix and resample_poly, processor_normalize's
    normalisation and padding, in ONE device call (FrontendPlan; include/fdm_hip.h, fdm_frontend_forward).  wav[b, :lens[b]] is
    the clip's waveform, bit for bit what its own prepare_audio() returns; the rest of the row is zeros."""
    rates = [int(rates)] * len(pcms) if np.isscalar(rates) else [int(r) for r in rates]
    ts = [_pcm_tensor(p, device) for p in pcms]
    return _frontend(rates, device).forward(ts, rates, pad=int(pad_seconds * 16000), normalize=normalize)


def prepare_audio(pcm, rate, pad_seconds=1.0, device="cuda:0", normalize=True):
    """One raw PCM clip at `rate` Hz -> the [n] fp32 device waveform animate() takes (prepare_audio_many with B = 1)."""
    wav, lens = prepare_audio_many([pcm], [rate], pad_seconds, device, normalize)
    return wav[0, :lens[0]]


def _mesh_plan(faces, V, device):
    """The mesh hand-off plan of `device`, the current stream and this topology (V, digest of the faces): handoff.cached_plan."""
    import hashlib
    from .mesh import MeshOutPlan, faces_array
    dv, at = _on_stream(device)
    f = faces_array(faces)
    return cached_plan(at, "mesh", (int(V), hashlib.sha1(f.tobytes()).hexdigest()), lambda: MeshOutPlan(f, V, dv))


def _mesh_fps(p, in_fps, out_fps):
    """(fps_in, fps_out) of a hand-off, or None without out_fps: fps_in is the preset's frame rate unless in_fps= states one."""
    if out_fps is None:
        return None
    fi = in_fps or p.fps
    if not fi:
        raise ValueError(f"preset {p.name} states no frame rate: pass in_fps= with out_fps=")
    return float(fi), float(out_fps)


def _split_mesh(mf, _=None):
    """A batched MeshFrames -> one per clip, each cut to its own frames ([1, L_out, V, 3 or 6])."""
    return [type(mf)(mf.positions[b:b + 1, :n], None if mf.normals is None else mf.normals[b:b + 1, :n], [n]) for b, n in enumerate(mf.frames)]


def _pack_offsets(offsets, frames, device, who):
    """What to_mesh / to_rig hand their plan: (x [B, L_max, 3 V] on the device, frames per clip, whether `offsets` was a list).  A
    ragged list of [1, L_b, 3 V] / [L_b, 3 V] clips is packed into one zero-padded batch with frames = its own lengths; a tensor
    goes as it is with the caller's `frames`.  Host tensors or a host `device` are refused in the name of `who`."""
    many = isinstance(offsets, (list, tuple))
    if many:
        clips = [o.reshape(-1, o.shape[-1]) for o in offsets]
        frames = [int(c.shape[0]) for c in clips]
        x = torch.zeros(len(clips), max(frames + [1]), clips[0].shape[-1], device=clips[0].device)
        for b, c in enumerate(clips):
            x[b, :frames[b]] = c
    else:
        x = offsets if offsets.dim() == 3 else offsets.unsqueeze(0)
    dv = x.device if device is None else torch.device(device)
    if dv.type != "cuda" or not x.is_cuda:
        raise FdmError(f"{who} runs on the HIP path only (no CPU fallback)")
    return x.to(dv), frames, many


def _per_clip(who, offsets, frames, template, device, forward, split):
    """What to_mesh, to_rig, to_wrap and to_images share: a list of templates that comes with a ragged list of clips is stacked into
    rows, the offsets are packed (_pack_offsets, in the name of `who`), forward(x, frames, template) is the ONE device call, and for a
    list split(result, frames in) cuts the batch's result into one per clip."""
    if isinstance(offsets, (list, tuple)) and isinstance(template, (list, tuple)):
        template = torch.stack([torch.as_tensor(t, dtype=torch.float32).reshape(-1) for t in template])
    x, frames, many = _pack_offsets(offsets, frames, device, who)
    res = forward(x, frames, template)
    return split(res, frames) if many else res


@torch.no_grad()
def to_mesh(offsets, faces, template=None, frames=None, fps=None, normals=True, interleaved=False, half=False, device=None):
    """Vertex offsets (what the decoder writes; or vertices, with template=None) -> mesh.MeshFrames: positions = offsets + template,
    resampled in time when fps = (fps_in, fps_out) names two different rates, and area-weighted vertex normals over the triangle
    list `faces` [F, 3], in ONE device call (mesh.MeshOutPlan; include/fdm_hip.h, fdm_mesh_forward).
    offsets: a device tensor [B, L, 3 V] (or [L, 3 V]) with frames = L per clip (None: all L) -> one MeshFrames for the batch; or a
    ragged LIST of [1, L_b, 3 V] / [L_b, 3 V] clips -> a list of MeshFrames, each cut to its own frames and bit for bit what its
    own call returns.  template: [1 or B, 3 V], or for a list one per clip.  normals / interleaved / half: the output options."""
    return _per_clip("to_mesh", offsets, frames, template, device, lambda x, fr, tp: _mesh_plan(faces, x.shape[-1] // 3, x.device).forward(
        x, fr, tp, fps, normals, interleaved, half), _split_mesh)


def _bound_plan(kind, given, device):
    """The "rig" or "wrap" hand-off plan of `device`, the current stream and this rig or binding (RigPlan.key / WrapPlan.key).  given: a
    rig.RigPlan / wrap.WrapPlan (used as it is where it was made for this device and stream, made again from its arguments -- a
    binding it found included -- otherwise) or the dict of its arguments (every call then digests the arrays to recognise them:
    animate_many, animate_long and SlotServer come here once, in _Outputs, and go on with the plan)."""
    from . import rig, wrap
    mod, cls = {"rig": (rig, rig.RigPlan), "wrap": (wrap, wrap.WrapPlan)}[kind]
    dv, at = _on_stream(device)
    if isinstance(given, cls):
        return cached_plan(at, kind, given.key, lambda: cls(device=dv, **given.arguments()), given)
    return cached_plan(at, kind, mod.identity(**given), lambda: cls(device=dv, **given))


def _split_rig(rf, _=None):
    """A batched RigFrames -> one per clip, each cut to its own frames ([1, L_out, K])."""
    return [type(rf)(rf.weights[b:b + 1, :n], [n], rf.names) for b, n in enumerate(rf.frames)]


@torch.no_grad()
def to_rig(offsets, basis, frames=None, fps=None, weights=None, ridge=0.0, bounds=None, sweeps=16, names=None, device=None, smooth=0.0,
           smooth_weights=None):
    """Vertex offsets (what the decoder writes, BEFORE the template is added) -> rig.RigFrames: per frame the coefficients c of the
    ridge-regularised, box-constrained least-squares fit of the offsets onto the blendshape basis [K, 3 V] (weights [V] per vertex,
    bounds = (lo, hi), `sweeps` of projected Gauss-Seidel), resampled in time when fps = (fps_in, fps_out) names two different rates,
    in ONE device call (rig.RigPlan; include/fdm_hip.h, fdm_rig_forward).  basis may be a rig.RigPlan or the dict of its arguments
    (the other rig arguments are then not read).  offsets: a device tensor [B, L, 3 V] (or [L, 3 V]) with frames = L per clip (None:
    all L) -> one RigFrames for the batch; or a ragged LIST of [1, L_b, 3 V] / [L_b, 3 V] clips -> a list of RigFrames, each cut to
    its own frames and bit for bit what its own call returns.  smooth > 0 (with smooth_weights [K] or None) fits each clip's frames
    together under a penalty on the change between neighbouring OUTPUT frames (rig.RigPlan): smooth
    curves that still respect the bounds, on the device.  A clip's result does not depend on the clips batched with it."""
    from .rig import RigPlan
    rig = basis if isinstance(basis, (RigPlan, dict)) else dict(basis=basis, weights=weights, ridge=ridge, bounds=bounds, sweeps=sweeps, names=names,
                                                                smooth=smooth, smooth_weights=smooth_weights)
    return _per_clip("to_rig", offsets, frames, None, device, lambda x, fr, _: _bound_plan("rig", rig, x.device).forward(x, fr, fps), _split_rig)


def _flame_plan(model, device, landmarks=None):
    """The parametric-head plan of `device`, the current stream and this model with its landmarks (flame.FlamePlan.key).  model: a
    flame.FlamePlan (used as it is where it was made for this device and stream, made again from its model otherwise), a
    flame.FlameModel (digested once), or the path of a model file (loaded per call: pass a FlameModel)."""
    from .flame import FlameModel, FlamePlan, plan_key
    dv, at = _on_stream(device)
    if isinstance(model, FlamePlan):
        lm = None if model.lv is None else (model.lv, model.lb)
        return cached_plan(at, "flame", model.key, lambda: FlamePlan(model.model, lm, dv), model)
    if not isinstance(model, FlameModel):
        model = FlameModel.load(model)
    return cached_plan(at, "flame", plan_key(model, landmarks), lambda: FlamePlan(model, landmarks, dv))


@torch.no_grad()
def to_flame(pose, model, expression=None, shape=None, transl=None, extra=None, frames=None, landmarks=None, device=None):
    """Parameters -> flame.FlameFrames (posed vertices [B, L, V, 3], landmarks or None) in ONE device call (flame.FlamePlan;
    include/fdm_hip.h, fdm_flame_forward).  model: a flame.FlameModel, a flame.FlamePlan or a model file; pose [B, L, 3 J] (or
    [L, 3 J]) axis-angle; expression [B, L, NE]; shape [NS] or [B, NS]; transl [B, L, 3]; extra [B, L, 3 V]: displacements added before
    skinning -- the decoder's offsets; frames: L per clip; landmarks = (verts [NL, 3], bary [NL, 3]), the static embedding."""
    from .flame import FlamePlan
    if device is None:
        device = next((x.device for x in (extra, pose, expression) if isinstance(x, torch.Tensor) and x.is_cuda), None)
        if device is None and isinstance(model, FlamePlan):
            device = model.device
    if device is None or torch.device(device).type != "cuda":
        raise FdmError("to_flame runs on the HIP path only (no CPU fallback)")
    return _flame_plan(model, device, landmarks).forward(pose, expression, shape, transl, extra, frames)


FLAME_FIT_KEYS = ("model", "n_expr", "joints", "transl", "shape", "pose0", "weights", "iters", "lam", "ridge_expr", "ridge_pose", "pivot_tol", "return_vertices")


def _flame_fit_check(flame_fit):
    """flame_fit= of animate*: a dict with model and no key but FLAME_FIT_KEYS"""
    if not isinstance(flame_fit, dict) or "model" not in flame_fit or set(flame_fit) - set(FLAME_FIT_KEYS):
        raise ValueError(f"flame_fit= takes a dict with model and optionally {FLAME_FIT_KEYS[1:]}; got {sorted(flame_fit) if isinstance(flame_fit, dict) else type(flame_fit).__name__}")


def _split_fit(ft, _=None):
    """A batched FlameFit -> one per clip, each cut to its own frames"""
    cut = lambda x, b, n: None if x is None else x[b:b + 1, :n]  # noqa: E731
    return [type(ft)(cut(ft.expression, b, n), cut(ft.pose, b, n), cut(ft.transl, b, n), cut(ft.rms, b, n), cut(ft.status, b, n), [n], cut(ft.vertices, b, n))
            for b, n in enumerate(ft.frames)]


def _resample_rows(x, frames, fps):
    """x [B, L, C] with frames per clip -> (y [B, Lo_max, C], frames out) by the mesh hand-off's frame rule (interp_taps: ops.linear_interp)"""
    from . import ops
    from .handoff import fps_pair, frames_out
    fi, fo = fps_pair(fps)
    fr = [int(x.shape[1])] * int(x.shape[0]) if frames is None else [int(f) for f in frames]
    if not (fi > 0 and fo > 0 and fi != fo):
        return x, frames
    lo = [frames_out(f, fi, fo) for f in fr]
    y = torch.zeros(x.shape[0], max(lo + [1]), x.shape[2], device=x.device)
    for b, (n, m) in enumerate(zip(fr, lo)):
        if n:
            src, dst = x[b:b + 1, :n].contiguous(), torch.empty(1, m, x.shape[2], device=x.device)
            ops.linear_interp(src, dst, 1, n, m, int(x.shape[2]))
            y[b, :m] = dst[0]
    return y, lo


@torch.no_grad()
def to_flame_params(offsets, model, template=None, frames=None, fps=None, device=None, **fit):
    """Vertex offsets (or vertices, with template=None) -> flame.FlameFit: per frame the expression coefficients, joint rotations and
    optional translation of the head `model` that reproduce offsets + template (flame.FlamePlan.fit; include/fdm_hip.h,
    fdm_flame_fit_forward).  model: a flame.FlameModel, a flame.FlamePlan or a model file.  offsets: a device
    tensor [B, L, 3 V] (or [L, 3 V]) with frames = L per clip -> one FlameFit; or a ragged LIST of clips -> a list, each cut to its own
    frames and bit for bit what its own call returns.  template [1 or B, 3 V] (a list: one per clip).  fps = (in, out): the targets are
    resampled by the mesh hand-off's frame rule before the fit.  **fit: n_expr, joints, transl, shape, pose0, weights, iters, lam,
    ridge_expr, ridge_pose, return_vertices of FlamePlan.fit."""
    def forward(x, fr, tp):
        if tp is not None:
            x = x + _template_rows(tp, x.shape[-1], x.device, 1, int(x.shape[0])).unsqueeze(1)
        x, fr = _resample_rows(x.contiguous(), fr, fps)
        return _flame_plan(model, x.device).fit(x, frames=fr, **fit)
    return _per_clip("to_flame_params", offsets, frames, template, device, forward, _split_fit)


@torch.no_grad()
def to_wrap(offsets, wrap, template=None, frames=None, offsets_out=False, device=None):
    """Vertex offsets of the model's topology (or vertices, with template=None) -> the vertices [B, L, 3 Vt] of a mesh of ANOTHER
    topology that is bound to the model's rest surface, in ONE device call (wrap.WrapPlan; include/fdm_hip.h, fdm_wrap_forward).
    wrap: a wrap.WrapPlan or the dict of its arguments (src_rest, faces, dst_rest, face_idx, weights).  offsets: a device tensor
    [B, L, 3 V] (or [L, 3 V]) with frames = L per clip (None: all L; rows past a clip's frames come out as zeros); or a ragged LIST of
    [1, L_b, 3 V] / [L_b, 3 V] clips -> a list of [1, L_b, 3 Vt], each bit for bit what its own call returns.  template: [1 or B, 3 V] of
    the SOURCE, or for a list one per clip.  offsets_out: displacements from the target's rest position instead of positions -- a rig
    on the target's own blendshapes is to_rig(to_wrap(..., offsets_out=True), basis_t).  There is no frame-rate step here: resample
    AFTER, with to_mesh(wrapped, faces_t, None, fps=) or to_rig(..., fps=)."""
    return _per_clip("to_wrap", offsets, frames, template, device, lambda x, fr, tp: _bound_plan("wrap", wrap, x.device).forward(x, fr, tp, offsets_out),
                     lambda y, fr: [y[b:b + 1, :n] for b, n in enumerate(fr)])


TIME_FILTER_KEYS = ("taps", "kind", "sigma", "seconds", "order", "radius", "edge", "strength")
TIME_RECUR_KEYS = ("kind", "fps", "cutoff", "min_cutoff", "beta", "d_cutoff", "direction", "strength")      # kind="ema" | "one_euro"


def _time_filter_arguments(time_filter, fps=None):
    """time_filter= of animate* and to_filtered: a tfilter.TimeFilterPlan as it is, or the dict of its arguments after V (no key but
    TIME_FILTER_KEYS) with seconds= in place of sigma= converted by the model's frame rate `fps`; for kind="ema" | "one_euro" no key but
    TIME_RECUR_KEYS, fps= defaulting to the model's frame rate and direction= to "zero_phase".  A ValueError for anything else."""
    from .tfilter import RECUR_KINDS, TimeFilterPlan
    if isinstance(time_filter, TimeFilterPlan):
        return time_filter
    recur = isinstance(time_filter, dict) and time_filter.get("kind") in RECUR_KINDS
    keys = TIME_RECUR_KEYS if recur else TIME_FILTER_KEYS
    if not isinstance(time_filter, dict) or set(time_filter) - set(keys):
        raise ValueError(f"time_filter= takes a tfilter.TimeFilterPlan or a dict with {keys}; got "
                         f"{sorted(time_filter) if isinstance(time_filter, dict) else type(time_filter).__name__}")
    kw = dict(time_filter)
    if recur:
        if kw.get("fps") is None:
            if not fps:
                raise ValueError(f"time_filter=dict(kind={kw['kind']!r}) needs the model's frame rate: the preset states none, pass in_fps=")
            kw["fps"] = float(fps)
        kw["direction"] = kw.get("direction") or "zero_phase"
        return kw
    if kw.get("seconds") is not None:
        if kw.get("sigma") is not None:
            raise ValueError("time_filter= takes sigma= (frames) or seconds=, not both")
        if not fps:
            raise ValueError("time_filter=dict(seconds=) needs the model's frame rate: the preset states none, pass in_fps=")
        kw["sigma"] = float(kw["seconds"]) * float(fps)
    kw.pop("seconds", None)
    return kw


def _time_filter_plan(time_filter, V, device, fps=None):
    """The time filter plan of `device`, the current stream and this filter (tfilter.TimeFilterPlan.key): a plan is used as it is where
    it was made for this device and stream and made again from its arguments otherwise; a dict is digested to recognise it."""
    from .tfilter import TimeFilterPlan, identity
    dv, at = _on_stream(device)
    given = _time_filter_arguments(time_filter, fps)
    if isinstance(given, TimeFilterPlan):
        if given.V != int(V):
            raise FdmError(f"the time filter plan is for {given.V} vertices, the frames have {int(V)}")
        return cached_plan(at, "tfilter", given.key, lambda: TimeFilterPlan(device=dv, **given.arguments()), given)
    return cached_plan(at, "tfilter", identity(int(V), **given), lambda: TimeFilterPlan(int(V), device=dv, **given))


@torch.no_grad()
def to_filtered(offsets, time_filter, frames=None, fps=None, device=None):
    """Vertex offsets (what the decoder writes) -> the same offsets smoothed along time by a zero-phase FIR filter or by a recurrence,
    each clip at its own length, in ONE device call (tfilter.TimeFilterPlan; include/fdm_hip.h, fdm_tfilter_forward; DESIGN.md section
    2 items 27 and 28 state every operation).  time_filter: a tfilter.TimeFilterPlan, or the dict of its arguments after V (taps= |
    kind="gaussian" with sigma= frames or seconds= | kind="savgol" with radius= and order=; edge= "mirror" | "nearest"; or
    kind="one_euro" with min_cutoff= Hz, beta= (it depends on the mesh's scale) and d_cutoff= Hz | kind="ema" with cutoff= Hz, either
    with direction= "zero_phase" (the default: whole clips are filtered offline) | "causal"; strength= [V] in [0, 1], 0 keeps a
    vertex's input bits); seconds= is converted with fps, the MODEL's frame rate, which is also the recurrences' fps= unless given.  offsets: a device tensor [B, L, 3 V] (or [L, 3 V])
    with frames = L per clip (None: all L; rows past a clip's frames come out as zeros); or a ragged LIST of [1, L_b, 3 V] / [L_b, 3 V]
    clips -> a list of [1, L_b, 3 V], one padded call, each clip bit for bit what its own call returns.  What a filter does to
    perceptual quality or lip-sync metrics is unmeasured."""
    return _per_clip("to_filtered", offsets, frames, None, device,
                     lambda x, fr, _: _time_filter_plan(time_filter, x.shape[-1] // 3, x.device, fps).forward(x, fr),
                     lambda y, fr: [y[b:b + 1, :n] for b, n in enumerate(fr)])


# keys of a render= dict that choose outputs or bring a call's scalar field, not the plan
_RENDER_OUTPUTS = ("depth", "face_ids", "alpha", "yuv", "scalars", "error_to")


def _render_plan(render, faces, V, device):
    """The render hand-off plan of `device`, the current stream, this topology and this view (render.RenderPlan.key).  render: a
    render.RenderPlan (used as it is where it was made for this device and stream, made again from its arguments otherwise; `faces`
    is then not read) or the dict of RenderPlan's arguments after faces and V (camera, lights, ambient, base, background,
    chunk_frames, samples, yuv_matrix, yuv_range, yuv_layout, material; yuv="i420" | "nv12" among its outputs is the plan's yuv_layout)."""
    from .render import RenderPlan, identity
    dv, at = _on_stream(device)
    if isinstance(render, RenderPlan):
        if render.V != int(V):
            raise FdmError(f"the render plan is for {render.V} vertices, the frames have {int(V)}")
        key, make, given = render.key, (lambda: RenderPlan(device=dv, **render.arguments())), render
    else:
        if faces is None:
            raise ValueError("render= needs faces=: the triangle list of the mesh that is drawn")
        kw = {k: v for k, v in render.items() if k not in _RENDER_OUTPUTS}
        if isinstance(render.get("yuv"), str):
            kw["yuv_layout"] = render["yuv"]
        key, make, given = identity(faces, V, **kw), (lambda: RenderPlan(faces, V, device=dv, **kw)), None
    plan = cached_plan(at, "render", key, make, given)
    if plan.key != key:      # its view was changed (RenderPlan.set_view) after it was kept under this key
        from .handoff import _PLANS
        _PLANS[tuple(at) + ("render", key)] = plan = make()
    return plan


def _split_images(im, _=None):
    """A batched ImageFrames -> one per clip, each cut to its own frames ([1, L_out, H, W, 3])."""
    cut = lambda t, b, n: None if t is None else t[b:b + 1, :n]  # noqa: E731
    return [type(im)(cut(im.images, b, n), cut(im.depth, b, n), cut(im.face_ids, b, n), [n], cut(im.alpha, b, n), cut(im.yuv, b, n))
            for b, n in enumerate(im.frames)]


@torch.no_grad()
def _packed_scalars(scalars, x, frames):
    """The scalar field of a call as one batch [B, L_max, V] next to the packed positions x: a list with one [L_b, V] per clip is
    zero-padded as _pack_offsets pads the clips; a tensor goes as it is."""
    if not isinstance(scalars, (list, tuple)):
        return scalars
    V = int(x.shape[-1]) // 3
    if len(scalars) != int(x.shape[0]):
        raise ValueError(f"{len(scalars)} scalar fields for {int(x.shape[0])} clips")
    pad = torch.zeros(int(x.shape[0]), int(x.shape[1]), V, device=x.device)
    for b, c in enumerate(scalars):
        c = torch.as_tensor(c, dtype=torch.float32).reshape(-1, V)
        if int(c.shape[0]) != int(frames[b]):
            raise ValueError(f"the scalar field of clip {b} has {int(c.shape[0])} frames, the clip {int(frames[b])}")
        pad[b, :c.shape[0]] = c
    return pad


@torch.no_grad()
def to_images(offsets, faces, render, template=None, frames=None, fps=None, normals=None, depth=None, face_ids=None, device=None, alpha=None,
              yuv=None, scalars=None):
    """Vertices (or vertex offsets with template=) -> render.ImageFrames: shaded uint8 frames [B, L_out, H, W, 3] of the mesh with the
    triangle list `faces` [F, 3], drawn on the device in ONE call (render.RenderPlan; include/fdm_hip.h, fdm_render_forward; DESIGN.md
    section 2 item 23 states every operation).  render: a render.RenderPlan, or the dict of its arguments after faces and V -- camera (a
    render.Camera or "vocaset" | "biwi" | "mead"), lights, ambient, base, background, chunk_frames, samples (1, 4 or 16 coverage samples
    per pixel: anti-aliased frames), yuv_matrix, yuv_range -- which may also carry depth=True
    and face_ids=True for the depth [B, L_out, H, W] and face-id images, alpha=True for the coverage plane [B, L_out, H, W] uint8 and
    yuv="i420" | "nv12" for each frame's Y'CbCr 4:2:0 planes [B, L_out, 3 W H / 2] uint8 (even W and H; with a RenderPlan yuv=True: the
    layout is the plan's); without the last two the call is the one it was.  offsets: a device tensor [B, L, 3 V] (or [L, 3 V]) with
    frames = L per clip (None: all L); a ragged LIST of [1, L_b, 3 V] / [L_b, 3 V] clips -> a list of ImageFrames, each cut to its own
    frames and bit for bit what its own call returns; or a mesh.MeshFrames (planar fp32): its positions, normals and frames are drawn
    as they are.  template: [1 or B, 3 V], or for a list one per clip.  fps = (fps_in, fps_out): the positions are resampled by
    to_mesh's rule first.  normals [B, L_out, V, 3]: the caller's instead of the ones computed here (to_mesh's).  material= in the dict
    (a render.Material: vertex colours, a scalar map or a texture) colours the surface; a scalar map reads
    scalars [B, L, V] on the INPUT frames (for a list of clips a list of [L_b, V]), given here or in the dict."""
    from .mesh import MeshFrames
    opts = render if isinstance(render, dict) else {}
    depth = bool(opts.get("depth", False)) if depth is None else depth
    face_ids = bool(opts.get("face_ids", False)) if face_ids is None else face_ids
    alpha = bool(opts.get("alpha", False)) if alpha is None else alpha
    yuv = bool(opts.get("yuv", False)) if yuv is None else bool(yuv)
    scalars = opts.get("scalars") if scalars is None else scalars
    if isinstance(offsets, MeshFrames):
        mf = offsets
        if mf.positions.dtype != torch.float32 or mf.positions.shape[-1] != 3:
            raise FdmError("to_images draws planar float32 MeshFrames (not interleaved, not half)")
        B, Lo, V = (int(n) for n in mf.positions.shape[:3])
        offsets, frames, normals = mf.positions.reshape(B, Lo, 3 * V), mf.frames, (mf.normals if normals is None else normals)
    return _per_clip("to_images", offsets, frames, template, device, lambda x, fr, tp: _render_plan(render, faces, x.shape[-1] // 3, x.device).forward(
        x, fr, tp, fps, normals, depth, face_ids, alpha=alpha, yuv=yuv, scalars=_packed_scalars(scalars, x, fr)), _split_images)


def _render_material(render):
    """The render.Material of a render= argument (a dict or a render.RenderPlan), or None."""
    return render.get("material") if isinstance(render, dict) else getattr(render, "view", {}).get("material")


def _gt_rows(c, gt):
    """error_to for the clips c [B, L, 3 V] that are about to be drawn: [L', 3 V], [L', V, 3], [B, L', 3 V] or [B, L', V, 3] with L' >= L ->
    [B, L, 3 V] on c's device, cropped to the clip.  A wrong vertex count or too few frames is a ValueError."""
    B, L, V3 = (int(n) for n in c.shape)
    g = torch.as_tensor(gt, dtype=torch.float32)
    if g.dim() >= 3 and g.shape[-1] == 3 and int(g.shape[-2]) * 3 == V3:
        g = g.reshape(tuple(g.shape[:-2]) + (V3,))
    if g.dim() == 2:
        g = g.unsqueeze(0)
    if g.dim() != 3 or int(g.shape[-1]) != V3 or int(g.shape[0]) not in (1, B):
        raise ValueError(f"error_to has the shape {tuple(torch.as_tensor(gt).shape)}: the drawn mesh has {V3 // 3} vertices ({V3} numbers a frame), "
                         f"the call {B} clips")
    if int(g.shape[1]) < L:
        raise ValueError(f"error_to has {int(g.shape[1])} frames, the clip {L}")
    return g[:, :L].expand(B, L, V3).to(c.device).contiguous()


def _error_field(out, template, gt, device):
    """render=dict(error_to=gt): the scalars of the call, |drawn vertex - gt| per input frame and vertex (render.vertex_error), for a
    batch [B, L, 3 V] or a list of clips with one gt per clip.  The vertex count was checked when the call began (_Outputs); the
    lengths are checked here, for every clip before the first launch of the hand-off -- the model has run by then: a clip's length
    is known only from its encoded audio."""
    from .render import vertex_error
    drawn = lambda c, t: c.contiguous() if t is None else c + _template_rows(t, c.shape[-1], device).unsqueeze(1)  # noqa: E731
    if not isinstance(out, (list, tuple)):
        return vertex_error(drawn(out, template), _gt_rows(out, gt))
    if not isinstance(gt, (list, tuple)) or len(gt) != len(out):
        raise ValueError(f"error_to for {len(out)} clips is a list with one ground truth per clip")
    clips = [c.reshape(1, -1, c.shape[-1]) for c in out]
    gts = [_gt_rows(c, g) for c, g in zip(clips, gt)]
    tps = template if isinstance(template, (list, tuple)) else [template] * len(out)
    return [vertex_error(drawn(c, t), g)[0] for c, t, g in zip(clips, tps, gts)]


def _flame_rows(x, L, R, what):
    """A per-frame argument of flame= for R clips of L frames: [L', n] (for all) or [R, L', n], L' >= L -> [R, L, n]"""
    x = torch.as_tensor(x, dtype=torch.float32)
    x = x.unsqueeze(0).expand(R, -1, -1) if x.dim() == 2 else x
    if x.dim() != 3 or x.shape[0] != R or x.shape[1] < L:
        raise ValueError(f"flame {what}: {tuple(x.shape)} for {R} clips of {L} frames")
    return x[:, :L]


FLAME_KEYS = ("model", "pose", "shape", "expression", "transl")


def _flame_check(flame):
    """flame= of animate*: a dict with model and pose, and no key but FLAME_KEYS"""
    if not isinstance(flame, dict) or "model" not in flame or flame.get("pose") is None or set(flame) - set(FLAME_KEYS):
        raise ValueError(f"flame= takes a dict with model and pose, optionally shape, expression and transl; got {sorted(flame) if isinstance(flame, dict) else type(flame).__name__}")


def _flame_posed(out, flame, device, frames=None, S=1, B=1):
    """The decoder's offsets [R, L, V3] as `extra` of the head flame = dict(model=, pose=, shape=, expression=, transl=) -> posed
    vertices [R, L, V3], at the model's frame rate.  With S > 1 conditions per clip (R = B * S rows in (clip, condition) order) a
    per-clip argument [B, L', n] or shape [B, NS] repeats per condition, as a per-clip template does."""
    _flame_check(flame)
    R, L = int(out.shape[0]), int(out.shape[1])

    def rows(k):
        x = flame.get(k)
        if x is None:
            return None
        x = torch.as_tensor(x, dtype=torch.float32)
        if S > 1 and B > 1 and x.dim() == 3 and x.shape[0] == B:
            x = x.repeat_interleave(S, dim=0)
        return _flame_rows(x, L, R, k)
    shape = flame.get("shape")
    if shape is not None:
        shape = torch.as_tensor(shape, dtype=torch.float32)
        if S > 1 and B > 1 and shape.dim() == 2 and shape.shape[0] == B:
            shape = shape.repeat_interleave(S, dim=0)
    ff = to_flame(rows("pose"), flame["model"], rows("expression"), shape, rows("transl"), out, frames, device=device)
    return ff.vertices.reshape(R, L, -1)


def build_models(preset="vocaset", feature_dim=None, device="cuda:0", stage1=None, stage2=None, dtype=None, cfg_level=None, single_clip=False):
    """(diffusion, autoencoder) with reference-compatible state dicts; checkpoints are loaded when the
    files exist ('model' / 'state_dict' keys as samples/sample_diffusion_vocaset.py:26,91-97), otherwise the
    seeded random init is kept (there are no checkpoints in this environment).  single_clip: the caller samples one clip per call
    (the reference's batch size) -- the step program's single-clip setting (modules.SINGLE_CLIP_PLAN)."""
    from dropin_config import vq_args_for
    p = presets.get(preset)
    cls = {"vocaset": FDM, "mead": FDMMead, "biwi": FDMBiwi}[p.name]
    kw = dict(feature_dim=feature_dim or p.d, n_head=(feature_dim or p.d) // p.head_dim, dtype=dtype)
    model = cls(**kw)
    if single_clip:
        from .modules import SINGLE_CLIP_PLAN
        for k, v in SINGLE_CLIP_PLAN.items():
            model.set_plan_option(k, v)
    ae = VQAutoEncoder(vq_args_for(p.name), dtype=dtype)
    denoise = ClassifierFreeSampleModel(model, cfg_level) if cfg_level else model
    diffusion = GaussianDiffusion(denoise, timesteps=1000, loss_type="l2")
    if stage2 and os.path.exists(stage2):
        diffusion.load_state_dict(torch.load(stage2, map_location="cpu")["model"], strict=False)
    else:
        # untrained latent_decoder is zero-initialised in the reference (outputs would be identically 0):
        # give the synthetic model a non-trivial head so the pipeline is exercised end to end
        g = torch.Generator().manual_seed(7)
        model.latent_decoder.weight.data.copy_(torch.randn(model.latent_decoder.weight.shape, generator=g) * 0.02)
    if stage1 and os.path.exists(stage1):
        ck = torch.load(stage1, map_location="cpu")
        ae.load_state_dict(ck.get("state_dict", ck.get("model", ck)), strict=False)
    return diffusion, ae


# ---- one request path: what animate, animate_many, animate_long and SlotServer all do, stated once -------------------------------
def _unwrap(diffusion):
    """(model, preset, cfg, scale) of a GaussianDiffusion: cfg = it wraps a ClassifierFreeSampleModel (classifier-free guidance at
    that model's level); scale is 2.5 without guidance, where nothing reads it."""
    cfg = isinstance(diffusion.denoise_fn, ClassifierFreeSampleModel)
    model = diffusion.denoise_fn.model if cfg else diffusion.denoise_fn
    return model, model.preset, cfg, float(diffusion.denoise_fn.level) if cfg else 2.5


def _per(x, b):
    """Entry b of an argument given per clip (a list), or the one value given for all."""
    return x[b] if isinstance(x, (list, tuple)) else x


def _waveform(audio, rate, device):
    """One call's audio as [B, n] fp32 on `device` ([n] is one clip); rate: it is ONE raw PCM clip, through the front end first."""
    if rate is not None:
        audio = prepare_audio(audio, rate, device=device)
    audio = torch.as_tensor(audio, dtype=torch.float32, device=device)
    return audio.unsqueeze(0) if audio.dim() == 1 else audio


def _waveforms(audios, rate, device, upload=True):
    """A list of clips as [n_b] fp32 tensors; rate (one for all, or a list): they are raw PCM, through the front end in ONE call.
    upload=False leaves a host waveform where it is (encode_many packs the clips into its own device batch)."""
    if rate is not None:
        wav, lens = prepare_audio_many(audios, rate, device=device)
        audios = [wav[b, :lens[b]] for b in range(len(audios))]
    return [torch.as_tensor(a, dtype=torch.float32, device=device if upload else None).reshape(-1) for a in audios]


_STYLE_DEFAULT = 0        # eye(n_style)[:1]: the first subject, the one-hot the demos are written with (demo/demo_vocaset.py:88)
_EMOTION_DEFAULT = 4      # eye(n_emo)[4:5]: EMOTIONS[4], "happy" -- the default of the demo's --emotion


def _condition(x, width, default, rows, device=None):
    """A style or emotion argument as the fp32 [rows, width] tensor the samplers take, on `device` (None: where it is): None is row
    `default` of the identity, [width] / [1, width] is that one row for every row (expanded, not copied), [r, width] stays as it is."""
    x = torch.eye(width)[default:default + 1] if x is None else x
    x = torch.as_tensor(x, dtype=torch.float32, device=device).reshape(-1, width)
    return x.expand(rows, -1) if (x.shape[0] == 1 and rows > 1) else x


def _start_noise(shape, seed):
    """x_T of a request: ONE draw of `shape` from a CPU generator seeded with `seed`, so `seed=` reproduces a call on any device.
    The shape is the caller's: [B, n, c] drawn at once is not the bits of B draws of [1, n, c]."""
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _sampler_definition(p, ddim_steps, sampler, sampler_steps, eta, ddim_on_emotion=False):
    """The sampler of a request as a hashable definition: sampler= ("dpmpp2m" | "ddim_eta" with eta=, sampler_steps), else ddim_steps,
    else the DDPM chain.  animate, animate_many and SlotServer ignore ddim_steps on a preset with an emotion input (the reference
    samples those with DDPM only); animate_long honours it on every preset: ddim_on_emotion=True."""
    if sampler:
        return ("tables", str(sampler), int(sampler_steps), float(eta))
    if ddim_steps and (ddim_on_emotion or not p.n_emo):
        return ("ddim", int(ddim_steps))
    return ("ddpm",)


def _sampler_args(key, diffusion):
    """A definition as the kind / steps / t_list / tables arguments of the plan (sample_windows, open_slots, add_sampler)."""
    if key[0] == "tables":
        t_list, tables = schedule.sampler_tables(key[1], key[2], key[3], diffusion.num_timesteps)
        return dict(kind="tables", t_list=t_list, tables=tables)
    if key[0] == "ddim":
        return dict(kind="ddim", steps=key[1])
    ts = list(range(diffusion.num_timesteps - 1, -1, -1)) if diffusion.full_chain else list(range(999, 499, -1))
    return dict(kind="ddpm", t_list=ts)


def _sample(diffusion, key, audio, shape, cond, x_T, seed, clip0=0, **tracks):
    """One sampling call of a definition through the GaussianDiffusion methods; cond = (style,) or (emotion, style)."""
    if key[0] == "tables":
        return diffusion.fast_sample(audio, shape, *cond, steps=key[2], sampler=key[1], eta=key[3], seed=seed, x_T=x_T, clip0=clip0, **tracks)
    if key[0] == "ddim":      # (noise-free: no seed, no clip index)
        return diffusion.ddim_sample(audio, shape, cond[-1], key[1], x_T=x_T, **tracks)
    return diffusion.sample(audio, shape, *cond, seed=seed, x_T=x_T, clip0=clip0, **tracks)


def _quantise(autoencoder, p, latent, emo=None, emotion_track=None):
    """z_q of a latent: every frame in the codebook of the clip's emotion (of its own emotion with a track) where the preset has one."""
    if p.n_emo:
        return autoencoder.quant(latent, emo, stats=False, emotion_track=emotion_track)[0]
    return autoencoder.quant(latent, stats=False)[0]


def _template_rows(template, width, device, S=1, B=1):
    """template [1 or B, width] (any shape of that many numbers) as fp32 rows on `device`; with S > 1 conditions per clip, a
    template per clip repeats per condition: rows in (clip, condition) order."""
    tp = torch.as_tensor(template, dtype=torch.float32, device=device).reshape(-1, width)
    return tp.repeat_interleave(S, dim=0) if (S > 1 and tp.shape[0] == B and B > 1) else tp


def _padded_rows(rows, L):
    """A per-frame flame= argument given per clip -> one batch [n, >= L, width], zeros past each clip's rows (never read)."""
    rows = [torch.as_tensor(a, dtype=torch.float32).reshape(-1, torch.as_tensor(a).shape[-1]) for a in rows]
    pad = torch.zeros(len(rows), max(L, max(int(r.shape[0]) for r in rows)), rows[0].shape[-1])
    for b, r in enumerate(rows):
        pad[b, :r.shape[0]] = r
    return pad


class _Outputs:
    """What a call makes of its decoded offsets, resolved ONCE per animate / animate_many / animate_long call or per SlotServer from the
    preset, the device and the eight output keywords: the combinations that return nothing are refused, a rig= / wrap= dict is
    digested and made into its plan (_bound_plan: not per group, not per finished clip), and fps is (fps_in, fps_out) by _mesh_fps's
    rule where faces= or rig= asks for a hand-off that reads it (fps=: the pair itself, from a caller that holds it).  Calling it is
    the chain; `together` is the chain for the clips a SlotServer finishes in one step.  time_filter= (the last keyword) is stage 0:
    the decoded offsets are filtered along time (to_filtered) before anything below reads them."""

    def __init__(self, p, device, faces=None, out_fps=None, mesh=None, in_fps=None, rig=None, flame=None, wrap=None, render=None, fps=None, flame_fit=None,
                 time_filter=None):
        # the filter's arguments are checked here, before anything runs (seconds= by the model's frame rate); its plan is made at the
        # first call, when the vertex count is known from the decoded frames
        self.time_filter = None if time_filter is None else _time_filter_arguments(time_filter, in_fps or (p.fps if p is not None else None) or (fps[0] if fps else None))
        if flame_fit is not None:
            _flame_fit_check(flame_fit)
            if flame is not None:
                raise ValueError("flame_fit= with flame=: one poses the head and the other un-poses it; pass one of them")
            if wrap is not None:
                raise ValueError("flame_fit= with wrap=: the fit is of the model's own topology; fit first (to_flame_params), wrap the posed head after")
        self.flame_fit = flame_fit
        if render is not None and faces is None:
            raise ValueError("render= needs faces=: the triangle list of the mesh that is drawn (after wrap=, the target's)")
        if isinstance(render, dict) and (render.get("error_to") is not None or render.get("scalars") is not None):
            mat = _render_material(render)
            if render.get("error_to") is not None and render.get("scalars") is not None:
                raise ValueError("render= takes scalars= or error_to=, not both")
            if mat is None or mat.kind != 2:
                raise ValueError("render=dict(scalars= | error_to=) needs material=render.Material.scalar_map(...)")
        if flame is not None:
            _flame_check(flame)
            if rig is not None and faces is None:
                raise ValueError("flame= with rig= and no faces=: the call would return the fit of the un-posed offsets alone and never pose anything")
        if wrap is not None and rig is not None and faces is None:
            raise ValueError("wrap= with rig= and no faces=: the call would return the fit of the model's own offsets alone and never wrap anything")
        self.device, self.faces, self.mesh, self.flame, self.render = device, faces, dict(mesh or {}), flame, render
        self.rig = None if rig is None else _bound_plan("rig", rig, device)
        self.wrap = None if wrap is None else _bound_plan("wrap", wrap, device)
        self.fps = fps or (_mesh_fps(p, in_fps, out_fps) if (faces is not None or rig is not None) else None)
        if isinstance(render, dict) and render.get("error_to") is not None:
            # the vertex count of what will be drawn is known here, before anything runs: the wrap's target, else the model's own (a
            # posed head keeps it).  A clip's length is known only once its audio has been encoded: _gt_rows checks it at the hand-off.
            V = self.wrap.Vt if self.wrap is not None else (p.V3 // 3 if p is not None else None)
            gts = render["error_to"] if isinstance(render["error_to"], (list, tuple)) else [render["error_to"]]
            for g in gts:
                shp = tuple(torch.as_tensor(g).shape)
                if V is not None and not (len(shp) >= 2 and (shp[-1] == 3 * V or (len(shp) >= 3 and shp[-1] == 3 and shp[-2] == V))):
                    raise ValueError(f"error_to has the shape {shp}: the drawn mesh has {V} vertices ([L', {3 * V}] or [L', {V}, 3])")

    def __call__(self, out, template=None, S=1, B=1, flame=None):
        """What a call returns for a batch of decoded offsets [B*S, L, V3]: offsets + template; with faces= the mesh.MeshFrames (the
        template added there); with rig= the rig.RigFrames fitted to the offsets, never to the templated vertices; with both the pair.
        flame=: the offsets pose the model's head (_flame_posed) and the posed vertices stand where offsets + template stood (the
        template argument is not read); rig= still fits the un-posed offsets; rig= without faces= returns no vertices, so flame= is
        refused with it.  wrap=: the vertices of the bound mesh (to_wrap) stand where offsets + template stood -- after flame= they follow
        the posed head; with faces= the mesh hand-off runs on them with no template, so `faces` is then the TARGET's triangle list and fps
        applies there; rig= keeps fitting the model's own offsets (a rig on the target topology is to_rig(to_wrap(..., offsets_out=True),
        basis_t)), and rig= without faces= is refused with it as with flame=.  render=: the render.ImageFrames of the mesh `faces` (to_images)
        stand where its mesh.MeshFrames stood -- the template added, fps applied, the posed or wrapped vertices drawn; faces= is required
        and mesh= is not read.
        The ragged form: `out` a LIST of decoded clips [1, L_b, V3] with `template` None or one per clip -> a list with one result per
        clip, from ONE rig, ONE head, ONE wrap and ONE mesh or render call over the unequal lengths, each result bit for bit its own
        call's.  flame (this group's, in place of the call's): pose / expression / transl [L', n] for all clips or a list with one per clip."""
        if self.time_filter is not None:                                                         # 0. the time filter: every output below reads the filtered offsets
            first = out[0] if isinstance(out, (list, tuple)) else out
            if first.is_cuda:        # the plan, once: later calls do not digest the dict again (a host tensor is refused below)
                self.time_filter = _time_filter_plan(self.time_filter, first.shape[-1] // 3, first.device)
            out = to_filtered(out, self.time_filter)
        return self._chain(out, template, S, B, flame)

    def _chain(self, out, template=None, S=1, B=1, flame=None):
        """The chain of __call__ after the time filter."""
        if self.flame_fit is not None:                                                           # the head's parameters stand where the vertices stood
            return self._with_flame_fit(out, template, S, B)
        many, flame = isinstance(out, (list, tuple)), self.flame if flame is None else flame
        fit = None if self.rig is None else to_rig(out, self.rig, fps=self.fps)                  # 1. the fit, on the offsets as decoded
        if self.faces is None and fit is not None:
            return fit
        if flame is not None:                                                                    # 2. the head
            frames = None
            if many:     # one padded batch; an argument given per clip is padded with it
                out, frames, _ = _pack_offsets(out, None, self.device, "to_flame")
                flame = {k: _padded_rows(v, int(out.shape[1])) if (k in ("pose", "expression", "transl") and isinstance(v, (list, tuple))) else v
                         for k, v in flame.items()}
            out, template = _flame_posed(out, flame, self.device, frames, S, B), None
            if many:
                out = [out[b:b + 1, :n] for b, n in enumerate(frames)]
        if template is not None and not many:      # (a list of templates goes on as it is: one per clip)
            template = _template_rows(template, out.shape[-1], self.device, S, B)
        if self.wrap is not None:                                                                # 3. the wrap
            out, template = to_wrap(out, self.wrap, template, device=self.device), None
        if self.faces is None:                                                                   # 4. the template, the mesh or the images
            if template is None:
                return out
            return [c + _template_rows(t, c.shape[-1], self.device).unsqueeze(1) for c, t in zip(out, template)] if many else out + template.unsqueeze(1)
        if self.render is None:
            res = to_mesh(out, self.faces, template, fps=self.fps, **self.mesh)
        else:
            render = self.render
            if isinstance(render, dict) and render.get("error_to") is not None:      # the error field of what is about to be drawn
                render = dict(render, scalars=_error_field(out, template, render["error_to"], self.device))
            res = to_images(out, self.faces, render, template, fps=self.fps, device=self.device)
        if fit is None:                                                                          # 5. with the fit
            return res
        return list(zip(res, fit)) if many else (res, fit)

    def _with_flame_fit(self, out, template, S, B):
        """flame_fit=: the flame.FlameFit of offsets + template (to_flame_params, at the model's own frame rate) stands where the vertices
        stood; with faces= or rig= the rest of the chain runs as without the argument and the call returns (that result..., FlameFit)."""
        many = isinstance(out, (list, tuple))
        kw = {k: v for k, v in self.flame_fit.items() if k != "model"}
        tp = template
        if tp is not None and not many:
            tp = _template_rows(tp, out.shape[-1], self.device, S, B)
        ff = to_flame_params(out, self.flame_fit["model"], tp, device=self.device, **kw)
        if self.faces is None and self.rig is None:
            return ff
        saved, self.flame_fit = self.flame_fit, None
        try:
            rest = self._chain(out, template, S, B)
        finally:
            self.flame_fit = saved
        pair = self.faces is not None and self.rig is not None      # (the rest is then (mesh or images, rig fit); results are namedtuples themselves)
        if many:
            return [(tuple(r) + (f,)) if pair else (r, f) for r, f in zip(rest, ff)]
        return (tuple(rest) + (ff,)) if pair else (rest, ff)

    def together(self, clips, templates):
        """The chain for clips [1, L_b, V3] that were decoded together, `templates` holding one or None per clip -> one result per clip.
        They share the ragged form's calls where there is a call to share; with no hand-off asked for, or with a mesh or a wrap that
        reads templates and a template on some clips only, they go clip by clip."""
        given, reads_templates = [t is not None for t in templates], self.faces is not None or self.wrap is not None
        if self.flame_fit is not None:
            reads_templates = True
        if (not reads_templates and self.rig is None) or (reads_templates and any(given) and not all(given)):
            return [self(c.contiguous(), t) for c, t in zip(clips, templates)]
        return self(clips, templates if given[0] else None)


def _hand_off(out, template, device, faces=None, mesh=None, rig=None, fps=None, S=1, B=1, flame=None, wrap=None, render=None):
    """The chain (_Outputs) for a batch, from a caller that holds fps = (fps_in, fps_out) or None itself."""
    return _Outputs(None, device, faces, None, mesh, None, rig, flame, wrap, render, fps)(out, template, S, B)


def _hand_off_many(clips, templates, device, faces=None, mesh=None, rig=None, fps=None, flame=None, wrap=None, render=None):
    """_hand_off for a ragged list of decoded clips [1, L_b, V3] with templates None or one per clip."""
    return _Outputs(None, device, faces, None, mesh, None, rig, flame, wrap, render, fps)(clips, templates)


@torch.no_grad()
def animate(diffusion, autoencoder, audio, template=None, id_one_hot=None, emotion_one_hot=None, steps=None,
            ddim_steps=None, seed=0, device="cuda:0", sampler=None, sampler_steps=20, eta=0.0, style_track=None, emotion_track=None,
            rate=None, faces=None, out_fps=None, mesh=None, in_fps=None, rig=None, flame=None, wrap=None, render=None, flame_fit=None,
            time_filter=None):
    """audio [B, n] (processor-normalised) -> vertices [B, L, V3].  DDPM full chain by default, DDIM if ddim_steps.

    time_filter (a tfilter.TimeFilterPlan or the dict of its arguments after V: taps= | kind="gaussian" with sigma= frames or seconds= |
    kind="savgol" with radius= and order=; edge=, strength= [V]; or kind="one_euro" with min_cutoff=, beta=, d_cutoff= | kind="ema" with
    cutoff=, in Hz, fps= defaulting to the model's frame rate and direction= to "zero_phase"): the decoded offsets are smoothed along time on the device (to_filtered)
    BEFORE anything else reads them, at the model's own frame rate: the returned vertices, the mesh, wrap, render, rig and head
    outputs all follow the filtered offsets; the returned latent is untouched.  What a filter does to perceptual quality or
    lip-sync metrics is unmeasured.  None: every path as before, launch for launch.

    render (a render.RenderPlan or the dict of its arguments after faces and V: camera, lights, ambient, base, background,
    chunk_frames; depth=True / face_ids=True for those images too, alpha=True for the coverage plane, yuv="i420" | "nv12" for the
    4:2:0 planes with yuv_matrix / yuv_range, as to_images; material= a render.Material, and with a scalar map scalars= [B, L, V] or
    error_to= ground-truth vertices [L' >= L, 3 V] of the drawn mesh: the field is then render.vertex_error of what is about to be
    drawn, for a per-vertex error heat map; a wrong vertex count is a ValueError before anything runs, too few frames one before
    the hand-off's first launch, once the clip's length is known from its audio): with faces= the call returns (render.ImageFrames, latent) in place
    of the mesh.MeshFrames -- shaded uint8 frames [B, L_out, H, W, 3] of the mesh `faces`, drawn on the device (to_images) from the
    positions and normals the mesh hand-off would have returned; out_fps= is honoured; after flame= or wrap= the posed or wrapped mesh
    is drawn (faces= is then that mesh's triangle list).  faces= is required; mesh= is not read; with rig= the call returns
    ((render.ImageFrames, rig.RigFrames), latent).  None: every path as before.

    wrap (a wrap.WrapPlan or the dict of its arguments: src_rest, faces, dst_rest, face_idx, weights): a mesh of ANOTHER topology,
    bound once to the model's rest surface, follows the animation (to_wrap): its vertices [B, L, 3 Vt] are returned where
    offsets + template stood; after flame= they follow the posed head.  With faces= the mesh hand-off runs on the wrapped vertices, so
    faces= is then the TARGET's triangle list and out_fps= applies there.  rig= keeps fitting the model's own offsets exactly as
    without wrap= (and is refused with wrap= unless faces= is given, as with flame=); a rig on the target topology is
    to_rig(to_wrap(offsets, wrap, offsets_out=True), basis_t).  None: every path as before.

    flame = dict(model= a flame.FlameModel / FlamePlan / model file, pose= [L', 3 J] or [B, L', 3 J] axis-angle (L' >= L), shape=,
    expression=, transl=; per-clip arguments repeat per condition when S > 1): the decoder's offsets enter the parametric head as `extra` (to_flame) at the model's frame rate and the
    posed vertices are returned in place of offsets + template (the template argument is then not read: the model has its own).
    With faces= the mesh.MeshFrames are made from the posed vertices; rig= still fits the un-posed offsets (rig= without faces=
    returns no vertices: flame= is refused with it).  None: every path as before.  (SlotServer does not take it.)

    rig (a rig.RigPlan or the dict of its arguments: basis, weights, ridge, bounds, sweeps, names, smooth, smooth_weights): the decoder's offsets -- never the
    templated vertices -- go through the device rig hand-off (to_rig) and the call returns (rig.RigFrames, latent) in place of the
    vertices: blendshape coefficients [B, L_out, K] at out_fps.  With faces= too it returns ((mesh.MeshFrames, rig.RigFrames),
    latent); the two read the same offsets.  None: every path as before.  rig=dict(..., smooth=mu) fits each clip's frames together
    (to_rig); animate_many, animate_long and SlotServer pass the same dict on, and a clip's curves do not depend on its batch.

    faces [F, 3]: the decoder's output goes through the device mesh hand-off (to_mesh) and the call returns (mesh.MeshFrames,
    latent): positions [B, L_out, V, 3] -- the template added there, the same bits as the vertices returned without faces -- and
    vertex normals; out_fps: resampled in time from the preset's frame rate (in_fps= where the preset states none); mesh: a dict of
    to_mesh's output options (normals, interleaved, half).  None: every path as before.

    rate: `audio` is ONE raw PCM clip at that sample rate (int16 / int32 / uint8 / float32, [frames] or [frames, C]) and goes through
    the device front end first: animate(prepare_audio(audio, rate)), 1 s of trailing zeros included.  None: every path as before.

    style_track [L', n_style] / emotion_track [L', n_emo] (or [B, L', n]; L' >= L, fdm_amd.tracks.keyframes): one vector per latent
    frame instead of one per clip, either alone or both; the quantiser takes every frame in the codebook of its own emotion.  One
    condition per clip only (S = 1).  A track whose rows are all equal gives the result of the one-hot call, bit for bit.

    sampler "dpmpp2m" | "ddim_eta" (with eta=): `sampler_steps` steps of the table-driven multistep sampler
    (GaussianDiffusion.fast_sample) from the same per-clip x_T, on every preset; None = the paths below, unchanged.

    id_one_hot [B*S, n_style] (and emotion_one_hot [B*S, n_emo]) with S > 1 animates every clip under S conditions in ONE
    sampling call -- the reference sampler's style loop (samples/sample_diffusion_vocaset.py:71-83) batched: the audio
    encoder and the audio tables run once per clip, the S conditions ride the same step program.  Returns [B*S, L, V3] in
    (clip, condition) order.  x_T is drawn per CLIP from a CPU generator seeded with `seed` on every path (S = 1 too), so a call is
    reproducible from its seed and every condition of a clip starts from the clip's x_T -- what S sequential calls with the same
    seed do.  DDIM (eta = 0: x_T is the only random input): bit-identical to the sequential loop.  DDPM: the per-step noise is
    Philox keyed by (seed, ROW = clip * S + condition, step), so a sequential call (row 0) draws the stream of the batched call's
    row 0 only: the other conditions differ from their sequential calls by that stream -- equal in distribution (the reference's
    sequential calls draw from one running generator), not bit for bit."""
    model, p, _, _ = _unwrap(diffusion)
    outputs = _Outputs(p, device, faces, out_fps, mesh, in_fps, rig, flame, wrap, render, flame_fit=flame_fit, time_filter=time_filter)
    audio = _waveform(audio, rate, device)
    B = audio.shape[0]
    # the default style is a row per clip; a style that was given counts with the rows it has
    id_one_hot = _condition(id_one_hot, p.n_style, _STYLE_DEFAULT, B if id_one_hot is None else 1, device)
    rows = max(id_one_hot.shape[0], 1 if emotion_one_hot is None else emotion_one_hot.reshape(-1, emotion_one_hot.shape[-1]).shape[0], B)
    if rows % B:
        raise ValueError(f"{rows} condition rows for {B} clips")
    S = rows // B
    hub = model.audio_features(audio)
    L = min(hub.shape[1] // p.pair, p.max_len)        # samples/sample_diffusion_vocaset.py:76 (no interpolation, a17b)
    shape = (B, L * p.G, p.c)
    trk = {}
    if style_track is not None or emotion_track is not None:
        if S != 1:
            raise ValueError("condition tracks take one condition per clip")
        if emotion_track is not None and not p.n_emo:
            raise ValueError(f"preset {p.name} takes no emotion")
        trk = dict(style_track=style_track)
    cond, et = (id_one_hot,), None
    if p.n_emo:
        if trk:
            trk["emotion_track"] = emotion_track
        emotion_one_hot = _condition(emotion_one_hot, p.n_emo, _EMOTION_DEFAULT, rows, device)
        cond = (emotion_one_hot, _condition(id_one_hot, p.n_style, _STYLE_DEFAULT, rows))       # a one-row style rides every row
        et = None if emotion_track is None else torch.as_tensor(emotion_track)[..., :L, :]
    # one x_T per CLIP, shared by the clip's S conditions: the sequential S = 1 calls of a style loop start where this call starts
    x_T = _start_noise(shape, seed)
    key = _sampler_definition(p, ddim_steps, sampler, sampler_steps, eta)
    latent = _sample(diffusion, key, audio, shape, cond, x_T.repeat_interleave(S, dim=0) if S > 1 else x_T, seed, **trk)
    out = autoencoder.decode(_quantise(autoencoder, p, latent, emotion_one_hot, et))
    return outputs(out, template, S, B), latent


@torch.no_grad()
def animate_many(diffusion, autoencoder, audios, templates=None, id_one_hots=None, emotion_one_hots=None, ddim_steps=None,
                 seed=0, device="cuda:0", max_batch=8, bucket=16, sampler=None, sampler_steps=20, eta=0.0, batch_stages=False,
                 style_track=None, emotion_track=None, rate=None, faces=None, out_fps=None, mesh=None, in_fps=None, rig=None, flame=None,
                 wrap=None, render=None, flame_fit=None, time_filter=None):
    """A test set's clips (different durations) through ONE sampling call per group of `max_batch` clips.

    time_filter: as animate(); each group's decoded clips are filtered in ONE ragged call, each at its own length.

    render: as animate(); each group's clips are drawn in ONE ragged render call and the first returned list holds a
    render.ImageFrames per clip.

    wrap: as animate(); each group's decoded clips go through ONE ragged wrap call and the first returned list holds [1, L_b, 3 Vt]
    per clip (or what faces= makes of them).  None: every path as before.

    flame: as animate(), with pose / expression / transl one [L', n] for all clips or a list with one per clip; each group's decoded
    clips go through ONE ragged head call.  None: every path as before.

    rig: as animate(); each group's decoded clips go through ONE ragged rig hand-off call and the first returned list holds a
    rig.RigFrames per clip ([1, L_out_b, K]), or with faces= a (mesh.MeshFrames, rig.RigFrames) pair.  None: every path as before.

    faces / out_fps / mesh / in_fps: as animate(); each group's decoded clips go through ONE ragged hand-off call and the first
    returned list holds a mesh.MeshFrames per clip ([1, L_out_b, V, 3] positions and normals).  None: every path as before.

    rate (one for all, or a list): `audios` are raw PCM clips at those sample rates and go through the device front end in ONE call
    (prepare_audio_many) before anything else; None: every path as before.

    The reference's samplers take the clips of a loader one at a time (bs = 1: samples/sample_diffusion_vocaset.py:51,71-83),
    which is the few-hundred-row regime where this path reaches 1-2 % of the MFMA roofline.  Clips of different lengths batch
    EXACTLY: the denoiser's self-attention is causal (models/fdm_vocaset.py:85,107-115: key j > query i is masked), every other
    op is per row, and the in-kernel noise is keyed by (clip, element index inside the clip) -- so a clip padded at its END to
    the group's longest length computes, for its own frames, bit for bit what its B = 1 call computes; the tail rows are
    discarded.  The audio encoder and the VQ decoder are not causal: they run per clip at the clip's own length (once each, < 1 %
    of the job).  audios: list of processor-normalised waveforms [n_b]; returns (list of [1, L_b, V3] vertices, list of latents)
    in the caller's order.  DDIM (noise-free): clips are grouped by length (least padding).  DDPM: groups follow the caller's
    order and clip b draws the noise stream of index b (Philox key clip0 + position), so results do not depend on max_batch.
    A group's length is rounded up to a multiple of `bucket` frames (free: the padding is exact), so a long-running caller
    cycles through a handful of shapes whose recorded step programs and tuned tiles the plan keeps.  sampler / sampler_steps / eta:
    as animate() (groups follow the caller's order, noise keyed as for DDPM).
    batch_stages: the two stages that are not causal run batched too -- ONE audio-encoder call over all clips of the call
    (encode_many) and, per group, ONE padded quant and ONE decode (VQAutoEncoder.decode_many); every kernel that looks across time
    carries the clips' own lengths, and the returned lists are torch.equal to the per-clip path's.  Off by default: its gain is
    unmeasured (profiles/ragged/README.md).
    style_track / emotion_track: per-frame conditions as in animate(), one per clip: a list with a track [L', n] (L' >= the clip's
    frames) or None per clip, or one track for all.  A group with a track in it is sampled and quantised with tracks throughout (a
    clip without one rides its one-hot on every frame: the same bits); every result equals animate() on that clip."""
    model, p, _, _ = _unwrap(diffusion)
    outputs = _Outputs(p, device, faces, out_fps, mesh, in_fps, rig, flame, wrap, render, flame_fit=flame_fit, time_filter=time_filter)
    n = len(audios)
    wavs = _waveforms(audios, rate, device)
    if batch_stages:      # one encoder call over all clips of the call, each at its own length inside the padded batch
        hubs = model.audio_encoder.encode_many(wavs, device)
    else:
        hubs = [model.audio_encoder(w.reshape(1, -1)).last_hidden_state for w in wavs]             # [1, N_b, fw] each, own length
    Ls = [min(h.shape[1] // p.pair, p.max_len) for h in hubs]

    def row(x, b, width, default):
        """clip b's condition [1, width]: its entry of a list, its row of one [n, width] tensor, or the one row given for all"""
        x = _condition(_per(x, b), width, default, 1)
        return x[b:b + 1] if x.shape[0] == n else x[:1]

    def group_track(tr, vecs, grp, Lmax, width):
        """[len(grp), Lmax, width]: clip i's track on its own frames (its last row repeated on the tail rows, which belong to no
        frame), its one-hot on every frame when it has no track; None when no clip of the group has a track"""
        if not width or all(_per(tr, b) is None for b in grp):
            return None
        out = vecs.reshape(len(grp), 1, width).expand(len(grp), Lmax, width).clone()
        for i, b in enumerate(grp):
            t = _per(tr, b)
            if t is not None:
                t = torch.as_tensor(t, dtype=torch.float32).reshape(-1, width)
                if t.shape[0] < Ls[b]:
                    raise ValueError(f"clip {b}: a track of {t.shape[0]} rows for {Ls[b]} latent frames")
                out[i, :Ls[b]] = t[:Ls[b]].to(out.device)
                out[i, Ls[b]:] = out[i, Ls[b] - 1]
        return out
    key = _sampler_definition(p, ddim_steps, sampler, sampler_steps, eta)
    order = sorted(range(n), key=lambda b: Ls[b]) if key[0] == "ddim" else list(range(n))
    verts, lats = [None] * n, [None] * n
    prev = (model._hub_key, model._hub)
    try:
        for g0 in range(0, n, max_batch):
            grp = order[g0:g0 + max_batch]
            Lmax = max(Ls[b] for b in grp)
            if bucket and bucket > 1:
                Lmax = min(-(-Lmax // bucket) * bucket, p.max_len)
            Nmax = max(max(hubs[b].shape[1] for b in grp), Lmax * p.pair)
            hub = torch.zeros(len(grp), Nmax, hubs[grp[0]].shape[2], device=device)
            x_T = torch.zeros(len(grp), Lmax * p.G, p.c)
            for i, b in enumerate(grp):
                hub[i, :hubs[b].shape[1]] = hubs[b][0]
                x_T[i, :Ls[b] * p.G] = _start_noise((1, Ls[b] * p.G, p.c), seed)[0]      # what animate() draws for this clip alone
            ids = torch.cat([row(id_one_hots, b, p.n_style, _STYLE_DEFAULT) for b in grp]).to(device)
            model.set_audio_features(hub)
            dummy = torch.zeros(len(grp), 1, device=device)
            shape = (len(grp), Lmax * p.G, p.c)
            emos = torch.cat([row(emotion_one_hots, b, p.n_emo, _EMOTION_DEFAULT) for b in grp]).to(device) if p.n_emo else None
            st_g = group_track(style_track, ids, grp, Lmax, p.n_style)
            et_g = group_track(emotion_track, emos, grp, Lmax, p.n_emo) if p.n_emo else None
            trk = {}
            if st_g is not None or et_g is not None:
                trk = dict(style_track=st_g, emotion_track=et_g) if p.n_emo else dict(style_track=st_g)
            lat = _sample(diffusion, key, dummy, shape, (emos, ids) if p.n_emo else (ids,), x_T, seed, clip0=g0, **trk)
            outs, offs = None, []
            if batch_stages:        # one padded quant (per row) and one decode that knows each clip's length
                lat_g = lat[:, :max(Ls[b] for b in grp) * p.G].contiguous()        # (not the bucket's rows: they belong to no clip)
                etq = None if et_g is None else et_g[:, :lat_g.shape[1] // p.G]
                outs = autoencoder.decode_many(_quantise(autoencoder, p, lat_g, emos, etq), [Ls[b] for b in grp])
            for i, b in enumerate(grp):
                lats[b] = lat[i:i + 1, :Ls[b] * p.G].contiguous()
                if outs is not None:
                    offs.append(outs[i:i + 1, :Ls[b]].contiguous())
                else:
                    etq = None if et_g is None else et_g[i:i + 1, :Ls[b]]
                    offs.append(autoencoder.decode(_quantise(autoencoder, p, lats[b], emos[i:i + 1] if p.n_emo else None, etq)))
            # the group's clips, each at its own length, through one mesh and one rig hand-off call
            tps = None if templates is None else [_per(templates, b) for b in grp]
            fl = None if flame is None else {k: ([v[b] for b in grp] if (k in ("pose", "expression", "transl") and isinstance(v, (list, tuple))) else v) for k, v in flame.items()}
            for b, v in zip(grp, outputs(offs, tps, flame=fl)):
                verts[b] = v
    finally:
        model._hub_key, model._hub = prev
    return verts, lats


@torch.no_grad()
def animate_long(diffusion, autoencoder, audio, template=None, id_one_hot=None, emotion_one_hot=None, ddim_steps=None, seed=0,
                 window=None, overlap=60, device="cuda:0", sampler=None, sampler_steps=20, eta=0.0, style_track=None, emotion_track=None,
                 rate=None, faces=None, out_fps=None, mesh=None, in_fps=None, rig=None, flame=None, wrap=None, render=None, flame_fit=None,
                 time_filter=None):
    """rate: `audio` is ONE raw PCM clip at that sample rate, taken through the device front end first (as animate()).
    time_filter: as animate(): the whole decoded recording is filtered once.
    render: as animate(): the whole recording is drawn (a chunk of frames at a time inside the call).
    wrap: as animate(): the bound mesh follows the whole recording.
    flame: as animate(): the whole recording's offsets pose the model's head (pose [L', 3 J] with L' >= L_total).
    rig: as animate(): the whole recording's offsets go through the rig hand-off and the call returns (rig.RigFrames, latent), or
    ((mesh.MeshFrames, rig.RigFrames), latent) with faces=.
    faces / out_fps / mesh / in_fps: as animate(): the whole recording's decode goes through the mesh hand-off and the call returns
    (mesh.MeshFrames, latent).
    audio [B, n] (processor-normalised) of ANY length -> (vertices [B, L_total, V3], latent [B, L_total*G, c]), L_total =
    encoder frames // pair (no 600-frame cap: animate() keeps the reference's crop).

    The audio encoder runs once over each whole waveform; sampling runs on windows of `window` (default max_len) latent frames
    overlapping by >= `overlap`, blended in x0 space at every diffusion step (include/fdm_hip.h, fdm_audio_prepare_windows /
    fdm_sample_windows); the quantiser and the decoder then run on the whole clip.  One condition per clip (id_one_hot [B, n_style],
    emotion_one_hot [B, n_emo]; defaults as animate()).  x_T is drawn per long clip from a CPU generator seeded with `seed` (as
    animate() draws it) and the DDPM noise is Philox keyed by (seed, long clip, step), so with L_total <= window the result is
    bit-identical to animate()'s.  DDIM (eta = 0) when ddim_steps, on every preset; classifier-free guidance when `diffusion`
    wraps a ClassifierFreeSampleModel.  sampler / sampler_steps / eta: as animate() (the history of the multistep solver is the
    blended x0 in the long layout)."""
    model, p, cfg, scale = _unwrap(diffusion)
    outputs = _Outputs(p, device, faces, out_fps, mesh, in_fps, rig, flame, wrap, render, flame_fit=flame_fit, time_filter=time_filter)
    audio = _waveform(audio, rate, device)
    B = audio.shape[0]
    style = _condition(id_one_hot, p.n_style, _STYLE_DEFAULT, B, device)
    emo = _condition(emotion_one_hot, p.n_emo, _EMOTION_DEFAULT, B, device) if p.n_emo else None
    hub = model.audio_features(audio)
    L_total = hub.shape[1] // p.pair
    plan = model.plan(hub.device)
    model._prep_key = None            # the plan leaves the state FDM.prepare() cached
    # style_track / emotion_track [L', n] or [B, L', n], L' >= L_total: one vector per latent frame of the whole recording (animate())
    plan.prepare_windows(hub, style, emo, L_total=L_total, window=window, overlap=overlap, cfg=cfg, style_track=style_track,
                         emotion_track=emotion_track)
    key = _sampler_definition(p, ddim_steps, sampler, sampler_steps, eta, ddim_on_emotion=True)
    latent = plan.sample_windows(_start_noise((B, L_total * p.G, p.c), seed), seed=seed, cfg_scale=scale, **_sampler_args(key, diffusion))
    et = None if emotion_track is None else torch.as_tensor(emotion_track)[..., :L_total, :]
    out = autoencoder.decode(_quantise(autoencoder, p, latent, emo, et))
    return outputs(out, template), latent


class SlotServer:
    """In-flight batching for a long-running caller whose requests arrive one by one: `slots` clips share ONE step program, each
    at its own diffusion step (DenoiserPlan.open_slots; include/fdm_hip.h, "Slots").  A request joins the running batch at the next
    step boundary and leaves when its own chain ends; its result equals animate() on that audio alone with the same arguments
    (torch.equal on latent and vertices: DDIM, DDPM -- clip id 0, as the solo call keys its noise -- and sampler=).

    One sampler per server (more with a sampler bank, below), chosen as animate() chooses it: sampler= ("dpmpp2m" | "ddim_eta" with eta=, sampler_steps), else
    ddim_steps (presets without an emotion input), else the DDPM chain.  Guidance when `diffusion` wraps a
    ClassifierFreeSampleModel.  max_frames: latent frames a slot holds (default the model's max_len); a longer clip is refused.
    The server owns the model's plan while it runs: an animate*() call on the same model returns the plan to plain mode and the
    next submit() / step() raises.  batch_stages: the clips that finish in one step() call are quantised in one padded call and
    decoded in one call over their unequal lengths (VQAutoEncoder.decode_many) -- the same results, bit for bit.

    Long recordings (submit_long): long_frames > 0 reserves an arena of that many latent frames and long_groups group descriptors
    (DenoiserPlan.open_slots); a recording longer than a slot then rides the same step program as a GROUP of slots, one window of
    max_frames frames per slot overlapping by >= `overlap`, blended every step as animate_long blends them.  Its result equals
    animate_long(..., window=max_frames, overlap=overlap) with the server's sampler and the same seed (torch.equal).  The queue is
    strictly first in, first out: a long request that does not fit yet waits at the head and nothing behind it is admitted, so it
    cannot starve.  long_frames = 0 (default): the plain slot program, and submit_long refuses what needs a group.

    Samplers per request: samplers > 0 reserves a sampler bank of that many definitions beyond the server's own, holding
    bank_steps steps in all (DenoiserPlan.open_slots; the name sampler_steps= is taken: it is the step count of sampler=).  submit / submit_many / submit_long then take ddim_steps= / sampler= /
    sampler_steps= / eta= per request, resolved exactly as animate() resolves them (a request that names none gets the server's
    sampler), and cfg_scale= under guidance (None = the model's level).  The server keeps a {definition: bank id} map; when the
    bank is full it drops the least recently used sampler no slot holds, and if none can go the request waits at the head of the
    queue like a long request that does not fit.  Every result equals animate() / animate_long() with the same arguments and seed.
    samplers = 0 (default): the single-sampler slot program; a request that names another sampler is refused (ValueError).

    faces / out_fps / mesh / in_fps: as animate(): every finished clip's decode goes through the mesh hand-off (the template added
    there) and results() yields a mesh.MeshFrames in place of the vertices; the clips of one batched decode share one ragged call.
    None (default): unchanged.

    rig: as animate(): every finished clip's offsets go through the rig hand-off and results() yields a rig.RigFrames in place of
    the vertices (with faces= a (mesh.MeshFrames, rig.RigFrames) pair); the clips of one batched decode share one ragged call.

    wrap: as animate(): every finished clip's vertices are those of the bound mesh ([1, L, 3 Vt], or what faces= makes of them).

    render: as animate(): results() yields a render.ImageFrames in place of the mesh.MeshFrames (faces= is required).  Its material= may be
    vertex colours or a texture; a scalar map is refused (ValueError): per-request scalar fields are not built.

    time_filter: as animate(): every finished clip's decoded offsets are filtered first.  The server's one filter applies to all its
    requests (a filter per request is not built)."""

    def __init__(self, diffusion, autoencoder, slots=8, max_frames=None, ddim_steps=None, sampler=None, sampler_steps=20, eta=0.0,
                 device="cuda:0", batch_stages=False, long_frames=0, long_groups=4, overlap=60, samplers=0, bank_steps=0,
                 faces=None, out_fps=None, mesh=None, in_fps=None, rig=None, wrap=None, render=None, flame_fit=None, time_filter=None):
        self.diffusion, self.ae, self.device = diffusion, autoencoder, device
        self.model, p, self.cfg, self.scale = _unwrap(diffusion)
        self.p = p
        mat = _render_material(render) if render is not None else None
        if mat is not None and mat.kind == 2:
            raise ValueError("SlotServer draws materials of vertex colours and textures; a scalar map needs a field per request, which is not built")
        self.outputs = _Outputs(p, device, faces, out_fps, mesh, in_fps, rig, None, wrap, render, flame_fit=flame_fit, time_filter=time_filter)     # once, not per finished clip
        self.rig = self.outputs.rig
        self.batch_stages = bool(batch_stages)      # step(): one decode for all clips that finish together (as animate_many)
        self.batched_decodes = []                   # clips per batched decode, in call order
        self.n_slots = int(slots)
        self.L = min(int(max_frames), p.max_len) if max_frames else p.max_len
        self.plan = self.model.plan(device)
        self.model._prep_key = None           # the plan leaves the state FDM.prepare() cached
        kw = dict(cfg=self.cfg, cfg_scale=self.scale)
        self.long_frames, self.overlap = int(long_frames), int(overlap)
        if self.long_frames:
            if not 0 <= self.overlap < self.L:
                raise ValueError(f"overlap {self.overlap} outside [0, max_frames {self.L})")
            kw.update(long_frames=self.long_frames, long_groups=int(long_groups))
        self.bank_samplers, self.bank_steps = int(samplers), int(bank_steps)
        if self.bank_samplers and self.bank_steps:
            kw.update(samplers=self.bank_samplers, sampler_steps=self.bank_steps)
        self.default = self._definition(ddim_steps, sampler, sampler_steps, eta)
        self.chain = self.plan.open_slots(self.n_slots, self.L, **self._definition_args(self.default), **kw)
        self._defs, self._lru = {self.default: 0}, []        # definition -> bank id; ids beyond 0, least recently used first
        self._next, self._queue, self._slot, self._done = 0, [], [None] * self.n_slots, []

    def _definition(self, ddim_steps, sampler, sampler_steps, eta):
        """A sampler definition (hashable), chosen as animate() chooses it."""
        return _sampler_definition(self.p, ddim_steps, sampler, sampler_steps, eta)

    def _definition_args(self, key):
        """open_slots / add_sampler arguments of a definition."""
        return _sampler_args(key, self.diffusion)

    def _request(self, ddim_steps, sampler, sampler_steps, eta, cfg_scale):
        """(definition, cfg_scale) of a request; (None, None) = it names nothing: the server's sampler and scale, admitted as before.
        ValueError for what can never fit: another sampler or scale without a bank, or more steps than the bank holds."""
        if ddim_steps is None and sampler is None and cfg_scale is None:
            return None, None
        key = self.default if (ddim_steps is None and sampler is None) else \
            self._definition(ddim_steps, sampler, 20 if sampler_steps is None else sampler_steps, 0.0 if eta is None else eta)
        scale = None if (cfg_scale is None or not self.cfg) else float(cfg_scale)
        if key == self.default and (scale is None or scale == self.scale):
            return None, None
        if not (self.bank_samplers and self.bank_steps):
            raise ValueError(f"request with sampler {key} / cfg_scale {cfg_scale}: this server was opened without a sampler bank (samplers=, bank_steps=)")
        if key not in self._defs:
            a = self._definition_args(key)
            n = sum(1 for pr in schedule.ddim_time_pairs(a["steps"]) if pr[1] >= 0) if a["kind"] == "ddim" else len(a["t_list"])
            if n < 1 or n > self.bank_steps:
                raise ValueError(f"sampler {key} has {n} steps, the server's bank holds [1, {self.bank_steps}] (bank_steps=)")
        return key, scale

    def _sampler_id(self, key):
        """The bank id of a definition, added on first use.  A full bank drops its least recently used sampler that no slot holds;
        None = nothing can be dropped yet: the request waits."""
        if key in self._defs:
            sid = self._defs[key]
        else:
            while True:
                try:
                    sid = self.plan.add_sampler(**self._definition_args(key))
                    break
                except FdmError as e:
                    if getattr(e, "code", None) != -4:
                        raise
                held = {r["sid"] for r in self._slot if r is not None}
                victim = next((i for i in self._lru if i not in held), None)
                if victim is None:
                    return None
                self.plan.drop_sampler(victim)
                self._lru.remove(victim)
                self._defs = {k: v for k, v in self._defs.items() if v != victim}
            self._defs[key] = sid
        if sid:
            self._lru = [i for i in self._lru if i != sid] + [sid]
        return sid

    def _check(self):
        if self.plan.get("slots") != self.n_slots:
            raise FdmError("SlotServer: the model's plan left slot mode (another sampling call used it)")

    @torch.no_grad()
    def submit(self, audio, template=None, id_one_hot=None, emotion_one_hot=None, seed=0, ddim_steps=None, sampler=None,
               sampler_steps=None, eta=None, cfg_scale=None, style_track=None, emotion_track=None, rate=None):
        """rate: `audio` is raw PCM at that sample rate and goes through the device front end first (prepare_audio).
        One processor-normalised waveform [n] -> a handle.  Runs the audio encoder at the clip's own length, draws x_T as
        animate() does and admits the clip, or queues it until a slot is free.  ddim_steps / sampler / sampler_steps / eta /
        cfg_scale: the request's own sampler and guidance scale (class docstring); none given = the server's."""
        self._check()
        request = self._request(ddim_steps, sampler, sampler_steps, eta, cfg_scale)
        hub = self.model.audio_encoder(_waveform(audio, rate, self.device).reshape(1, -1)).last_hidden_state
        L = min(hub.shape[1] // self.p.pair, self.p.max_len)
        if L < 1 or L > self.L:
            raise ValueError(f"clip of {L} latent frames, slots hold [1, {self.L}]")
        h = self._enqueue(hub, L, template, id_one_hot, emotion_one_hot, seed, request, style_track, emotion_track)
        self._fill()
        return h

    def _enqueue(self, hub, L, template, id_one_hot, emotion_one_hot, seed, request, style_track, emotion_track, windows=0):
        """One request of L latent frames at the tail of the queue -> its handle.  The record holds the first row of its conditions
        (defaults as animate()), x_T drawn as animate() / animate_long() draw it for this clip alone, its sampler and scale
        (_request) and its tracks; windows > 0: a long request, a group of that many slots."""
        p, dev = self.p, self.device
        ids = _condition(id_one_hot, p.n_style, _STYLE_DEFAULT, 1)[:1].to(dev)
        emo = _condition(emotion_one_hot, p.n_emo, _EMOTION_DEFAULT, 1)[:1].to(dev) if p.n_emo else None
        h = self._next
        self._next += 1
        self._queue.append(dict(handle=h, hub=hub, L=L, ids=ids, emo=emo, x_T=_start_noise((1, L * p.G, p.c), int(seed)), seed=int(seed),
                                template=template, windows=windows, sampler=request[0], scale=request[1],
                                **self._tracks(L, style_track, emotion_track)))
        return h

    def _tracks(self, L, style_track, emotion_track):
        """The request's condition tracks (animate()): [L', n] with L' >= L, cut to the clip's frames; {} for a request without."""
        if style_track is None and emotion_track is None:
            return {}
        cut = lambda t, n: None if (t is None or not n) else torch.as_tensor(t, dtype=torch.float32).reshape(-1, n)[:L].to(self.device)  # noqa: E731
        return dict(st=cut(style_track, self.p.n_style), et=cut(emotion_track, self.p.n_emo), tracks=True)

    def _quant(self, lat, r):
        return _quantise(self.ae, self.p, lat, r["emo"], r.get("et"))

    @torch.no_grad()
    def submit_many(self, audios, templates=None, id_one_hots=None, emotion_one_hots=None, seeds=0, ddim_steps=None, sampler=None,
                    sampler_steps=None, eta=None, cfg_scale=None, style_track=None, emotion_track=None, rate=None):
        """rate (one for all, or a list): `audios` are raw PCM clips; ONE front-end call over all of them (prepare_audio_many), then
        the one encoder call.
        Several requests at once: ONE audio-encoder call over the waveforms' unequal lengths (encode_many), then each request is
        admitted or queued exactly as submit() does it, in the given order.  templates / id_one_hots / emotion_one_hots / seeds:
        one per request (lists) or one for all, and so are ddim_steps / sampler / sampler_steps / eta / cfg_scale (submit()).
        style_track / emotion_track: a list with one track (or None) per request, or one for all (submit()).
        Returns the handles; results equal submit() in a loop bit for bit."""
        self._check()
        p, n = self.p, len(audios)
        reqs = [self._request(_per(ddim_steps, b), _per(sampler, b), _per(sampler_steps, b), _per(eta, b), _per(cfg_scale, b)) for b in range(n)]
        hubs = self.model.audio_encoder.encode_many(_waveforms(audios, rate, self.device, upload=False), self.device)
        Ls = [min(h.shape[1] // p.pair, p.max_len) for h in hubs]
        for L in Ls:
            if L < 1 or L > self.L:
                raise ValueError(f"clip of {L} latent frames, slots hold [1, {self.L}]")
        handles = [self._enqueue(hubs[b], Ls[b], _per(templates, b), _per(id_one_hots, b), _per(emotion_one_hots, b), _per(seeds, b), reqs[b],
                                 _per(style_track, b), _per(emotion_track, b)) for b in range(n)]
        self._fill()
        return handles

    def _fill(self):
        """Admit from the head of the queue while the head fits: a plain request needs one idle slot (the lowest), a long one needs
        its window count in idle slots, an arena range and a descriptor (FDM_ERR_STATE from admit_long = not yet); a request with
        its own sampler also needs that sampler in the bank (_sampler_id).  Nothing passes a request that waits."""
        while self._queue:
            r = self._queue[0]
            free = [s for s in range(self.n_slots) if self._slot[s] is None]
            if len(free) < max(r.get("windows", 0), 1):
                return
            own, r["sid"] = {}, 0          # a request that names nothing is admitted exactly as before
            if r.get("sampler") is not None or r.get("scale") is not None:
                r["sid"] = self._sampler_id(r["sampler"])
                if r["sid"] is None:       # the bank is full of samplers in use: wait for a slot to leave
                    return
                own = dict(sampler=r["sid"], cfg_scale=r["scale"])
            if r.get("tracks"):                # per-frame conditions (fdm_slot_admit_tracks / fdm_slot_admit_long_tracks)
                own = dict(own, style_track=r["st"], emotion_track=r["et"])
            if r.get("windows"):
                try:
                    self.plan.admit_long(free[:r["windows"]], r["hub"], r["ids"], r["emo"], r["x_T"], L_total=r["L"], overlap=self.overlap,
                                         seed=r["seed"], clip_id=0, **own)
                except FdmError as e:
                    if getattr(e, "code", None) == -4:       # arena or descriptors busy: the plan is untouched, wait for a group to leave
                        return
                    raise
                r["slots"] = free[:r["windows"]]
            else:
                self.plan.admit(free[0], r["hub"], r["ids"], r["emo"], r["x_T"], L=r["L"], seed=r["seed"], clip_id=0, **own)
                r["slots"] = free[:1]
            self._queue.pop(0)
            r.pop("hub"), r.pop("x_T")
            for s in r["slots"]:
                self._slot[s] = r

    @torch.no_grad()
    def submit_long(self, audio, template=None, id_one_hot=None, emotion_one_hot=None, seed=0, ddim_steps=None, sampler=None,
                    sampler_steps=None, eta=None, cfg_scale=None, style_track=None, emotion_track=None, rate=None):
        """rate: `audio` is raw PCM at that sample rate and goes through the device front end first (prepare_audio).
        One processor-normalised waveform [n] of ANY length -> a handle.  The audio encoder runs over the whole waveform and
        L_total = frames // pair is kept whole (submit() crops to a slot).  L_total <= max_frames is an ordinary request; a longer
        one becomes a group of slots (class docstring) with x_T drawn as animate_long draws it.  ValueError if the request can
        never fit: more windows than slots, or L_total > long_frames.  ddim_steps / sampler / sampler_steps / eta / cfg_scale as
        submit(): the result equals animate_long() with them."""
        from .denoiser import window_starts
        self._check()
        request = self._request(ddim_steps, sampler, sampler_steps, eta, cfg_scale)
        hub = self.model.audio_encoder(_waveform(audio, rate, self.device).reshape(1, -1)).last_hidden_state
        L = hub.shape[1] // self.p.pair
        if L < 1:
            raise ValueError(f"clip of {L} latent frames")
        windows = 0
        if L > self.L:
            if L > self.long_frames:
                raise ValueError(f"recording of {L} latent frames, the server's long arena holds {self.long_frames} (long_frames=)")
            windows = len(window_starts(L, self.L, self.overlap))
            if windows > self.n_slots:
                raise ValueError(f"recording of {L} latent frames needs {windows} windows of {self.L}, the server has {self.n_slots} slots")
        h = self._enqueue(hub, L, template, id_one_hot, emotion_one_hot, seed, request, style_track, emotion_track, windows)
        self._fill()
        return h

    @torch.no_grad()
    def step(self, n=10):
        """n diffusion steps for every running clip; clips whose chain ended are read, quantised and decoded at their own length
        (as animate_many does) and their slots go to the queue.  Returns the number of clips finished by this call."""
        self._check()
        self._fill()
        self.plan.run(n)
        fin = self._finish_long()
        if self.batch_stages:
            fin += self._finish_batched()
        else:
            for s in range(self.n_slots):
                r = self._slot[s]
                if r is not None and self.plan.slot_state(s)[2] == SLOT_FINISHED:
                    fin += self._finish_one([s], self.plan.read_slot(s, r["L"]), r)
        self._fill()
        return fin

    def _finish_one(self, slots, lat, r):
        """One finished request: its latent quantised and decoded at its own length, the result kept for results(), its slots idle."""
        out = self.ae.decode(self._quant(lat, r))
        self._done.append((r["handle"], self.outputs(out, r["template"]), lat))
        for s in slots:
            self._slot[s] = None
        return 1

    def _finish_long(self):
        """The groups whose chains ended: read the long latent, quantise and decode the whole L_total (the decoder is not causal), as
        animate_long does; every member slot goes back to the queue.  A long result has its own decode call, batch_stages or not."""
        fin = 0
        for s in range(self.n_slots):
            r = self._slot[s]
            if r is not None and r.get("windows") and r["slots"][0] == s and self.plan.slot_state(s)[2] == SLOT_FINISHED:
                fin += self._finish_one(r["slots"], self.plan.read_long(s), r)
        return fin

    def _finish_batched(self):
        """batch_stages: the clips whose chains ended in this call through ONE padded quant and ONE decode over their unequal lengths."""
        p = self.p
        done = [s for s in range(self.n_slots) if self._slot[s] is not None and self.plan.slot_state(s)[2] == SLOT_FINISHED]
        if not done:
            return 0
        reqs = [self._slot[s] for s in done]
        lats = [self.plan.read_slot(s, r["L"]) for s, r in zip(done, reqs)]
        pad = torch.zeros(len(done), max(r["L"] for r in reqs) * p.G, p.c, device=lats[0].device)
        for i, lat in enumerate(lats):
            pad[i, :lat.shape[1]] = lat[0]
        if p.n_emo and any(r.get("et") is not None for r in reqs):      # a track in the batch: every clip as a track (its one-hot on every frame otherwise)
            Lm = pad.shape[1] // p.G
            et = torch.stack([r["emo"].reshape(1, -1).expand(Lm, -1).clone() for r in reqs])
            for i, r in enumerate(reqs):
                if r.get("et") is not None:
                    et[i, :r["L"]] = r["et"]
            qs = _quantise(self.ae, p, pad, None, et)
        else:
            qs = _quantise(self.ae, p, pad, torch.cat([r["emo"] for r in reqs]) if p.n_emo else None)
        outs = self.ae.decode_many(qs, [r["L"] for r in reqs])
        self.batched_decodes.append(len(done))
        res = self.outputs.together([outs[i:i + 1, :r["L"]] for i, r in enumerate(reqs)], [r["template"] for r in reqs])
        for s, r, out, lat in zip(done, reqs, res, lats):
            self._done.append((r["handle"], out, lat))
            self._slot[s] = None
        return len(done)

    @property
    def pending(self):
        """Requests queued or in a slot."""
        return len(self._queue) + len({r["handle"] for r in self._slot if r is not None})

    def results(self):
        """[(handle, vertices [1, L, V3] -- with faces= a mesh.MeshFrames, with rig= a rig.RigFrames --, latent [1, L*G, c])] of the clips
        finished since the last call."""
        out, self._done = self._done, []
        return out

    def drain(self, n=10):
        """step(n) until nothing is queued or running; returns results()."""
        while self.pending:
            self.step(n)
        return self.results()


def add_track_arguments(ap, p):
    """--style_track / --emotion_track / --track_ramp of the demo and sampler command lines (fdm_amd.tracks.from_spec)."""
    ap.add_argument("--style_track", type=str, default=None,
                    help='build-added: style per time, "seconds:index,..." e.g. "0:0,3.5:2" (one vector per latent frame)')
    if p.n_emo:
        ap.add_argument("--emotion_track", type=str, default=None,
                        help=f'build-added: emotion per time, "seconds:name,..." e.g. "0:happy,21.0:sad,40.0:happy" ({" | ".join(EMOTIONS)})')
    ap.add_argument("--track_ramp", type=float, default=0.0, help="build-added: seconds of linear cross-fade centred on every change of a track")


def track_arguments(a, p, L):
    """{style_track=, emotion_track=} of animate() from the parsed flags, as tracks of L latent frames; {} when none was given."""
    from . import tracks
    out = {}
    if a.style_track:
        out["style_track"] = tracks.from_spec(p, L, a.style_track, [str(i) for i in range(p.n_style)], ramp=a.track_ramp)
    if p.n_emo and a.emotion_track:
        out["emotion_track"] = tracks.from_spec(p, L, a.emotion_track, EMOTIONS, ramp=a.track_ramp)
    return out


def add_time_filter_arguments(ap):
    """--time_filter / --time_filter_seconds / --time_filter_edge / --time_filter_direction / --time_filter_keep /
    --time_filter_keep_strength of the demo and sampler command lines (the device time filter, to_filtered)."""
    ap.add_argument("--time_filter", type=str, default=None,
                    help="build-added: smooth the decoded offsets along time on the device before anything reads them: gaussian:SIGMA (frames) | "
                         "savgol:RADIUS:ORDER | one_euro:MIN_CUTOFF:BETA[:D_CUTOFF] | ema:CUTOFF (cutoffs in Hz; BETA in Hz per (mesh unit per second): "
                         "it depends on the mesh's scale).  Off by default; its effect on quality or lip-sync metrics is unmeasured")
    ap.add_argument("--time_filter_direction", type=str, default=None, choices=("zero_phase", "causal"),
                    help="build-added: one_euro / ema only: zero_phase (default: forward, then backward over the result) | causal (it lags)")
    ap.add_argument("--time_filter_seconds", type=float, default=None, help="build-added: a Gaussian time filter of that many seconds (by the model's frame rate)")
    ap.add_argument("--time_filter_edge", type=str, default=None, choices=("mirror", "nearest"), help="build-added: the edge rule of the time filter (default mirror)")
    ap.add_argument("--time_filter_keep", type=str, default=None,
                    help="build-added: idx.npy, vertex indices that take the filter at --time_filter_keep_strength only (the lips keep their closures); 1 elsewhere")
    ap.add_argument("--time_filter_keep_strength", type=float, default=0.0, help="build-added: the strength in [0, 1] on the vertices of --time_filter_keep (0: untouched)")


def time_filter_arguments(a, p):
    """time_filter= of animate() from the parsed flags (the dict of tfilter.TimeFilterPlan's arguments), or None without a filter."""
    spec, seconds = getattr(a, "time_filter", None), getattr(a, "time_filter_seconds", None)
    edge, keep = getattr(a, "time_filter_edge", None), getattr(a, "time_filter_keep", None)
    direction = getattr(a, "time_filter_direction", None)
    if spec is None and seconds is None:
        if edge is not None or keep is not None or direction is not None:
            raise ValueError("--time_filter_edge / --time_filter_direction / --time_filter_keep need --time_filter or --time_filter_seconds")
        return None
    if spec is not None and seconds is not None:
        raise ValueError("--time_filter and --time_filter_seconds are two filters: give one of them")
    if seconds is not None:
        kw = dict(kind="gaussian", seconds=float(seconds))
    else:
        parts = spec.split(":")
        try:
            if parts[0] == "gaussian" and len(parts) == 2:
                kw = dict(kind="gaussian", sigma=float(parts[1]))
            elif parts[0] == "savgol" and len(parts) == 3:
                kw = dict(kind="savgol", radius=int(parts[1]), order=int(parts[2]))
            elif parts[0] == "one_euro" and len(parts) in (3, 4):
                kw = dict(kind="one_euro", min_cutoff=float(parts[1]), beta=float(parts[2]))
                if len(parts) == 4:
                    kw["d_cutoff"] = float(parts[3])
            elif parts[0] == "ema" and len(parts) == 2:
                kw = dict(kind="ema", cutoff=float(parts[1]))
            else:
                raise ValueError
        except ValueError:
            raise ValueError(f"--time_filter {spec!r}: gaussian:SIGMA, savgol:RADIUS:ORDER, one_euro:MIN_CUTOFF:BETA[:D_CUTOFF] or ema:CUTOFF") from None
    if kw["kind"] in ("one_euro", "ema"):
        if edge is not None:
            raise ValueError("--time_filter_edge belongs to gaussian and savgol: a recurrence has no edge rule")
        kw["direction"] = direction or "zero_phase"
    else:
        if direction is not None:
            raise ValueError("--time_filter_direction belongs to one_euro and ema: an FIR filter is zero-phase")
        kw["edge"] = edge or "mirror"
    if keep is not None:
        from .tfilter import strength_from_region
        kw["strength"] = strength_from_region(p.V3 // 3, np.load(keep), float(getattr(a, "time_filter_keep_strength", 0.0)))
    return kw


def add_rig_arguments(ap):
    """--rig_file / --rig_ridge / --rig_sweeps / --rig_smooth of the demo command lines (the device rig hand-off, to_rig)."""
    ap.add_argument("--rig_file", type=str, default=None,
                    help="build-added: blendshape rig (.npz: basis [K, 3V], optional names, weights [V], lo, hi, smooth_weights [K]): also save <stem>_rig.npy "
                         "[1, L_out, K], the coefficients fitted to the decoded offsets on the device.  Without --faces_file, --out_fps resamples "
                         "<stem>_rig.npy alone: <stem>.npy keeps the model's frame rate")
    ap.add_argument("--rig_ridge", type=float, default=0.0, help="build-added: ridge of the fit (with --rig_file)")
    ap.add_argument("--rig_sweeps", type=int, default=16, help="build-added: projected Gauss-Seidel sweeps of a bounded fit (with --rig_file)")
    ap.add_argument("--rig_smooth", type=float, default=0.0,
                    help="build-added: strength of the smoothness penalty between neighbouring saved frames, in the units of the rig's Gram "
                         "matrix (with --rig_file; 0: every frame is fitted on its own).  The .npz key smooth_weights [K] scales it per coefficient")


def rig_arguments(a):
    """rig= of animate() from the parsed flags (the dict of rig.RigPlan's arguments), or None without --rig_file."""
    if not a.rig_file:
        return None
    with np.load(a.rig_file, allow_pickle=False) as z:
        if "basis" not in z or ("lo" in z) != ("hi" in z):
            raise ValueError(f"{a.rig_file}: needs the key basis, and lo and hi together (has {sorted(z.files)})")
        kw = dict(basis=z["basis"], weights=z["weights"] if "weights" in z else None, ridge=a.rig_ridge,
                  bounds=(z["lo"], z["hi"]) if "lo" in z else None, sweeps=a.rig_sweeps,
                  names=[str(n) for n in z["names"]] if "names" in z else None)
        if getattr(a, "rig_smooth", 0.0):      # (a per-frame rig keeps the dict it always had)
            kw.update(smooth=a.rig_smooth, smooth_weights=z["smooth_weights"] if "smooth_weights" in z else None)
        return kw


def add_wrap_arguments(ap):
    """--wrap_file / --wrap_falloff of the demo command lines (the device wrap hand-off, to_wrap)."""
    ap.add_argument("--wrap_file", type=str, default=None,
                    help="build-added: a mesh of another topology (.npz: vertices [Vt, 3] in the template's space, optional faces [Ft, 3], "
                         "weights [Vt], face_idx [Vt]) that follows the animation: also save <stem>_wrap.npy [1, L, 3 Vt], one frame per frame "
                         "of <stem>.npy, which keeps its content.  Needs --faces_file (the model's triangles) and a template.  With faces in "
                         "the file and --save_normals: <stem>_wrap_normals.npy")
    ap.add_argument("--wrap_falloff", type=str, default=None,
                    help="build-added: r0,r1 -- target vertices closer than r0 to the face follow it fully, those beyond r1 stay at rest, "
                         "smoothstep between (with --wrap_file; for a body mesh of which only the face should move)")


def add_render_arguments(ap):
    """--render / --render_size / --render_samples / --background_black / --render_alpha / --render_yuv (+ _matrix, _full) of the demo
    command lines (the device render hand-off, to_images)."""
    ap.add_argument("--render", action="store_true",
                    help="build-added: also save <stem>_frames.npy, uint8 [1, L_out, N, N, 3]: the frames of <stem>.npy drawn on the device with the "
                         "reference's camera and light directions (needs --faces_file), and print the ffmpeg line that makes an .mp4 of them")
    ap.add_argument("--render_size", type=int, default=800, help="build-added: N, the side of the rendered frames in pixels (with --render)")
    ap.add_argument("--render_samples", type=int, default=1, choices=(1, 4, 16),
                    help="build-added: coverage samples per pixel of the rendered frames, 4 or 16 for anti-aliased edges (with --render)")
    ap.add_argument("--background_black", action="store_true", help="a black background instead of white (with --render)")
    ap.add_argument("--render_alpha", action="store_true",
                    help="build-added: also save <stem>_alpha.npy, uint8 [1, L_out, N, N]: the coverage of every pixel; with --background_black "
                         "the frames are premultiplied by it (with --render)")
    ap.add_argument("--render_yuv", choices=("i420", "nv12"), default=None,
                    help="build-added: also save the frames as Y'CbCr 4:2:0 made on the device, <stem>.y4m (i420) or raw <stem>.nv12, and print "
                         "the ffmpeg line that encodes them without a colour conversion (with --render; N even)")
    ap.add_argument("--render_yuv_matrix", type=int, default=709, choices=(601, 709), help="build-added: the matrix of --render_yuv (BT.601 or BT.709)")
    ap.add_argument("--render_yuv_full", action="store_true", help="build-added: full-range --render_yuv (0 .. 255) instead of limited (16 .. 235)")
    ap.add_argument("--render_colors", default=None, help="build-added: c.npy, float [V, 3] >= 0: vertex colours in place of the grey base (with --render)")
    ap.add_argument("--render_texture", default=None,
                    help="build-added: tex.npy, uint8 [Ht, Wt, 3] with row 0 at the top (no image formats are decoded), drawn with --render_uv")
    ap.add_argument("--render_uv", default=None, help="build-added: uv.npz with the keys vt [T, 2] and ft [F, 3] (FLAME's) or uv [F, 3, 2] (with --render_texture)")
    ap.add_argument("--render_error_to", default=None,
                    help="build-added: gt.npy, ground-truth vertices [L' >= L, 3 V]: the frames show the per-vertex distance to them as a heat map (with --render)")
    ap.add_argument("--render_error_max", type=float, default=0.01, help="build-added: the distance that takes the last colour of the table (with --render_error_to)")
    ap.add_argument("--render_colormap", default="heat", choices=("heat", "jet", "grey"), help="build-added: the table of --render_error_to")
    ap.add_argument("--render_unlit", action="store_true", help="build-added: the material's colour as it is, without the lights (with --render)")


def material_arguments(a):
    """dict(material=, error_to=) of the --render_colors / --render_texture + --render_uv / --render_error_to flags (at most one of the
    three), empty without them; --render_unlit alone is the base colour unlit."""
    from .render import Material, uv_corners
    unlit = bool(getattr(a, "render_unlit", False))
    colors, tex, uvf, gt = (getattr(a, k, None) for k in ("render_colors", "render_texture", "render_uv", "render_error_to"))
    if sum(x is not None for x in (colors, tex, gt)) > 1:
        raise ValueError("--render_colors, --render_texture and --render_error_to are three materials: one at a time")
    if (tex is None) != (uvf is None):
        raise ValueError("--render_texture and --render_uv go together")
    if colors is not None:
        return dict(material=Material.vertex_colors(np.load(colors), unlit=unlit))
    if tex is not None:
        z = np.load(uvf)
        uv = z["uv"] if "uv" in z.files else uv_corners(z["vt"], z["ft"])
        return dict(material=Material.texture(np.load(tex), uv, unlit=unlit))
    if gt is not None:
        g = np.load(gt).astype(np.float32)
        return dict(material=Material.scalar_map(getattr(a, "render_colormap", "heat"), 0.0, float(getattr(a, "render_error_max", 0.01)), unlit=unlit),
                    error_to=g.reshape(g.shape[-3] if g.ndim >= 3 and g.shape[-1] == 3 else g.shape[-2], -1))
    return dict(material=Material.base(unlit=True)) if unlit else {}


def save_frames(a, p, verts, faces, dst):
    """--render: verts [1, L_out, 3 V] -> <dst>_frames.npy and the ffmpeg line (not run: video encoding is not part of this project);
    --render_alpha: <dst>_alpha.npy; --render_yuv: <dst>.y4m or <dst>.nv12 and their ffmpeg line."""
    from .render import Camera, write_y4m
    name = next((n for n in ("biwi", "mead") if n in p.name.lower()), "vocaset")
    N = int(a.render_size)
    bg = (0.0, 0.0, 0.0) if a.background_black else (1.0, 1.0, 1.0)
    view = dict(camera=Camera.preset(name).resized(N, N), background=bg, samples=int(getattr(a, "render_samples", 1)))
    layout, full = getattr(a, "render_yuv", None), bool(getattr(a, "render_yuv_full", False))
    if getattr(a, "render_alpha", False):
        view["alpha"] = True
    if layout:
        view.update(yuv=layout, yuv_matrix=int(getattr(a, "render_yuv_matrix", 709)), yuv_range="full" if full else "limited")
    mat = material_arguments(a)
    if "error_to" in mat:      # the error field of the saved vertices
        v = verts if verts.dim() == 3 else verts.unsqueeze(0)
        mat = dict(material=mat["material"], scalars=_error_field(v, None, mat["error_to"], v.device))
    view.update(mat)
    im = to_images(verts, faces, view)
    np.save(dst + "_frames", im.images.detach().cpu().numpy())
    print(f"saved {dst}_frames.npy {tuple(im.images.shape)}")
    rate = a.out_fps or a.in_fps or p.fps or 30
    print(f"python -c \"import numpy as np, sys; sys.stdout.buffer.write(np.load('{dst}_frames.npy').tobytes())\" | "
          f"ffmpeg -f rawvideo -pix_fmt rgb24 -s {N}x{N} -r {rate:g} -i - -i {a.audio_file} -c:v libx264 -pix_fmt yuv420p -shortest {dst}.mp4")
    if im.alpha is not None:
        np.save(dst + "_alpha", im.alpha.detach().cpu().numpy())
        print(f"saved {dst}_alpha.npy {tuple(im.alpha.shape)}")
    if layout == "i420":
        size = write_y4m(dst + ".y4m", im.yuv, im.frames, N, N, rate, full)
        print(f"saved {dst}.y4m ({size} bytes)")
        print(f"ffmpeg -i {dst}.y4m -i {a.audio_file} -c:v libx264 -pix_fmt yuv420p -shortest {dst}_yuv.mp4")
    elif layout == "nv12":
        with open(dst + ".nv12", "wb") as f:
            f.write(im.yuv[0, :im.frames[0]].detach().cpu().numpy().tobytes())
        print(f"saved {dst}.nv12 ({im.frames[0]} frames of {3 * N * N // 2} bytes)")
        tags = f"-color_range {'pc' if full else 'tv'} -colorspace {'bt709' if view['yuv_matrix'] == 709 else 'smpte170m'}"
        print(f"ffmpeg -f rawvideo -pix_fmt nv12 -s {N}x{N} -r {rate:g} {tags} -i {dst}.nv12 -i {a.audio_file} -c:v libx264 -pix_fmt yuv420p "
              f"-shortest {dst}_yuv.mp4")


def wrap_arguments(a, faces, template, device):
    """(wrap.WrapPlan, the target's faces or None) from the parsed flags, or (None, None) without --wrap_file.  faces: the model's
    triangle list; template: its rest vertices [1, 3 V]."""
    if not getattr(a, "wrap_file", None):
        if getattr(a, "wrap_falloff", None):
            raise ValueError("--wrap_falloff needs --wrap_file")
        return None, None
    if faces is None or template is None:
        raise ValueError("--wrap_file binds to the model's rest surface: it needs --faces_file and a template")
    from .wrap import WrapPlan, falloff_weights
    src = torch.as_tensor(template, dtype=torch.float32).detach().cpu().numpy().reshape(-1, 3)
    with np.load(a.wrap_file, allow_pickle=False) as z:
        if "vertices" not in z:
            raise ValueError(f"{a.wrap_file}: needs the key vertices (has {sorted(z.files)})")
        kw = dict(src_rest=src, faces=faces, dst_rest=z["vertices"], face_idx=z["face_idx"] if "face_idx" in z else None,
                  weights=z["weights"] if "weights" in z else None)
        faces_t = z["faces"] if "faces" in z else None
    plan = WrapPlan(device=device, **kw)
    if a.wrap_falloff:
        if kw["weights"] is not None:
            raise ValueError("--wrap_falloff with weights in the file: give one of them")
        r0, r1 = (float(x) for x in a.wrap_falloff.split(","))
        fi, _, dist = plan.binding()
        plan = WrapPlan(device=device, **dict(kw, face_idx=fi, weights=falloff_weights(dist, r0, r1)))
    return plan, faces_t


def add_flame_arguments(ap):
    """--flame_model / --flame_expr_at / --template_params of the MEAD command lines (the device parametric head, to_flame)."""
    ap.add_argument("--flame_model", type=str, default=None,
                    help="build-added: FLAME-type model file (.npz or a pickled dict of plain arrays: flame.FlameModel.load): the template is "
                         "made from parameters on the device as the reference's torch2mesh does (the neutral face without --template_params)")
    ap.add_argument("--flame_expr_at", type=int, default=None, help="build-added: index of the first expression coefficient (FLAME: 300; default the file's expr_at, else NB)")
    ap.add_argument("--template_params", type=str, default=None, help="build-added: .npy of [1, NE + 6] FLAME parameters (expression, then global and jaw pose) for the template (with --flame_model)")


def add_flame_fit_arguments(ap, has_flame_model):
    """--flame_fit / --fit_joints / --fit_expr / --fit_iters of the demo command lines (to_flame_params of the saved frames); --flame_model
    too where the preset's command line has none of its own."""
    if not has_flame_model:
        ap.add_argument("--flame_model", type=str, default=None, help="build-added: FLAME-type model file (.npz or a pickled dict of plain arrays: flame.FlameModel.load) for --flame_fit")
        ap.add_argument("--flame_expr_at", type=int, default=None, help="build-added: index of the first expression coefficient (FLAME: 300; default the file's expr_at, else NB)")
    ap.add_argument("--flame_fit", action="store_true",
                    help="build-added: fit the head of --flame_model to every saved frame on the device and write <stem>_flame.npz (expression [1, L, n], "
                         "pose [1, L, 3 J], transl [1, L, 3], rms [1, L]) beside <stem>.npy")
    ap.add_argument("--fit_joints", type=str, default="jaw", help="build-added: free joints of --flame_fit, names (global neck jaw eye_l eye_r) or indices, comma-separated; 'none': expression only")
    ap.add_argument("--fit_expr", type=int, default=50, help="build-added: expression coefficients fitted by --flame_fit")
    ap.add_argument("--fit_iters", type=int, default=None, help="build-added: Gauss-Newton steps of --flame_fit (default: flame.FIT_DEFAULTS, a setting)")


def flame_fit_arguments(a):
    """flame_fit= of to_flame_params from the parsed flags, or None without --flame_fit."""
    if not getattr(a, "flame_fit", False):
        return None
    if not a.flame_model:
        raise ValueError("--flame_fit needs --flame_model")
    from .flame import FlameModel
    names = [] if a.fit_joints.strip().lower() in ("", "none") else [j.strip() for j in a.fit_joints.split(",")]
    return dict(model=FlameModel.load(a.flame_model, expr_at=a.flame_expr_at), n_expr=a.fit_expr, joints=tuple(int(j) if j.lstrip("-").isdigit() else j for j in names),
                iters=a.fit_iters)


def save_flame_fit(fit_args, out, dst):
    """<dst>_flame.npz: the FlameFit of the saved frames `out` [1, L, 3 V] (absolute vertices)"""
    kw = {k: v for k, v in fit_args.items() if k != "model"}
    ff = to_flame_params(out, fit_args["model"], **kw)
    np.savez(dst + "_flame.npz", expression=ff.expression.cpu().numpy(), pose=ff.pose.cpu().numpy(), transl=ff.transl.cpu().numpy(), rms=ff.rms.cpu().numpy())
    print(f"saved {dst}_flame.npz expression {tuple(ff.expression.shape)} pose {tuple(ff.pose.shape)} (rms max {float(ff.rms.max()):.3g}, {int((ff.status != 0).sum())} failed frames)")


def flame_template(model, params=None, device="cuda:0", n_expr=50):
    """The MEAD template of samples/sample_diffusion_mead.py:76 from parameters: params [..., NE + 6] (expression, then global and jaw
    pose; None: zeros, the neutral face) -> [1, 3 V] on the device (flame.torch2mesh: zero shape, 4 decimals).  model: a
    flame.FlameModel / FlamePlan / model file."""
    from .flame import torch2mesh
    plan = _flame_plan(model, device)
    if params is None:
        prm = torch.zeros(1, min(n_expr, plan.NB - plan.model.expr_at) + 6)
    else:
        prm = torch.as_tensor(params, dtype=torch.float32).detach().cpu()
        prm = prm.reshape(-1, prm.shape[-1])[:1]
    if prm.shape[-1] < 6:
        raise ValueError(f"template parameters are expression coefficients then 6 pose numbers, got {prm.shape[-1]} numbers")
    return torch2mesh(plan, prm[:, :prm.shape[-1] - 6], prm[:, prm.shape[-1] - 6:])[0]


def flame_arguments(a, device):
    """template of animate() from the parsed flags ([1, 3 V] on the device), or None without --flame_model."""
    if not getattr(a, "flame_model", None):
        if getattr(a, "template_params", None):
            raise ValueError("--template_params needs --flame_model")
        return None
    from .flame import FlameModel
    return flame_template(FlameModel.load(a.flame_model, expr_at=a.flame_expr_at), None if not a.template_params else np.load(a.template_params), device)


def demo_main(preset, argv=None):
    """CLI of demo/demo_{vocaset,biwi,3d_mead}.py:109-121: same flags, output = np.save(<audio_path>/<stem>.npy, [1, L, V3])."""
    import argparse
    p = presets.get(preset)
    ap = argparse.ArgumentParser(description="Expressive 3D Facial Animation Generation Based on Local-to-global Latent Diffusion")
    ap.add_argument("--audio_file", type=str, help="the audio file path for prediction")
    if p.n_emo:
        ap.add_argument("--emotion", type=str, default="happy", choices=EMOTIONS)
    ap.add_argument("--vertice_dim", type=int, default=p.V3)
    ap.add_argument("--feature_dim", type=int, default=p.d)
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--template_file", type=str, default="templates.pkl")
    ap.add_argument("--stage1_model_path", type=str, default=f"{p.name}/{p.name}_stage1.mpt")
    ap.add_argument("--stage2_model_path", type=str, default=f"{p.name}/{p.name}_stage2.mpt")
    ap.add_argument("--audio_path", type=str, default=f"{p.name}/result")
    ap.add_argument("--ddim_steps", type=int, default=0, help="build-added: DDIM steps (0 = full DDPM chain)")
    ap.add_argument("--sampler", type=str, default=None, choices=["dpmpp2m", "ddim_eta"],
                    help="build-added: table-driven multistep sampler (DPM-Solver++ 2M | DDIM with --eta) instead of DDPM / DDIM")
    ap.add_argument("--sampler_steps", type=int, default=20, help="build-added: steps of --sampler")
    ap.add_argument("--eta", type=float, default=0.0, help="build-added: eta of --sampler ddim_eta, in [0, 1]")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--long_audio", type=str, default="truncate", choices=["truncate", "window"],
                    help="build-added: audio past max_len latent frames: truncate (the reference's crop) or window (animate it all)")
    ap.add_argument("--window_overlap", type=int, default=60, help="build-added: frames shared by neighbouring windows (--long_audio window)")
    ap.add_argument("--device_audio", action="store_true",
                    help="build-added: convert, downmix, resample and normalise the file's raw samples on the device (prepare_audio)")
    ap.add_argument("--faces_file", type=str, default=None,
                    help="build-added: triangle list (.npy, int [F, 3]): positions and vertex normals through the device mesh hand-off")
    ap.add_argument("--out_fps", type=float, default=None, help=f"build-added: frame rate of the saved motion (with --faces_file or --rig_file; the model's is {p.fps or 'given by --in_fps'})")
    ap.add_argument("--in_fps", type=float, default=None, help="build-added: the model's frame rate where the preset states none (with --out_fps)")
    ap.add_argument("--save_normals", action="store_true", help="build-added: also save <stem>_normals.npy [1, L_out, 3V] (with --faces_file)")
    add_track_arguments(ap, p)
    add_rig_arguments(ap)
    add_wrap_arguments(ap)
    add_render_arguments(ap)
    if p.n_emo:        # MEAD: the template comes from FLAME parameters
        add_flame_arguments(ap)
    add_flame_fit_arguments(ap, bool(p.n_emo))
    add_time_filter_arguments(ap)
    a = ap.parse_args(argv)
    ffa = flame_fit_arguments(a)
    tfa = time_filter_arguments(a, p)
    if a.render and not a.faces_file:
        raise ValueError("--render draws the model's triangles: it needs --faces_file")
    rig = rig_arguments(a)
    diffusion, ae = build_models(p.name, a.feature_dim, a.device, a.stage1_model_path, a.stage2_model_path,
                                 cfg_level=None)
    if a.device_audio:
        wav = prepare_audio(*load_pcm(a.audio_file), device=a.device)
    else:
        wav = processor_normalize(load_wav(a.audio_file))
    template = None
    if os.path.exists(a.template_file) and a.template_file.endswith(".npy"):
        template = np.load(a.template_file).reshape(1, -1)
    # --flame_model on the MEAD command line: the template from parameters, in place of --template_file (elsewhere it serves --flame_fit alone)
    ft = flame_arguments(a, a.device) if p.n_emo else None
    if ft is not None:
        template = ft
    wp, faces_t = wrap_arguments(a, np.load(a.faces_file) if a.faces_file else None, template, a.device)
    emo = None
    if p.n_emo:
        emo = torch.eye(p.n_emo)[EMOTIONS.index(a.emotion)].unsqueeze(0)
    fast = dict(sampler=a.sampler, sampler_steps=a.sampler_steps, eta=a.eta)
    # tracks cover every latent frame the audio can give (16 kHz, 320 samples per encoder frame); the calls take the frames they need
    fast.update(track_arguments(a, p, max(len(wav) // 320 // p.pair + 2, p.max_len)))
    if tfa is not None:      # everything saved below follows the filtered offsets (seconds= by --in_fps or the preset's frame rate)
        fast.update(time_filter=tfa)
        if not a.faces_file:
            fast.update(in_fps=a.in_fps)
    if a.faces_file:
        fast.update(faces=np.load(a.faces_file), out_fps=a.out_fps, in_fps=a.in_fps, mesh=dict(normals=a.save_normals), rig=rig)
    if rig is not None and not a.faces_file:        # the offsets come back bare: the rig is fitted to them, the template added after
        tmpl_after, template = template, None
    if a.long_audio == "window":
        out, _ = animate_long(diffusion, ae, wav, template, None, emo, ddim_steps=a.ddim_steps, seed=a.seed,
                              overlap=a.window_overlap, device=a.device, **fast)
    else:
        out, _ = animate(diffusion, ae, wav, template, None, emo, ddim_steps=a.ddim_steps, seed=a.seed, device=a.device, **fast)
    os.makedirs(a.audio_path, exist_ok=True)
    dst = os.path.join(a.audio_path, os.path.basename(a.audio_file)[:-4])
    if rig is not None:
        if a.faces_file:
            out, rf = out
        else:
            rf = to_rig(out, rig, fps=_mesh_fps(p, a.in_fps, a.out_fps))
            out = _hand_off(out, tmpl_after, a.device)
        np.save(dst + "_rig", rf.weights.detach().cpu().numpy())
        print(f"saved {dst}_rig.npy {tuple(rf.weights.shape)}" + (f" ({', '.join(rf.names[:4])}, ...)" if rf.names else ""))
    if a.faces_file:        # positions keep the reference's name and shape
        if a.save_normals:
            nr = out.normals.reshape(out.normals.shape[0], out.normals.shape[1], -1)
            np.save(dst + "_normals", nr.detach().cpu().numpy())
            print(f"saved {dst}_normals.npy {tuple(nr.shape)}")
        out = out.positions.reshape(out.positions.shape[0], out.positions.shape[1], -1)
    if wp is not None:      # the bound mesh follows the saved frames: one wrapped frame per frame of <stem>.npy
        wv = to_wrap(out, wp)
        if faces_t is not None and a.save_normals:
            nr = to_mesh(wv, faces_t, None, normals=True).normals.reshape(wv.shape[0], wv.shape[1], -1)
            np.save(dst + "_wrap_normals", nr.detach().cpu().numpy())
            print(f"saved {dst}_wrap_normals.npy {tuple(nr.shape)}")
        np.save(dst + "_wrap", wv.detach().cpu().numpy())
        print(f"saved {dst}_wrap.npy {tuple(wv.shape)}")
    if a.render:            # the saved frames drawn on the device: one image per frame of <stem>.npy
        save_frames(a, p, out, np.load(a.faces_file), dst)
    if ffa is not None:     # the head's parameters of the saved frames: one fit per frame of <stem>.npy
        save_flame_fit(ffa, out, dst)
    np.save(dst, out.detach().cpu().numpy())
    print(f"saved {dst}.npy {tuple(out.shape)}")
    return dst + ".npy"
