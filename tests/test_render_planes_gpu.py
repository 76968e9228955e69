"""MI355X: the planes of the render hand-off (fdm_render_forward_planes; csrc/render_out.hpp, render_resolve_kernel<S, YUV>) -- rgb,
depth and face equal to fdm_render_forward on the same inputs, alpha equal to the numpy restatement from the per-sample coverage, the
4:2:0 planes equal byte for byte to the restatement applied to the call's own rgb (tests/render_planes_cases.py; DESIGN.md section 2
item 24), on the smallest shapes that can go wrong: one chroma sample, a chroma grid that no block of lanes divides, a partial last
workgroup, odd sizes for alpha alone, every subset of the outputs, ragged clips, chunks, and the visibility buffer left clear.  The
view is coloured (a grey one has U = V = 128 everywhere).  Outputs are filled with junk before every call."""
import functools
import itertools

import numpy as np
import pytest
import torch

import mesh_cases as MC
import render_aa_cases as RA
import render_cases as RC
import render_planes_cases as RP
import wrap_cases as WC
from fdm_amd import pipeline, render
from fdm_amd._lib import FdmError
from test_render_gpu import DEV, PIPE_MESH, dev, pipe_view, plan_of, run, tiny_audio, tiny_models

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = ("rgb", "depth", "face_ids", "alpha", "yuv")
SAMPLES = [1, 4, 16]
EVEN = [(2, 2), (6, 4), (34, 18), (66, 2)]      # 34 x 18: 612 pixels, 153 blocks (a partial workgroup either way), chroma 17 x 9
ODD = [(3, 3), (33, 17)]                        # alpha alone
COMBOS = [(m, r, l) for m in (601, 709) for r in ("limited", "full") for l in ("i420", "nv12")]


def coloured(W, H, **kw):
    return RC.view(W, H, base=(0.9, 0.45, 0.15), background=(0.1, 0.5, 0.9), **kw)


def mesh_of(name):
    if name == "icosphere1":             # silhouettes: partly covered pixels
        return RC.icosphere(1, 0.3)
    if name == "whole_viewport":         # one triangle over every sample of the view
        return RC.tris([(-9, -9, -0.5), (9, -9, -0.5), (0, 9, 0.2)], [(0, 1, 2)])
    if name == "off_screen":             # nothing on the screen
        return RC.tris([(3, 3, 0), (4, 3, 0), (3, 4, 0), (-5, 0, 0), (-4, 0, 0), (-5, 1, 0)], [(0, 1, 2), (3, 4, 5)])
    return RC.strip(40)


MESHES = ["icosphere1", "whole_viewport", "off_screen", "strip40"]
JUNK = dict(rgb=0x5A, depth=float("nan"), face_ids=12345, alpha=0x5A, yuv=0x5A)
DTYPE = dict(rgb=torch.uint8, depth=torch.float32, face_ids=torch.int32, alpha=torch.uint8, yuv=torch.uint8)


def shape_of(k, B, Lo, plan):
    H, W = plan.H, plan.W
    return (B, Lo) + dict(rgb=(H, W, 3), depth=(H, W), face_ids=(H, W), alpha=(H, W), yuv=(3 * W * H // 2,))[k]


def planes(plan, x, names=NAMES, frames=None, tmpl=None, fps=None, Lo=None):
    """dict of numpy arrays (and "frames") of one planes call into junk-filled outputs of L_out_max = Lo (None: the longest clip's)"""
    x = dev(x)
    B = x.shape[0]
    if Lo is None:
        Lo = max([MC.frames_out(L, fps) for L in (frames if frames is not None else [x.shape[1]] * B)] + [1])
    out = {k: torch.full(shape_of(k, B, Lo, plan), JUNK[k], dtype=DTYPE[k], device=DEV) for k in names}
    got = plan.forward(x, frames, None if tmpl is None else dev(tmpl), fps, out=out)
    pairs = dict(rgb=got.images, depth=got.depth, face_ids=got.face_ids, alpha=got.alpha, yuv=got.yuv)
    for k in NAMES:
        assert (pairs[k] is out[k]) if k in names else (pairs[k] is None), k
    res = {k: out[k].cpu().numpy() for k in names}
    res["frames"] = got.frames
    return res


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def set_combo(plan, combo):
    plan.set_yuv(*combo)
    return RP.coeffs(combo[0], combo[1] == "full"), combo[2]


@functools.lru_cache(maxsize=None)
def static_case(name, wh, S):
    """(p, faces, view, the plain call's (rgb, depth, face) of one frame, the restatement's alpha); computed once per case"""
    vw = coloured(*wh)
    p, f = mesh_of(name)
    base = run(plan_of(f, len(p), vw, samples=S), p.reshape(1, 1, -1))
    return p, f, vw, base[:3], RP.alpha_of(p, f, vw, S)


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("wh", EVEN, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", MESHES)
def test_every_plane_on_even_sizes(name, wh, S):
    p, f, vw, (rgb, depth, face), want_alpha = static_case(name, wh, S)
    plan = plan_of(f, len(p), vw, samples=S)
    x = p.reshape(1, 1, -1)
    for combo in COMBOS:
        k, layout = set_combo(plan, combo)
        got = planes(plan, x)
        assert same_bytes(got["rgb"], rgb) and same_bytes(got["depth"], depth) and same_bytes(got["face_ids"], face), combo
        assert np.array_equal(got["alpha"][0, 0], want_alpha), combo
        want = RP.yuv(got["rgb"][0, 0], k, layout)
        assert got["yuv"][0, 0].tobytes() == want, f"{combo}: {int((got['yuv'][0, 0] != np.frombuffer(want, np.uint8)).sum())} bytes differ"
        assert planes(plan, x, ("yuv",))["yuv"].tobytes() == want, f"{combo}: yuv alone (no rgb in memory)"
    # what each mesh is there for, on the restatement the device has just been held to
    if name == "whole_viewport":
        assert (want_alpha == 255).all() and (face == 0).all()
    if name == "off_screen":
        assert (want_alpha == 0).all() and (face == -1).all()
        bg = rgb[0, 0, 0, 0].astype(np.int64)                                # the background's (int)(255 c + 0.5f)
        assert (rgb == rgb[0, 0, 0, 0]).all() and bg[0] < 40 and bg[2] > 200
        y = int(RP.luma(bg, k))
        u, v = (int(c) for c in RP.chroma(4 * bg, k))
        n = wh[0] * wh[1]
        assert (got["yuv"][0, 0, :n] == y).all() and (got["yuv"][0, 0, n::2] == u).all() and (got["yuv"][0, 0, n + 1::2] == v).all()      # (nv12 is last)
        assert u > 160 and v < 100                                           # a blue that is no grey
    if name == "icosphere1" and wh == (34, 18):
        seen = set(np.unique(want_alpha).tolist())
        assert seen == {0, 255} if S == 1 else seen - {0, 255}, "a silhouette leaves partly covered pixels at S > 1"
        if S == 4:
            assert seen <= {0, 64, 128, 191, 255}
        assert len(np.unique(got["yuv"][0, 0, 34 * 18:])) > 4               # chroma that varies


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("wh", ODD, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", MESHES)
def test_alpha_on_odd_sizes(name, wh, S):
    p, f, vw, (rgb, depth, face), want_alpha = static_case(name, wh, S)
    plan = plan_of(f, len(p), vw, samples=S)
    got = planes(plan, p.reshape(1, 1, -1), ("rgb", "depth", "face_ids", "alpha"))
    assert same_bytes(got["rgb"], rgb) and same_bytes(got["depth"], depth) and same_bytes(got["face_ids"], face)
    assert np.array_equal(got["alpha"][0, 0], want_alpha)
    assert np.array_equal(planes(plan, p.reshape(1, 1, -1), ("alpha",))["alpha"][0, 0], want_alpha)
    if name == "icosphere1" and wh == (33, 17) and S == 4:
        seen = set(np.unique(want_alpha).tolist())
        assert seen <= {0, 64, 128, 191, 255} and seen - {0, 255}


def test_odd_sizes_refuse_yuv_and_still_give_alpha():
    p, f, vw, _, want_alpha = static_case("icosphere1", (33, 17), 4)
    plan = plan_of(f, len(p), vw, samples=4)
    x = dev(p.reshape(1, 1, -1))
    out = {k: torch.full(shape_of(k, 1, 1, plan), JUNK[k], dtype=DTYPE[k], device=DEV) for k in ("rgb", "alpha", "yuv")}
    with pytest.raises(FdmError, match="even width and height") as e:
        plan.forward(x, out=out)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert all(bool((out[k] == 0x5A).all()) for k in out)                     # nothing was launched
    with pytest.raises(FdmError, match="even"):
        plan.forward(x, rgb=False, yuv=True)
    with pytest.raises(FdmError, match="no output"):
        plan.forward(x, rgb=False)
    with pytest.raises(FdmError, match="the outputs are"):
        plan.forward(x, out=dict(images=None))
    got = plan.forward(x, alpha=True)
    assert np.array_equal(got.alpha.cpu().numpy()[0, 0], want_alpha) and got.yuv is None and got.images is not None and got.depth is None


@pytest.mark.parametrize("S", SAMPLES)
def test_every_subset_of_the_outputs(S):
    p, f, vw, _, _ = static_case("icosphere1", (34, 18), S)
    plan = plan_of(f, len(p), vw, samples=S, yuv_layout="nv12", yuv_matrix=601)
    x = p.reshape(1, 1, -1)
    every = planes(plan, x)
    for n in range(1, 5):
        for names in itertools.combinations(NAMES, n):
            got = planes(plan, x, names)
            for k in names:
                assert same_bytes(got[k], every[k]), f"{k} of {names}"


@functools.lru_cache(maxsize=None)
def clips_case(S):
    """the small grid mesh in front of a 34 x 18 camera, two clips of 3 and 1 frames at 30 -> 60 frames a second, NaN past every clip's
    frames; per clip the restatement's alpha [L_out, H, W]"""
    faces, V, _ = MC.mesh("grid")
    frames, fps = [3, 1], (30, 60)
    off = MC.offsets("grid", 2, 4, seed=31)
    tmpl = (MC.template("grid", seed=3, rows=2) - np.tile(np.array([0.35, 0.15, 0.0], F32), V)).astype(F32)
    vw = coloured(34, 18)
    alphas = [np.stack([RP.alpha_of(q[t].reshape(V, 3), faces, vw, S) for t in range(len(q))]) for q in MC.positions(off, tmpl, frames, fps)]
    x = off.copy()
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return x, tmpl, frames, fps, faces, V, vw, alphas


@pytest.mark.parametrize("S", SAMPLES)
def test_ragged_clips_padding_and_chunks(S):
    x, tmpl, frames, fps, faces, V, vw, alphas = clips_case(S)
    plan = plan_of(faces, V, vw, samples=S)
    k = RP.coeffs(709, False)
    batch = planes(plan, x, NAMES, frames, tmpl, fps, Lo=7)
    assert batch["frames"] == [6, 2] == [len(a) for a in alphas]
    plain = run(plan_of(faces, V, vw, samples=S), x, frames, tmpl, fps, Lo=7)
    for i, name in enumerate(("rgb", "depth", "face_ids")):
        assert same_bytes(batch[name], plain[i]), name
    for b, n in enumerate(batch["frames"]):
        assert np.array_equal(batch["alpha"][b, :n], alphas[b]) and (alphas[b] > 0).any()
        assert np.array_equal(batch["yuv"][b, :n], RP.yuv_frames(batch["rgb"][b, :n], k, "i420"))
        for name in NAMES:                                                    # zeros, not video black
            assert not batch[name][b, n:].view(np.uint8).any(), f"{name}: padding of clip {b}"
        alone = planes(plan, x[b:b + 1, :frames[b]], NAMES, [frames[b]], tmpl[b:b + 1], fps)
        assert alone["frames"] == [n]
        for name in NAMES:
            assert same_bytes(alone[name][0, :n], batch[name][b, :n]), f"{name}: clip {b} alone"
    for chunk in (1, 3):
        plan.set_chunk_frames(chunk)
        got = planes(plan, x, NAMES, frames, tmpl, fps, Lo=7)
        for name in NAMES:
            assert same_bytes(got[name], batch[name]), f"{name}: chunk_frames = {chunk}"
    only = planes(plan, x, ("yuv", "alpha"), frames, tmpl, fps, Lo=7)
    assert same_bytes(only["yuv"], batch["yuv"]) and same_bytes(only["alpha"], batch["alpha"])


@pytest.mark.parametrize("S", SAMPLES)
def test_the_visibility_buffer_is_left_clear(S):
    """the same call twice, a plain call between two planes calls and after one: every picture as from a fresh object"""
    p, f, vw, base, _ = static_case("icosphere1", (34, 18), S)
    plan = plan_of(f, len(p), vw, samples=S)
    x = p.reshape(1, 1, -1)
    a = planes(plan, x)
    b = planes(plan, x)
    mid = run(plan, x)
    c = planes(plan, x, ("yuv",))
    d = planes(plan, x)
    last = run(plan, x)
    for name in NAMES:
        assert same_bytes(a[name], b[name]) and same_bytes(a[name], d[name]), name
    assert same_bytes(c["yuv"], a["yuv"])
    for i in range(3):
        assert same_bytes(mid[i], base[i]) and same_bytes(last[i], base[i])


def test_over_black_rgb_is_premultiplied_by_alpha():
    """a surface lit by the ambient term alone over a black background: every covered sample adds the same c, every other one 0, so a
    pixel's channel is n c / S (exact partial sums: n <= 4, c = 0.5) and its 8-bit value follows from alpha's n"""
    p, f = mesh_of("icosphere1")
    vw = RC.view(34, 18, lights=np.zeros((0, 4), F32), ambient=1.0, base=(0.5, 0.5, 0.5), background=(0.0, 0.0, 0.0))
    got = planes(plan_of(f, len(p), vw, samples=4), p.reshape(1, 1, -1), ("rgb", "alpha"))
    al = got["alpha"][0, 0]
    assert np.array_equal(al, RP.alpha_of(p, f, vw, 4)) and set(np.unique(al).tolist()) - {0, 255}
    n = np.select([al == a for a in (0, 64, 128, 191, 255)], [0, 1, 2, 3, 4], -1)
    want = (F32(255) * (n.astype(F32) * F32(0.5) * F32(0.25)) + F32(0.5)).astype(np.int32).astype(np.uint8)
    assert (n >= 0).all() and (got["rgb"][0, 0] == want[..., None]).all() and not got["rgb"][0, 0][al == 0].any()


def test_animate_with_alpha_and_yuv():
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    S, _ = WC.source(PIPE_MESH)
    tmpl = S.reshape(1, -1)
    wav = tiny_audio(0.2, 1)
    kw = dict(ddim_steps=2, seed=2, device=DEV)
    rv = dict(pipe_view(), samples=4, background=(0.0, 0.0, 0.0), base=(0.9, 0.45, 0.15))
    mf, lat = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, **kw)
    im, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, render=dict(rv, alpha=True, yuv="i420"), **kw)
    old, _ = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, render=rv, **kw)
    n, (W, H) = mf.frames[0], (32, 24)
    assert torch.equal(lat, lat2) and im.frames == mf.frames and old.alpha is None and old.yuv is None
    assert im.alpha.shape == (1, n, H, W) and im.alpha.dtype == torch.uint8 and im.yuv.shape == (1, n, 3 * W * H // 2) and im.yuv.dtype == torch.uint8
    assert torch.equal(im.images, old.images) and torch.equal(im.depth, old.depth) and torch.equal(im.face_ids, old.face_ids)
    plan = render.RenderPlan(faces, V, rv["camera"], samples=4, background=rv["background"], base=rv["base"], device=DEV)
    direct = plan.forward(mf.positions.reshape(1, n, 3 * V), mf.frames, normals=mf.normals, depth=True, face_ids=True, alpha=True, yuv=True)
    for a, b in zip(im, direct):
        assert (a == b) if isinstance(a, list) else torch.equal(a, b)
    nv = pipeline.to_images(mf, faces, dict(rv, yuv="nv12", yuv_range="full"))
    rgb = im.images.cpu().numpy()[0]
    assert np.array_equal(im.yuv.cpu().numpy()[0], RP.yuv_frames(rgb, RP.coeffs(709, False), "i420"))
    assert np.array_equal(nv.yuv.cpu().numpy()[0], RP.yuv_frames(rgb, RP.coeffs(709, True), "nv12")) and nv.alpha is None
    assert (im.alpha > 0).any()
    many, _ = pipeline.animate_many(diffusion, ae, [wav], [tmpl], faces=faces, out_fps=60, render=dict(rv, alpha=True, yuv="i420"), **kw)
    assert torch.equal(many[0].alpha, im.alpha) and torch.equal(many[0].yuv, im.yuv) and torch.equal(many[0].images, im.images)
