"""MI355X: the render hand-off (include/fdm_hip.h, fdm_render_*; csrc/render_out.hpp) -- rgb, depth and face-id images equal to the
numpy restatement of tests/render_cases.py on every element (coverage is exact integer work, everything
else fixed-order fp32), chunk and batch independence, set_view, then animate / animate_many / SlotServer with render=.  Outputs are
filled with junk before every call."""
import functools

import numpy as np
import pytest
import torch

import mesh_cases as MC
import render_cases as RC
import wrap_cases as WC
from fdm_amd import pipeline, render, wrap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def camera_of(vw):
    return render.Camera(float(vw["fx"]), float(vw["fy"]), float(vw["cx"]), float(vw["cy"]), vw["W"], vw["H"], float(vw["near"]), float(vw["far"]),
                         vw["R"], vw["t"])


def plan_of(faces, V, vw, **kw):
    return render.RenderPlan(faces, V, camera_of(vw), lights=vw["lights"], ambient=float(vw["ambient"]), base=vw["base"],
                             background=vw["background"], device=DEV, **kw)


def run(plan, x, frames=None, tmpl=None, fps=None, Lo=None, normals=None):
    """(rgb, depth, face) numpy of one forward into junk-filled outputs of L_out_max = Lo (None: the longest clip's)"""
    x = dev(x)
    B = x.shape[0]
    if Lo is None:
        Lo = max([MC.frames_out(L, fps) for L in (frames if frames is not None else [x.shape[1]] * B)] + [1])
    out = (torch.full((B, Lo, plan.H, plan.W, 3), 0x5A, dtype=torch.uint8, device=DEV),
           torch.full((B, Lo, plan.H, plan.W), float("nan"), device=DEV), torch.full((B, Lo, plan.H, plan.W), 12345, dtype=torch.int32, device=DEV))
    got = plan.forward(x, frames, None if tmpl is None else dev(tmpl), fps, normals, True, True, out=out)
    assert got.images is out[0] and got.depth is out[1] and got.face_ids is out[2]
    return got.images.cpu().numpy(), got.depth.cpu().numpy(), got.face_ids.cpu().numpy(), got.frames


def check(got, want, what=""):
    """got: (rgb, depth, face, frames) of the batch; want: render_clips' list.  Every element; padding rows exactly zero."""
    rgb, dep, face, frames = got
    assert frames == [len(w[0]) for w in want], what
    for b, (wr, wd, wf) in enumerate(want):
        n = len(wr)
        assert np.array_equal(face[b, :n], wf), f"{what} clip {b}: face ids differ at {int((face[b, :n] != wf).sum())} pixels"
        assert np.array_equal(dep[b, :n].view(np.uint32), wd.view(np.uint32)), f"{what} clip {b}: depth bits differ at {int((dep[b, :n].view(np.uint32) != wd.view(np.uint32)).sum())} pixels"
        assert np.array_equal(rgb[b, :n], wr), f"{what} clip {b}: rgb differs at {int((rgb[b, :n] != wr).any(-1).sum())} pixels"
        assert not rgb[b, n:].any() and not dep[b, n:].view(np.uint32).any() and not face[b, n:].any(), f"{what} padding of clip {b}"


def static(p, faces, vw, **kw):
    """one frame of vertices p through a fresh plan against the restatement; returns the face image"""
    p = np.asarray(p, F32)
    got = run(plan_of(faces, len(p), vw, **kw), p.reshape(1, 1, -1))
    want = RC.render_static(p, faces, vw)
    check(got, [tuple(a[None] for a in want)])
    return want[2]


# ---- viewports and meshes
VIEWPORTS = [(1, 1), (37, 29), (64, 64)]


def scene(name, vw):
    """named small scenes in front of view()'s camera (world z = 0 is at distance 1)"""
    W, H = vw["W"], vw["H"]
    px = lambda x, y, d=1.0: RC.pixel_to_world(vw, x, y, d)  # noqa: E731
    if name == "one":
        return RC.tris([(-0.3, -0.25, 0.0), (0.35, -0.1, 0.1), (0.0, 0.4, -0.2)], [(0, 1, 2)])
    if name == "shared_edge":            # whole-pixel corners: the diagonal runs through pixel centres
        return RC.tris([px(0, 0), px(W, 0), px(W, H), px(0, H)], [(0, 2, 1), (0, 3, 2)])
    if name == "zero_area":
        return RC.tris([(-0.3, -0.3, 0), (0.3, 0.3, 0), (0.0, 0.0, 0), (0.2, -0.3, 0), (0.3, 0.2, 0.1)], [(0, 1, 2), (0, 0, 1), (0, 3, 4)])
    if name == "behind_near":            # z = 0.995: d = 0.005 <= near; and one that straddles it (vanishes whole)
        return RC.tris([(-0.001, 0, 0.995), (0.001, 0, 0.995), (0, 0.001, 0.995), (-0.2, -0.2, 0), (0.2, -0.2, 0), (0, 0.0, 0.999), (-0.3, 0.1, 0), (0.3, 0.1, 0), (0, 0.4, 0)],
                       [(0, 1, 2), (3, 4, 5), (6, 7, 8)])
    if name == "beyond_far":
        return RC.tris([(-0.9, -0.9, -2.5), (0.9, -0.9, -2.5), (0, 0.9, -2.5), (-0.3, -0.3, -1.9), (0.3, -0.3, -1.9), (0, 0.3, -1.9)], [(0, 1, 2), (3, 4, 5)])
    if name == "off_screen":             # one partly, one wholly outside, one far outside (|X| > 2^20: bad)
        return RC.tris([(-1.5, -0.2, 0), (0.1, -0.3, 0), (-0.2, 1.4, 0), (3, 3, 0), (4, 3, 0), (3, 4, 0), (0, 0, 0), (1e5, 0, 0), (0, 1e5, 0)],
                       [(0, 1, 2), (3, 4, 5), (6, 7, 8)])
    if name == "whole_viewport":
        return RC.tris([(-9, -9, -0.5), (9, -9, -0.5), (0, 9, 0.2)], [(0, 1, 2)])
    if name == "interpenetrating":
        return RC.tris([(-0.4, -0.3, -0.3), (0.4, -0.3, 0.3), (0.0, 0.4, 0.0), (-0.4, -0.2, 0.3), (0.4, -0.2, -0.3), (0.0, 0.35, 0.05)], [(0, 1, 2), (3, 4, 5)])
    if name == "coplanar_duplicates":
        return RC.tris([(-0.3, -0.3, 0.1), (0.3, -0.3, 0.0), (0, 0.3, -0.1)], [(0, 1, 2), (0, 1, 2), (0, 2, 1)])       # the mirrored one is oriented into the same triangle: equal iw bits
    if name == "nan_vertex":
        p, f = RC.tris([(-0.3, -0.3, 0), (0.3, -0.3, 0), (0, 0.3, 0), (0.1, 0.1, np.nan), (-0.4, 0.3, 0.1), (0.4, 0.3, 0.1), (np.inf, 0, 0)],
                       [(0, 1, 2), (0, 1, 3), (2, 4, 5), (4, 5, 6)])
        return p, f
    if name == "icosphere":
        return RC.icosphere(2, 0.3)
    raise KeyError(name)


SCENES = ["one", "shared_edge", "zero_area", "behind_near", "beyond_far", "off_screen", "whole_viewport", "interpenetrating", "coplanar_duplicates",
          "nan_vertex", "icosphere"]


@pytest.mark.parametrize("wh", VIEWPORTS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_scene_equals_the_restatement(name, wh):
    vw = RC.view(*wh)
    p, f = scene(name, vw)
    face = static(p, f, vw)
    seen = set(np.unique(face)) - {-1}
    if wh == (64, 64):                   # what each scene is there for, on the restatement the device has just been held to
        if name == "shared_edge":
            assert (face >= 0).all() and seen == {0, 1}
        if name == "zero_area":
            assert seen == {2}          # faces 0 (collinear) and 1 (a repeated vertex) have no area
        if name == "behind_near":
            assert seen == {2}
        if name == "beyond_far":
            assert seen == {1}
        if name == "off_screen":
            assert seen == {0} and (face[:, 0] >= 0).any()
        if name == "whole_viewport":
            assert (face == 0).all()
        if name == "interpenetrating":
            assert seen == {0, 1}
        if name == "coplanar_duplicates":
            assert seen == {0}
        if name == "nan_vertex":
            assert seen == {0, 2}
        if name == "icosphere":
            assert len(seen) > 100


@pytest.mark.parametrize("F", [1, 255, 256, 257, 513])
def test_face_counts_around_the_block_size(F):
    p, f = RC.strip(F)
    face = static(p, f, RC.view(64, 64))
    assert len(set(np.unique(face)) - {-1}) > min(F, 40) // 2 and face.max() <= F - 1


def test_icosphere_back_faces_are_lit_like_front_faces():
    """seen from outside every pixel shows a front face; with the faces' winding reversed the vertex normals point inwards and the flip
    rule gives the same picture"""
    vw = RC.view(64, 64)
    p, f = RC.icosphere(2, 0.3)
    a = RC.render_static(p, f, vw)
    static(p, f, vw)
    b = RC.render_static(p, f[:, ::-1].copy(), vw)
    static(p, f[:, ::-1].copy(), vw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


LIGHTS = {"none": np.zeros((0, 4), F32), "one": [(0, 0, 1, 0.7)], "default": "default", "eight": RC.eight_lights()}


@pytest.mark.parametrize("lights", list(LIGHTS))
def test_lights(lights):
    p, f = RC.icosphere(2, 0.3)
    static(p, f, RC.view(64, 64, lights=LIGHTS[lights], background=(0.1, 0.5, 0.9)))


def test_a_base_colour_that_saturates():
    p, f = RC.icosphere(2, 0.3)
    vw = RC.view(64, 64, base=(0.2, 0.6, 1.5))
    static(p, f, vw)
    rgb, _, face = RC.render_static(p, f, vw)
    assert (rgb[face >= 0][:, 2] == 255).all() and (rgb[face >= 0][:, 0] < 255).all()


def test_800_by_800_grid_head():
    off, tmpl, faces, vw, want = RC.head_case()
    plan = plan_of(faces, tmpl.shape[1] // 3, vw)
    check(run(plan, off, [2], tmpl), want, "default chunk")
    assert (want[0][2] >= 0).mean() > 0.1 and len(np.unique(want[0][2])) > 5000


# ---- clips, rates, templates, chunks
@functools.lru_cache(maxsize=None)
def clips_case(fps, rows):
    """B = 3, frames = [0, 1, 5], L_max = 7 with NaN past every clip's frames, the small grid mesh in front of a 37 x 29 camera"""
    faces, V, xyz = MC.mesh("grid")
    frames, B, L_max = [0, 1, 5], 3, 7
    off = MC.offsets("grid", B, L_max, seed=31)
    tmpl = None
    if rows:
        tmpl = (MC.template("grid", seed=3, rows=rows) - np.tile(np.array([0.35, 0.15, 0.0], F32), V)).astype(F32)
    else:
        off = (off + (xyz.reshape(1, 1, -1) - np.tile([0.35, 0.15, 0.0], V))).astype(F32)
    vw = RC.view(37, 29)
    want = RC.render_clips(off, tmpl, frames, fps, faces, V, vw)
    x = off.copy()
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return x, tmpl, frames, faces, V, vw, want


@pytest.mark.parametrize("fps", [None, (30, 60), (30, 25), (30, 30)], ids=str)
@pytest.mark.parametrize("rows", [0, 1, 3])
def test_ragged_clips_rates_and_templates(fps, rows):
    x, tmpl, frames, faces, V, vw, want = clips_case(fps, rows)
    plan = plan_of(faces, V, vw)
    check(run(plan, x, frames, tmpl, fps), want)
    check(run(plan, x, frames, tmpl, fps, Lo=13), want, "a longer output")
    assert (want[2][2] >= 0).any()


def test_chunking_gives_equal_bits():
    x, tmpl, frames, faces, V, vw, want = clips_case((30, 60), 3)
    for n in (1, 2, 0):
        check(run(plan_of(faces, V, vw, chunk_frames=n), x, frames, tmpl, (30, 60)), want, f"chunk_frames = {n}")
    plan = plan_of(faces, V, vw)
    for n in (4, 1, 0):                  # the same object, its scratch reused
        plan.set_chunk_frames(n)
        check(run(plan, x, frames, tmpl, (30, 60)), want, f"set chunk_frames = {n}")


def test_a_clip_alone_equals_the_clip_in_the_batch():
    x, tmpl, frames, faces, V, vw, want = clips_case((30, 25), 3)
    plan = plan_of(faces, V, vw)
    for b, L in enumerate(frames):
        if L:
            check(run(plan, x[b:b + 1, :L], [L], tmpl[b:b + 1], (30, 25)), want[b:b + 1], f"clip {b} alone")


def test_normals_from_the_caller():
    """to_mesh's normals handed in are the normals computed inside: the same images"""
    x, tmpl, frames, faces, V, vw, want = clips_case((30, 60), 1)
    mf = pipeline.to_mesh(dev(x), faces, dev(tmpl), frames, fps=(30, 60))
    plan = plan_of(faces, V, vw)
    check(run(plan, x, frames, tmpl, (30, 60), Lo=mf.normals.shape[1], normals=mf.normals), want)
    im = pipeline.to_images(mf, faces, plan, depth=True, face_ids=True)
    check((im.images.cpu().numpy(), im.depth.cpu().numpy(), im.face_ids.cpu().numpy(), im.frames), want, "to_images(MeshFrames)")


def test_set_view_changes_the_picture_without_a_new_create():
    p, f = RC.icosphere(2, 0.3)
    p = (p + np.array([0.1, 0.0, 0.0], F32)).astype(F32)
    vw = RC.view(64, 64)
    plan = plan_of(f, len(p), vw)
    h = plan.h.value
    check(run(plan, p.reshape(1, 1, -1)), [tuple(a[None] for a in RC.render_static(p, f, vw))])
    R = RC.rot_y(0.6)
    vw2 = RC.view(64, 64, f=40.0, R=R, t=(0.05, -0.02, -1.2), lights=[(0.6, 0.0, 0.8, 0.9)], ambient=0.1)
    plan.set_view(camera_of(vw2), vw2["lights"], float(vw2["ambient"]))
    assert plan.h.value == h
    a, b = RC.render_static(p, f, vw), RC.render_static(p, f, vw2)
    assert not np.array_equal(a[2], b[2])
    check(run(plan, p.reshape(1, 1, -1)), [tuple(x[None] for x in b)], "after set_view")


# ---- the pipeline
PIPE_MESH = "vocaset_size"


@functools.lru_cache(maxsize=None)
def tiny_models():
    """As tests/test_mesh_out_gpu.py: the pipeline decodes on the full VOCASET geometry only; short audio and 2-3 DDIM steps."""
    return pipeline.build_models("vocaset", None, DEV)


def tiny_audio(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(int(16000 * seconds), generator=g)).numpy()


def pipe_view():
    """a 32 x 24 camera that sees the 3.5 x 3.5 grid of mesh_cases from 4 units (small: the random-weight decoder's offsets make
    every triangle span much of the view, and the restatement visits every pixel of every box)"""
    return dict(camera=render.Camera(24.0, 24.0, 16.0, 12.0, 32, 24, 0.01, 10.0, None, (-1.75, -1.75, -4.0)), depth=True, face_ids=True)


def same(a, b):
    return a.frames == b.frames and torch.equal(a.images, b.images) and torch.equal(a.depth, b.depth) and torch.equal(a.face_ids, b.face_ids)


def test_animate_with_render():
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    S, _ = WC.source(PIPE_MESH)
    tmpl = S.reshape(1, -1)
    wav = tiny_audio(0.3, 1)
    kw = dict(ddim_steps=3, seed=2, device=DEV)
    rv = pipe_view()
    mf, lat = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, **kw)
    im, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, render=rv, **kw)
    assert torch.equal(lat, lat2) and im.images.shape == (1, mf.frames[0], 24, 32, 3) and im.images.dtype == torch.uint8
    assert same(im, pipeline.to_images(mf, faces, rv)) and (im.face_ids >= 0).float().mean() > 0.2
    # against the restatement, from the offsets
    offs, _ = pipeline.animate(diffusion, ae, wav, None, **kw)
    vw = RC.view(32, 24, f=24.0, c=(16.0, 12.0), far=10.0, t=(-1.75, -1.75, -4.0))
    want = RC.render_clips(offs.cpu().numpy(), tmpl, [offs.shape[1]], (30, 60), faces, V, vw)
    check((im.images.cpu().numpy(), im.depth.cpu().numpy(), im.face_ids.cpu().numpy(), im.frames), want, "animate(render=)")
    # a plan in place of the dict; with rig= the pair; animate_long on one window
    plan = render.RenderPlan(faces, V, rv["camera"], device=DEV)
    assert torch.equal(pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, render=plan, **kw)[0].images, im.images)
    E = (1e-2 * np.random.default_rng(3).standard_normal((4, 3 * V))).astype(F32)
    (im_r, rf), _ = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, render=rv, rig=dict(basis=E, ridge=1e-3), **kw)
    assert same(im_r, im) and rf.weights.shape[:2] == (1, mf.frames[0])
    assert same(pipeline.animate_long(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, render=rv, **kw)[0], im)
    # render=None: today's output
    a, _ = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, render=None, **kw)
    assert torch.equal(a.positions, mf.positions) and torch.equal(a.normals, mf.normals)
    b, _ = pipeline.animate(diffusion, ae, wav, tmpl, render=None, **kw)
    assert torch.equal(b, offs + dev(tmpl).unsqueeze(1))
    with pytest.raises(ValueError, match="render= needs faces="):
        pipeline.animate(diffusion, ae, wav, tmpl, render=rv, **kw)


def test_animate_with_wrap_and_render():
    diffusion, ae = tiny_models()
    S, faces_s, T = WC.case(PIPE_MESH, "lifted", 257)
    plan = wrap.WrapPlan(S, faces_s, T, device=DEV)
    faces_t = np.array([(k, k + 1, k + 2) for k in range(255)], dtype=np.int32)
    tmpl, wav, kw, rv = S.reshape(1, -1), tiny_audio(0.5, 4), dict(ddim_steps=2, seed=3, device=DEV), pipe_view()
    mf, _ = pipeline.animate(diffusion, ae, wav, tmpl, wrap=plan, faces=faces_t, **kw)
    im, _ = pipeline.animate(diffusion, ae, wav, tmpl, wrap=plan, faces=faces_t, render=rv, **kw)
    assert same(im, pipeline.to_images(mf, faces_t, rv)) and (im.face_ids >= 0).any()


@pytest.mark.parametrize("batch_stages", [False, True])
def test_animate_many_and_slot_server_with_render(batch_stages):
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    S, _ = WC.source(PIPE_MESH)
    wavs = [tiny_audio(s, i) for i, s in enumerate((0.6, 0.4))]
    tmpls = [S.reshape(1, -1), MC.template(PIPE_MESH, seed=21)]
    kw, rv = dict(ddim_steps=2, seed=1, device=DEV), pipe_view()
    got, lats = pipeline.animate_many(diffusion, ae, wavs, tmpls, batch_stages=batch_stages, faces=faces, render=rv, **kw)
    plain, lats0 = pipeline.animate_many(diffusion, ae, wavs, tmpls, batch_stages=batch_stages, faces=faces, **kw)
    plain_none, _ = pipeline.animate_many(diffusion, ae, wavs, tmpls, batch_stages=batch_stages, faces=faces, render=None, **kw)
    solo = [pipeline.animate(diffusion, ae, wavs[b], tmpls[b], faces=faces, render=rv, **kw)[0] for b in range(2)]
    assert got[0].images.shape[1] != got[1].images.shape[1]
    for b in range(2):
        assert torch.equal(lats[b], lats0[b]) and torch.equal(plain[b].positions, plain_none[b].positions)
        assert same(got[b], solo[b]) and same(got[b], pipeline.to_images(plain[b], faces, rv))
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, batch_stages=batch_stages, faces=faces, render=rv)
    hs = srv.submit_many(wavs, tmpls, seeds=1)
    res = {h: v for h, v, _ in srv.drain(2)}
    for b, h in enumerate(hs):
        assert same(res[h], solo[b])
