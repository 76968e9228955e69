"""MI355X: the render hand-off at 4 and 16 coverage samples per pixel (fdm_render_set "samples"; csrc/render_out.hpp,
render_raster_kernel<S> / render_resolve_kernel<S, YUV>) -- rgb, depth and face-id images equal to the numpy restatement of
tests/render_aa_cases.py on every element (the anti-aliasing paragraph), on the smallest shapes that can go
wrong: viewports whose W H is no multiple of the block and whose W is odd, sub-pixel slivers, boxes of one pixel and of the whole
view, a triangle larger than the view, face counts around the block size, chunks, ragged batches, one plan switched between sample
counts, and (the pipeline test) thousands of view-sized triangles over many frames of one chunk: atomics under load.  Outputs are filled with junk before every call (test_render_gpu.run)."""
import functools

import numpy as np
import pytest
import torch

import mesh_cases as MC
import render_aa_cases as RA
import render_cases as RC
import wrap_cases as WC
from fdm_amd import pipeline, render
from test_render_gpu import DEV, PIPE_MESH, camera_of, check, dev, pipe_view, plan_of, run, same, scene, tiny_audio, tiny_models

pytestmark = pytest.mark.gpu
F32 = np.float32
SAMPLES = [4, 16]
VIEWPORTS = [(33, 17), (64, 48)]


def static(p, faces, vw, S, plan=None):
    """one frame of vertices p through a plan of S samples (a fresh one unless given) against the restatement; returns the restatement"""
    p = np.asarray(p, F32)
    got = run(plan if plan is not None else plan_of(faces, len(p), vw, samples=S), p.reshape(1, 1, -1))
    want = RA.render_static(p, faces, vw, S)
    check(got, [tuple(a[None] for a in want)], f"S = {S}")
    return want


def aa_scene(name, vw):
    if name == "strip40":                # 40 triangles across the view: slivers narrower than a pixel at 33 x 17
        return RC.strip(40)
    if name == "icosphere1":             # 80 faces, back faces behind front faces, depth ties along shared edges
        return RC.icosphere(1, 0.3)
    if name == "larger_than_view":       # snapped vertices far left of 0 and far right of W: the clamp, the floor shift, the wavefront path
        return RC.tris([(-9, -9, -0.5), (9, -9, -0.5), (0, 9, 0.2)], [(0, 1, 2)])
    return scene(name, vw)


SCENES = ["strip40", "icosphere1", "larger_than_view", "behind_near", "one", "shared_edge", "zero_area", "off_screen", "interpenetrating",
          "coplanar_duplicates", "nan_vertex"]


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("wh", VIEWPORTS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_scene_equals_the_restatement(name, wh, S):
    vw = RC.view(*wh)
    p, f = aa_scene(name, vw)
    rgb, depth, face = static(p, f, vw, S)
    seen = set(np.unique(face)) - {-1}
    # what each scene is there for, on the restatement the device has just been held to
    if name == "strip40" and wh == (33, 17):
        centre = RC.render_static(p, f, vw)[2]
        assert ((centre < 0) & (face >= 0)).any(), "a sliver that misses the pixel centre and catches another sample"
        assert len(np.unique(rgb)) > 4      # partly covered pixels: values between the shade and the background
    if name == "icosphere1":
        assert len(seen) > 20
    if name == "larger_than_view":
        X = RC.vertex_stage(p, np.zeros_like(p), vw)[0]
        assert X.min() < 0 and X.max() > 256 * wh[0] and (face == 0).all()
    if name == "behind_near":
        assert seen == {2}
    if name == "shared_edge":
        assert (face >= 0).all() and seen == {0, 1}
    if name == "nan_vertex":
        assert seen == {0, 2}


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("F", [255, 256, 257])
def test_face_counts_around_the_block_size(F, S):
    p, f = RC.strip(F)
    face = static(p, f, RC.view(33, 17), S)[2]
    assert len(set(np.unique(face)) - {-1}) > 20 and face.max() <= F - 1


@pytest.mark.parametrize("S", SAMPLES)
def test_a_background_and_lights_of_their_own(S):
    p, f = RC.icosphere(1, 0.3)
    static(p, f, RC.view(33, 17, lights=RC.eight_lights(), background=(0.1, 0.5, 0.9), base=(0.2, 0.6, 1.5)), S)


# ---- clips, rates, templates, chunks
@functools.lru_cache(maxsize=None)
def clips_case(frames, fps, rows, S):
    """the small grid mesh in front of a 33 x 17 camera, NaN past every clip's frames; the restatement is computed once per case"""
    faces, V, xyz = MC.mesh("grid")
    frames, B, L_max = list(frames), len(frames), max(frames) + 1
    off = MC.offsets("grid", B, L_max, seed=31)
    tmpl = (MC.template("grid", seed=3, rows=rows) - np.tile(np.array([0.35, 0.15, 0.0], F32), V)).astype(F32)
    vw = RC.view(33, 17)
    want = RA.render_clips(off, tmpl, frames, fps, faces, V, vw, S)
    x = off.copy()
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return x, tmpl, frames, faces, V, vw, want


@pytest.mark.parametrize("S", SAMPLES)
def test_chunking_gives_equal_bits(S):
    x, tmpl, frames, faces, V, vw, want = clips_case((3,), None, 1, S)
    assert len(want[0][0]) == 3 and (want[0][2] >= 0).any()
    for n in (1, 2, 0):
        check(run(plan_of(faces, V, vw, chunk_frames=n, samples=S), x, frames, tmpl), want, f"chunk_frames = {n}")
    plan = plan_of(faces, V, vw, samples=S)
    for n in (2, 1, 0):                  # the same object, its scratch reused
        plan.set_chunk_frames(n)
        check(run(plan, x, frames, tmpl), want, f"set chunk_frames = {n}")


@pytest.mark.parametrize("S", SAMPLES)
def test_a_clip_alone_equals_the_clip_in_the_batch(S):
    x, tmpl, frames, faces, V, vw, want = clips_case((0, 1, 3), (30, 60), 3, S)
    plan = plan_of(faces, V, vw, samples=S)
    batch = run(plan, x, frames, tmpl, (30, 60))
    check(batch, want, "the ragged batch")
    check(run(plan, x, frames, tmpl, (30, 60), Lo=9), want, "a longer output")
    for b, L in enumerate(frames):
        if L:
            alone = run(plan, x[b:b + 1, :L], [L], tmpl[b:b + 1], (30, 60))
            check(alone, want[b:b + 1], f"clip {b} alone")
            n = alone[3][0]
            for k in range(3):
                assert np.array_equal(alone[k][0, :n].view(np.uint8), batch[k][b, :n].view(np.uint8))


def test_switching_the_sample_count_on_one_plan():
    """4, 16, 4, 1 on one object: the visibility buffer is shared, grown once, and must be all zero whenever a call starts"""
    vw = RC.view(64, 48)
    p, f = RC.icosphere(1, 0.3)
    p = (p + np.array([0.07, -0.03, 0.0], F32)).astype(F32)
    plan = plan_of(f, len(p), vw)
    h = plan.h.value
    for S in (4, 16, 4):
        plan.set_samples(S)
        static(p, f, vw, S, plan)
    plan.set_samples(1)
    last = run(plan, p.reshape(1, 1, -1))
    assert plan.h.value == h
    check(last, [tuple(a[None] for a in RC.render_static(p, f, vw))], "back at one sample")
    check(last, [tuple(a[None] for a in RA.render_static(p, f, vw, 1))], "back at one sample, the restatement of any S")
    fresh = run(plan_of(f, len(p), vw), p.reshape(1, 1, -1))
    for a, b in zip(last[:3], fresh[:3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_normals_from_the_caller():
    """to_mesh's normals handed in are the normals computed inside: the same images"""
    x, tmpl, frames, faces, V, vw, want = clips_case((0, 1, 3), (30, 60), 3, 4)
    mf = pipeline.to_mesh(dev(x), faces, dev(tmpl), frames, fps=(30, 60))
    plan = plan_of(faces, V, vw, samples=4)
    check(run(plan, x, frames, tmpl, (30, 60), Lo=mf.normals.shape[1], normals=mf.normals), want)
    im = pipeline.to_images(mf, faces, plan, depth=True, face_ids=True)
    check((im.images.cpu().numpy(), im.depth.cpu().numpy(), im.face_ids.cpu().numpy(), im.frames), want, "to_images(MeshFrames)")


# ---- the pipeline
def test_to_images_with_samples():
    x, tmpl, frames, faces, V, vw, want = clips_case((0, 1, 3), (30, 60), 3, 4)
    kw = dict(camera=camera_of(vw), lights=vw["lights"], ambient=float(vw["ambient"]), base=vw["base"], background=vw["background"])
    xs = dev(x)
    im = pipeline.to_images(xs, faces, dict(kw, samples=4, depth=True, face_ids=True), dev(tmpl), frames, (30, 60))
    direct = plan_of(faces, V, vw, samples=4).forward(xs, frames, dev(tmpl), (30, 60), None, True, True)
    assert same(im, direct)
    check((im.images.cpu().numpy(), im.depth.cpu().numpy(), im.face_ids.cpu().numpy(), im.frames), want, "to_images(samples = 4)")
    # plans of different sample counts do not alias in the plan cache
    one = pipeline.to_images(xs, faces, dict(kw, depth=True, face_ids=True), dev(tmpl), frames, (30, 60))
    again = pipeline.to_images(xs, faces, dict(kw, samples=4, depth=True, face_ids=True), dev(tmpl), frames, (30, 60))
    assert same(again, im) and not torch.equal(one.images, im.images)
    assert same(one, plan_of(faces, V, vw).forward(xs, frames, dev(tmpl), (30, 60), None, True, True))


def test_animate_with_render_samples():
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    S, _ = WC.source(PIPE_MESH)
    tmpl = S.reshape(1, -1)
    wav = tiny_audio(0.2, 1)             # (short: the restatement below visits every sample of every box of 9.7k large triangles)
    kw = dict(ddim_steps=2, seed=2, device=DEV)
    rv = dict(pipe_view(), samples=4)
    mf, lat = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, **kw)
    im, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, render=rv, **kw)
    assert torch.equal(lat, lat2) and im.images.shape == (1, mf.frames[0], 24, 32, 3) and im.images.dtype == torch.uint8
    assert same(im, pipeline.to_images(mf, faces, rv)) and (im.face_ids >= 0).float().mean() > 0.2
    assert not torch.equal(pipeline.to_images(mf, faces, pipe_view()).images, im.images)      # one sample per pixel is another picture
    # against the restatement, from the vertices and normals the device drew
    vw = RC.view(32, 24, f=24.0, c=(16.0, 12.0), far=10.0, t=(-1.75, -1.75, -4.0))
    P, N = mf.positions.cpu().numpy()[0], mf.normals.cpu().numpy()[0]
    ts = sorted({0, mf.frames[0] // 2, mf.frames[0] - 1})      # (three frames: the restatement takes a good part of a second per frame here)
    fr = [RA.render_frame(P[t], N[t], faces, vw, 4) for t in ts]
    want = [tuple(np.stack([f[k] for f in fr]) for k in range(3))]
    check((im.images[:, ts].cpu().numpy(), im.depth[:, ts].cpu().numpy(), im.face_ids[:, ts].cpu().numpy(), [len(ts)]), want, "animate(render=dict(samples=4))")
    assert mf.frames[0] >= 8             # enough frames in one chunk that workgroups of several frames run side by side
