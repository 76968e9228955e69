"""The numpy restatement of the render hand-off (tests/render_cases.py) against things that can be derived
by hand, and the host-side refusals of fdm_render_create / _set_view / _set / _forward (no device needed: the object validates without
one and forward ends in FDM_ERR_STATE)."""
import ctypes as C

import numpy as np
import pytest

import render_cases as RC
from fdm_amd import render
from fdm_amd._lib import FdmError, lib

F32 = np.float32


def flat_view(W, H, **kw):
    """f = 256 at distance 1 with the principal point on a pixel corner: world (x / 256, y / 256) lands on whole sub-pixel counts"""
    return RC.view(W, H, f=256.0, c=(W / 2.0, H / 2.0), **kw)


def rect(vw, x0, y0, x1, y1, d):
    """two triangles over the pixel rectangle [x0, x1] x [y0, y1] at distance d, facing the camera"""
    pts = [RC.pixel_to_world(vw, x, y, d) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    return RC.tris(pts, [(0, 2, 1), (0, 3, 2)])


def test_a_rectangle_on_whole_pixels_covers_w_times_h_at_its_depth():
    vw = flat_view(32, 24)
    for (x0, y0, w, h, d) in ((4, 6, 8, 4, 2.0), (0, 0, 32, 24, 1.0), (0, 0, 32, 16, 1.0), (30, 20, 2, 4, 0.5), (7, 3, 16, 16, 1.0), (5, 5, 3, 7, 1.5)):
        p, f = rect(vw, x0, y0, x0 + w, y0 + h, d)
        X, Y, _, bad, _ = RC.vertex_stage(p, np.zeros_like(p), vw)
        assert not bad.any() and (X % 256 == 0).all() and (Y % 256 == 0).all()       # whole pixels after the snap
        rgb, depth, face = RC.render_static(p, f, vw)
        inside = np.zeros((24, 32), bool)
        inside[y0:y0 + h, x0:x0 + w] = True
        assert np.array_equal(face >= 0, inside) and int((face >= 0).sum()) == w * h
        if (w * h) & (w * h - 1) == 0:       # A = 2^16 w h is a power of two: every l_i is exact, they sum to 1 and iw = 1 / d exactly
            assert np.array_equal(depth, np.where(inside, F32(d), F32(0)))
        else:                                # three rounded l_i, three products, two sums, one division: a few ulp of d
            assert (depth[~inside] == 0).all() and np.abs(depth[inside] - F32(d)).max() <= 4 * np.spacing(F32(d))
        assert set(np.unique(face)) <= {-1, 0, 1} and (rgb[~inside] == 255).all()


def covering_counts(p, f, vw):
    """per pixel, how many triangles of the list cover it (each rendered alone)"""
    n = np.zeros((vw["H"], vw["W"]), int)
    for k in range(len(f)):
        n += RC.render_static(p, f[k:k + 1], vw)[2] >= 0
    return n


QUADS = [  # snapped corners a, b, c, d in sub-pixel units of a convex quad cut along a - c
    ((0, 0), (2048, 0), (2048, 2048), (0, 2048)),                  # the diagonal of a square runs through 8 pixel centres
    ((2048, 0), (2048, 2048), (0, 2048), (0, 0)),                  # the other diagonal
    ((128, 384), (2176, 384), (3200, 384 + 1024), (128, 1408)),    # a - c of slope 1/3 from a pixel centre
    ((384, 128), (384, 2000), (1152, 3200), (1408, 1664)),      # a - c of slope 4 from a pixel centre, through two more
    ((0, 128 + 512), (1024, 128), (2048, 128 + 512), (1024, 128 + 1024)),  # a horizontal cut along a row of centres
    ((128 + 768, 0), (128 + 1536, 1024), (128 + 768, 2048), (128, 1024)),  # a vertical cut along a column of centres
]


@pytest.mark.parametrize("quad", QUADS, ids=[str(i) for i in range(len(QUADS))])
def test_two_triangles_sharing_an_edge_cover_their_union_once(quad):
    vw = flat_view(16, 16)
    pts = [RC.pixel_to_world(vw, x / 256.0, y / 256.0, 1.0) for x, y in quad]
    for faces in ([(0, 1, 2), (0, 2, 3)], [(0, 2, 1), (0, 2, 3)], [(2, 0, 1), (3, 0, 2)]):      # every winding and starting corner
        p, f = RC.tris(pts, faces)
        X, Y, _, _, _ = RC.vertex_stage(p, np.zeros_like(p), vw)
        assert [(int(a), int(b)) for a, b in zip(X, Y)] == list(quad)
        n = covering_counts(p, f, vw)
        # the union by exact integer work of its own: strictly inside the convex quad (either orientation)
        ys, xs = np.mgrid[0:16, 0:16]
        px, py = 256 * xs + 128, 256 * ys + 128
        side = [(quad[(i + 1) % 4][0] - quad[i][0]) * (py - quad[i][1]) - (quad[(i + 1) % 4][1] - quad[i][1]) * (px - quad[i][0]) for i in range(4)]
        strictly_in = np.all([s > 0 for s in side], axis=0) | np.all([s < 0 for s in side], axis=0)
        strictly_out = np.any([s > 0 for s in side], axis=0) & np.any([s < 0 for s in side], axis=0)
        on_cut = ((quad[2][0] - quad[0][0]) * (py - quad[0][1]) - (quad[2][1] - quad[0][1]) * (px - quad[0][0]) == 0) & strictly_in
        assert on_cut.sum() >= 2, "the shared edge must pass through pixel centres"
        assert n.max() == 1 and (n[strictly_in] == 1).all() and (n[strictly_out] == 0).all()
        both = RC.render_static(p, f, vw)[2]
        assert np.array_equal(both >= 0, n == 1)


def test_a_triangle_and_its_mirror_cover_the_same_pixels():
    vw = RC.view(37, 29)
    g = np.random.default_rng(5)
    for _ in range(20):
        p = (g.uniform(-0.5, 0.5, (3, 3)) * [1, 1, 0.2]).astype(F32)
        a = RC.render_static(p, np.array([[0, 1, 2]], np.int32), vw)
        b = RC.render_static(p, np.array([[0, 2, 1]], np.int32), vw)
        assert (a[2] >= 0).any()
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))              # coverage, depth bits and shade (the normal is flipped back)
    # exactly on a grid too: a triangle whose edges run through pixel centres
    vw = flat_view(16, 16)
    pts = [RC.pixel_to_world(vw, x, y, 1.0) for x, y in ((1.5, 1.5), (9.5, 1.5), (1.5, 9.5))]
    a = RC.render_static(*RC.tris(pts, [(0, 1, 2)]), vw)[2] >= 0
    b = RC.render_static(*RC.tris(pts, [(0, 2, 1)]), vw)[2] >= 0
    assert np.array_equal(a, b) and a[1, 1] and a[1, 8] and not a[1, 9] and not a[9, 1]      # top and left edges in, the others out


@pytest.mark.parametrize("ambient,I,base", [(0.2, 0.5, 0.3), (0.0, 1.0, 0.5), (0.2, 2.0, 0.3), (0.25, 0.125, 1.0), (0.2, 3.0, 0.9)])
def test_a_facing_normal_under_one_head_on_light(ambient, I, base):
    vw = flat_view(8, 8, lights=[(0, 0, 1, I)], ambient=ambient, base=(base, base, base), background=(0, 0, 0))
    p, f = rect(vw, 2, 2, 6, 6, 1.0)
    rgb, _, face = RC.render_static(p, f, vw)
    want = int(F32(255) * min(F32(1), F32(base) * (F32(ambient) + F32(I))) + F32(0.5))
    assert (rgb[face >= 0] == want).all() and (rgb[face < 0] == 0).all() and (face >= 0).sum() == 16
    if base * (ambient + I) > 1:
        assert want == 255


def test_the_default_lights_do_not_saturate_a_facing_normal():
    lt = render.reference_lights()
    assert np.array_equal(lt["lights"], RC.reference_lights(render.LIGHT_INTENSITY)) and lt["ambient"] == 0.2
    k = RC.shade(np.array([[0, 0, 1]], F32), RC.view(4, 4))
    assert abs(float(k[0]) - (0.2 + 0.5 * (1 + 4 * np.cos(np.pi / 6)))) < 1e-5 and 0.3 * float(k[0]) < 1.0
    assert np.allclose(np.linalg.norm(lt["lights"][:, :3], axis=1), 1.0, atol=1e-6)


def test_camera_presets_and_resize():
    v, b, m = (render.Camera.preset(n) for n in ("vocaset", "biwi", "mead"))
    assert (v.fx, v.cx, v.width, v.height, v.near, v.far) == (4754.97941935 / 2, 400.0, 800, 800, 0.01, 3.0) and b.fy == 4754.97941935 / 8 and m.fx == v.fx
    assert np.array_equal(v.t, [0, 0, -1]) and np.array_equal(v.R, np.eye(3))
    h = v.resized(200, 100)
    assert (h.fx, h.fy, h.cx, h.cy, h.width, h.height) == (v.fx / 4, v.fy / 8, 100.0, 50.0, 200, 100)
    with pytest.raises(ValueError):
        render.Camera.preset("other")


# ---- the host side: refusals with a message, before any device work
ARG, SHAPE, STATE = -1, -2, -4      # include/fdm_hip.h FDM_ERR_*
FACES = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def make(**kw):
    a = dict(faces=FACES, V=4, camera=render.Camera(64, 64, 16, 16, 32, 32))
    a.update(kw)
    return render.RenderPlan(device="cuda:0", **a)


def cam(**kw):
    a = dict(fx=64, fy=64, cx=16, cy=16, width=32, height=32)
    a.update(kw)
    return render.Camera(**a)


@pytest.mark.parametrize("kw,msg", [
    (dict(camera=cam(width=0)), "viewport"), (dict(camera=cam(height=4097)), "viewport"), (dict(camera=cam(width=4097)), "viewport"),
    (dict(lights=np.tile(np.array([0, 0, 1, 0.1], F32), (9, 1))), "9 lights"),
    (dict(lights=[(0, 0, 1.1, 1.0)]), "unit vector"), (dict(lights=[(0, 0, 0, 1.0)]), "unit vector"),
    (dict(lights=[(0, 0, 1, -1.0)]), "light 0"), (dict(lights=[(0, np.nan, 1, 1.0)]), "light 0"),
    (dict(camera=cam(near=3.0, far=3.0)), "near"), (dict(camera=cam(near=4.0)), "near"), (dict(camera=cam(near=0.0)), "near"),
    (dict(camera=cam(fx=0)), "focal"), (dict(camera=cam(t=(0, np.inf, 0))), "non-finite"),
    (dict(faces=np.array([[0, 1, 4]], np.int32)), "names vertex 4 of 4"), (dict(faces=np.array([[0, -1, 2]], np.int32)), "names vertex -1"),
    (dict(faces=np.zeros((0, 3), np.int32)), "F = 0"), (dict(V=0), "V = 0"),
    (dict(ambient=-0.1), "ambient"), (dict(base=(0.3, -1, 0.3)), "base"), (dict(background=(0, 0, 1.5)), "background"),
])
def test_create_refuses(kw, msg):
    with pytest.raises(FdmError, match=msg) as e:
        make(**kw)
    assert e.value.code == ARG


def test_set_view_set_and_forward_refuse():
    plan = make()
    L = lib()
    good = plan.view["camera"]
    with pytest.raises(FdmError, match="near"):
        plan.set_view(camera=cam(near=1.0, far=0.5))
    with pytest.raises(FdmError, match="unit vector"):
        plan.set_view(lights=[(1, 1, 1, 1.0)])
    with pytest.raises(FdmError, match="lights"):
        plan.set_view(lights=np.tile(np.array([0, 0, 1, 0.1], F32), (9, 1)))
    with pytest.raises(FdmError, match="image size"):
        plan.set_view(camera=cam(width=16))
    assert plan.view["camera"] is good                                    # a refused view changes nothing
    plan.set_view(camera=cam(t=(0, 0, -2)), lights=[], ambient=1.0)       # no lights is a view
    assert L.fdm_render_set_view(None, None, None, None, None, 0, 0.0) == ARG and b"null" in L.fdm_last_error()
    assert L.fdm_render_set_view(plan.h, None, None, None, None, 0, 0.0) == ARG
    assert L.fdm_render_set(plan.h, b"chunk", 1) == ARG and b"unknown key" in L.fdm_last_error()
    assert L.fdm_render_set(plan.h, b"chunk_frames", -1) == ARG and L.fdm_render_set(plan.h, b"chunk_frames", 4097) == ARG
    assert L.fdm_render_set(plan.h, None, 1) == ARG and L.fdm_render_set(None, b"chunk_frames", 1) == ARG
    plan.set_chunk_frames(3)
    # forward: never a launch (the pointers are not dereferenced), every refusal a code and a message
    x, y, fr, bad = C.c_void_p(0x1000), C.c_void_p(0x2000), (C.c_int * 2)(3, 0), (C.c_int * 2)(3, 4)
    fw = lambda *a: L.fdm_render_forward(*a)  # noqa: E731
    assert fw(None, x, fr, 2, 3, None, 0, 0.0, 0.0, None, y, None, None, 3, None, None) == ARG
    assert fw(plan.h, None, fr, 2, 3, None, 0, 0.0, 0.0, None, y, None, None, 3, None, None) == ARG
    assert fw(plan.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, None, None, None, 3, None, None) == ARG
    assert fw(plan.h, x, fr, 2, 3, x, 3, 0.0, 0.0, None, y, None, None, 3, None, None) == ARG and b"tmpl_rows" in L.fdm_last_error()
    assert fw(plan.h, x, fr, 2, 3, None, 1, 0.0, 0.0, None, y, None, None, 3, None, None) == ARG
    assert fw(plan.h, x, fr, 2, 3, None, 0, -1.0, 30.0, None, y, None, None, 3, None, None) == ARG and b"frame rates" in L.fdm_last_error()
    assert fw(plan.h, x, fr, 0, 3, None, 0, 0.0, 0.0, None, y, None, None, 3, None, None) == SHAPE
    assert fw(plan.h, x, fr, 2, 0, None, 0, 0.0, 0.0, None, y, None, None, 3, None, None) == SHAPE
    assert fw(plan.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, y, None, None, 0, None, None) == SHAPE
    assert fw(plan.h, x, bad, 2, 3, None, 0, 0.0, 0.0, None, y, None, None, 3, None, None) == SHAPE and b"clip 1 has 4 frames" in L.fdm_last_error()
    assert fw(plan.h, x, fr, 2, 3, None, 0, 30.0, 60.0, None, y, None, None, 5, None, None) == SHAPE and b"gives 6 frames" in L.fdm_last_error()
    import torch
    if not torch.cuda.is_available():
        assert fw(plan.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, y, None, None, 3, None, None) == STATE and b"no gfx950 device" in L.fdm_last_error()
