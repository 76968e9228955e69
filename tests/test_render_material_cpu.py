"""No GPU: the materials of the render hand-off -- the restatement of tests/render_material_cases.py pinned
to the one of tests/render_aa_cases.py where the two must agree, the colour tables, uv_corners, the refusals of
fdm_render_set_material through ctypes on an object without a device, and the ValueErrors of the Python side."""
import ctypes as C

import numpy as np
import pytest

import render_aa_cases as RA
import render_cases as RC
import render_material_cases as RM
from fdm_amd import _lib, pipeline, render
from fdm_amd._lib import FdmError, RenderMaterial, lib

F32 = np.float32
SAMPLES = [1, 4, 16]
COLOUR = (0.8, 0.4, 0.2)             # 204, 102 and 51 of 255: 204 / 255 and its kin as the texel division rounds them


def sphere():
    p, f = RC.icosphere(1, 0.3)
    return p, f, RC.view(34, 18, base=COLOUR, background=(0.1, 0.5, 0.9))


def corner_uv(F, seed=5):
    return np.random.default_rng(seed).uniform(-0.5, 1.5, (F, 3, 2)).astype(F32)


@pytest.mark.parametrize("S", SAMPLES)
def test_one_colour_texture_and_flat_table_equal_the_base_render_bit_for_bit(S):
    """t + f (t - t) is exact, so a single-colour texture or an all-equal table gives m = that colour on every fragment, and the new
    text equals the old yardstick with base set to it"""
    p, f, vw = sphere()
    tex8 = np.array([204, 102, 51], np.uint8)
    col = tex8.astype(F32) / F32(255)
    want = RA.render_static(p, f, dict(vw, base=col), S)
    for shape in ((1, 1), (5, 3)):
        for flt in ("nearest", "bilinear"):
            got = RM.render_static(p, f, vw, S, RM.texture(np.broadcast_to(tex8, shape + (3,)), corner_uv(len(f)), flt))
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got[:3], want)), (shape, flt)
    s = np.random.default_rng(3).uniform(-1, 2, len(p)).astype(F32)
    for N in (2, 7):
        got = RM.render_static(p, f, vw, S, RM.scalar_map(np.broadcast_to(col, (N, 3)), 0.0, 1.0), s)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got[:3], want)), N
    got = RM.render_static(p, f, vw, S, RM.base())
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got[:3], RA.render_static(p, f, vw, S)))
    assert (want[2] >= 0).any()


@pytest.mark.parametrize("S", SAMPLES)
def test_vertex_colours_all_equal_to_base_are_within_one_unit(S):
    """(b0 c + b1 c) + b2 c is c up to the rounding of the weights, which do not sum to exactly 1: within one unit of the last uint8
    place.  The count of bytes that differ is printed: on this scene it is 0 of 1836 at S = 1, 4 and 16 (the rounding of the weights
    does not cross a half in any byte)"""
    p, f, vw = sphere()
    want = RA.render_static(p, f, vw, S)[0].astype(np.int32)
    got = RM.render_static(p, f, vw, S, RM.vertex_colors(np.broadcast_to(np.asarray(COLOUR, F32), (len(p), 3))))[0].astype(np.int32)
    differ = int((got != want).sum())
    print(f"S = {S}: {differ} of {want.size} bytes differ")
    assert np.abs(got - want).max() <= 1


def test_unlit_is_the_material_colour_itself():
    p, f, vw = sphere()
    rgb, _, face, _ = RM.render_static(p, f, vw, 1, RM.base(unlit=True))
    assert (rgb[face >= 0] == RC.to_u8(np.asarray(COLOUR, F32), vw["background"])).all()


def test_colormaps():
    for name, (pts, monotone) in render.COLORMAPS.items():
        for n in (2, 5, 256, 1024):
            t = render.colormap(name, n)
            assert t.dtype == F32 and t.shape == (n, 3) and np.isfinite(t).all() and (t >= 0).all() and (t <= 1).all()
            assert np.array_equal(t[0], np.asarray(pts[0][1], F32)) and np.array_equal(t[-1], np.asarray(pts[-1][1], F32)), (name, n)
            if monotone:
                assert (np.diff(t.astype(np.float64), axis=0) >= 0).all(), (name, n)
    assert render.COLORMAPS["heat"][1] and render.COLORMAPS["grey"][1] and not render.COLORMAPS["jet"][1]
    g = render.colormap("grey", 256)
    assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 0], (np.arange(256) / 255.0).astype(F32))
    j = render.colormap("jet", 9)          # the control points lie on i / 8
    assert np.array_equal(j[1], [0, 0, 1]) and np.array_equal(j[3], [0, 1, 1]) and np.array_equal(j[5], [1, 1, 0]) and np.array_equal(j[7], [1, 0, 0])
    for bad in (("viridis", 256), ("heat", 1), ("heat", 1025)):
        with pytest.raises(ValueError):
            render.colormap(*bad)


def test_uv_corners_on_a_seam():
    """two triangles that share the edge 1-2; on the second, vertices 1 and 2 carry other uv (a seam): four vertices, six vt"""
    vt = np.array([(0, 0), (1, 0), (0, 1), (0.5, 0.5), (0.75, 0.5), (0.5, 0.75)], F32)
    ft = np.array([(0, 1, 2), (4, 3, 5)])
    uv = render.uv_corners(vt, ft)
    assert uv.dtype == F32 and uv.shape == (2, 3, 2) and uv.flags["C_CONTIGUOUS"]
    assert np.array_equal(uv[0], [(0, 0), (1, 0), (0, 1)]) and np.array_equal(uv[1], [(0.75, 0.5), (0.5, 0.5), (0.5, 0.75)])
    for bad in ((vt, np.array([(0, 1, 6)])), (vt, np.array([(0, -1, 2)])), (vt[:, :1], ft), (vt, ft.astype(F32)), (vt, ft[:, :2])):
        with pytest.raises(ValueError):
            render.uv_corners(*bad)


def make_object():
    faces = np.array([0, 1, 2, 0, 2, 3], np.int32)
    cam, R, t = np.array([48, 48, 16, 16, 0.01, 3], F32), np.eye(3, dtype=F32), np.array([0, 0, -1], F32)
    light, base, bg = np.array([0, 0.6, 0.8, 0.25], F32), np.full(3, 0.3, F32), np.ones(3, F32)
    h = C.c_void_p()
    assert lib().fdm_render_create(faces.ctypes.data, 2, 4, 32, 32, cam.ctypes.data, R.ctypes.data, t.ctypes.data, light.ctypes.data, 1, 0.2,
                                   base.ctypes.data, bg.ctypes.data, C.byref(h)) == 0
    return h


def test_set_material_refusals_through_ctypes():
    l = lib()
    assert _lib.STRUCTS["fdm_render_material"] is RenderMaterial and l.fdm_abi_struct_size(b"fdm_render_material") == C.sizeof(RenderMaterial)
    assert l.fdm_version() == 105
    h = make_object()
    col, lut, uv, tex = np.full((4, 3), 0.5, F32), np.full((2, 3), 0.5, F32), np.zeros((2, 3, 2), F32), np.zeros((2, 2, 3), np.uint8)
    ptr = lambda a: a.ctypes.data  # noqa: E731

    def mat(kind=0, unlit=0, colors=None, lut=None, n_lut=0, lo=0.0, hi=1.0, uv=None, texture=None, w=0, h=0, flt=0):
        return RenderMaterial(kind, unlit, colors, lut, n_lut, lo, hi, uv, texture, w, h, flt)

    def refused(m, word):
        assert l.fdm_render_set_material(h, C.byref(m)) == -1 and word in l.fdm_last_error().decode(), (word, l.fdm_last_error().decode())

    good = [mat(), mat(0, 1), mat(1, 0, ptr(col)), mat(2, 1, lut=ptr(lut), n_lut=2, lo=-1.0, hi=2.0), mat(3, 0, uv=ptr(uv), texture=ptr(tex), w=2, h=2, flt=1)]
    for m in good:
        assert l.fdm_render_set_material(h, C.byref(m)) == 0, l.fdm_last_error().decode()
    assert l.fdm_render_set_material(h, None) == 0
    assert l.fdm_render_set_material(None, C.byref(good[0])) == -1
    refused(mat(4), "kind")
    refused(mat(-1), "kind")
    refused(mat(0, 2), "unlit")
    refused(mat(1), "null colors")
    refused(mat(2, n_lut=2), "null lut")
    refused(mat(3, texture=ptr(tex), w=2, h=2), "null uv or texture")
    refused(mat(3, uv=ptr(uv), w=2, h=2), "null uv or texture")
    for n in (1, 0, -5, 1025):
        refused(mat(2, lut=ptr(lut), n_lut=n), "n_lut")
    for w, hh in ((0, 2), (2, 0), (8193, 2), (2, 8193), (-1, -1)):
        refused(mat(3, uv=ptr(uv), texture=ptr(tex), w=w, h=hh), "texture of")
    for flt in (2, -1):
        refused(mat(3, uv=ptr(uv), texture=ptr(tex), w=2, h=2, flt=flt), "filter")
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (-3e38, 3e38)):
        refused(mat(2, lut=ptr(lut), n_lut=2, lo=lo, hi=hi), "range")
    for badv in (-0.25, float("nan"), float("inf")):
        c = col.copy()
        c[3, 1] = badv
        refused(mat(1, 0, ptr(c)), "colors[3][1]")
        t = lut.copy()
        t[1, 2] = badv
        refused(mat(2, lut=ptr(t), n_lut=2), "lut[1][2]")
    # a refusal leaves the object as it was (kind 3): the plain call still gets as far as the missing device, not the kind-2 refusal
    assert l.fdm_render_set_material(h, C.byref(good[4])) == 0
    refused(mat(2, lut=ptr(lut), n_lut=1), "n_lut")
    planes = _lib.RenderPlanes(0x2000, None, None, None, None)
    args = (h, 0x1000, None, 1, 1, None, 0, 0.0, 0.0, None)
    if not l.fdm_device_ok():
        assert l.fdm_render_forward(*args, 0x2000, None, None, 1, None, None) == -4 and "no gfx950 device" in l.fdm_last_error().decode()
    # scalars go with kind 2 and with no other; the plain calls refuse a kind-2 object
    assert l.fdm_render_forward_material(*args, C.byref(planes), 1, None, None, 0x3000) == -1 and "scalars" in l.fdm_last_error().decode()
    assert l.fdm_render_set_material(h, C.byref(good[3])) == 0
    assert l.fdm_render_forward_material(*args, C.byref(planes), 1, None, None, None) == -1 and "null scalars" in l.fdm_last_error().decode()
    assert l.fdm_render_forward(*args, 0x2000, None, None, 1, None, None) == -4 and "scalar-map" in l.fdm_last_error().decode()
    assert l.fdm_render_forward_planes(*args, C.byref(planes), 1, None, None) == -4 and "scalar-map" in l.fdm_last_error().decode()
    if not l.fdm_device_ok():
        assert l.fdm_render_forward_material(*args, C.byref(planes), 1, None, None, 0x3000) == -4 and "no gfx950 device" in l.fdm_last_error().decode()
    assert l.fdm_render_destroy(h) == 0
    assert l.fdm_op_vertex_dist(None, 0x1000, 0x2000, 1, 1, None) == -1
    assert l.fdm_op_vertex_dist(0x1000, 0x1000, 0x2000, 0, 1, None) == -2 and l.fdm_op_vertex_dist(0x1000, 0x1000, 0x2000, 1, 0, None) == -2


def test_python_value_errors():
    M = render.Material
    col, uv, tex = np.full((4, 3), 0.5, F32), np.zeros((2, 3, 2), F32), np.zeros((2, 2, 3), np.uint8)
    bad = [lambda: M.vertex_colors(col[:, :2]), lambda: M.vertex_colors(-col), lambda: M.vertex_colors(col * np.nan),
           lambda: M.scalar_map("viridis", 0, 1), lambda: M.scalar_map(np.zeros((1, 3), F32), 0, 1), lambda: M.scalar_map(np.zeros((1025, 3), F32), 0, 1),
           lambda: M.scalar_map("heat", 1, 1), lambda: M.scalar_map("heat", 0, float("nan")), lambda: M.scalar_map("heat", -3e38, 3e38),
           lambda: M.scalar_map(-np.ones((2, 3), F32), 0, 1),
           lambda: M.texture(tex.astype(F32), uv), lambda: M.texture(tex[..., :2], uv), lambda: M.texture(tex, uv[:, :2]), lambda: M.texture(tex, uv, "cubic"),
           lambda: M.texture(np.zeros((0, 2, 3), np.uint8), uv), lambda: M(7)]
    for make in bad:
        with pytest.raises(ValueError):
            make()
    a, b = M.scalar_map("heat", 0, 1), M.scalar_map("heat", 0, 1)
    assert a.token == b.token != M.scalar_map("heat", 0, 2).token and a.token != M.scalar_map("heat", 0, 1, unlit=True).token
    assert M.texture(tex, uv).token != M.texture(tex, uv, "nearest").token and M.vertex_colors(col).token != M.vertex_colors(col * 2).token
    faces, cam = np.array([(0, 1, 2), (0, 2, 3)], np.int32), render.Camera(48, 48, 16, 16, 32, 32)
    assert render.identity(faces, 4, cam) != render.identity(faces, 4, cam, material=a) != render.identity(faces, 4, cam, material=M.vertex_colors(col))
    assert render.identity(faces, 4, cam, material=a) == render.identity(faces, 4, cam, material=b)
    plan = render.RenderPlan(faces, 4, cam, device="cuda:0")
    key = plan.key
    for m in (M.vertex_colors(np.zeros((5, 3), F32)), M.texture(tex, np.zeros((3, 3, 2), F32)), "heat"):
        with pytest.raises(ValueError):
            plan.set_material(m)
        with pytest.raises(ValueError):
            render.RenderPlan(faces, 4, cam, material=m, device="cuda:0")
    assert plan.key == key
    plan.set_material(a)
    assert plan.key == render.identity(faces, 4, cam, material=a) and plan.arguments()["material"] is a
    plan.set_material(None)
    assert plan.key == key
    # the pipeline's refusals come before any model or device is touched
    with pytest.raises(ValueError, match="scalar_map"):
        pipeline._Outputs(None, "cpu", faces, render=dict(camera=cam, error_to=np.zeros((2, 12), F32)), fps=(30, 30))
    with pytest.raises(ValueError, match="scalar_map"):
        pipeline._Outputs(None, "cpu", faces, render=dict(camera=cam, material=M.vertex_colors(col), scalars=np.zeros((2, 4), F32)), fps=(30, 30))
    with pytest.raises(ValueError, match="not both"):
        pipeline._Outputs(None, "cpu", faces, render=dict(camera=cam, material=a, scalars=np.zeros((2, 4), F32), error_to=np.zeros((2, 12), F32)), fps=(30, 30))
    import torch
    clip = torch.zeros(1, 3, 12)
    for gt in (np.zeros((3, 15), F32), np.zeros((2, 12), F32), np.zeros((2, 3, 12), F32), np.zeros((3, 5, 3), F32)):
        with pytest.raises(ValueError, match="error_to"):
            pipeline._gt_rows(clip, gt)
    assert tuple(pipeline._gt_rows(clip, np.zeros((5, 4, 3), F32)).shape) == (1, 3, 12)


def test_material_arrays_are_its_own_and_error_to_is_checked_when_the_call_begins():
    import types
    M = render.Material
    col = np.full((4, 3), 0.5, F32)
    m = M.vertex_colors(col)
    token = m.token
    col[0, 0] = 0.25                                  # the caller's array is not the material's
    assert m.colors[0, 0] == 0.5 and m.token == token == M.vertex_colors(np.full((4, 3), 0.5, F32)).token
    t = M.texture(np.zeros((2, 2, 3), np.uint8), np.zeros((2, 3, 2), F32))
    for a in (m.colors, M.scalar_map(np.zeros((2, 3), F32), 0, 1).lut, M.scalar_map("heat", 0, 1).lut, t.uv, t.image):
        with pytest.raises(ValueError):
            a[0] = 1
    # a wrong vertex count in error_to: refused by _Outputs itself, before a model, a device or a clip exists
    faces, cam, heat = np.array([(0, 1, 2), (0, 2, 3)], np.int32), render.Camera(48, 48, 16, 16, 32, 32), M.scalar_map("heat", 0, 1)
    p = types.SimpleNamespace(V3=12)
    for gt in (np.zeros((3, 15), F32), np.zeros((3, 5, 3), F32), np.zeros(12, F32), [np.zeros((3, 12), F32), np.zeros((3, 9), F32)]):
        with pytest.raises(ValueError, match="error_to"):
            pipeline._Outputs(p, "cpu", faces, render=dict(camera=cam, material=heat, error_to=gt), fps=(30, 30))
    for gt in (np.zeros((3, 12), F32), np.zeros((3, 4, 3), F32), np.zeros((1, 3, 12), F32), [np.zeros((3, 12), F32), np.zeros((2, 4, 3), F32)]):
        pipeline._Outputs(p, "cpu", faces, render=dict(camera=cam, material=heat, error_to=gt), fps=(30, 30))
