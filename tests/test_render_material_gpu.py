"""MI355X: the materials of the render hand-off (fdm_render_set_material, fdm_render_forward_material, fdm_op_vertex_dist;
csrc/render_out.hpp, render_resolve_kernel<S, YUV, true>) equal to the numpy restatement of
tests/render_material_cases.py byte for byte, on the smallest shapes that can go wrong.  Outputs are filled with junk before every call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mesh_cases as MC
import render_cases as RC
import render_material_cases as RM
import render_planes_cases as RP
import wrap_cases as WC
from fdm_amd import pipeline, render
from fdm_amd._lib import FdmError, RenderPlanes, check, lib
from test_render_gpu import DEV, PIPE_MESH, dev, pipe_view, plan_of, run, tiny_audio, tiny_models
from test_render_planes_gpu import DTYPE, JUNK, coloured, mesh_of, same_bytes, shape_of

pytestmark = pytest.mark.gpu
F32 = np.float32
SAMPLES = [1, 4, 16]
SIZES = [(2, 2), (34, 18), (33, 17), (66, 2)]
MESHES = ["icosphere1", "whole_viewport", "off_screen", "strip40", "mixed_winding"]
NAMES = ("rgb", "depth", "face_ids", "alpha")


def mesh(name):
    if name != "mixed_winding":
        return mesh_of(name)
    p, f = RC.strip(12)                   # a zigzag strip alternates its winding; with every third face reversed neither sign has a pattern
    f = f.copy()
    f[::3] = f[::3, ::-1]
    return p, f


def checker(n=64, cell=8):
    i = np.arange(n) // cell
    on = ((i[:, None] + i[None, :]) & 1).astype(bool)
    return np.where(on[..., None], np.array([230, 40, 10], np.uint8), np.array([20, 90, 250], np.uint8)).astype(np.uint8)


def textures():
    g = np.random.default_rng(11)
    return {"1x1": np.array([[[204, 102, 51]]], np.uint8), "2x2": g.integers(0, 256, (2, 2, 3), dtype=np.uint8),
            "5x3": g.integers(0, 256, (3, 5, 3), dtype=np.uint8), "checker": checker()}


def corner_uv(F, tex, seed):
    """distinct uv on the three corners of every face; the first faces carry the exact values: 0, 1, texel centres and edges of `tex`,
    values outside [0, 1], +-1e30, infinities and NaN"""
    Ht, Wt = tex.shape[:2]
    uv = np.random.default_rng(seed).uniform(-0.25, 1.25, (F, 3, 2)).astype(F32)
    exact = [[(0, 0), (1, 0), (0, 1)], [(1, 1), (0, 1), (1, 0)], [(0.5 / Wt, 0.5 / Ht), ((Wt - 0.5) / Wt, 0.5 / Ht), (0.5 / Wt, (Ht - 0.5) / Ht)],
             [(1.0 / Wt, 0), (1, 1.0 / Ht), (0, 1)], [(-2, 3), (2.5, -1), (0.5, 0.5)], [(1e30, 0), (0, -1e30), (1, 1)],
             [(np.inf, 0), (0, 1), (1, 0)], [(0, 0), (np.nan, 1), (1, 0)], [(0, -np.inf), (1, 0), (0, 1)]]
    step = max(1, F // len(exact))
    for i, e in enumerate(exact):
        if i * step < F:
            uv[i * step] = np.asarray(e, F32)
    return uv


def materials(p, f, unlit=False):
    """name -> (the restatement's dict, the render.Material, scalars [V] or None)"""
    V, F = len(p), len(f)
    g = np.random.default_rng(V + F)
    out = {"base": (RM.base(unlit), render.Material.base(unlit), None)}
    c = g.uniform(0, 1.2, (V, 3)).astype(F32)
    out["colors"] = (RM.vertex_colors(c, unlit), render.Material.vertex_colors(c, unlit), None)
    s = g.uniform(-0.5, 1.5, V).astype(F32)
    s[:5] = [0.25, 0.75, 0.0, 1.5, np.nan][:min(5, V)]          # exactly lo and hi, below, above, NaN
    for N in (2, 256):
        lut = render.colormap("jet", N)
        out[f"map{N}"] = (RM.scalar_map(lut, 0.25, 0.75, unlit), render.Material.scalar_map(lut, 0.25, 0.75, unlit), s)
    for tn, tex in textures().items():
        uv = corner_uv(F, tex, 7)
        for flt in ("nearest", "bilinear"):
            out[f"tex{tn}_{flt}"] = (RM.texture(tex, uv, flt, unlit), render.Material.texture(tex, uv, flt, unlit), None)
    return out


def call(plan, x, names=NAMES, frames=None, tmpl=None, fps=None, Lo=None, scalars=None):
    x = dev(x)
    B = x.shape[0]
    if Lo is None:
        Lo = max([MC.frames_out(L, fps) for L in (frames if frames is not None else [x.shape[1]] * B)] + [1])
    out = {k: torch.full(shape_of(k, B, Lo, plan), JUNK[k], dtype=DTYPE[k], device=DEV) for k in names}
    got = plan.forward(x, frames, None if tmpl is None else dev(tmpl), fps, out=out, scalars=None if scalars is None else dev(scalars))
    res = {k: out[k].cpu().numpy() for k in names}
    res["frames"] = got.frames
    return res


def equal(got, want, what):
    """got: call()'s dict of [1, 1, ...]; want: the restatement's (rgb, depth, face, alpha) of one frame"""
    for k, w in zip(NAMES, want):
        assert same_bytes(got[k][0, 0], w), f"{what}: {k} differs at {int((got[k][0, 0] != w).sum())} elements"


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("name", MESHES)
def test_every_material_equals_the_restatement(name, S):
    p, f = mesh(name)
    x = p.reshape(1, 1, -1)
    for wh in SIZES if name in ("icosphere1", "mixed_winding") else [(34, 18)]:
        vw = coloured(*wh)
        plan = plan_of(f, len(p), vw, samples=S)
        plain = call(plan, x)
        for mn, (rm, m, s) in materials(p, f).items():
            plan.set_material(m)
            sc = None if s is None else s.reshape(1, 1, -1)
            got = call(plan, x, scalars=sc)
            equal(got, RM.render_static(p, f, vw, S, rm, s), f"{name} {wh} {mn}")
            for k in ("depth", "face_ids", "alpha"):                             # the material changes the colour alone
                assert same_bytes(got[k], plain[k]), (mn, k)
            if mn == "base":
                assert same_bytes(got["rgb"], plain["rgb"])
            if wh[0] % 2 == 0 and wh[1] % 2 == 0 and mn in ("colors", "map256", "texchecker_bilinear"):
                yuv = call(plan, x, ("yuv",), scalars=sc)["yuv"]
                assert yuv[0, 0].tobytes() == RP.yuv(got["rgb"][0, 0], RP.coeffs(709, False), "i420"), mn
        plan.set_material(None)
        after = call(plan, x)                                                     # the visibility buffer was left clear, base is back
        for k in NAMES:
            assert same_bytes(after[k], plain[k]), k
    if name == "mixed_winding":
        X, Y, w, bad, _ = RC.vertex_stage(p, np.zeros_like(p), coloured(34, 18))
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
        assert (A < 0).any() and (A > 0).any()


@pytest.mark.parametrize("S", SAMPLES)
def test_unlit_on_each_kind(S):
    p, f = mesh("icosphere1")
    vw = coloured(34, 18)
    plan = plan_of(f, len(p), vw, samples=S)
    for mn, (rm, m, s) in materials(p, f, unlit=True).items():
        if mn in ("base", "colors", "map256", "tex5x3_bilinear", "texchecker_nearest"):
            plan.set_material(m)
            equal(call(plan, p.reshape(1, 1, -1), scalars=None if s is None else s.reshape(1, 1, -1)), RM.render_static(p, f, vw, S, rm, s), mn)


@pytest.mark.parametrize("S", SAMPLES)
def test_single_colour_texture_is_the_base_render(S):
    p, f = mesh("icosphere1")
    tex = textures()["1x1"]
    col = tex[0, 0].astype(F32) / F32(255)
    vw = coloured(34, 18)
    want = run(plan_of(f, len(p), dict(vw, base=col), samples=S), p.reshape(1, 1, -1))
    for flt in ("nearest", "bilinear"):
        plan = plan_of(f, len(p), vw, samples=S, material=render.Material.texture(tex, np.random.default_rng(3).uniform(-0.5, 1.5, (len(f), 3, 2)).astype(F32), flt))
        got = run(plan, p.reshape(1, 1, -1))                                      # fdm_render_forward on a kind-3 object
        for i in range(3):
            assert same_bytes(got[i], want[i]), (flt, i)


def test_existing_calls_with_a_material():
    p, f = mesh("icosphere1")
    vw = coloured(34, 18)
    x = p.reshape(1, 1, -1)
    plan = plan_of(f, len(p), vw, samples=4)
    base = run(plan, x)
    rm, m, _ = materials(p, f)["colors"]
    plan.set_material(m)
    plain, planes = run(plan, x), call(plan, x)
    want = RM.render_static(p, f, vw, 4, rm)
    assert same_bytes(plain[0][0, 0], want[0]) and same_bytes(planes["rgb"], plain[0]) and not same_bytes(plain[0], base[0])
    xx = dev(x)
    head = (plan.h, xx.data_ptr(), None, 1, 1, None, 0, 0.0, 0.0, None)

    def c_material_call(scalars=None):
        """fdm_render_forward_material itself, into junk-filled rgb, depth, face and alpha"""
        o = {k: torch.full(shape_of(k, 1, 1, plan), JUNK[k], dtype=DTYPE[k], device=DEV) for k in NAMES}
        got_n = (C.c_int * 1)(-7)
        check(lib().fdm_render_forward_material(*head, C.byref(RenderPlanes(*[o[k].data_ptr() for k in NAMES], None)), 1, got_n, None, scalars))
        torch.cuda.synchronize()
        assert got_n[0] == 1
        return {k: o[k].cpu().numpy() for k in NAMES}

    # fdm_render_forward_material without scalars on a kind-1 and on a kind-3 object (both filters): fdm_render_forward's bytes
    tex_names = ("tex5x3_bilinear", "texchecker_nearest")
    for mn in ("colors",) + tex_names:
        rmk, mk, _ = materials(p, f)[mn]
        plan.set_material(mk)
        fwd, mat = run(plan, x), c_material_call()
        for i, k in enumerate(("rgb", "depth", "face_ids")):
            assert same_bytes(mat[k], fwd[i]), (mn, k)
        assert same_bytes(mat["rgb"][0, 0], RM.render_static(p, f, vw, 4, rmk)[0]) and same_bytes(mat["alpha"], planes["alpha"]), mn
    plan.set_material(None)                                                       # and on an object with no material
    mat = c_material_call()
    for i, k in enumerate(("rgb", "depth", "face_ids")):
        assert same_bytes(mat[k], base[i]), k
    plan.set_material(m)
    _, m2, s = materials(p, f)["map2"]
    sdev = dev(s.reshape(1, 1, -1))
    with pytest.raises(FdmError, match="scalars on an object") as e:             # scalars on a kind-1 object: refused in C too
        c_material_call(sdev.data_ptr())
    assert e.value.code == -1
    plan.set_material(m2)
    with pytest.raises(FdmError, match="null scalars") as e:
        c_material_call()
    assert e.value.code == -1
    rm2 = materials(p, f)["map2"][0]
    assert same_bytes(c_material_call(sdev.data_ptr())["rgb"][0, 0], RM.render_static(p, f, vw, 4, rm2, s)[0])
    out = torch.full((1, 1, 18, 34, 3), 0x5A, dtype=torch.uint8, device=DEV)     # the older C calls on the kind-2 object
    for planes in (False, True):
        with pytest.raises(FdmError, match="scalar-map") as e:
            if planes:
                check(lib().fdm_render_forward_planes(*head, C.byref(RenderPlanes(out.data_ptr(), None, None, None, None)), 1, None, None))
            else:
                check(lib().fdm_render_forward(*head, out.data_ptr(), None, None, 1, None, None))
        assert e.value.code == -4
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                                              # nothing was launched
    with pytest.raises(ValueError, match="scalars"):
        plan.forward(dev(x))
    plan.set_material(m)
    with pytest.raises(ValueError, match="scalars"):
        plan.forward(dev(x), scalars=dev(s.reshape(1, 1, -1)))
    plan.set_material(None)
    again = run(plan, x)
    for i in range(3):
        assert same_bytes(again[i], base[i])


@functools.lru_cache(maxsize=None)
def clips_case():
    """B = 3, frames (0, 1, 5), L_max = 5, the small grid mesh in front of a 34 x 18 camera; NaN junk past every clip's frames in the
    positions and in the scalars"""
    faces, V, _ = MC.mesh("grid")
    frames, B, L = [0, 1, 5], 3, 5
    off = MC.offsets("grid", B, L, seed=31)
    tmpl = (MC.template("grid", seed=3, rows=B) - np.tile(np.array([0.35, 0.15, 0.0], F32), V)).astype(F32)
    sc = np.random.default_rng(9).uniform(0.0, 1.0, (B, L, V)).astype(F32) + F32(0.125)
    x, s = off.copy(), sc.copy()
    for b, n in enumerate(frames):
        x[b, n:] = np.nan
        s[b, n:] = np.nan
    return off, sc, x, s, tmpl, frames, faces, V


@pytest.mark.parametrize("fps", [None, (30, 60)], ids=["same_rate", "double_rate"])
@pytest.mark.parametrize("S", [1, 4])
def test_ragged_clips_scalars_and_chunks(S, fps):
    off, sc, x, s, tmpl, frames, faces, V = clips_case()
    vw = coloured(34, 18)
    lut = render.colormap("heat", 256)
    rm, m = RM.scalar_map(lut, 0.25, 1.0), render.Material.scalar_map(lut, 0.25, 1.0)
    plan = plan_of(faces, V, vw, samples=S, material=m)
    Lo = 11
    want = RM.render_clips(off, tmpl, frames, fps, faces, V, vw, S, rm, sc)
    got = call(plan, x, NAMES, frames, tmpl, fps, Lo=Lo, scalars=s)
    assert got["frames"] == [len(w[0]) for w in want] == [MC.frames_out(n, fps) for n in frames]
    for b, w in enumerate(want):
        n = len(w[0])
        for k, a in zip(NAMES, w):
            assert same_bytes(got[k][b, :n], a), f"clip {b}: {k}"
            assert not got[k][b, n:].view(np.uint8).any(), f"padding of clip {b}: {k}"
    assert (want[2][3] > 0).any() and len(np.unique(want[2][0].reshape(-1, 3), axis=0)) > 20
    plan.set_chunk_frames(1)
    one = call(plan, x, NAMES, frames, tmpl, fps, Lo=Lo, scalars=s)
    for k in NAMES:
        assert same_bytes(one[k], got[k]), f"chunk_frames = 1: {k}"
    # vertex colours and a texture through the same ragged call, chunked or not
    c = np.random.default_rng(1).uniform(0, 1, (V, 3)).astype(F32)
    tex = textures()["5x3"]
    uv = corner_uv(len(faces), tex, 2)
    for rmk, mk in ((RM.vertex_colors(c), render.Material.vertex_colors(c)), (RM.texture(tex, uv), render.Material.texture(tex, uv))):
        wantk = RM.render_clips(off, tmpl, frames, fps, faces, V, vw, S, rmk)
        for chunk in (1, 0):
            plan.set_chunk_frames(chunk)
            plan.set_material(mk)
            gotk = call(plan, x, NAMES, frames, tmpl, fps, Lo=Lo)
            for b, w in enumerate(wantk):
                assert same_bytes(gotk["rgb"][b, :len(w[0])], w[0]) and not gotk["rgb"][b, len(w[0]):].any(), (rmk["kind"], chunk, b)


@pytest.mark.parametrize("V", [1, 7, 5023])
@pytest.mark.parametrize("rows", [1, 3])
def test_vertex_dist(V, rows):
    g = np.random.default_rng(V + rows)
    a, b = g.standard_normal((rows, 3 * V)).astype(F32), g.standard_normal((rows, 3 * V)).astype(F32)
    b[0, :3] = a[0, :3]                                                           # a distance of exactly 0
    want = RM.vertex_dist(a, b)
    got = render.vertex_error(dev(a), dev(b)).cpu().numpy()                       # finite data: every element, bit for bit
    assert got.shape == (rows, V) and np.isfinite(want).all() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0, 0] == 0 and (V == 1 or (got[0, 1:] > 0).all())
    four = render.vertex_error(dev(a.reshape(1, rows, V, 3)), dev(b.reshape(1, rows, V, 3))).cpu().numpy()
    assert four.shape == (1, rows, V) and np.array_equal(four[0].view(np.uint32), got.view(np.uint32))
    an = a.copy()                                                                 # the last row NaN: it comes out NaN (whatever its bits),
    an[rows - 1, :] = np.nan                                                      # the rows before it keep their bits
    gn = render.vertex_error(dev(an), dev(b)).cpu().numpy()
    assert np.isnan(gn[rows - 1]).all() and np.array_equal(gn[:rows - 1].view(np.uint32), want[:rows - 1].view(np.uint32))
    for bad in (torch.zeros((), device=DEV), torch.zeros(4, device=DEV), torch.zeros(1, 1, 2, 2, device=DEV), torch.zeros(0, 3, device=DEV)):
        with pytest.raises(ValueError, match="vertex_error takes"):
            render.vertex_error(bad, bad)
    one = a.copy()                                                                # one NaN coordinate: that vertex alone is NaN
    one[0, 3 * (V - 1) + 1] = np.nan
    g1 = render.vertex_error(dev(one), dev(b)).cpu().numpy()
    keep = np.ones((rows, V), bool)
    keep[0, V - 1] = False
    assert np.isnan(g1[0, V - 1]) and np.array_equal(g1[keep].view(np.uint32), want[keep].view(np.uint32))


def test_pipeline_materials():
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    S, _ = WC.source(PIPE_MESH)
    tmpl = S.reshape(1, -1)
    wav = tiny_audio(0.2, 1)
    kw = dict(ddim_steps=2, seed=2, device=DEV)
    rv = dict(pipe_view(), samples=4, background=(0.0, 0.0, 0.0))
    verts, lat = pipeline.animate(diffusion, ae, wav, tmpl, **kw)                 # [1, L, 3 V]
    L = int(verts.shape[1])
    gt = (verts[0] + 0.01 * torch.randn(L, 3 * V, generator=torch.Generator().manual_seed(5)).to(DEV))
    gt_long = torch.cat([gt, gt[-1:].expand(3, -1)])                              # longer than the clip: cropped
    m = render.Material.scalar_map("heat", 0.0, 0.02, unlit=True)
    im, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, render=dict(rv, material=m, error_to=gt_long), **kw)
    err = render.vertex_error(verts, gt.unsqueeze(0))
    direct = pipeline.to_images(verts, faces, dict(rv, material=m), scalars=err)
    plain, _ = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, render=rv, **kw)
    assert torch.equal(lat, lat2) and im.frames == direct.frames == [L]
    assert torch.equal(im.images, direct.images) and torch.equal(im.depth, direct.depth) and torch.equal(im.face_ids, direct.face_ids)
    assert torch.equal(im.face_ids, plain.face_ids) and not torch.equal(im.images, plain.images)
    for bad in (gt[:L - 1], gt[:, :-3]):
        with pytest.raises(ValueError, match="error_to"):
            pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, render=dict(rv, material=m, error_to=bad), **kw)
    many, _ = pipeline.animate_many(diffusion, ae, [wav], [tmpl], faces=faces, render=dict(rv, material=m, error_to=[gt_long]), **kw)
    assert torch.equal(many[0].images, im.images)
    c = np.random.default_rng(2).uniform(0, 1, (V, 3)).astype(F32)
    mc = render.Material.vertex_colors(c)
    many_c, _ = pipeline.animate_many(diffusion, ae, [wav], [tmpl], faces=faces, render=dict(rv, material=mc), **kw)
    assert torch.equal(many_c[0].images, pipeline.to_images(verts, faces, dict(rv, material=mc)).images)
    tex = checker()
    mt = render.Material.texture(tex, np.random.default_rng(4).uniform(0, 1, (len(faces), 3, 2)).astype(F32))
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, faces=faces, render=dict(rv, material=mt))
    hs = srv.submit_many([wav], [tmpl], seeds=2)
    res = {h: v for h, v, _ in srv.drain(1)}
    solo, _ = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, render=dict(rv, material=mt), **kw)
    assert torch.equal(res[hs[0]].images, solo.images) and not torch.equal(solo.images, plain.images)
    with pytest.raises(ValueError, match="scalar map"):
        pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, faces=faces, render=dict(rv, material=m))
