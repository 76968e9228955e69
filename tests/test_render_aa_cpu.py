"""Multi-sample rendering without a device (the anti-aliasing paragraph): the numpy restatement of
tests/render_aa_cases.py at S = 1 against tests/render_cases.py and at S = 4, 16 against things that can be derived by hand; the host
table fdm_render_sample_pattern_host; the refusals of fdm_render_set "samples"; the sample count in a plan's identity."""
import ctypes as C

import numpy as np
import pytest

import render_aa_cases as RA
import render_cases as RC
from fdm_amd import render
from fdm_amd._lib import FdmError, lib
from test_render_cpu import flat_view, make, cam, rect
from test_render_gpu import SCENES, scene

F32 = np.float32
ARG = -1


@pytest.mark.parametrize("wh", [(1, 1), (37, 29)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_one_sample_is_the_existing_restatement(name, wh):
    vw = RC.view(*wh)
    p, f = scene(name, vw)
    for a, b in zip(RC.render_static(p, f, vw), RA.render_static(p, f, vw, 1)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_strips_at_one_sample_are_the_existing_restatement():
    vw = RC.view(33, 17)
    for F in (1, 255, 257):
        p, f = RC.strip(F)
        for a, b in zip(RC.render_static(p, f, vw), RA.render_static(p, f, vw, 1)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_sample_pattern_host():
    assert render.sample_pattern(1).tolist() == [[128, 128]]
    assert render.sample_pattern(4).tolist() == [[96, 32], [224, 96], [32, 160], [160, 224]]
    assert render.sample_pattern(16).tolist() == [[32 + 64 * i, 32 + 64 * j] for j in range(4) for i in range(4)]
    for S in (1, 4, 16):
        assert np.array_equal(render.sample_pattern(S), RA.pattern(S)) and render.sample_pattern(S).dtype == np.int32
    L = lib()
    buf = (C.c_int * 64)(*([-7] * 64))
    for n in (0, 2, 8, 32, -4):
        assert L.fdm_render_sample_pattern_host(n, buf) == ARG and b"1, 4 or 16" in L.fdm_last_error()
        with pytest.raises(FdmError):
            render.sample_pattern(n)
    assert list(buf) == [-7] * 64                                        # a refused call writes nothing
    assert L.fdm_render_sample_pattern_host(4, None) == ARG and b"null" in L.fdm_last_error()
    assert L.fdm_render_sample_pattern_host(16, buf) == 0 and list(buf)[32:] == [-7] * 32 and list(buf)[:4] == [32, 32, 96, 32]


@pytest.mark.parametrize("ambient,base", [(0.0, 0.3), (1.0, 0.25)], ids=["black", "quarter"])
@pytest.mark.parametrize("S", [4, 16])
def test_a_right_edge_at_half_a_pixel_gives_half_the_samples(S, ambient, base):
    """a rectangle over the pixels [3, 6.5) x [2, 7) on white, lit by the ambient term alone: k = ambient, c = base ambient (0, or 0.25);
    column 6 has the samples with ox < 128 inside -- half of them in both patterns --, so its channel is (S/2 c + S/2 bg) / S, every
    partial sum exact in fp32"""
    vw = flat_view(12, 9, lights=np.zeros((0, 4), F32), ambient=ambient, base=(base, base, base), background=(1.0, 1.0, 1.0))
    p, f = rect(vw, 3, 2, 6.5, 7, 1.0)
    X, Y, _, bad, _ = RC.vertex_stage(p, np.zeros_like(p), vw)
    assert not bad.any() and sorted(set(X.tolist())) == [768, 256 * 6 + 128] and sorted(set(Y.tolist())) == [512, 1792]
    cov = RA.coverage(p, f, vw, S)
    ox = RA.pattern(S)[:, 0]
    assert cov[2:7, 3:6].all() and np.array_equal(cov[4, 6], ox < 128) and int((ox < 128).sum()) == S // 2
    assert not cov[:, 7:].any() and not cov[:2].any() and not cov[7:].any() and not cov[:, :3].any()
    rgb, depth, face = RA.render_static(p, f, vw, S)
    c, bg, half = F32(base) * F32(ambient), F32(1), F32(S // 2)
    edge_value = (half * c + half * bg) * F32(1.0 / S)                      # (2 c + 2 bg) / 4, (8 c + 8 bg) / 16
    assert edge_value == F32(0.5) * (c + bg)
    u8 = lambda v: int(F32(255) * F32(v) + F32(0.5))  # noqa: E731
    assert (rgb[2:7, 6] == u8(edge_value)).all() and (rgb[2:7, 3:6] == u8(c)).all()
    outside = np.ones((9, 12), bool)
    outside[2:7, 3:7] = False
    assert (rgb[outside] == 255).all() and (face[outside] == -1).all() and (depth[outside] == 0).all()
    assert (face[2:7, 3:7] >= 0).all() and np.abs(depth[2:7, 3:7] - F32(1)).max() <= 4 * np.spacing(F32(1))      # (as test_render_cpu)
    if ambient == 0.0:
        assert u8(edge_value) == 128 and u8(c) == 0


CUTS = {  # a convex quad a, b, c, d in sub-pixel units, cut along a - c, which runs through sample coordinates of both patterns
    "vertical at 256 x + 96": ((256 * 5 + 96, 0), (2560, 1024), (256 * 5 + 96, 2048), (256, 1024)),
    "horizontal at 256 y + 32": ((0, 256 * 4 + 32), (1024, 256), (2304, 256 * 4 + 32), (1024, 2048)),
    "diagonal through (96, 32) of every pixel": ((96, 32), (2048 + 96, 32), (2048 + 96, 2048 + 32), (96, 2048 + 32)),
}


@pytest.mark.parametrize("S", [4, 16])
@pytest.mark.parametrize("cut", list(CUTS))
def test_an_edge_on_a_sample_follows_the_top_left_rule_and_covers_it_once(cut, S):
    quad = CUTS[cut]
    vw = flat_view(16, 16)
    pts = [RC.pixel_to_world(vw, x / 256.0, y / 256.0, 1.0) for x, y in quad]
    ys, xs = np.mgrid[0:16, 0:16]
    pat = RA.pattern(S)
    px, py = 256 * xs[..., None] + pat[:, 0], 256 * ys[..., None] + pat[:, 1]                # [16, 16, S]
    side = [(quad[(i + 1) % 4][0] - quad[i][0]) * (py - quad[i][1]) - (quad[(i + 1) % 4][1] - quad[i][1]) * (px - quad[i][0]) for i in range(4)]
    strictly_in = np.all([s > 0 for s in side], axis=0) | np.all([s < 0 for s in side], axis=0)
    strictly_out = np.any([s > 0 for s in side], axis=0) & np.any([s < 0 for s in side], axis=0)
    dx, dy = quad[2][0] - quad[0][0], quad[2][1] - quad[0][1]
    e = dx * (py - quad[0][1]) - dy * (px - quad[0][0])                                       # > 0: on the side of d (y down)
    on_cut = (e == 0) & strictly_in
    assert on_cut.sum() >= 2, "the shared edge must pass through sample positions"
    for faces in ([(0, 1, 2), (0, 2, 3)], [(0, 2, 1), (0, 2, 3)], [(2, 0, 1), (3, 0, 2)]):
        p, f = RC.tris(pts, faces)
        X, Y, _, _, _ = RC.vertex_stage(p, np.zeros_like(p), vw)
        assert [(int(a), int(b)) for a, b in zip(X, Y)] == list(quad)
        one = [RA.coverage(p, f[k:k + 1], vw, S) for k in range(2)]                           # triangle a b c, triangle a c d
        n = one[0].astype(int) + one[1].astype(int)
        assert n.max() == 1 and (n[strictly_in] == 1).all() and (n[strictly_out] == 0).all()
        assert np.array_equal(RA.coverage(p, f, vw, S), n == 1)
        # a sample on the cut belongs to the triangle that travels the cut as a left edge (dy < 0) or a top edge (dy == 0, dx > 0)
        owns = [_owns_the_cut(quad[0], quad[1], quad[2], quad[0], quad[2]), _owns_the_cut(quad[0], quad[2], quad[3], quad[0], quad[2])]
        assert owns[0] != owns[1]
        k = 0 if owns[0] else 1
        assert one[k][on_cut].all() and not one[1 - k][on_cut].any()


def _owns_the_cut(t0, t1, t2, a, c):
    """whether the triangle (t0, t1, t2), oriented to A > 0 with y down as the setup orients it, travels its edge between its corners
    a and c as a left or a top edge"""
    A = (t1[0] - t0[0]) * (t2[1] - t0[1]) - (t1[1] - t0[1]) * (t2[0] - t0[0])
    order = [t0, t1, t2] if A > 0 else [t0, t2, t1]
    src, dst = (a, c) if order[(order.index(a) + 1) % 3] == c else (c, a)
    dx, dy = dst[0] - src[0], dst[1] - src[1]
    return dy < 0 or (dy == 0 and dx > 0)


def test_set_samples_refuses_and_the_identity_follows():
    L = lib()
    plan = make()
    for n in (2, -1, 17, 0, 8):
        assert L.fdm_render_set(plan.h, b"samples", n) == ARG and b"1, 4 or 16" in L.fdm_last_error()
        with pytest.raises(FdmError, match="1, 4 or 16"):
            plan.set_samples(n)
    assert plan.view["samples"] == 1
    assert L.fdm_render_set(plan.h, b"sample", 4) == ARG and b"unknown key" in L.fdm_last_error()
    assert b"chunk_frames" in L.fdm_last_error() and b"samples" in L.fdm_last_error()
    with pytest.raises(FdmError, match="1, 4 or 16"):
        make(samples=2)
    # W H S <= 2^26 keys per frame
    big = make(camera=cam(width=4096, height=4096))
    big.set_samples(4)
    assert L.fdm_render_set(big.h, b"samples", 16) == ARG and b"2^26" in L.fdm_last_error() and big.view["samples"] == 4
    make(camera=cam(width=2048, height=2048), samples=16)
    with pytest.raises(FdmError, match="2\\^26"):
        make(camera=cam(width=2049, height=2048), samples=16)
    with pytest.raises(FdmError, match="2\\^26"):
        make(camera=cam(width=4096, height=4097 - 1), samples=4).set_samples(16)
    # the sample count is part of what a plan is
    keys = set()
    for n in (1, 4, 16):
        plan.set_samples(n)
        assert plan.view["samples"] == n and plan.arguments()["samples"] == n
        assert plan.key == render.identity(plan.faces, plan.V, **plan.view) == make(samples=n).key
        keys.add(plan.key)
    assert len(keys) == 3
    cm = cam()
    assert render.identity(plan.faces, 4, cm) == render.identity(plan.faces, 4, cm, samples=1) != render.identity(plan.faces, 4, cm, samples=4)


def test_the_command_line_takes_render_samples():
    import argparse
    from fdm_amd import pipeline
    ap = argparse.ArgumentParser()
    pipeline.add_render_arguments(ap)
    assert ap.parse_args([]).render_samples == 1 and ap.parse_args(["--render_samples", "16"]).render_samples == 16
    with pytest.raises(SystemExit):
        ap.parse_args(["--render_samples", "2"])
