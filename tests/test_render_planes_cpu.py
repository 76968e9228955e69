"""The planes of the render hand-off without a device (include/fdm_hip.h, fdm_render_forward_planes,
fdm_render_yuv_coeffs_host): the new symbols and their binding, the four coefficient tables against the header's numbers and the numpy
restatement of tests/render_planes_cases.py, what those tables do to all 2^24 colours, every refusal of fdm_render_set "yuv_*" and of
the planes call on an object without a device, write_y4m byte for byte, the ImageFrames defaults and the command-line flags."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_planes_cases as RP
from fdm_amd import _lib, render
from fdm_amd._lib import FdmError, RenderPlanes, lib
from test_render_cpu import ARG, SHAPE, STATE, cam, make


def test_the_symbols_are_exported_and_bound_and_the_version_stays():
    l = lib()
    assert l.fdm_version() == _lib.LIB_VERSION == 105          # the feature is detected by the symbols
    for name in ("fdm_render_forward_planes", "fdm_render_yuv_coeffs_host"):
        assert name in _lib.SYMBOLS and getattr(l, name).argtypes == _lib.SYMBOLS[name][1]
    assert [f[0] for f in RenderPlanes._fields_] == ["rgb", "depth", "face", "alpha", "yuv"] and C.sizeof(RenderPlanes) == 5 * C.sizeof(C.c_void_p)
    assert _lib.STRUCTS["fdm_render_planes"] is RenderPlanes and l.fdm_abi_struct_size(b"fdm_render_planes") == C.sizeof(RenderPlanes)
    assert l.fdm_render_forward_planes.argtypes[10] == C.POINTER(RenderPlanes) and len(l.fdm_render_forward_planes.argtypes) == 14


@pytest.mark.parametrize("matrix,full", list(RP.TABLES))
def test_coefficients_equal_the_tables_and_the_restatement(matrix, full):
    k = render.yuv_coeffs(matrix, full)
    assert k.dtype == np.int32 and k.tolist() == list(RP.TABLES[(matrix, full)]) == RP.coeffs(matrix, full).tolist()
    assert k[0] + k[1] + k[2] == (65536 if full else 56284) and k[3] + k[4] + k[5] == 0 and k[6] + k[7] + k[8] == 0      # greys are exact
    buf = (C.c_int * 12)(*([-7] * 12))
    assert lib().fdm_render_yuv_coeffs_host(matrix, 5 if full else 0, buf) == 0 and list(buf)[:10] == k.tolist() and list(buf)[10:] == [-7, -7]


def test_coefficients_refuse():
    L = lib()
    buf = (C.c_int * 10)(*([-7] * 10))
    for m in (0, 2020, 600, -709):
        assert L.fdm_render_yuv_coeffs_host(m, 0, buf) == ARG and b"601 or 709" in L.fdm_last_error()
        with pytest.raises(FdmError):
            render.yuv_coeffs(m, False)
    assert L.fdm_render_yuv_coeffs_host(709, 0, None) == ARG and b"null" in L.fdm_last_error()
    assert list(buf) == [-7] * 10                              # a refused call writes nothing


@pytest.mark.parametrize("matrix,full", list(RP.TABLES))
def test_all_colours(matrix, full):
    """every one of the 2^24 colours as a pixel (luma) and as a uniform 2 x 2 block (chroma: the sums are four times the colour)"""
    k = render.yuv_coeffs(matrix, full).astype(np.int64)
    g = np.arange(256, dtype=np.int64)
    lo_y, hi_y, lo_c, hi_c = 255, 0, 255, 0
    raw_max = 0
    for r in range(256):                                      # 2^16 colours at a time
        rgb = np.stack(np.broadcast_arrays(np.int64(r), g[:, None], g[None, :]), axis=-1).reshape(-1, 3)
        y = RP.luma(rgb, k)
        u, v = RP.chroma(4 * rgb, k, before_clamp=True)
        lo_y, hi_y = min(lo_y, int(y.min())), max(hi_y, int(y.max()))
        lo_c, hi_c = min(lo_c, int(u.min()), int(v.min())), max(hi_c, int(u.max()), int(v.max()))
        raw_max = max(raw_max, int(np.abs(k[3] * 4 * rgb[:, 0] + k[4] * 4 * rgb[:, 1] + k[5] * 4 * rgb[:, 2]).max()))
    assert raw_max < 2 ** 31 - 2 ** 18                        # int32 suffices
    px = lambda c: (int(RP.luma(np.array(c), k)),) + tuple(int(x) for x in RP.chroma(4 * np.array(c), k))  # noqa: E731
    grey = np.stack([g, g, g], axis=-1)
    u, v = RP.chroma(4 * grey, k)
    assert (u == 128).all() and (v == 128).all()              # every grey
    if not full:
        assert (lo_y, hi_y, lo_c, hi_c) == (16, 235, 16, 240)
        assert px((255, 255, 255)) == (235, 128, 128) and px((0, 0, 0)) == (16, 128, 128)
        assert (RP.luma(grey, k) == 16 + ((56284 * g + 32768) >> 16)).all()
    else:
        assert (lo_y, hi_y) == (0, 255) and hi_c == 256 and lo_c >= 0      # pure blue / red reach 256 before the clamp
        assert px((255, 255, 255)) == (255, 128, 128) and px((0, 0, 0)) == (0, 128, 128)
        assert px((0, 0, 255))[1] == 255 and px((255, 0, 0))[2] == 255
        assert int(RP.chroma(4 * np.array((0, 0, 255)), k, before_clamp=True)[0]) == 256
        assert (RP.luma(grey, k) == g).all()


def test_the_restatement_lays_the_planes_out_as_ffmpeg_reads_them():
    """a 4 x 2 frame by hand: i420 = Y rows, U row, V row; nv12 = Y rows, U V pairs"""
    k = RP.coeffs(709, False)
    rgb = np.zeros((2, 4, 3), np.uint8)
    rgb[:, :2] = (255, 255, 255)                               # the left block white, the right block: one blue pixel of four
    rgb[1, 3] = (0, 0, 255)
    yb = int(RP.luma(np.array((0, 0, 255)), k))
    ub, vb = (int(x) for x in RP.chroma(np.array((0, 0, 255)), k))
    assert yb == 16 + ((4064 * 255 + 32768) >> 16) and ub == 128 + ((28784 * 255 + (1 << 17)) >> 18) and vb == 128 + ((-2639 * 255 + (1 << 17)) >> 18)
    want_y = [235, 235, 16, 16, 235, 235, 16, yb]
    assert list(RP.yuv(rgb, k, "i420")) == want_y + [128, ub] + [128, vb]
    assert list(RP.yuv(rgb, k, "nv12")) == want_y + [128, 128, ub, vb]
    assert RP.alpha(np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 1], [1, 1, 1, 1]], bool)).tolist() == [0, 64, 128, 191, 255]
    assert RP.alpha(np.array([[0], [1]], bool)).tolist() == [0, 255]
    assert RP.alpha(np.arange(17)[:, None] > np.arange(16)[None, :]).tolist() == [(255 * n + 8) // 16 for n in range(17)]


def test_set_yuv_refuses_and_the_identity_follows():
    L = lib()
    plan = make()
    for key, bad, word in ((b"yuv_matrix", (0, 2020, 600, 1), b"601 or 709"), (b"yuv_range", (-1, 2, 16), b"0 limited, 1 full"),
                           (b"yuv_layout", (-1, 2, 420), b"0 I420, 1 NV12")):
        for v in bad:
            assert L.fdm_render_set(plan.h, key, v) == ARG and word in L.fdm_last_error()
    assert L.fdm_render_set(plan.h, b"yuv", 1) == ARG and b"unknown key" in L.fdm_last_error()
    for key in (b"chunk_frames", b"samples", b"yuv_matrix", b"yuv_range", b"yuv_layout"):
        assert key in L.fdm_last_error()
    for kw in (dict(matrix=2020), dict(range="video"), dict(layout="yv12"), dict(range=2)):
        with pytest.raises(FdmError):
            plan.set_yuv(**kw)
    with pytest.raises(FdmError):
        make(yuv_layout="nv21")
    assert (plan.view["yuv_matrix"], plan.view["yuv_range"], plan.view["yuv_layout"]) == (709, "limited", "i420")
    keys = {plan.key}
    assert plan.key == render.identity(plan.faces, plan.V, cam()) == make().key
    for kw in (dict(matrix=601), dict(range="full"), dict(layout="nv12"), dict(matrix=709, range="limited")):
        plan.set_yuv(**kw)
        assert plan.key == render.identity(plan.faces, plan.V, **plan.view) and plan.key not in keys
        assert plan.key == make(**{k: plan.view[k] for k in ("yuv_matrix", "yuv_range", "yuv_layout")}).key
        assert plan.arguments()["yuv_layout"] == plan.view["yuv_layout"]
        keys.add(plan.key)
    assert plan.view["yuv_layout"] == "nv12" and plan.view["yuv_matrix"] == 709 and plan.view["yuv_range"] == "limited"


def test_forward_planes_refuses():
    """never a launch (the pointers are not dereferenced): every refusal a code and a message, then FDM_ERR_STATE without a device"""
    L = lib()
    plan, odd = make(), make(camera=cam(width=31, cx=15.5))
    x, fr, bad = C.c_void_p(0x1000), (C.c_int * 2)(3, 0), (C.c_int * 2)(3, 4)
    only = lambda **kw: C.byref(RenderPlanes(**{k: C.c_void_p(v) for k, v in kw.items()}))  # noqa: E731
    y = only(yuv=0x2000)
    fw = lambda *a: L.fdm_render_forward_planes(*a)  # noqa: E731
    assert fw(None, x, fr, 2, 3, None, 0, 0.0, 0.0, None, y, 3, None, None) == ARG and b"null" in L.fdm_last_error()
    assert fw(plan.h, None, fr, 2, 3, None, 0, 0.0, 0.0, None, y, 3, None, None) == ARG
    assert fw(plan.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, None, 3, None, None) == ARG and b"null" in L.fdm_last_error()
    assert fw(plan.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, C.byref(RenderPlanes()), 3, None, None) == ARG and b"every output is null" in L.fdm_last_error()
    assert fw(odd.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, y, 3, None, None) == ARG and b"even" in L.fdm_last_error() and b"31 x 32" in L.fdm_last_error()
    assert fw(make(camera=cam(height=17)).h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, only(rgb=0x2000, yuv=0x3000), 3, None, None) == ARG
    assert fw(plan.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, only(yuv=0x2001), 3, None, None) == ARG and b"aligned" in L.fdm_last_error()
    assert fw(plan.h, x, fr, 2, 3, x, 3, 0.0, 0.0, None, y, 3, None, None) == ARG and b"tmpl_rows" in L.fdm_last_error()
    assert fw(plan.h, x, fr, 2, 3, None, 1, 0.0, 0.0, None, y, 3, None, None) == ARG
    assert fw(plan.h, x, fr, 2, 3, None, 0, -1.0, 30.0, None, y, 3, None, None) == ARG and b"frame rates" in L.fdm_last_error()
    assert fw(plan.h, x, fr, 0, 3, None, 0, 0.0, 0.0, None, y, 3, None, None) == SHAPE
    assert fw(plan.h, x, fr, 2, 0, None, 0, 0.0, 0.0, None, y, 3, None, None) == SHAPE
    assert fw(plan.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, y, 0, None, None) == SHAPE
    assert fw(plan.h, x, bad, 2, 3, None, 0, 0.0, 0.0, None, y, 3, None, None) == SHAPE and b"clip 1 has 4 frames" in L.fdm_last_error()
    assert fw(plan.h, x, fr, 2, 3, None, 0, 30.0, 60.0, None, y, 5, None, None) == SHAPE and b"gives 6 frames" in L.fdm_last_error()
    assert b"render_forward_planes" in L.fdm_last_error()
    if not torch.cuda.is_available():
        for planes in (y, only(alpha=0x2000), only(rgb=0x2000), only(depth=0x2000, face=0x3000), only(alpha=0x2001)):
            assert fw(plan.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, planes, 3, None, None) == STATE and b"no gfx950 device" in L.fdm_last_error()
        assert fw(odd.h, x, fr, 2, 3, None, 0, 0.0, 0.0, None, only(alpha=0x2000, rgb=0x3000), 3, None, None) == STATE      # alpha has no even-size limit


@pytest.mark.parametrize("fps,rate", [(30, "30:1"), (25.0, "25:1"), ((30000, 1001), "30000:1001"), (29.97, "2997:100")])
@pytest.mark.parametrize("full", [False, True])
def test_write_y4m(tmp_path, fps, rate, full):
    W, H, Lmax, L = 6, 4, 5, 3
    n = 3 * W * H // 2
    yuv = np.random.default_rng(3).integers(0, 256, (1, Lmax, n), dtype=np.uint8)
    path = tmp_path / "clip.y4m"
    for data in (yuv, torch.from_numpy(yuv), yuv[0]):
        size = render.write_y4m(path, data, [L], W, H, fps, full) if full else render.write_y4m(path, data, L, W, H, fps)
        raw = path.read_bytes()
        head = f"YUV4MPEG2 W6 H4 F{rate} Ip A1:1 C420jpeg XCOLORRANGE={'FULL' if full else 'LIMITED'}\n".encode()
        assert raw.startswith(head) and len(raw) == size == len(head) + L * (6 + n)
        body = raw[len(head):]
        for t in range(L):
            rec = body[t * (6 + n):(t + 1) * (6 + n)]
            assert rec[:6] == b"FRAME\n" and rec[6:] == yuv[0, t].tobytes()
    assert render.write_y4m(path, yuv, 0, W, H, fps) == len(path.read_bytes()) == len(head.replace(b"FULL", b"LIMITED"))
    for bad in (dict(yuv=yuv[:, :, :-1]), dict(yuv=yuv.astype(np.int32)), dict(frames=Lmax + 1), dict(width=5), dict(yuv=np.concatenate([yuv, yuv]))):
        a = dict(dict(yuv=yuv, frames=L, width=W, height=H), **bad)
        with pytest.raises(FdmError, match="write_y4m"):
            render.write_y4m(path, a["yuv"], a["frames"], a["width"], a["height"], fps)


def test_image_frames_defaults():
    im = render.ImageFrames(1, 2, 3, [4])
    assert im._fields == ("images", "depth", "face_ids", "frames", "alpha", "yuv") and im.alpha is None and im.yuv is None
    assert tuple(im) == (1, 2, 3, [4], None, None) and render.ImageFrames(1, 2, 3, [4], 5, yuv=6)[4:] == (5, 6)


def test_the_command_line_takes_the_planes():
    import argparse
    from fdm_amd import pipeline
    ap = argparse.ArgumentParser()
    pipeline.add_render_arguments(ap)
    a = ap.parse_args([])
    assert (a.render_alpha, a.render_yuv, a.render_yuv_matrix, a.render_yuv_full) == (False, None, 709, False)
    a = ap.parse_args(["--render_alpha", "--render_yuv", "nv12", "--render_yuv_matrix", "601", "--render_yuv_full"])
    assert (a.render_alpha, a.render_yuv, a.render_yuv_matrix, a.render_yuv_full) == (True, "nv12", 601, True)
    for bad in (["--render_yuv", "yv12"], ["--render_yuv_matrix", "2020"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
