"""The numpy restatement of the planes of the render hand-off (include/fdm_hip.h,
fdm_render_forward_planes): the alpha plane from the per-sample coverage of tests/render_aa_cases.py, the ten fixed-point numbers of
fdm_render_yuv_coeffs_host, and the Y'CbCr 4:2:0 planes (I420 or NV12) of a frame's uint8 rgb.  Everything is integer work: int64 here,
which holds every value the device's int32 holds (the largest product sum is 6.7e7)."""
import math

import numpy as np

import render_aa_cases as RA
import render_cases as RC  # noqa: F401  (the scenes and views the tests of the planes use)

TABLES = {  # (matrix, full range): yr yg yb ur ug ub vr vg vb y0, as the header prints them
    (601, False): (16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, 16),
    (601, True): (19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329, 0),
    (709, False): (11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639, 16),
    (709, True): (13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005, 0),
}
LAYOUTS = ("i420", "nv12")


def coeffs(matrix, full):
    """int64 [10] from the definition (fp64, q(x) = floor(65536 x + 0.5))"""
    Kr, Kb = {601: (0.299, 0.114), 709: (0.2126, 0.0722)}[matrix]
    sy, sc = (1.0, 1.0) if full else (219.0 / 255.0, 224.0 / 255.0)
    q = lambda x: int(math.floor(65536.0 * x + 0.5))  # noqa: E731
    yr, yb = q(Kr * sy), q(Kb * sy)
    yg = q(sy) - yr - yb
    ub, ur = q(sc / 2), q(-Kr * sc / (2 * (1 - Kb)))
    vr, vb = q(sc / 2), q(-Kb * sc / (2 * (1 - Kr)))
    return np.array([yr, yg, yb, ur, -(ur + ub), ub, vr, -(vr + vb), vb, 0 if full else 16], dtype=np.int64)


def alpha(cov):
    """cov bool [..., S] (render_aa_cases.coverage) -> uint8 [...]: (255 n + S / 2) / S in integers"""
    S = cov.shape[-1]
    n = cov.sum(axis=-1).astype(np.int64)
    return ((255 * n + S // 2) // S).astype(np.uint8)


def alpha_of(p, faces, vw, S):
    return alpha(RA.coverage(p, faces, vw, S))


def luma(rgb, k):
    """rgb integer [..., 3] -> int64 [...] (clamped)"""
    c = rgb.astype(np.int64)
    return np.clip(((k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2] + 32768) >> 16) + k[9], 0, 255)


def chroma(sums, k, before_clamp=False):
    """sums integer [..., 3] = the four pixels of a 2 x 2 block added per channel -> (U, V) int64 [...]"""
    s = sums.astype(np.int64)
    u = ((k[3] * s[..., 0] + k[4] * s[..., 1] + k[5] * s[..., 2] + (1 << 17)) >> 18) + 128
    v = ((k[6] * s[..., 0] + k[7] * s[..., 1] + k[8] * s[..., 2] + (1 << 17)) >> 18) + 128
    return (u, v) if before_clamp else (np.clip(u, 0, 255), np.clip(v, 0, 255))


def yuv(rgb, k, layout):
    """rgb uint8 [H, W, 3] (H, W even) -> the frame's 3 W H / 2 bytes: Y [H][W], then U [H/2][W/2] and V [H/2][W/2] (i420) or
    [H/2][W/2][2] interleaved U, V (nv12)"""
    H, W = rgb.shape[:2]
    assert H % 2 == 0 and W % 2 == 0 and rgb.dtype == np.uint8 and layout in LAYOUTS
    k = np.asarray(k, dtype=np.int64)
    Y = luma(rgb, k)
    sums = rgb.astype(np.int64).reshape(H // 2, 2, W // 2, 2, 3).sum(axis=(1, 3))
    U, V = chroma(sums, k)
    tail = [U.ravel(), V.ravel()] if layout == "i420" else [np.stack([U, V], axis=-1).ravel()]
    return np.concatenate([Y.ravel()] + tail).astype(np.uint8).tobytes()


def yuv_frames(rgb, k, layout):
    """rgb uint8 [L, H, W, 3] -> uint8 [L, 3 W H / 2]"""
    L, H, W = rgb.shape[:3]
    return np.stack([np.frombuffer(yuv(f, k, layout), np.uint8) for f in rgb]) if L else np.zeros((0, 3 * W * H // 2), np.uint8)
