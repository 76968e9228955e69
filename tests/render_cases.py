"""Scenes, views and the numpy restatement of the render hand-off (include/fdm_hip.h, fdm_render_*).
Integer work is int64; float work is float32 in exactly the stated order (every numpy float32 operation is one rounded IEEE operation:
no contraction).  Coverage, depth and resolve are vectorised over every (triangle, pixel of its clamped box) pair of a frame, so an
800 x 800 frame of 10k faces takes about a second.  Positions and vertex normals are those of tests/mesh_cases.py (item 18)."""
import functools
import math

import numpy as np

import mesh_cases as MC

F32 = np.float32
SNAP_MAX = 1 << 20
PAIRS = 1 << 22          # (triangle, pixel) pairs worked on at a time


# ---- views: plain dicts of what fdm_render_create reads
def reference_lights(intensity=0.5):
    s, c = math.sin(math.pi / 6.0), math.cos(math.pi / 6.0)
    d = [(0.0, 0.0, 1.0), (0.0, -s, c), (0.0, s, c), (-s, 0.0, c), (s, 0.0, c)]
    return np.array([x + (intensity,) for x in d], dtype=F32)


def eight_lights():
    """the five defaults and three more from below and the sides, all unit vectors"""
    extra = np.array([(0.6, 0.0, 0.8, 0.25), (0.0, -0.6, 0.8, 0.125), (-0.28, 0.0, 0.96, 0.375)], dtype=F32)
    return np.concatenate([reference_lights(0.25), extra])


def view(W, H, f=None, c=None, near=0.01, far=3.0, R=None, t=(0.0, 0.0, -1.0), lights="default", ambient=0.2, base=(0.3, 0.3, 0.3),
         background=(1.0, 1.0, 1.0)):
    f = (0.75 * W, 0.75 * W) if f is None else ((f, f) if np.isscalar(f) else f)
    c = (W / 2.0, H / 2.0) if c is None else c
    lt = reference_lights() if isinstance(lights, str) else np.asarray(lights, dtype=F32).reshape(-1, 4)
    return dict(W=int(W), H=int(H), fx=F32(f[0]), fy=F32(f[1]), cx=F32(c[0]), cy=F32(c[1]), near=F32(near), far=F32(far),
                R=np.eye(3, dtype=F32) if R is None else np.asarray(R, dtype=F32).reshape(3, 3), t=np.asarray(t, dtype=F32),
                lights=lt, ambient=F32(ambient), base=np.asarray(base, dtype=F32), background=np.asarray(background, dtype=F32))


def rot_y(a):
    s, c = math.sin(a), math.cos(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=F32)


# ---- scenes: (vertices float32 [V, 3], faces int32 [F, 3]); the camera of view() stands at z = +1 and looks down -z
def pixel_to_world(vw, x, y, d=1.0):
    """the world point (camera R = I) whose screen coordinates are (x, y) pixels at distance d, in double"""
    return ((x - float(vw["cx"])) * d / float(vw["fx"]) - float(vw["t"][0]), (float(vw["cy"]) - y) * d / float(vw["fy"]) - float(vw["t"][1]),
            -d - float(vw["t"][2]))


def tris(points, faces):
    return np.asarray(points, dtype=F32).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)


def icosphere(level=2, radius=0.3):
    """a closed sphere of 20 * 4^level faces (320 at level 2), outward orientation"""
    g = (1 + math.sqrt(5)) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return tris(radius * np.array(v), f)


def grid_head(n=5023, half=0.11):
    """the V = 5023 grid of mesh_cases scaled into [-half, half]^2 and bent over a dome: about 9.9k faces"""
    faces, V, xyz = MC.mesh("vocaset_size")
    lo, hi = xyz[:, :2].min(0), xyz[:, :2].max(0)
    xy = (xyz[:, :2] - (lo + hi) / 2) / (hi - lo).max() * 2 * half
    z = 0.08 * np.cos(xy[:, 0] / half * 1.3) * np.cos(xy[:, 1] / half * 1.3) + 0.3 * (xyz[:, 2] - xyz[:, 2].mean()) * 0.06
    return np.concatenate([xy, z[:, None]], axis=1).astype(F32), faces


def strip(F):
    """F triangles over F + 2 vertices in a zigzag band that crosses the view, slightly tilted in depth"""
    i = np.arange(F + 2)
    x = -0.45 + 0.9 * i / (F + 1)
    p = np.stack([x, np.where(i % 2 == 0, -0.12, 0.13) + 0.05 * np.sin(7 * x), 0.1 * x], axis=1)
    return tris(p, [(k, k + 1, k + 2) for k in range(F)])


# ---- the definition
def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def vertex_stage(p, n, vw):
    """p, n [V, 3] float32 -> X, Y int64 [V], w float32 [V], bad bool [V], nc float32 [V, 3]"""
    with np.errstate(all="ignore"):
        R, t = vw["R"], vw["t"]
        pc = [dot3(R[k, 0], R[k, 1], R[k, 2], p[:, 0], p[:, 1], p[:, 2]) + t[k] for k in range(3)]
        d = -pc[2]
        w = F32(1) / d
        sx = vw["fx"] * (pc[0] * w) + vw["cx"]
        sy = vw["cy"] - vw["fy"] * (pc[1] * w)
        rx, ry = np.rint(F32(256) * sx), np.rint(F32(256) * sy)
        bad = ~(np.isfinite(p).all(axis=1) & np.isfinite(d) & np.isfinite(sx) & np.isfinite(sy))
        bad |= ~(d > vw["near"]) | ~(d < vw["far"]) | ~(np.abs(rx) <= F32(SNAP_MAX)) | ~(np.abs(ry) <= F32(SNAP_MAX))
        X = np.where(bad, 0, np.where(bad, F32(0), rx)).astype(np.int64)
        Y = np.where(bad, 0, np.where(bad, F32(0), ry)).astype(np.int64)
        nc = np.stack([dot3(R[k, 0], R[k, 1], R[k, 2], n[:, 0], n[:, 1], n[:, 2]) for k in range(3)], axis=1)
    assert w.dtype == F32 and nc.dtype == F32
    return X, Y, w, bad, nc


def setup(X, Y, w, bad, faces):
    """The oriented triangles that survive: dict of per-triangle arrays (face index, vertex ids v0 v1 v2, A > 0)."""
    a, b, c = faces[:, 0].astype(np.int64), faces[:, 1].astype(np.int64), faces[:, 2].astype(np.int64)
    A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
    keep = ~(bad[a] | bad[b] | bad[c]) & (A != 0)
    sw = A < 0
    v1, v2 = np.where(sw, c, b), np.where(sw, b, c)
    f = np.nonzero(keep)[0]
    return dict(face=f, v0=a[f], v1=v1[f], v2=v2[f], A=np.abs(A[f]))


def edge(Xa, Ya, Xb, Yb, px, py):
    """E of the edge a -> b at (px, py) and whether the point is on the triangle's side of it, top-left rule on the snapped edge vector"""
    dx, dy = Xb - Xa, Yb - Ya
    E = dx * (py - Ya) - dy * (px - Xa)
    return E, (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def fragments(T, k, x, y, X, Y, w):
    """For pairs (triangle T[k], pixel (x, y)): covered, l0, l1, l2, iw"""
    v0, v1, v2 = T["v0"][k], T["v1"][k], T["v2"][k]
    px, py = 256 * x + 128, 256 * y + 128
    E0, in0 = edge(X[v1], Y[v1], X[v2], Y[v2], px, py)
    E1, in1 = edge(X[v2], Y[v2], X[v0], Y[v0], px, py)
    E2, in2 = edge(X[v0], Y[v0], X[v1], Y[v1], px, py)
    fA = T["A"][k].astype(F32)
    with np.errstate(all="ignore"):
        l0, l1, l2 = E0.astype(F32) / fA, E1.astype(F32) / fA, E2.astype(F32) / fA
        iw = (l0 * w[v0] + l1 * w[v1]) + l2 * w[v2]
    return in0 & in1 & in2, l0, l1, l2, iw


def boxes(T, X, Y, W, H):
    xs, ys = np.stack([X[T["v0"]], X[T["v1"]], X[T["v2"]]]), np.stack([Y[T["v0"]], Y[T["v1"]], Y[T["v2"]]])
    x0, x1 = np.maximum((xs.min(0) + 127) >> 8, 0), np.minimum((xs.max(0) - 128) >> 8, W - 1)
    y0, y1 = np.maximum((ys.min(0) + 127) >> 8, 0), np.minimum((ys.max(0) - 128) >> 8, H - 1)
    bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    return x0, y0, bw, bw * bh


def visibility(T, X, Y, w, W, H):
    """keys uint64 [H * W]: (bits(iw) << 32) | (0xFFFFFFFF - face), the maximum over the covering fragments; 0 = none"""
    vis = np.zeros(W * H, dtype=np.uint64)
    x0, y0, bw, npix = boxes(T, X, Y, W, H)
    order = np.nonzero(npix > 0)[0]
    at = 0
    while at < len(order):
        cum = np.cumsum(npix[order[at:]])
        m = max(1, int(np.searchsorted(cum, PAIRS, side="right")))
        ks = order[at:at + m]
        at += m
        cnt = npix[ks]
        k = np.repeat(ks, cnt)
        i = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        yy = i // bw[k]
        x, y = x0[k] + (i - yy * bw[k]), y0[k] + yy
        cov, _, _, _, iw = fragments(T, k, x, y, X, Y, w)
        ok = cov & (iw > 0) & np.isfinite(iw)
        key = (iw[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - T["face"][k[ok]].astype(np.uint64))
        np.maximum.at(vis, (y[ok] * W + x[ok]), key)
    return vis


def to_u8(c, bg):
    with np.errstate(all="ignore"):
        c = np.where(np.isnan(c), bg, c).astype(F32)
        c = np.where(c < 1, c, F32(1))
        return (F32(255) * c + F32(0.5)).astype(np.int32).astype(np.uint8)


def shade(nh, vw):
    """k [n] for unit normals nh [n, 3] (already flipped towards the camera)"""
    k = np.full(len(nh), vw["ambient"], dtype=F32)
    for l in vw["lights"]:
        d = dot3(nh[:, 0], nh[:, 1], nh[:, 2], l[0], l[1], l[2])
        k = k + l[3] * np.where(d > 0, d, F32(0))
    return k


def render_frame(p, n, faces, vw):
    """p, n [V, 3] float32 -> (rgb uint8 [H, W, 3], depth float32 [H, W], face int32 [H, W])"""
    W, H = vw["W"], vw["H"]
    X, Y, w, bad, nc = vertex_stage(p, n, vw)
    T = setup(X, Y, w, bad, faces)
    vis = visibility(T, X, Y, w, W, H)
    bg = vw["background"]
    rgb = np.empty((H * W, 3), dtype=np.uint8)
    rgb[:] = to_u8(bg, bg)
    depth, face = np.zeros(H * W, dtype=F32), np.full(H * W, -1, dtype=np.int32)
    hit = np.nonzero(vis)[0]
    if len(hit):
        fid = (np.uint64(0xFFFFFFFF) - (vis[hit] & np.uint64(0xFFFFFFFF))).astype(np.int64)
        k = np.searchsorted(T["face"], fid)
        assert (T["face"][k] == fid).all()
        cov, l0, l1, l2, iw = fragments(T, k, hit % W, hit // W, X, Y, w)
        assert cov.all() and (iw.view(np.uint32) == (vis[hit] >> np.uint64(32)).astype(np.uint32)).all()
        v = [T["v0"][k], T["v1"][k], T["v2"][k]]
        with np.errstate(all="ignore"):
            b = [(l * w[vi]) / iw for l, vi in zip((l0, l1, l2), v)]
            nn = np.stack([(b[0] * nc[v[0], j] + b[1] * nc[v[1], j]) + b[2] * nc[v[2], j] for j in range(3)], axis=1)
            s = dot3(nn[:, 0], nn[:, 1], nn[:, 2], nn[:, 0], nn[:, 1], nn[:, 2])
            ok = s > 0
            nh = np.where(ok[:, None], nn / np.sqrt(np.where(ok, s, F32(1)))[:, None], F32(0)).astype(F32)
            nh = np.where((nh[:, 2] < 0)[:, None], -nh, nh)
            kk = shade(nh, vw)
            assert kk.dtype == F32
            for ch in range(3):
                rgb[hit, ch] = to_u8(vw["base"][ch] * kk, bg[ch])
            depth[hit] = F32(1) / iw
        face[hit] = fid
    return rgb.reshape(H, W, 3), depth.reshape(H, W), face.reshape(H, W)


def render_static(p, faces, vw):
    """One frame of vertices p [V, 3] with item 18's normals."""
    p = np.asarray(p, dtype=F32)
    with np.errstate(all="ignore"):
        n = MC.normals(p.reshape(1, -1), faces, len(p))[0]
    return render_frame(p, n, faces, vw)


def render_clips(off, tmpl, frames, fps, faces, V, vw):
    """list over clips of (rgb [L_out, H, W, 3], depth [L_out, H, W], face [L_out, H, W]).  off [B, L_max, 3 V], tmpl [1 or B, 3 V] or None."""
    out = []
    for p in MC.positions(off, tmpl, frames, fps):
        with np.errstate(all="ignore"):
            n = MC.normals(p, faces, V) if len(p) else np.zeros((0, V, 3), F32)
        fr = [render_frame(p[t].reshape(V, 3), n[t], faces, vw) for t in range(len(p))]
        H, W = vw["H"], vw["W"]
        out.append((np.stack([f[0] for f in fr]) if fr else np.zeros((0, H, W, 3), np.uint8),
                    np.stack([f[1] for f in fr]) if fr else np.zeros((0, H, W), F32),
                    np.stack([f[2] for f in fr]) if fr else np.zeros((0, H, W), np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def head_case():
    """The 800 x 800 case: 2 frames of the grid head under the vocaset camera; (off [1, 2, 3 V], tmpl [1, 3 V], faces, view, reference)"""
    P, faces = grid_head()
    V = len(P)
    off = (2e-3 * np.random.default_rng(77).standard_normal((1, 2, 3 * V))).astype(F32)
    vw = view(800, 800, f=4754.97941935 / 2, c=(400.0, 400.0))
    tmpl = P.reshape(1, -1)
    return off, tmpl, faces, vw, render_clips(off, tmpl, [2], None, faces, V, vw)
