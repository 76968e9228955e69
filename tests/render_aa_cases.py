"""The numpy restatement of the render hand-off at S = 1, 4 or 16 coverage samples per pixel (the
anti-aliasing paragraph; include/fdm_hip.h, fdm_render_set "samples").  The vertex stage, the triangle setup, the edge function, the
light sum, the 8-bit conversion and the scenes are those of tests/render_cases.py; what is restated here is everything per sample:
coverage and depth at (256 x + ox_s, 256 y + oy_s), a maximum key per sample, and the resolve that shades every sample, sums the
channels in sample order and scales by 1 / S.  Integer work is int64, float work float32 in the stated order.  The (triangle, pixel)
pairs are enumerated here on their own: every pixel column minX >> 8 .. maxX >> 8 and row minY >> 8 .. maxY >> 8 of the viewport."""
import numpy as np

import mesh_cases as MC
import render_cases as RC

F32 = np.float32
PATTERNS = {
    1: [(128, 128)],
    4: [(96, 32), (224, 96), (32, 160), (160, 224)],
    16: [(32 + 64 * i, 32 + 64 * j) for j in range(4) for i in range(4)],
}


def pattern(S):
    return np.array(PATTERNS[S], dtype=np.int64)


def fragments_at(T, k, px, py, X, Y, w):
    """For pairs (triangle T[k], sample position (px, py)): covered, l0, l1, l2, iw"""
    v0, v1, v2 = T["v0"][k], T["v1"][k], T["v2"][k]
    E0, in0 = RC.edge(X[v1], Y[v1], X[v2], Y[v2], px, py)
    E1, in1 = RC.edge(X[v2], Y[v2], X[v0], Y[v0], px, py)
    E2, in2 = RC.edge(X[v0], Y[v0], X[v1], Y[v1], px, py)
    fA = T["A"][k].astype(F32)
    with np.errstate(all="ignore"):
        l0, l1, l2 = E0.astype(F32) / fA, E1.astype(F32) / fA, E2.astype(F32) / fA
        iw = (l0 * w[v0] + l1 * w[v1]) + l2 * w[v2]
    return in0 & in1 & in2, l0, l1, l2, iw


def pairs(T, X, Y, W, H):
    """(k, x, y) of every (triangle, pixel of its conservative box) pair"""
    xs, ys = np.stack([X[T["v0"]], X[T["v1"]], X[T["v2"]]]), np.stack([Y[T["v0"]], Y[T["v1"]], Y[T["v2"]]])
    x0, x1 = np.maximum(xs.min(0) >> 8, 0), np.minimum(xs.max(0) >> 8, W - 1)
    y0, y1 = np.maximum(ys.min(0) >> 8, 0), np.minimum(ys.max(0) >> 8, H - 1)
    bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    cnt = bw * bh
    k = np.repeat(np.arange(len(cnt)), cnt)
    i = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    yy = i // np.maximum(bw[k], 1)
    return k, x0[k] + (i - yy * bw[k]), y0[k] + yy


def visibility(T, X, Y, w, W, H, S):
    """keys uint64 [H * W, S]: per sample the maximum of (bits(iw) << 32) | (0xFFFFFFFF - face) over the covering fragments; 0 = none"""
    vis = np.zeros((W * H, S), dtype=np.uint64)
    k, x, y = pairs(T, X, Y, W, H)
    for s, (ox, oy) in enumerate(pattern(S)):
        cov, _, _, _, iw = fragments_at(T, k, 256 * x + ox, 256 * y + oy, X, Y, w)
        ok = cov & (iw > 0) & np.isfinite(iw)
        key = (iw[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - T["face"][k[ok]].astype(np.uint64))
        np.maximum.at(vis[:, s], y[ok] * W + x[ok], key)
    return vis


def sample_colours(T, X, Y, w, nc, vw, keys, px, py):
    """c [n, 3] float32 of the samples at (px, py) [n] whose winning keys are `keys` [n] (all non-zero): step 5 up to min(1, c)"""
    bg = vw["background"]
    fid = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    k = np.searchsorted(T["face"], fid)
    assert (T["face"][k] == fid).all()
    cov, l0, l1, l2, iw = fragments_at(T, k, px, py, X, Y, w)
    assert cov.all() and (iw.view(np.uint32) == (keys >> np.uint64(32)).astype(np.uint32)).all()
    v = [T["v0"][k], T["v1"][k], T["v2"][k]]
    with np.errstate(all="ignore"):
        b = [(l * w[vi]) / iw for l, vi in zip((l0, l1, l2), v)]
        nn = np.stack([(b[0] * nc[v[0], j] + b[1] * nc[v[1], j]) + b[2] * nc[v[2], j] for j in range(3)], axis=1)
        s = RC.dot3(nn[:, 0], nn[:, 1], nn[:, 2], nn[:, 0], nn[:, 1], nn[:, 2])
        ok = s > 0
        nh = np.where(ok[:, None], nn / np.sqrt(np.where(ok, s, F32(1)))[:, None], F32(0)).astype(F32)
        nh = np.where((nh[:, 2] < 0)[:, None], -nh, nh)
        kk = RC.shade(nh, vw)
        assert kk.dtype == F32
        c = np.stack([vw["base"][ch] * kk for ch in range(3)], axis=1)
        c = np.where(np.isnan(c), bg[None, :], c).astype(F32)
        c = np.where(c < 1, c, F32(1))
    assert c.dtype == F32
    return c


def render_frame(p, n, faces, vw, S):
    """p, n [V, 3] float32 -> (rgb uint8 [H, W, 3], depth float32 [H, W], face int32 [H, W]) at S samples per pixel"""
    W, H = vw["W"], vw["H"]
    X, Y, w, bad, nc = RC.vertex_stage(p, n, vw)
    T = RC.setup(X, Y, w, bad, faces)
    vis = visibility(T, X, Y, w, W, H, S)
    bg = vw["background"].astype(F32)
    acc = None
    for s, (ox, oy) in enumerate(pattern(S)):
        c = np.empty((W * H, 3), dtype=F32)
        c[:] = bg
        hit = np.nonzero(vis[:, s])[0]
        if len(hit):
            c[hit] = sample_colours(T, X, Y, w, nc, vw, vis[hit, s], 256 * (hit % W) + ox, 256 * (hit // W) + oy)
        acc = c if acc is None else acc + c          # ascending s, one rounded addition each
    assert acc.dtype == F32
    mean = acc * F32(1.0 / S)
    rgb = np.stack([RC.to_u8(mean[:, ch], bg[ch]) for ch in range(3)], axis=1)
    best = vis.max(axis=1)
    any_ = best != 0
    depth, face = np.zeros(W * H, dtype=F32), np.full(W * H, -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        depth[any_] = F32(1) / (best[any_] >> np.uint64(32)).astype(np.uint32).view(F32)
    face[any_] = (np.uint64(0xFFFFFFFF) - (best[any_] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return rgb.reshape(H, W, 3), depth.reshape(H, W), face.reshape(H, W)


def coverage(p, faces, vw, S):
    """bool [H, W, S]: which samples have a fragment (one frame of vertices p, item 18's normals are not needed)"""
    X, Y, w, bad, _ = RC.vertex_stage(np.asarray(p, F32), np.zeros_like(np.asarray(p, F32)), vw)
    T = RC.setup(X, Y, w, bad, faces)
    return (visibility(T, X, Y, w, vw["W"], vw["H"], S) != 0).reshape(vw["H"], vw["W"], S)


def render_static(p, faces, vw, S):
    """One frame of vertices p [V, 3] with item 18's normals."""
    p = np.asarray(p, dtype=F32)
    with np.errstate(all="ignore"):
        n = MC.normals(p.reshape(1, -1), faces, len(p))[0]
    return render_frame(p, n, faces, vw, S)


def render_clips(off, tmpl, frames, fps, faces, V, vw, S):
    """list over clips of (rgb [L_out, H, W, 3], depth [L_out, H, W], face [L_out, H, W]), as render_cases.render_clips"""
    out = []
    H, W = vw["H"], vw["W"]
    for p in MC.positions(off, tmpl, frames, fps):
        with np.errstate(all="ignore"):
            n = MC.normals(p, faces, V) if len(p) else np.zeros((0, V, 3), F32)
        fr = [render_frame(p[t].reshape(V, 3), n[t], faces, vw, S) for t in range(len(p))]
        out.append((np.stack([f[0] for f in fr]) if fr else np.zeros((0, H, W, 3), np.uint8),
                    np.stack([f[1] for f in fr]) if fr else np.zeros((0, H, W), F32),
                    np.stack([f[2] for f in fr]) if fr else np.zeros((0, H, W), np.int32)))
    return out
