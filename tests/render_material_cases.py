"""The numpy restatement of the render hand-off's materials at S = 1, 4 or 16 samples per pixel (DESIGN.md section 2 item 25;
include/fdm_hip.h, fdm_render_set_material).  Everything but the colour m that stands where `base` stands is tests/render_cases.py and
tests/render_aa_cases.py as they are: the vertex stage, the setup, coverage, keys, the light sum, the sample sum and the 8-bit
conversion.  A material here is a plain dict: kind (0 base, 1 vertex colours, 2 scalar map, 3 texture), unlit, and colors [V, 3] |
lut [N, 3], lo, hi | uv [F, 3, 2], tex [Ht, Wt, 3] uint8, filter ("nearest" | "bilinear").  Float work is float32 in the stated
order; fmax and fmin are np.fmax and np.fmin (the operand that is not NaN)."""
import numpy as np

import mesh_cases as MC
import render_aa_cases as RA
import render_cases as RC

F32 = np.float32


def base(unlit=False):
    return dict(kind=0, unlit=unlit)


def vertex_colors(c, unlit=False):
    return dict(kind=1, unlit=unlit, colors=np.asarray(c, F32))


def scalar_map(lut, lo, hi, unlit=False):
    return dict(kind=2, unlit=unlit, lut=np.asarray(lut, F32), lo=F32(lo), hi=F32(hi))


def texture(tex, uv, filter="bilinear", unlit=False):  # noqa: A002
    return dict(kind=3, unlit=unlit, tex=np.asarray(tex, np.uint8), uv=np.asarray(uv, F32), filter=filter)


def interp(b, a0, a1, a2):
    return (b[0] * a0 + b[1] * a1) + b[2] * a2


def clamp(x, lo, hi):
    return np.fmin(np.fmax(x, F32(lo)), F32(hi))


def unit_scalars(s, mat):
    """u_v [V] float32 of one output frame's scalars s [V]"""
    with np.errstate(all="ignore"):
        return clamp((s.astype(F32) - mat["lo"]) / (mat["hi"] - mat["lo"]), 0, 1).astype(F32)


def resample(sc, frames, fps):
    """list over clips of [L_out, V]: the scalar field on the output frames (item 18's rule, no template; rows past frames[b] unread)"""
    return MC.positions(sc, None, frames, fps)


def texel(tex, col, row):
    return tex[row, col].astype(F32) / F32(255)


def lerp(a, b, f):
    return a + f * (b - a)


def material_colour(mat, vw, b, v, fid, swapped, u):
    """m [n, 3] float32 for n fragments: weights b (three [n]), oriented vertex ids v (three [n]), face ids fid [n], swapped [n], u [V]"""
    n = len(fid)
    with np.errstate(all="ignore"):
        if mat["kind"] == 0:
            return np.broadcast_to(vw["base"].astype(F32), (n, 3)).copy()
        if mat["kind"] == 1:
            c = mat["colors"]
            return np.stack([interp(b, c[v[0], ch], c[v[1], ch], c[v[2], ch]) for ch in range(3)], axis=1).astype(F32)
        if mat["kind"] == 2:
            lut = mat["lut"]
            N = len(lut)
            uu = clamp(interp(b, u[v[0]], u[v[1]], u[v[2]]), 0, 1).astype(F32)
            x = uu * F32(N - 1)
            i = np.minimum(x.astype(np.int64), N - 2)
            f = x - i.astype(F32)
            return np.stack([lerp(lut[i, ch], lut[i + 1, ch], f) for ch in range(3)], axis=1).astype(F32)
        uv, tex = mat["uv"], mat["tex"]
        Ht, Wt = tex.shape[:2]
        k1, k2 = np.where(swapped, 2, 1), np.where(swapped, 1, 2)
        q = [uv[fid, 0], uv[fid, k1], uv[fid, k2]]
        tu, tv = interp(b, q[0][:, 0], q[1][:, 0], q[2][:, 0]), interp(b, q[0][:, 1], q[1][:, 1], q[2][:, 1])
        assert tu.dtype == F32 and tv.dtype == F32
        if mat["filter"] == "nearest":
            col = clamp(np.floor(tu * F32(Wt)), 0, Wt - 1).astype(np.int64)
            row = clamp(np.floor((F32(1) - tv) * F32(Ht)), 0, Ht - 1).astype(np.int64)
            return texel(tex, col, row)
        x, y = tu * F32(Wt) - F32(0.5), (F32(1) - tv) * F32(Ht) - F32(0.5)
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        c0, c1 = clamp(x0, 0, Wt - 1).astype(np.int64), clamp(x0 + F32(1), 0, Wt - 1).astype(np.int64)
        r0, r1 = clamp(y0, 0, Ht - 1).astype(np.int64), clamp(y0 + F32(1), 0, Ht - 1).astype(np.int64)
        top = lerp(texel(tex, c0, r0), texel(tex, c1, r0), fx)
        bot = lerp(texel(tex, c0, r1), texel(tex, c1, r1), fx)
        m = lerp(top, bot, fy)
        assert m.dtype == F32
        return m


def sample_colours(T, X, Y, w, nc, vw, mat, u, faces, keys, px, py):
    """c [n, 3] float32 of the samples at (px, py) [n] whose winning keys are `keys` [n]: step 5 up to min(1, c), with m for base"""
    bg = vw["background"]
    fid = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    k = np.searchsorted(T["face"], fid)
    assert (T["face"][k] == fid).all()
    cov, l0, l1, l2, iw = RA.fragments_at(T, k, px, py, X, Y, w)
    assert cov.all() and (iw.view(np.uint32) == (keys >> np.uint64(32)).astype(np.uint32)).all()
    v = [T["v0"][k], T["v1"][k], T["v2"][k]]
    a, bb, cc = (faces[fid, j].astype(np.int64) for j in range(3))
    swapped = ((X[bb] - X[a]) * (Y[cc] - Y[a]) - (Y[bb] - Y[a]) * (X[cc] - X[a])) < 0
    with np.errstate(all="ignore"):
        b = [(l * w[vi]) / iw for l, vi in zip((l0, l1, l2), v)]
        if mat["unlit"]:
            kk = np.ones(len(fid), F32)
        else:
            nn = np.stack([(b[0] * nc[v[0], j] + b[1] * nc[v[1], j]) + b[2] * nc[v[2], j] for j in range(3)], axis=1)
            s = RC.dot3(nn[:, 0], nn[:, 1], nn[:, 2], nn[:, 0], nn[:, 1], nn[:, 2])
            ok = s > 0
            nh = np.where(ok[:, None], nn / np.sqrt(np.where(ok, s, F32(1)))[:, None], F32(0)).astype(F32)
            nh = np.where((nh[:, 2] < 0)[:, None], -nh, nh)
            kk = RC.shade(nh, vw)
        m = material_colour(mat, vw, b, v, fid, swapped, u)
        assert kk.dtype == F32 and m.dtype == F32
        c = m * kk[:, None]
        c = np.where(np.isnan(c), bg[None, :], c).astype(F32)
        c = np.where(c < 1, c, F32(1))
    assert c.dtype == F32
    return c


def render_frame(p, n, faces, vw, S, mat, s=None):
    """p, n [V, 3] float32, s [V] the output frame's scalars (kind 2) -> (rgb uint8 [H, W, 3], depth [H, W], face [H, W], alpha [H, W])"""
    W, H = vw["W"], vw["H"]
    X, Y, w, bad, nc = RC.vertex_stage(p, n, vw)
    T = RC.setup(X, Y, w, bad, faces)
    vis = RA.visibility(T, X, Y, w, W, H, S)
    u = unit_scalars(np.asarray(s, F32), mat) if mat["kind"] == 2 else None
    bg = vw["background"].astype(F32)
    acc = None
    for si, (ox, oy) in enumerate(RA.pattern(S)):
        c = np.empty((W * H, 3), dtype=F32)
        c[:] = bg
        hit = np.nonzero(vis[:, si])[0]
        if len(hit):
            c[hit] = sample_colours(T, X, Y, w, nc, vw, mat, u, faces, vis[hit, si], 256 * (hit % W) + ox, 256 * (hit // W) + oy)
        acc = c if acc is None else acc + c
    mean = acc * F32(1.0 / S)
    rgb = np.stack([RC.to_u8(mean[:, ch], bg[ch]) for ch in range(3)], axis=1)
    best = vis.max(axis=1)
    any_ = best != 0
    depth, face = np.zeros(W * H, dtype=F32), np.full(W * H, -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        depth[any_] = F32(1) / (best[any_] >> np.uint64(32)).astype(np.uint32).view(F32)
    face[any_] = (np.uint64(0xFFFFFFFF) - (best[any_] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    cnt = (vis != 0).sum(axis=1)
    alpha = ((255 * cnt + S // 2) // S).astype(np.uint8)
    return rgb.reshape(H, W, 3), depth.reshape(H, W), face.reshape(H, W), alpha.reshape(H, W)


def render_static(p, faces, vw, S, mat, s=None):
    """One frame of vertices p [V, 3] with item 18's normals."""
    p = np.asarray(p, dtype=F32)
    with np.errstate(all="ignore"):
        n = MC.normals(p.reshape(1, -1), faces, len(p))[0]
    return render_frame(p, n, faces, vw, S, mat, s)


def render_clips(off, tmpl, frames, fps, faces, V, vw, S, mat, sc=None):
    """list over clips of (rgb [L_out, H, W, 3], depth, face, alpha); sc [B, L_max, V]: the scalar field on the input frames (kind 2)"""
    out = []
    H, W = vw["H"], vw["W"]
    ss = resample(sc, frames, fps) if sc is not None else None
    for b, p in enumerate(MC.positions(off, tmpl, frames, fps)):
        with np.errstate(all="ignore"):
            n = MC.normals(p, faces, V) if len(p) else np.zeros((0, V, 3), F32)
        fr = [render_frame(p[t].reshape(V, 3), n[t], faces, vw, S, mat, None if ss is None else ss[b][t]) for t in range(len(p))]
        empty = (np.zeros((0, H, W, 3), np.uint8), np.zeros((0, H, W), F32), np.zeros((0, H, W), np.int32), np.zeros((0, H, W), np.uint8))
        out.append(tuple(np.stack([f[i] for f in fr]) for i in range(4)) if fr else empty)
    return out


def vertex_dist(a, b):
    """[rows, V] float32 of a, b [rows, 3 V]"""
    with np.errstate(all="ignore"):
        d = (a.astype(F32) - b.astype(F32)).reshape(a.shape[0], -1, 3)
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(F32)
