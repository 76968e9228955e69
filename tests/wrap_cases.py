"""Sources, target sets and the two restatements of the wrap hand-off tests (include/fdm_hip.h, fdm_wrap_*).
Topologies and seeded inputs come from tests/mesh_cases.py.  The float32 restatement is the header's definition in numpy float32 in
exactly the stated order (every numpy float32 operation is one rounded IEEE operation), vectorised over (Vt, F) with np.where for the
region walk; it refuses subnormal intermediates as mesh_cases._normal does.  The float64 restatement is the same expression in double."""
import functools

import numpy as np

import mesh_cases as MC
from fdm_amd.wrap import FACE_TILE

SOURCES = ["grid", "fan", "strip", "degenerate", "grid_extra"]
CUTS = [1, 63, 64, 65, 257]
REGIONS = ["vertex a", "vertex b", "edge ab", "vertex c", "edge ac", "edge bc", "interior"]


# ---- sources: name -> (rest S float32 [V, 3], faces int32 [F, 3])
@functools.lru_cache(maxsize=None)
def source(name):
    if name == "one_face":                  # F = 1: face 0 of the grid
        S, f = source("grid")
        return S, f[:1].copy()
    if name == "ridge":                     # two wings under a shared edge (0, 1); dyadic coordinates: the two distances tie exactly
        S = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, -1], [0.5, -1, -1]], dtype=np.float32)
        return S, np.array([[0, 1, 2], [3, 0, 1]], dtype=np.int32)        # the shared edge is ab of face 0 and bc of face 1
    if name.startswith("tile"):             # tile-1 / tile+0 / tile+1: that many faces of a 20 x 20 grid_like mesh
        f, V, xyz = MC.grid_like(400)
        return xyz.astype(np.float32), f[:FACE_TILE + int(name[4:])].copy()
    if name == "vocaset_size":              # F of several splits of the search, each of several tiles
        f, V, xyz = MC.mesh(name)
        return xyz.astype(np.float32), f
    faces, V, _ = MC.mesh(name)
    return MC.template(name, seed=0, rows=1)[0].reshape(V, 3), faces


def _face_frames(S, faces):
    """float64 (a, e1, e2, unit normal, mean edge length) of the faces with area"""
    a, b, c = (S[faces[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1)
    ok = ln > 0
    return a[ok], (b - a)[ok], (c - a)[ok], n[ok] / ln[ok, None], (np.linalg.norm(b - a, axis=1)[ok] + np.linalg.norm(c - a, axis=1)[ok]) / 2


@functools.lru_cache(maxsize=None)
def targets(name, kind, n=257):
    """T float32 [Vt, 3] over source `name`.  own: the source's vertices; lifted: n points spread over the faces (every other one
    starting outside its face) and lifted off the surface by signed heights of the order of an edge (cut to its first k points for the
    Vt cases); regions: one point in each of the
    seven regions of face 0; ties: points whose closest point lies on the shared edge of `ridge`, at the same distance from both."""
    S, faces = source(name)
    if kind == "own":
        return S.copy()
    if kind == "lifted":
        a, e1, e2, nh, edge = _face_frames(S, faces)
        g = np.random.default_rng(3000 + len(S))
        k = np.arange(n) % len(a)
        uv = g.random((n, 2))
        uv = np.where(uv.sum(1, keepdims=True) > 1, 1 - uv, uv)
        uv = np.where((np.arange(n) % 2 == 1)[:, None], 1.6 * uv - 0.3, uv)      # every other point starts outside its face: edges, corners
        h = g.choice([-1.0, 1.0], n) * (0.25 + 0.75 * g.random(n)) * edge[k]
        return (a[k] + uv[:, :1] * e1[k] + uv[:, 1:] * e2[k] + h[:, None] * nh[k]).astype(np.float32)
    if kind == "regions":
        a, e1, e2, nh, edge = (x[0] for x in _face_frames(S, faces[:1]))
        b, c, m = a + e1, a + e2, a + (e1 + e2) / 3
        pts = [a + 0.5 * (a - m), b + 0.5 * (b - m), (a + b) / 2 + 0.3 * ((a + b) / 2 - c), c + 0.5 * (c - m),
               (a + c) / 2 + 0.3 * ((a + c) / 2 - b), (b + c) / 2 + 0.3 * ((b + c) / 2 - a), m]
        return (np.array(pts) + 0.5 * edge * nh).astype(np.float32)
    if kind == "ties":
        assert name == "ridge"
        return np.array([[0.5, 0, 1], [0.5, 0, 2], [0.5, 0, 0.5], [0.25, 0, 1], [0.75, 0, 0.25]], dtype=np.float32)
    raise KeyError(kind)


# every (source, target kind, Vt) the search is checked on
SEARCH_CASES = list(dict.fromkeys(
    [(s, "own", None) for s in SOURCES] + [(s, "lifted", 257) for s in SOURCES] + [("grid", "lifted", k) for k in CUTS] +
    [("one_face", "regions", None), ("ridge", "ties", None), ("one_face", "lifted", 65)] +
    [(f"tile{d:+d}", "lifted", 65) for d in (-1, 0, 1)] + [("vocaset_size", "lifted", 257)]))


def case(name, kind, k):
    """(S, faces, T) of a search case"""
    S, faces = source(name)
    T = targets(name, kind) if k is None else targets(name, kind)[:k]
    return S, faces, np.ascontiguousarray(T)


# ---- the definition
def _ops(dt):
    N = lambda x: MC._normal(x, dt)  # noqa: E731
    sub = lambda x, y: N(x - y)  # noqa: E731
    m = lambda x, y: N(x * y)  # noqa: E731
    dot = lambda x, y: N(N(m(x[..., 0], y[..., 0]) + m(x[..., 1], y[..., 1])) + m(x[..., 2], y[..., 2]))  # noqa: E731
    pms = lambda x, y, z, w: N(m(x, y) - m(z, w))  # noqa: E731
    cross = lambda x, y: np.stack([pms(x[..., 1], y[..., 2], x[..., 2], y[..., 1]), pms(x[..., 2], y[..., 0], x[..., 0], y[..., 2]),  # noqa: E731
                                   pms(x[..., 0], y[..., 1], x[..., 1], y[..., 0])], axis=-1)
    return N, sub, m, dot, pms, cross


def walk(q, a, b, c, dt=np.float32):
    """(dist2, region code) of the region walk for q against triangles (a, b, c), arrays [..., 3] that broadcast against each other"""
    N, sub, m, dot, pms, _ = _ops(dt)
    ab, ac, bc = sub(b, a), sub(c, a), sub(c, b)
    ap, bp, cp = sub(q, a), sub(q, b), sub(q, c)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = pms(d1, d4, d3, d2), pms(d5, d2, d1, d6), pms(d3, d6, d5, d4)
    d43, d56 = N(d4 - d3), N(d5 - d6)
    rA = (d1 <= 0) & (d2 <= 0)
    rB = ~rA & (d3 >= 0) & (d4 <= d3)
    rAB = ~rA & ~rB & (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    v01 = rA | rB | rAB
    rC = ~v01 & (d6 >= 0) & (d5 <= d6)
    rAC = ~v01 & ~rC & (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    v04 = v01 | rC | rAC
    rBC = ~v04 & (va <= 0) & (d43 >= 0) & (d56 >= 0)
    rIn = ~v04 & ~rBC
    s = N(N(va + vb) + vc)
    zero, one = dt(0), dt(1)
    n1 = np.where(rAB, d1, np.where(rBC, d43, np.where(rIn, vb, zero)))
    m1 = np.where(rAB, N(d1 - d3), np.where(rBC, N(d43 + d56), np.where(rIn, s, one)))
    n2 = np.where(rAC, d2, np.where(rIn, vc, zero))
    m2 = np.where(rAC, N(d2 - d6), np.where(rIn, s, one))
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = N(n1 / m1), N(n2 / m2)
    fromB = (rB | rBC)[..., None]
    o = np.where(fromB, b, np.where(rC[..., None], c, a))
    u = np.where(rBC[..., None], bc, ab)
    with np.errstate(invalid="ignore"):
        p = N(N(o + m(t1[..., None], u)) + m(t2[..., None], ac))
        r = sub(q, p)
        dist2 = dot(r, r)
    code = np.select([rA, rB, rAB, rC, rAC, rBC], [0, 1, 2, 3, 4, 5], 6)
    assert dist2.dtype == dt
    return dist2, code


def face_area2(S, faces, dt=np.float32):
    """d = dot(n, n) of every rest face: a candidate only when d > 0"""
    _, sub, _, dot, _, cross = _ops(dt)
    a, b, c = (S[faces[:, k]].astype(dt) for k in range(3))
    n = cross(sub(b, a), sub(c, a))
    return dot(n, n)


def nearest(S, faces, T, dt=np.float32, chunk=64):
    """(face_idx [Vt] (-1: no candidate), dist2 [Vt] of the chosen face, its region code [Vt]): the strictly smallest dist2 scanning
    the faces ascending, which is the first occurrence of the minimum over the candidates with a finite distance"""
    a, b, c = (S[faces[:, k]].astype(dt)[None] for k in range(3))
    ok = face_area2(S, faces, dt) > 0
    idx, best, reg = [], [], []
    for j0 in range(0, len(T), chunk):
        d2, code = walk(T[j0:j0 + chunk].astype(dt)[:, None], a, b, c, dt)
        d2 = np.where(ok[None] & np.isfinite(d2), d2, np.inf)
        k = np.argmin(d2, axis=1)
        hit = np.isfinite(d2[np.arange(len(k)), k])
        idx.append(np.where(hit, k, -1))
        best.append(d2[np.arange(len(k)), k])
        reg.append(code[np.arange(len(k)), k])
    return np.concatenate(idx).astype(np.int32), np.concatenate(best), np.concatenate(reg)


def all_dist2_f64(S, faces, T, chunk=64):
    """float64 dist2 [Vt, F] of every target vertex to every face (inf for a face without area): the brute force"""
    a, b, c = (S[faces[:, k]].astype(np.float64)[None] for k in range(3))
    ok = face_area2(S, faces, np.float64) > 0
    out = [np.where(ok[None], walk(T[j0:j0 + chunk].astype(np.float64)[:, None], a, b, c, np.float64)[0], np.inf) for j0 in range(0, len(T), chunk)]
    return np.concatenate(out)


def coords(S, faces, T, face_idx):
    """(uvh [Vt, 3], dist [Vt]) of fdm_wrap_coords_host: float64 in the header's order, rounded once to float32"""
    _, sub, _, dot, _, cross = _ops(np.float64)
    a, b, c = (S[faces[face_idx, k]].astype(np.float64) for k in range(3))
    q = T.astype(np.float64)
    e1, e2, r = b - a, c - a, q - a
    n = cross(e1, e2)
    nn, g11, g12, g22, r1, r2 = dot(n, n), dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(e1, r), dot(e2, r)
    det = g11 * g22 - g12 * g12
    nh = n / np.sqrt(nn)[:, None]
    uvh = np.stack([(g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det, dot(r, nh)], axis=1)
    return uvh.astype(np.float32), np.sqrt(walk(q, a, b, c, np.float64)[0]).astype(np.float32)


def follow(off, tmpl, frames, faces, face_idx, uvh, T, weights=None, offsets_out=False, dt=np.float32):
    """list over clips of [L, 3 Vt] in dtype dt: the follow step on rows [0, frames[b]) of off [B, L_max, 3 V]; tmpl [1 or B, 3 V] or
    None; uvh, T, weights are the float32 binding values (cast to dt)."""
    N, sub, m, dot, _, cross = _ops(dt)
    V = off.shape[-1] // 3
    ia, ib, ic = (faces[face_idx, k] for k in range(3))
    u, v, h = (uvh[:, k].astype(dt)[None, :, None] for k in range(3))
    Tt = T.astype(dt)[None]
    out = []
    for bi, L in enumerate(frames):
        p = off[bi, :L].astype(dt)
        if tmpl is not None:
            p = N(p + tmpl[bi if tmpl.shape[0] > 1 else 0].astype(dt)[None])
        p = p.reshape(L, V, 3)
        a, b, c = p[:, ia], p[:, ib], p[:, ic]
        e1, e2 = sub(b, a), sub(c, a)
        n = cross(e1, e2)
        d = dot(n, n)
        ok = d > 0
        root = np.sqrt(np.where(ok, d, dt(1)))
        nh = np.where(ok[..., None], N(n / root[..., None]), dt(0))
        y = N(N(N(a + m(u, e1)) + m(v, e2)) + m(h, nh))
        if weights is not None or offsets_out:
            o = sub(y, Tt)
            if weights is not None:
                o = m(weights.astype(dt)[None, :, None], o)
            y = o if offsets_out else N(Tt + o)
        assert y.dtype == dt
        out.append(y.reshape(L, 3 * T.shape[0]))
    return out


def incident_binding(faces, V):
    """face_idx [V] for a target with the source's own vertex count: the lowest face with area that names vertex j, else face 0 -- a
    binding `brought by the caller`, cheap at any size (the coordinates reproduce q from any face's plane)"""
    fi = np.zeros(V, dtype=np.int32)
    seen = np.zeros(V, dtype=bool)
    for f in range(len(faces) - 1, -1, -1):
        if len(set(faces[f])) == 3:
            fi[faces[f]] = f
            seen[faces[f]] = True
    return fi


def rotation():
    """(R [3, 3], t [3]) float64: the rotation by one radian about (1, 2, 3) by Rodrigues' formula, and a translation of the order of
    the meshes"""
    x, y, z = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(1.0) * K + (1 - np.cos(1.0)) * (K @ K), np.array([0.3, -0.2, 0.45])
