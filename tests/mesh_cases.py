"""Meshes, seeded inputs and the two oracles of the mesh hand-off tests (include/fdm_hip.h, fdm_mesh_*).
The float32 oracle restates the definition in numpy float32 in exactly the stated order (every numpy float32 operation is one
rounded IEEE operation: no contraction); it refuses subnormal intermediates, so flush-to-zero could never explain a difference.
The float64 oracle is the same expression in double on the same inputs."""
import functools

import numpy as np

RATES = [(30, 60), (30, 25), (25, 30), (30, 24), (30, 30)]
TINY = float(np.finfo(np.float32).tiny)


# ---- topologies: (name) -> (faces int32 [F, 3], V, base coordinates float64 [V, 3])
def _grid_faces(rows, cols):
    f = []
    for r in range(rows - 1):
        for c in range(cols - 1):
            a = r * cols + c
            f += [(a, a + 1, a + cols), (a + 1, a + cols + 1, a + cols)]
    return f


def _grid_xyz(rows, cols, step):
    r, c = np.divmod(np.arange(rows * cols), cols)
    return np.stack([c * step, r * step, 0.3 * step * np.sin(0.9 * c + 0.4 * r)], axis=1)


def grid_like(V, step=0.05):
    """A rows x cols grid over the first rows * cols vertices; every vertex left over hangs on by one triangle."""
    cols = int(np.sqrt(V))
    rows = V // cols
    f, xyz = _grid_faces(rows, cols), _grid_xyz(rows, cols, step)
    extra = []
    for k in range(rows * cols, V):
        f.append((k, k - 1, k - cols))
        extra.append([(k - rows * cols + 1) * step + (cols - 1) * step, rows * step, 0.1 * step])
    if extra:
        xyz = np.concatenate([xyz, np.array(extra)])
    return np.array(f, dtype=np.int32), V, xyz


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "grid":                      # 4 x 8: V = 32, the tiny presets' V3 = 96
        return np.array(_grid_faces(4, 8), dtype=np.int32), 32, _grid_xyz(4, 8, 0.1)
    if name == "grid_extra":                # three more vertices; 34 is isolated
        f = _grid_faces(4, 8) + [(31, 32, 33), (30, 32, 31)]
        xyz = np.concatenate([_grid_xyz(4, 8, 0.1), np.array([[0.8, 0.3, 0.05], [0.8, 0.2, -0.05], [2.0, 2.0, 2.0]])])
        return np.array(f, dtype=np.int32), 35, xyz
    if name == "fan":                       # vertex 0 has valence 40
        n = 40
        ang = 2 * np.pi * np.arange(n) / n
        xyz = np.concatenate([[[0.0, 0.0, 0.2]], np.stack([0.5 * np.cos(ang), 0.5 * np.sin(ang), 0.05 * np.cos(3 * ang)], axis=1)])
        f = [(0, 1 + i, 1 + (i + 1) % n) for i in range(n)]
        return np.array(f, dtype=np.int32), n + 1, xyz
    if name == "strip":                     # V = 67: a block of 64 vertices ends inside the second wavefront
        V = 67
        i = np.arange(V)
        xyz = np.stack([0.02 * i, 0.03 * (i % 2), 0.01 * np.sin(0.5 * i)], axis=1)
        f = [(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(V - 2)]
        return np.array(f, dtype=np.int32), V, xyz
    if name == "degenerate":                # face 42 = (5, 5, 9) has no area
        return np.array(_grid_faces(4, 8) + [(5, 5, 9)], dtype=np.int32), 32, _grid_xyz(4, 8, 0.1)
    if name == "vocaset_size":              # V = 5023: real row widths
        return grid_like(5023)
    raise KeyError(name)


SMALL = ["grid", "grid_extra", "fan", "strip", "degenerate"]
ISOLATED = {"grid_extra": 34}
DEGENERATE = {"degenerate": 42}


# ---- inputs
def template(name, seed=0, rows=1):
    """[rows, 3 V] float32: the base coordinates (edges of order 1e-2 .. 1) plus N(0, 2e-3) per row."""
    _, V, xyz = mesh(name)
    g = np.random.default_rng(1000 + seed)
    return (xyz.reshape(1, -1) + 2e-3 * g.standard_normal((rows, 3 * V))).astype(np.float32)


def offsets(name, B, L, seed=0):
    """[B, L, 3 V] float32, N(0, 1e-2)."""
    _, V, _ = mesh(name)
    return (1e-2 * np.random.default_rng(2000 + seed).standard_normal((B, L, 3 * V))).astype(np.float32)


# ---- the definition
def frames_out(L, fps):
    if L == 0 or fps is None or not (fps[0] > 0 and fps[1] > 0) or fps[0] == fps[1]:
        return L
    return max(1, int(float(L) / fps[0] * fps[1]))


def adjacency(faces, V):
    """CSR lists by the plainest means: for every vertex the rows of `faces` that name it, one per occurrence, ascending."""
    items = [np.nonzero(faces == v)[0] for v in range(V)]
    off = np.concatenate([[0], np.cumsum([len(i) for i in items])]).astype(np.int32)
    return off, (np.concatenate(items) if len(faces) else np.zeros(0)).astype(np.int32)


def _normal(x, dt):
    """float32 only: no intermediate may be subnormal (exact zeros are fine)"""
    if dt == np.float32:
        a = np.abs(x[np.isfinite(x)])
        assert not ((a > 0) & (a < TINY)).any(), "subnormal intermediate in the float32 oracle: rescale the inputs"
    return x


def positions(off, tmpl, frames, fps, dt=np.float32):
    """list over clips of [L_out, 3 V] positions in dtype dt.  off [B, L_max, 3 V], tmpl [1 or B, 3 V] or None."""
    out = []
    resample = fps is not None and fps[0] > 0 and fps[1] > 0 and fps[0] != fps[1]
    for b, L in enumerate(frames):
        p = off[b, :L].astype(dt)
        if tmpl is not None:
            p = _normal(p + tmpl[b if tmpl.shape[0] > 1 else 0].astype(dt)[None], dt)
        if resample and L > 0:
            Lo = frames_out(L, fps)
            scale = dt(L - 1) / dt(Lo - 1) if Lo > 1 else dt(0)
            rows = []
            for t in range(Lo):
                src = _normal(scale * dt(t), dt)
                i0 = min(int(src), L - 1)
                i1 = i0 + (1 if i0 < L - 1 else 0)
                l1 = _normal(src - dt(i0), dt)
                l0 = dt(1) - l1
                rows.append(_normal(_normal(l0 * p[i0], dt) + _normal(l1 * p[i1], dt), dt))
            p = np.stack(rows).astype(dt)
        out.append(p)
    return out


def normals(p, faces, V, dt=np.float32):
    """p [L, 3 V] positions of dtype dt -> [L, V, 3] area-weighted vertex normals, summed over valence rank in ascending face index."""
    L = p.shape[0]
    p = p.reshape(L, V, 3)
    off, items = adjacency(faces, V)
    pa, pb, pc = p[:, faces[:, 0]], p[:, faces[:, 1]], p[:, faces[:, 2]]
    e1, e2 = _normal(pb - pa, dt), _normal(pc - pa, dt)
    m = lambda a, b: _normal(a * b, dt)  # noqa: E731
    n = np.stack([_normal(m(e1[..., 1], e2[..., 2]) - m(e1[..., 2], e2[..., 1]), dt),
                  _normal(m(e1[..., 2], e2[..., 0]) - m(e1[..., 0], e2[..., 2]), dt),
                  _normal(m(e1[..., 0], e2[..., 1]) - m(e1[..., 1], e2[..., 0]), dt)], axis=-1)
    val = off[1:] - off[:-1]
    s = np.zeros((L, V, 3), dtype=dt)
    for r in range(int(val.max()) if V else 0):
        vs = np.nonzero(val > r)[0]
        term = n[:, items[off[vs] + r]]
        s[:, vs] = term if r == 0 else _normal(s[:, vs] + term, dt)
    d = _normal(_normal(m(s[..., 0], s[..., 0]) + m(s[..., 1], s[..., 1]), dt) + m(s[..., 2], s[..., 2]), dt)
    ok = d > 0
    root = np.sqrt(np.where(ok, d, dt(1)))
    return np.where(ok[..., None], _normal(s / root[..., None], dt), dt(0)).astype(dt)


def oracle(off, tmpl, frames, fps, faces, V, dt=np.float32):
    """list over clips of (positions [L_out, V, 3], normals [L_out, V, 3]) in dtype dt"""
    return [(p.reshape(-1, V, 3), normals(p, faces, V, dt)) for p in positions(off, tmpl, frames, fps, dt)]
