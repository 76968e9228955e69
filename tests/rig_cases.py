"""Seeded cases and the numpy restatement of the rig hand-off tests (include/fdm_hip.h, fdm_rig_*).
solve() restates stage 2 in numpy float32 in exactly the stated column order, vectorised over frames (every numpy float32 operation
is one rounded IEEE operation: no contraction).  lerp() is the frame rule applied to the projections."""
import numpy as np

CHUNK = 768                       # csrc/handoff.hpp ROW_CHUNK: elements of 3V per partial sum
V3S = [3, 15, (CHUNK - 1) // 3 * 3, (CHUNK // 3 + 1) * 3, 2 * CHUNK + 3]       # 3, 15, 765, 771, 1539 -> chunks 1, 1, 1, 2, 3
KS = [1, 3, 52, 64, 65, 128]
FRAMES, L_MAX = [0, 1, 7], 7
RATES = [(30, 60), (25, 30), (30, 30)]
f32 = np.float32


def chunks(V3):
    return (V3 + CHUNK - 1) // CHUNK


def frames_out(L, fps):
    if L == 0 or fps is None or not (fps[0] > 0 and fps[1] > 0) or fps[0] == fps[1]:
        return L
    return max(1, int(float(L) / fps[0] * fps[1]))


def lerp(r, L, fps):
    """r [L_max, K] float32 native-rate projections of a clip of L frames -> [L_out, K] by the rule of fdm_mesh_forward on r."""
    Lo = frames_out(L, fps)
    if L == 0 or fps is None or not (fps[0] > 0 and fps[1] > 0) or fps[0] == fps[1]:
        return r[:L].copy()
    scale = f32(L - 1) / f32(Lo - 1) if Lo > 1 else f32(0)
    rows = []
    for t in range(Lo):
        src = f32(scale * f32(t))
        i0 = min(int(src), L - 1)
        i1 = i0 + (1 if i0 < L - 1 else 0)
        l1 = f32(src - f32(i0))
        l0 = f32(f32(1) - l1)
        rows.append(f32(l0) * r[i0] + f32(l1) * r[i1])
    return np.stack(rows).astype(f32) if rows else np.zeros((0, r.shape[1]), f32)


def solve(r, G, Lc, lo=None, hi=None, sweeps=16):
    """r [F, K], G [K, K], Lc [K, K] (lower factor), lo / hi [K] or None, all float32 -> c [F, K] float32."""
    r, G, Lc = np.asarray(r, f32), np.asarray(G, f32), np.asarray(Lc, f32)
    K = G.shape[0]
    g = r.copy()
    y = np.zeros_like(g)
    for i in range(K):
        y[:, i] = g[:, i] / Lc[i, i]
        if i + 1 < K:
            g[:, i + 1:] = g[:, i + 1:] - Lc[i + 1:, i][None, :] * y[:, i:i + 1]
    x = np.zeros_like(g)
    for i in range(K - 1, -1, -1):
        x[:, i] = y[:, i] / Lc[i, i]
        if i:
            y[:, :i] = y[:, :i] - Lc[i, :i][None, :] * x[:, i:i + 1]
    if lo is None:
        return x
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    c = np.minimum(np.maximum(x, lo[None]), hi[None])
    g = r.copy()
    for j in range(K):
        g = g - G[:, j][None, :] * c[:, j:j + 1]
    for _ in range(sweeps):
        for j in range(K):
            n = np.minimum(np.maximum(c[:, j] + g[:, j] / G[j, j], lo[j]), hi[j])
            delta = n - c[:, j]
            c[:, j] = n
            g = g - G[:, j][None, :] * delta[:, None]
    assert c.dtype == f32 and g.dtype == f32
    return c


# ---- seeded cases
def random_rig(K, V3, seed=0, weighted=True):
    """(E [K, V3] float32 normal, w [V3 / 3] float32 in [0.5, 1.5] or None, ridge = 1e-2 tr(E W E^T) / K)"""
    g = np.random.default_rng(100 + seed)
    E = g.standard_normal((K, V3)).astype(f32)
    w = (0.5 + g.random(V3 // 3)).astype(f32) if weighted else None
    W = np.ones(V3) if w is None else np.repeat(w.astype(np.float64), 3)
    ridge = 1e-2 * float(((E.astype(np.float64) ** 2) * W).sum()) / K
    return E, w, ridge


def targets_on_bounds(E, n, seed=0):
    """d [n, V3] float32 = E^T c* + noise with c* drawn from [-0.5, 1.5]: under bounds [0, 1] some coefficients end on each bound."""
    g = np.random.default_rng(200 + seed)
    c = g.uniform(-0.5, 1.5, size=(n, E.shape[0]))
    return (c @ E.astype(np.float64) + 0.1 * g.standard_normal((n, E.shape[1]))).astype(f32)


def integer_case(K, V3, B, L, seed=0):
    """P [K, V3] in {-2..2} and d [B, L, V3] in {-3..3}: every partial sum stays below 2^24 (|sum| <= 6 V3), so any order is exact."""
    g = np.random.default_rng(300 + seed)
    return g.integers(-2, 3, size=(K, V3)).astype(f32), g.integers(-3, 4, size=(B, L, V3)).astype(f32)


def disjoint_rig(K, V3):
    """Rows with disjoint supports, entries +-1, a power-of-FOUR count each (so G is diagonal with power-of-two entries and its
    Cholesky factor is exact too), or None when 3V cannot hold K such rows."""
    n = 1
    while 4 * n * K <= V3:
        n *= 4
    if n * K > V3:
        return None
    E = np.zeros((K, V3), f32)
    for k in range(K):
        E[k, k * n:(k + 1) * n] = np.where((np.arange(n) + k) % 2, -1.0, 1.0)
    return E
