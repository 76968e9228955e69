"""The numpy restatement of the temporal rig fit (include/fdm_hip.h, fdm_rig_set_temporal), steps 2-5 of
the rule in float32: every numpy float32 operation is one rounded IEEE operation, vectorised over frames with the loops over j that
the header states.  The tables come from fdm_rig_temporal_tables_host and are rounded as the object rounds them: eigenvectors are
only defined up to the library's own order and sign rule.  rig_cases.py supplies the seeded rigs, the frame rule and lerp()."""
import numpy as np

import rig_cases as RC

f32 = np.float32


def tables32(G64, smooth, weights=None):
    """(lam [K], Q [K, K], QT [K, K], mvec [K]) float32 as the object keeps them: the fp64 tables of the library, each rounded once."""
    from fdm_amd import rig
    lam, Q = rig.temporal_tables(G64, smooth, weights)
    K = len(lam)
    m = np.ones(K) if weights is None else np.asarray(weights, f32).astype(np.float64)
    Q32 = Q.astype(f32)
    return lam.astype(f32), Q32, np.ascontiguousarray(Q32.T), (float(smooth) * m).astype(f32)


def modal(T, v):
    """o[:, k] = sum_j T[k, j] v[:, j]: j ascending, the first product starts the sum"""
    o = T[:, 0][None, :] * v[:, 0:1]
    for j in range(1, T.shape[0]):
        o = o + T[:, j][None, :] * v[:, j:j + 1]
    return o


def neighbours(Lo):
    n = np.full(Lo, 2, np.int64)
    n[0] = n[-1] = 1
    return n if Lo > 1 else np.zeros(1, np.int64)


def time_solve(z, lam):
    """z [Lo, K] -> y [Lo, K]: the tridiagonal solve along time, all k at once"""
    Lo = z.shape[0]
    d = lam[None, :] + neighbours(Lo).astype(f32)[:, None]
    iw, u = np.zeros_like(z), np.zeros_like(z)
    iw[0] = f32(1) / d[0]
    u[0] = z[0]
    for f in range(1, Lo):
        w = d[f] - iw[f - 1]
        iw[f] = f32(1) / w
        u[f] = z[f] + u[f - 1] * iw[f - 1]
    y = np.zeros_like(z)
    y[Lo - 1] = u[Lo - 1] * iw[Lo - 1]
    for f in range(Lo - 2, -1, -1):
        y[f] = (u[f] + y[f + 1]) * iw[f]
    return y


def half_sweep(c, r, G, mvec, lo, hi, colour):
    """one colour of one sweep, in place in c [Lo, K]: the frames f = colour, colour + 2, .. read their neighbours' current values"""
    Lo, K = c.shape
    fs = np.arange(colour, Lo, 2)
    if not len(fs):
        return
    n = neighbours(Lo)[fs]
    g = r[fs].copy()
    prev, nxt = c[np.maximum(fs - 1, 0)], c[np.minimum(fs + 1, Lo - 1)]
    both, first, last = (n == 2), (n == 1) & (fs == 0), (n == 1) & (fs > 0)
    g[both] = r[fs][both] + mvec[None, :] * (prev[both] + nxt[both])
    g[first] = r[fs][first] + mvec[None, :] * nxt[first]
    g[last] = r[fs][last] + mvec[None, :] * prev[last]
    cc = c[fs].copy()
    for j in range(K):
        g = g - G[:, j][None, :] * cc[:, j:j + 1]
    e = n.astype(f32)[:, None] * mvec[None, :]
    g = g - e * cc
    for j in range(K):
        den = G[j, j] + e[:, j]
        nj = np.minimum(np.maximum(cc[:, j] + g[:, j] / den, lo[j]), hi[j])
        delta = nj - cc[:, j]
        cc[:, j] = nj
        g = g - G[:, j][None, :] * delta[:, None]
        g[:, j] = g[:, j] - e[:, j] * delta
    assert cc.dtype == f32 and g.dtype == f32
    c[fs] = cc


def solve(r, G, tables, lo=None, hi=None, sweeps=16):
    """One clip: r [Lo, K] float32 (the projections at the output rate), G [K, K] float32, tables = tables32(...) -> c [Lo, K] float32."""
    lam, Q, QT, mvec = tables
    r, G = np.asarray(r, f32), np.asarray(G, f32)
    if r.shape[0] == 0:
        return r.copy()
    x = modal(Q, time_solve(modal(QT, r), lam))
    assert x.dtype == f32
    if lo is None:
        return x
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    c = np.minimum(np.maximum(x, lo[None]), hi[None])
    for _ in range(sweeps):
        half_sweep(c, r, G, mvec, lo, hi, 0)
        half_sweep(c, r, G, mvec, lo, hi, 1)
    return c


# ---- fp64 references on the stacked system of one clip
def stacked(G64, M64, Lo):
    """H [Lo K, Lo K]: the Hessian of sum_f 1/2 c_f^T G c_f + 1/2 sum_{f>=1} (c_f - c_{f-1})^T M (c_f - c_{f-1})"""
    K = G64.shape[0]
    T = np.diag(neighbours(Lo).astype(np.float64)) - np.eye(Lo, k=1) - np.eye(Lo, k=-1)
    return np.kron(np.eye(Lo), G64) + np.kron(T, M64)


def objective(c, r, G64, M64):
    c, r = c.astype(np.float64), r.astype(np.float64)
    d = np.diff(c, axis=0)
    return float(0.5 * np.einsum("fk,kj,fj->", c, G64, c) - (r * c).sum() + 0.5 * np.einsum("fk,kj,fj->", d, M64, d))


def bend(c):
    """second-difference energy of the curves"""
    return float((np.diff(c.astype(np.float64), n=2, axis=0) ** 2).sum())


def smooth_case(K, V3, Lo, seed=0):
    """A clip whose per-frame fit is rough: a slow drift of the true coefficients from [-0.5, 1.5] plus white noise on the vertices.
    (E, w, ridge, d [Lo, V3] float32)"""
    E, w, ridge = RC.random_rig(K, V3, seed=seed)
    g = np.random.default_rng(400 + seed)
    a, b = g.uniform(-0.5, 1.5, size=(2, K))
    t = np.linspace(0.0, 1.0, Lo)[:, None]
    c = a[None] * (1 - t) + b[None] * t
    d = (c @ E.astype(np.float64) + 0.5 * g.standard_normal((Lo, V3))).astype(f32)
    return E, w, ridge, d
