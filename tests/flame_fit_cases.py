"""Seeded cases and the numpy restatement, in fp32 and in fp64, of the parametric-head fit (include/fdm_hip.h, fdm_flame_fit_*; DESIGN
section 2 item 26), shared by tests/test_flame_fit_cpu.py and tests/test_flame_fit_gpu.py.  Models are FlameModel.synthetic; the forward
half is tests/flame_cases.py's (pose_stage, rodrigues, fma32).

Every function takes dt = np.float32 or np.float64.  In fp32 the operation order is the header's: every product and sum of the pose and
derivative stages rounded on its own; the blends, the columns, the normal equations, the Cholesky factor and the substitutions with
their fused multiply-adds emulated through fp64 (flame_cases.fma32: a double rounding, so fp32 figures are error figures, never
torch.equal).  In fp64 the same expressions run unrounded on the SAME fp32 tables (FlameModel.tables(), pinned bit for bit by
tests/test_flame_out_cpu.py), so a difference to the device is rounding in the fit, not in the tables.

Bounds (u = 2^-24):

H and g, per element (step_bounds).  Z = [J | r] has P + 1 columns; an entry of Z^T M Z is a sum of n = 3 V products m Z_ia Z_ib.
  * The sum itself: chunked or not, a recursive fp32 sum of n terms with one rounded product m Z_ia and one fused multiply-add per term
    is within gamma_(n + 2) sum_i |m Z_ia Z_ib| of the exact sum of the SAME Z (Higham, Accuracy and Stability, 2nd ed., section 4.2; the
    chunk partials and their ascending sum are one particular order of at most n additions).
  * Z's own rounding: a column entry is a 3-term fused product sum of a blended transform (J terms) and a blended vertex (the forward's
    NT + 1 terms) plus a blended translation derivative (J terms): at most k = NT + 2 J + 8 roundings on the path of any term, so
    |dZ_ia| <= gamma_k Zabs_ia with Zabs the same expression with every term replaced by its absolute value.
  * The stage-1 inputs (the forward's propagated input error): every entry of the transforms, the pose feature and the derivative tables
    dX, dE carries at most e = flame_cases.pose_bound's figure for the forward's tables, and deriv_bound's (the same construction: 4 x the
    fp32 restatement's own error against fp64, floored at 2^-22 x the largest joint coordinate or 1) for dX, dE.  A column entry moves by
    at most e S_ia, S the sum of the absolute values of what each table entry is multiplied by (sensitivity()).
  Together: |dH_ab| <= gamma_(n + 2) W_ab + sum_i m (dz_ia Zabs_ib + Zabs_ia dz_ib), dz = gamma_k Zabs + e S, W = sum_i m Zabs_ia Zabs_ib,
  times 1.01 for the second-order terms.  Nothing here is measured on the device.

delta (solve_bound).  The computed Cholesky solution solves (A + dA) x = b with |dA| <= gamma_(3 P + 1) |L^T| |L| and
  || |L^T| |L| ||_2 <= P ||A||_2 (Higham, theorems 10.3 and 10.4), so ||dA||_2 / ||A||_2 <= P (3 P + 1) u: the stated constant is
  C_P = P (3 P + 1).  With the data's own error from above (eA = ||dH||_F / ||A||_2, eb = ||dg||_2 / ||b||_2) the classical perturbation
  bound (Higham, theorem 7.2) gives ||x - x64||_2 <= kappa_2(A) (C_P u + eA + eb) / (1 - kappa_2(A) (C_P u + eA)) ||x64||_2 as long as
  kappa_2(A) (C_P u + eA) < 1 (asserted: past that the theory says nothing).  kappa_2(A) is computed in fp64 in the test.

Recovery (RMS_MARGIN).  F = the forward's own a-priori per-vertex bound at the solution ((n + 2) u S + propagated, flame_cases), as an
  RMS over the vertices.  A fit in fp32 cannot do better than that floor: its residual is the forward's noise at its own solution
  (<= F), plus the movement of the vertices by the parameter error that the noise's projection on the column space causes (<= F: a
  projection does not lengthen), plus the same two again for the rounding of g itself, which step_bounds shows to be of the order of
  the noise term (<= 2 F).  So rms_device <= rms_fp64 + RMS_MARGIN F with RMS_MARGIN = 4, fixed here and in profiles/flame_fit/README.md.
  Parameters: |theta_device - theta_fp64| <= RMS_MARGIN F sqrt(3 V) / sigma_min(sqrt(M) J at the truth) (the same vertex movement
  through the smallest singular value), compared against truth through the fp64 restatement's own distance to the truth.
"""
import functools

import numpy as np

import flame_cases as FC
from fdm_amd import flame

U = 2.0 ** -24
RMS_MARGIN = 4.0
PIVOT_TOL = 2.0 ** -18
L_MAX = 7
FRAMES3 = (7, 3, 1)
FREE_SETS = {"none": ((), False), "jaw": ((2,), False), "jaw_neck": ((1, 2), False), "all_t": ((0, 1, 2, 3, 4), True)}

# name: V, J, NB, expr_at, NS, n_expr, free joints, transl, B, parents
CASES = {
    "v3_none": dict(V=3, J=2, NB=3, expr_at=1, NS=1, n_expr=1, free=(), transl=False, B=3, parents=[0, 0]),
    "v255_j2": dict(V=255, J=2, NB=3, expr_at=1, NS=1, n_expr=1, free=(1,), transl=False, B=3, parents=[0, 0]),
    "v5_none": dict(V=5, J=5, NB=9, expr_at=2, NS=2, n_expr=7, free=(), transl=False, B=3, parents=[0, 0, 1, 1, 1]),
    "v257_jaw": dict(V=257, J=5, NB=12, expr_at=4, NS=3, n_expr=7, free=(2,), transl=False, B=3, parents=[0, 0, 1, 1, 1]),
    "v257_jn": dict(V=257, J=5, NB=60, expr_at=8, NS=4, n_expr=50, free=(1, 2), transl=False, B=3, parents=[0, 0, 1, 1, 1]),
    "v513_all": dict(V=513, J=5, NB=12, expr_at=4, NS=2, n_expr=7, free=(0, 1, 2, 3, 4), transl=True, B=3, parents=[0, 0, 1, 1, 1]),
    # the free-translation sets again (all five joints + translation, and the P = 128 edge) with expression directions 30 x larger
    # (coefficients 30 x smaller) and a template 8 x larger: the columns of J are then of comparable size, kappa_2 of the barely damped
    # matrix is ~150 (fp64) and solve_bound's precondition holds at the DEFAULT lambda.  One-step tests only (STEP_EXTRA).
    "v513_all_s": dict(V=513, J=5, NB=12, expr_at=4, NS=2, n_expr=7, free=(0, 1, 2, 3, 4), transl=True, B=3, parents=[0, 0, 1, 1, 1], sd_scale=30.0, vt_scale=8.0),
    "v257_p128_s": dict(V=257, J=5, NB=114, expr_at=2, NS=0, n_expr=110, free=(0, 1, 2, 3, 4), transl=True, B=1, parents=[0, 0, 1, 1, 1], sd_scale=30.0, vt_scale=8.0),
    "v257_p128": dict(V=257, J=5, NB=114, expr_at=2, NS=0, n_expr=110, free=(0, 1, 2, 3, 4), transl=True, B=1, parents=[0, 0, 1, 1, 1]),
}
FULL = dict(V=5023, J=5, NB=400, expr_at=300, NS=100, n_expr=50, free=(1, 2), transl=False, B=2, parents=[0, 0, 1, 1, 1], L_max=9)
STEP_EXTRA = ("v513_all_s", "v257_p128_s")
SMALL = ("v3_none", "v5_none", "v255_j2", "v257_jaw", "v257_jn", "v513_all", "v257_p128")


def step_lam(c):
    """lambda of the one-step tests: the default, but 1.0 where the translation is free -- its columns put V on H's diagonal, kappa_2 of the
    barely damped matrix is then in the thousands and solve_bound's condition kappa (C_P u + eA) < 1 cannot hold in fp32 at all"""
    return 1.0 if (c["transl"] and not c.get("sd_scale")) else flame.FIT_DEFAULTS["lam"]


def n_params(c):
    return c["n_expr"] + 3 * len(c["free"]) + 3 * int(c["transl"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, model, truth): truth = dict(shape [B, NS], expr [B, L, n_expr] in [-2, 2], pose [B, L, 3J] (free joints up to 0.4 rad, the
    others fixed at pose0), pose0, transl [B, L, 3], frames)."""
    c = dict(FULL if name == "full" else CASES[name])
    seed = 7 + sum(map(ord, name))
    m = flame.FlameModel.synthetic(c["V"], c["J"], c["NB"], c["expr_at"], seed, parents=c["parents"])
    sc = float(c.get("sd_scale", 1.0))
    if sc != 1.0:
        sd = m.shapedirs.copy()
        sd[:, :, c["expr_at"]:] *= np.float32(sc)
        m = flame.FlameModel(m.v_template * np.float32(c.get("vt_scale", 1.0)), sd, m.posedirs, m.j_regressor, m.parents, m.lbs_weights, m.expr_at)
    g = np.random.default_rng(seed + 1)
    B, L, J = c["B"], c.get("L_max", L_MAX), c["J"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    pose0 = f32(0.05 * g.standard_normal((B, L, 3 * J)))
    pose = pose0.copy()
    for j in c["free"]:
        ax = g.standard_normal((B, L, 3))
        ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
        pose[..., 3 * j:3 * j + 3] = f32(ax * g.uniform(0.0, 0.4, (B, L, 1)))
    frames = list(FRAMES3) if B == 3 else ([L, L - 4] if name == "full" else [L] * B)
    truth = dict(shape=f32(g.standard_normal((B, c["NS"]))), expr=f32(g.uniform(-2, 2, (B, L, c["n_expr"])) / sc), pose=pose, pose0=pose0,
                 transl=f32(0.05 * g.standard_normal((B, L, 3))) * (1.0 if c["transl"] else 0.0), frames=frames)
    return c, m, truth


def live_rows(truth):
    """index arrays (b, t) of the live rows in (clip, frame) order"""
    bt = [(b, t) for b, n in enumerate(truth["frames"]) for t in range(n)]
    return np.array([x[0] for x in bt], dtype=np.int64), np.array([x[1] for x in bt], dtype=np.int64)


def tabs(m, dt):
    """(D [NB + PF, 3V], JT [3J], JD [NB, 3J]): the library's fp32 tables, cast"""
    if not hasattr(m, "_fit_tabs"):
        m._fit_tabs = {}
        D, JT, JD = m.tables()
        for t in (np.float32, np.float64):
            m._fit_tabs[t] = (D.astype(t), JT.reshape(-1).astype(t), JD.astype(t))
    return m._fit_tabs[dt]


def fma(a, b, c, dt):
    if dt is np.float64:
        return a * b + c
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    return FC.fma32(a, b, c)


def forward(m, sh, ex, ps, tr, dt):
    """The forward at N rows: sh [N, NS], ex [N, ne], ps [N, 3J], tr [N, 3] or None -> dict(Jf, A [N, J, 12], pf, v [N, V, 3] (blended, before
    skinning), T [N, V, 12], out [N, V, 3] (with the translation), R [N, J, 9] the joints' own rotations)"""
    D, JT, JD = tabs(m, dt)
    N, NS, ne, J, PF = ps.shape[0], sh.shape[1], ex.shape[1], m.J, 9 * (m.J - 1)
    sh, ex, ps = sh.astype(dt), ex.astype(dt), ps.astype(dt)
    Jf = np.broadcast_to(JT[None], (N, 3 * J)).copy()
    for k in range(NS):
        Jf = Jf + sh[:, k:k + 1] * JD[k][None]
    for k in range(ne):
        Jf = Jf + ex[:, k:k + 1] * JD[m.expr_at + k][None]
    A, pf = FC.pose_stage(Jf, m.parents, ps, dt)
    R = np.stack([FC.rodrigues(ps[:, 3 * j:3 * j + 3], dt) for j in range(J)], 1)
    v = np.broadcast_to(m.v_template.reshape(1, -1).astype(dt), (N, 3 * m.V)).copy()
    for k in range(NS):
        v = fma(sh[:, k:k + 1], D[k][None], v, dt)
    for k in range(ne):
        v = fma(ex[:, k:k + 1], D[m.expr_at + k][None], v, dt)
    for p in range(PF):
        v = fma(pf[:, p:p + 1], D[m.NB + p][None], v, dt)
    v = v.reshape(N, m.V, 3)
    w = m.lbs_weights.astype(dt)
    T = w[None, :, 0, None] * A[:, None, 0]
    for j in range(1, J):
        T = fma(w[None, :, j, None], A[:, None, j], T, dt)
    out = np.zeros((N, m.V, 3), dt)
    for c in range(3):
        out[..., c] = fma(T[..., 4 * c + 2], v[..., 2], fma(T[..., 4 * c + 1], v[..., 1], T[..., 4 * c] * v[..., 0], dt), dt) + T[..., 4 * c + 3]
        if tr is not None:
            out[..., c] = out[..., c] + tr[:, c:c + 1].astype(dt)
    return dict(Jf=Jf, A=A, pf=pf, v=v, T=T, out=out, R=R)


def drodrigues(r, dt):
    """[N, 3] -> dR [N, 3, 9]: the header's closed form with its small-angle branch at t2 < 1e-2"""
    r = r.astype(dt)
    N = r.shape[0]
    t2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    small = t2 < dt(1e-2)
    c_ = lambda x: dt(np.float32(x)) if dt is np.float32 else dt(x)  # noqa: E731 (fp64 uses the exact coefficients)
    a_s = dt(1) + t2 * (c_(-1 / 6) + t2 * c_(1 / 120))
    b_s = dt(0.5) + t2 * (c_(-1 / 24) + t2 * c_(1 / 720))
    a1_s = c_(-1 / 3) + t2 * (c_(1 / 30) + t2 * c_(-1 / 840))
    b1_s = c_(-1 / 12) + t2 * (c_(1 / 180) + t2 * c_(-1 / 6720))
    t2s = np.where(small, dt(1), t2)
    th = np.sqrt(t2s)
    s, co = np.sin(th), np.cos(th)
    a_l = s / th
    b_l = (dt(1) - co) / t2s
    a1_l = (co - a_l) / t2s
    b1_l = (a_l - dt(2) * b_l) / t2s
    a, b, a1, b1 = (np.where(small, x, y).astype(dt) for x, y in ((a_s, a_l), (b_s, b_l), (a1_s, a1_l), (b1_s, b1_l)))
    o = np.zeros(N, dt)
    K = [o, -r[:, 2], r[:, 1], r[:, 2], o, -r[:, 0], -r[:, 1], r[:, 0], o]
    dR = np.zeros((N, 3, 9), dt)
    for c in range(3):
        ar, br = a1 * r[:, c], b1 * r[:, c]
        for i in range(3):
            for j in range(3):
                h = dt(1) if (i == (c + 2) % 3 and j == (c + 1) % 3) else (dt(-1) if (i == (c + 1) % 3 and j == (c + 2) % 3) else dt(0))
                S = o
                if i == c:
                    S = S + r[:, j]
                if j == c:
                    S = S + r[:, i]
                if i == j:
                    S = S - dt(2) * r[:, c]
                kk = r[:, i] * r[:, j] - (t2 if i == j else dt(0))
                dR[:, c, 3 * i + j] = ((a * h + b * S) + ar * K[3 * i + j]) + br * kk
    return dR


def _mat3(G, R):
    """G [N, 12] rotation part times R [N, 9] -> [N, 3, 3] with the header's 3-term order"""
    out = np.zeros((G.shape[0], 3, 3), G.dtype)
    for a in range(3):
        for e in range(3):
            out[:, a, e] = FC.dot3(G[:, 4 * a], G[:, 4 * a + 1], G[:, 4 * a + 2], R[:, e], R[:, 3 + e], R[:, 6 + e])
    return out


def deriv(m, st, ps, free, ne, dt):
    """(dX [N, 3 nf, J, 12], dE [N, ne, J, 3]) from the forward state st (A, Jf, R) at ps"""
    _, _, JD = tabs(m, dt)
    N, J = ps.shape[0], m.J
    A, Jf, R = st["A"], st["Jf"].reshape(N, J, 3), st["R"]
    dX = np.zeros((N, 3 * len(free), J, 12), dt)
    for f, jf in enumerate(free):
        dR = drodrigues(ps[:, 3 * jf:3 * jf + 3], dt)
        for c in range(3):
            G = np.zeros((N, J, 12), dt)
            for j in range(J):
                if j == 0:
                    if jf == 0:
                        for a in range(3):
                            G[:, 0, 4 * a:4 * a + 3] = dR[:, c, 3 * a:3 * a + 3]
                else:
                    p = int(m.parents[j])
                    d = Jf[:, j] - Jf[:, p]
                    Gp = G[:, p]
                    rot = _mat3(A[:, p], dR[:, c]) if j == jf else _mat3(Gp, R[:, j])
                    for a in range(3):
                        G[:, j, 4 * a:4 * a + 3] = rot[:, a]
                        G[:, j, 4 * a + 3] = FC.dot3(Gp[:, 4 * a], Gp[:, 4 * a + 1], Gp[:, 4 * a + 2], d[:, 0], d[:, 1], d[:, 2]) + Gp[:, 4 * a + 3]
                dX[:, 3 * f + c, j] = G[:, j]
                for a in range(3):
                    dX[:, 3 * f + c, j, 4 * a + 3] = G[:, j, 4 * a + 3] - FC.dot3(G[:, j, 4 * a], G[:, j, 4 * a + 1], G[:, j, 4 * a + 2], Jf[:, j, 0], Jf[:, j, 1], Jf[:, j, 2])
    dE = np.zeros((N, ne, J, 3), dt)
    for k in range(ne):
        e = JD[m.expr_at + k].reshape(J, 3)
        h = np.zeros((N, J, 3), dt)
        for j in range(J):
            if j == 0:
                h[:, 0] = e[0][None]
            else:
                p = int(m.parents[j])
                d = e[j] - e[p]
                for a in range(3):
                    h[:, j, a] = FC.dot3(A[:, p, 4 * a], A[:, p, 4 * a + 1], A[:, p, 4 * a + 2], d[0], d[1], d[2]) + h[:, p, a]
            for a in range(3):
                dE[:, k, j, a] = h[:, j, a] - FC.dot3(A[:, j, 4 * a], A[:, j, 4 * a + 1], A[:, j, 4 * a + 2], e[j, 0], e[j, 1], e[j, 2])
    return dX, dE


def columns(m, st, dX, dE, y, free, ne, transl, dt):
    """Z [N, V, 3, P + 1] = [J | r] at the forward state st; y [N, V, 3] the targets"""
    D, _, _ = tabs(m, dt)
    N, V, J = y.shape[0], m.V, m.J
    P = ne + 3 * len(free) + 3 * int(transl)
    w = m.lbs_weights.astype(dt)
    T, v = st["T"], st["v"]
    Z = np.zeros((N, V, 3, P + 1), dt)
    for k in range(ne):
        d = D[m.expr_at + k].reshape(1, V, 3)
        for c in range(3):
            E = w[None, :, 0] * dE[:, k, 0, c][:, None]
            for j in range(1, J):
                E = fma(w[None, :, j], dE[:, k, j, c][:, None], E, dt)
            Z[:, :, c, k] = fma(T[..., 4 * c + 2], d[..., 2], fma(T[..., 4 * c + 1], d[..., 1], T[..., 4 * c] * d[..., 0], dt), dt) + E
    for q in range(3 * len(free)):
        Uq = w[None, :, 0, None] * dX[:, q, 0][:, None]
        for j in range(1, J):
            Uq = fma(w[None, :, j, None], dX[:, q, j][:, None], Uq, dt)
        for c in range(3):
            Z[:, :, c, ne + q] = fma(Uq[..., 4 * c + 2], v[..., 2], fma(Uq[..., 4 * c + 1], v[..., 1], Uq[..., 4 * c] * v[..., 0], dt), dt) + Uq[..., 4 * c + 3]
    if transl:
        for c in range(3):
            Z[:, :, c, ne + 3 * len(free) + c] = 1
    Z[..., P] = st["out"] - y.astype(dt)
    return Z


def normal(Z, mw, dt):
    """G [N, P + 1, P + 1] = Z^T M Z (upper triangle meaningful; H = G[:, :P, :P], g = G[:, :P, P]); mw [V] or None.  fp32: the chunked order"""
    N, V = Z.shape[:2]
    Q = Z.shape[3]
    mw = np.ones(V, dt) if mw is None else mw.astype(dt)
    if dt is np.float64:
        Zf = Z.reshape(N, 3 * V, Q)
        return np.matmul((Zf * np.repeat(mw, 3)[None, :, None]).transpose(0, 2, 1), Zf)
    G = None
    for v0 in range(0, V, 256):
        s = np.zeros((N, Q, Q), np.float32)
        for v in range(v0, min(V, v0 + 256)):
            for c in range(3):
                z = Z[:, v, c]
                s = fma((mw[v] * z)[:, :, None], z[:, None, :], s, dt)
        G = s if G is None else G + s
    return G


def rho_of(ne, free, transl, ridge_expr, ridge_pose, dt):
    return np.concatenate([np.full(ne, ridge_expr), np.full(3 * len(free), ridge_pose), np.zeros(3 * int(transl))]).astype(dt)


def solve(G, theta, theta0, rho, lam, dt):
    """(delta [N, P], status [N]) of the header's solve; a failed row has delta 0"""
    N, P = theta.shape
    A = G[:, :P, :P].copy()
    for a in range(P):
        A[:, a:, a] = G[:, a, a:P]                  # the lower triangle from the upper
    lam, rho = dt(lam), rho.astype(dt)
    damp = rho + lam
    idx = np.arange(P)
    A[:, idx, idx] = A[:, idx, idx] + damp[None]
    dg = A[:, idx, idx].copy()
    b = -(G[:, :P, P] + rho[None] * (theta.astype(dt) - theta0.astype(dt)))
    status = np.zeros(N, np.int32)
    ok = np.ones(N, bool)
    for j in range(P):
        p = A[:, j, j]
        bad = ok & ~(p > dt(PIVOT_TOL) * dg[:, j])
        status[bad] = j + 1
        ok &= ~bad
        l = np.sqrt(np.where(ok, p, dt(1)))
        A[:, j + 1:, j] = A[:, j + 1:, j] / l[:, None]
        A[:, j, j] = l
        if j + 1 < P:
            col = A[:, j + 1:, j]
            A[:, j + 1:, j + 1:] = fma(-col[:, :, None], col[:, None, :], A[:, j + 1:, j + 1:], dt)
    for j in range(P):
        yj = b[:, j] / A[:, j, j]
        b[:, j] = yj
        if j + 1 < P:
            b[:, j + 1:] = fma(-A[:, j + 1:, j], yj[:, None], b[:, j + 1:], dt)
    for j in range(P - 1, -1, -1):
        xj = b[:, j] / A[:, j, j]
        b[:, j] = xj
        if j > 0:
            b[:, :j] = fma(-A[:, j, :j], xj[:, None], b[:, :j], dt)
    b[~ok] = 0
    return b.astype(dt), status


def split(theta, p0, free, ne, transl):
    """theta [N, P] -> (expr [N, ne], pose [N, 3J], transl [N, 3]) on the fixed joints of p0"""
    ps = p0.astype(theta.dtype).copy()
    for f, j in enumerate(free):
        ps[:, 3 * j:3 * j + 3] = theta[:, ne + 3 * f:ne + 3 * f + 3]
    tr = theta[:, ne + 3 * len(free):] if transl else np.zeros((theta.shape[0], 3), theta.dtype)
    return theta[:, :ne], ps, tr


def join(ex, ps, tr, free, transl):
    parts = [ex] + [ps[:, 3 * j:3 * j + 3] for j in free] + ([tr] if transl else [])
    return np.concatenate(parts, 1)


def step(m, theta, y, sh, p0, free, ne, transl, dt, mw=None, lam=1e-6, ridge_expr=0.0, ridge_pose=0.0, parts=False):
    """One Gauss-Newton step at theta [N, P] (rows = live frames): -> (delta, status[, dict of the intermediate arrays])"""
    ex, ps, tr = split(theta.astype(dt), p0, free, ne, transl)
    st = forward(m, sh, ex, ps, tr if transl else None, dt)
    dX, dE = deriv(m, st, ps, free, ne, dt)
    Z = columns(m, st, dX, dE, y, free, ne, transl, dt)
    G = normal(Z, mw, dt)
    theta0 = join(np.zeros_like(ex), p0.astype(dt), np.zeros_like(tr), free, transl)
    d, status = solve(G, theta.astype(dt), theta0, rho_of(ne, free, transl, ridge_expr, ridge_pose, dt), lam, dt)
    return (d, status, dict(st=st, dX=dX, dE=dE, Z=Z, G=G, theta0=theta0, sh=sh, ex=ex)) if parts else (d, status)


def rms_of(out, y, mw, dt):
    """[N]: the header's rms (fp32: the 256-slot halving tree per chunk, chunks ascending)"""
    N, V = out.shape[:2]
    mw = np.ones(V, dt) if mw is None else mw.astype(dt)
    d = out.astype(dt) - y.astype(dt)
    e = mw[None] * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    msum = dt(mw.astype(np.float64).sum())
    if dt is np.float64:
        return np.sqrt(e.sum(1) / msum)
    S = np.zeros(N, np.float32)
    for v0 in range(0, V, 256):
        s = np.zeros((N, 256), np.float32)
        s[:, :min(256, V - v0)] = e[:, v0:v0 + 256]
        h = 128
        while h >= 1:
            s[:, :h] = s[:, :h] + s[:, h:2 * h]
            h //= 2
        S = S + s[:, 0]
    return np.sqrt(S / msum)


def fit(m, y, sh, p0, free, ne, transl, dt, iters=flame.FIT_DEFAULTS["iters"], mw=None, lam=flame.FIT_DEFAULTS["lam"], ridge_expr=0.0, ridge_pose=0.0):
    """The whole fit over N live rows: -> dict(theta, expr, pose, transl, status, out, rms)"""
    N, P = y.shape[0], ne + 3 * len(free) + 3 * int(transl)
    theta = join(np.zeros((N, ne), dt), p0.astype(dt), np.zeros((N, 3), dt), free, transl)
    status = np.zeros(N, np.int32)
    for _ in range(iters):
        d, stt = step(m, theta, y, sh, p0, free, ne, transl, dt, mw, lam, ridge_expr, ridge_pose)
        theta = (theta + d).astype(dt)
        status = np.where(stt > 0, stt, status)
    ex, ps, tr = split(theta, p0, free, ne, transl)
    out = forward(m, sh, ex, ps, tr if transl else None, dt)["out"]
    assert theta.shape[1] == P
    return dict(theta=theta, expr=ex, pose=ps, transl=tr, status=status, out=out, rms=rms_of(out, y, mw, dt))


def truth_rows(name):
    """(spec, model, dict over the LIVE rows: b, t, sh [N, NS], ex, ps, p0, tr, theta [N, P])"""
    c, m, tru = case(name)
    b, t = live_rows(tru)
    r = dict(b=b, t=t, sh=tru["shape"][b], ex=tru["expr"][b, t], ps=tru["pose"][b, t], p0=tru["pose0"][b, t], tr=tru["transl"][b, t])
    r["theta"] = join(r["ex"], r["ps"], r["tr"], c["free"], c["transl"]).astype(np.float64)
    return c, m, r


def bbox_diag(m):
    v = m.v_template.astype(np.float64)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


# ---- bounds (module docstring)

def deriv_bound(m, sh, ex, ps, free, ne):
    """(e_pose, e_deriv): the input error of the forward's tables (flame_cases.pose_bound's construction on these rows) and of dX, dE"""
    s64, s32 = forward(m, sh, ex, ps, None, np.float64), forward(m, sh, ex, ps, None, np.float32)
    jmax = float(np.abs(s64["Jf"]).max())
    E = max(float(np.abs(s32["A"].astype(np.float64) - s64["A"]).max()), float(np.abs(s32["pf"].astype(np.float64) - s64["pf"]).max()) if s64["pf"].size else 0.0)
    x64, e64 = deriv(m, s64, ps.astype(np.float64), free, ne, np.float64)
    x32, e32 = deriv(m, s32, ps.astype(np.float32), free, ne, np.float32)
    Ed = max([float(np.abs(a.astype(np.float64) - b).max()) for a, b in ((x32, x64), (e32, e64)) if b.size] + [0.0])
    return max(4 * E, 2.0 ** -22 * jmax), max(4 * Ed, 2.0 ** -22 * max(jmax, 1.0))


def step_bounds(m, P64, y, mw, free, ne, transl, NS, e_pose, e_deriv):
    """dG [N, P + 1, P + 1]: the per-element bound of the module docstring on Z^T M Z, from the fp64 intermediates P64 (step(..., parts=True))"""
    f = np.float64
    D, _, _ = tabs(m, f)
    st, dX, dE, Z = P64["st"], P64["dX"], P64["dE"], P64["Z"]
    N, V, J, PF = Z.shape[0], m.V, m.J, 9 * (m.J - 1)
    P = Z.shape[3] - 1
    w = np.abs(m.lbs_weights.astype(f))
    W1 = w.sum(1)                                                            # [V]
    Ta = np.einsum("vj,nje->nve", w, np.abs(st["A"]))                       # |T|
    # |v|: every term of the blend by its absolute value (the coefficients are recovered from the state: v's own terms)
    co = np.concatenate([np.abs(P64["sh"]), np.abs(P64["ex"]), np.abs(st["pf"])], 1).astype(f)
    Dr = np.abs(np.concatenate([D[:NS], D[m.expr_at:m.expr_at + ne], D[m.NB:]]))
    va = (np.abs(m.v_template.reshape(1, -1).astype(f)) + co @ Dr).reshape(N, V, 3)      # |v|: every term of the blend by its absolute value
    Dp = np.abs(D[m.NB:]).sum(0).reshape(V, 3) if PF else np.zeros((V, 3))   # sum_p |D_pose|: what a pose-feature error multiplies
    Zabs, S = np.zeros_like(Z), np.zeros_like(Z)
    v1 = va.sum(-1)                                                          # [N, V]
    for k in range(ne):
        d = np.abs(D[m.expr_at + k].reshape(1, V, 3))
        Ea = np.einsum("vj,njc->nvc", w, np.abs(dE[:, k]))
        for c in range(3):
            Zabs[:, :, c, k] = (Ta[..., 4 * c:4 * c + 3] * d).sum(-1) + Ea[..., c]
            S[:, :, c, k] = e_pose * W1[None] * d.sum(-1) + e_deriv * W1[None]
    for q in range(3 * len(free)):
        Ua = np.einsum("vj,nje->nve", w, np.abs(dX[:, q]))
        for c in range(3):
            Zabs[:, :, c, ne + q] = (Ua[..., 4 * c:4 * c + 3] * va).sum(-1) + Ua[..., 4 * c + 3]
            S[:, :, c, ne + q] = e_deriv * W1[None] * (v1 + 1) + e_pose * (Ua[..., 4 * c:4 * c + 3] * Dp[None]).sum(-1)
    if transl:
        for c in range(3):
            Zabs[:, :, c, ne + 3 * len(free) + c] = 1
    for c in range(3):
        Zabs[:, :, c, P] = (Ta[..., 4 * c:4 * c + 3] * va).sum(-1) + Ta[..., 4 * c + 3] + np.abs(y[..., c]) + (np.abs(st["out"][..., c]) if transl else 0)
        S[:, :, c, P] = e_pose * W1[None] * (v1 + 1) + e_pose * (Ta[..., 4 * c:4 * c + 3] * Dp[None]).sum(-1)
    k = (1 + NS + ne + PF) + 2 * J + 8
    dz = k * U * Zabs + S
    mw = np.ones(V) if mw is None else mw.astype(f)
    n = 3 * V
    Q = P + 1
    mz = (Zabs.reshape(N, n, Q) * np.repeat(mw, 3)[None, :, None]).transpose(0, 2, 1)
    Wab = np.matmul(mz, Zabs.reshape(N, n, Q))
    cross = np.matmul((dz.reshape(N, n, Q) * np.repeat(mw, 3)[None, :, None]).transpose(0, 2, 1), Zabs.reshape(N, n, Q))
    return 1.01 * ((n + 2) * U * Wab + cross + cross.transpose(0, 2, 1))


def solve_bound(A64, b64, x64, dH, dg, P):
    """[N]: the bound on ||x - x64||_2 of the module docstring; asserts its own condition"""
    out = np.zeros(A64.shape[0])
    for i in range(A64.shape[0]):
        sv = np.linalg.svd(A64[i], compute_uv=False)
        kappa, nA = sv[0] / sv[-1], sv[0]
        eA = np.linalg.norm(dH[i]) / nA
        eb = np.linalg.norm(dg[i]) / max(np.linalg.norm(b64[i]), 1e-300)
        q = kappa * (P * (3 * P + 1) * U + eA)
        assert q < 1, (i, kappa, eA)
        out[i] = kappa * (P * (3 * P + 1) * U + eA + eb) / (1 - q) * np.linalg.norm(x64[i])
    return out


def full_sym(G, P):
    """the symmetric P x P matrix and the vector of an upper-triangle G [N, P + 1, P + 1]"""
    H = np.triu(G[:, :P, :P])
    H = H + np.triu(H, 1).transpose(0, 2, 1)
    return H, G[:, :P, P]


def unpack(Hp, P):
    """packed upper triangle [N, (P + 1)(P + 2) / 2] -> [N, P + 1, P + 1] (upper; the rest zeros)"""
    N = Hp.shape[0]
    G = np.zeros((N, P + 1, P + 1), Hp.dtype)
    iu = np.triu_indices(P + 1)
    G[:, iu[0], iu[1]] = Hp
    return G
