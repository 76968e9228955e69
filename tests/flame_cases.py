"""Seeded models, inputs and two numpy restatements of the parametric-head rule (include/fdm_hip.h, fdm_flame_*), shared by
tests/test_flame_out_cpu.py and tests/test_flame_out_gpu.py.  No FLAME data: every model is FlameModel.synthetic from a seed.

restate(model, inp, np.float64)   the rule in fp64 from the model's own arrays: joints as j_regressor . v_shaped (NOT the folded
                                  tables), so it also checks the folding.
restate(model, inp, np.float32)   the rule in float32 in the stated order on tables rounded once from fp64: the pose stage bit for
                                  bit the header's (every operation rounded; sin / cos are numpy's), the blend and the skinning with
                                  their fused multiply-adds emulated through fp64 (a double rounding: almost always the same bits,
                                  so it is used for error figures, never for torch.equal).
blend_skin64(...)                 stage B alone in fp64 from GIVEN fp32 transforms and pose features (the device's own), with the
                                  magnitude S (every term replaced by its absolute value) and the term count n of the a-priori
                                  bound (n + 2) 2^-24 S.

E, the float32 restatement's own max-abs error against fp64 in the pose stage (xforms and posefeat together), measured on the CPU
by pose_error() on exactly the inputs the GPU test uses; the device must be within 4 E, floored at 2^-22 x the largest joint
coordinate (tests/test_flame_out_gpu.py recomputes it on every run and checks it against this table within a factor 2):
#   case      3V    J  NB   NS  NE   B   E (xforms, posefeat)
#   v3         3    1   0    0   0   1   9.41e-08
#   v15       15    2   1    0   1   3   1.58e-07
#   v765     765    5   7    3   2   3   2.52e-07
#   v771     771    8 150   60  30   3   2.52e-07
#   v1539   1539    5   7    4   3   1   2.52e-07
#   full   15069    5 400  100  50   2   2.52e-07
"""
import functools

import numpy as np

from fdm_amd import flame

L_MAX = 7
FRAMES3 = (0, 1, 7)
U = 2.0 ** -24
E_TABLE = {"v3": 9.41e-08, "v15": 1.58e-07, "v765": 2.52e-07, "v771": 2.52e-07, "v1539": 2.52e-07, "full": 2.52e-07}

# name: V, J, NB, expr_at, NS, NE, B, shape_rows, parents, transl, extra, NL, L_max
CASES = {
    "v3": dict(V=1, J=1, NB=0, expr_at=0, NS=0, NE=0, B=1, shape_rows=1, parents=[0], transl=False, extra=False, NL=0),
    "v15": dict(V=5, J=2, NB=1, expr_at=0, NS=0, NE=1, B=3, shape_rows=1, parents=[0, 0], transl=True, extra=False, NL=2),
    "v765": dict(V=255, J=5, NB=7, expr_at=4, NS=3, NE=2, B=3, shape_rows=1, parents=[0, 0, 1, 1, 1], transl=True, extra=True, NL=5),
    "v771": dict(V=257, J=8, NB=150, expr_at=100, NS=60, NE=30, B=3, shape_rows=3, parents=[0, 0, 1, 2, 0, 4, 1, 0], transl=False, extra=True, NL=0),
    "v1539": dict(V=513, J=5, NB=7, expr_at=4, NS=4, NE=3, B=1, shape_rows=1, parents=[0, 0, 1, 1, 1], transl=False, extra=False, NL=3),
}
FULL = dict(V=5023, J=5, NB=400, expr_at=300, NS=100, NE=50, B=2, shape_rows=1, parents=[0, 0, 1, 1, 1], transl=True, extra=True, NL=8, L_max=9)


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, model, inputs): inputs = dict(shape [rows, NS], expr [B, L, NE], pose [B, L, 3J], transl, extra, frames, lv, lb)"""
    c = dict(FULL if name == "full" else CASES[name])
    seed = sum(map(ord, name))
    m = flame.FlameModel.synthetic(c["V"], c["J"], c["NB"], c["expr_at"], seed, parents=c["parents"])
    g = np.random.default_rng(seed + 1)
    B, L, J = c["B"], c.get("L_max", L_MAX), c["J"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    pose = f32(0.3 * g.standard_normal((B, L, 3 * J)))
    for b in range(B):            # rows 0..3 of every clip: zero, 1e-8-small, a quarter turn about an axis, more than pi
        pose[b, 0] = 0
        pose[b, 1] = 1e-8 * g.standard_normal(3 * J)
        pose[b, 2] = np.tile(np.array([0, np.pi / 2, 0]), J)
        pose[b, 3] = np.tile(np.array([2.0, -2.5, 1.5]), J)
    frames = list(FRAMES3) if B == 3 else [L] * B
    if name == "full":
        frames = [L, L - 4]
    inp = dict(shape=f32(g.standard_normal((c["shape_rows"], c["NS"]))), expr=f32(g.standard_normal((B, L, c["NE"]))), pose=pose,
               transl=f32(g.standard_normal((B, L, 3))) if c["transl"] else None,
               extra=f32(1e-2 * g.standard_normal((B, L, 3 * c["V"]))) if c["extra"] else None, frames=frames, lv=None, lb=None)
    if c["NL"]:
        inp["lv"] = np.ascontiguousarray(g.integers(0, c["V"], size=(c["NL"], 3)), dtype=np.int32)
        w = g.random((c["NL"], 3)) + 0.05
        inp["lb"] = f32(w / w.sum(1, keepdims=True))
    return c, m, inp


def tables64(m):
    """(D [NB + P, 3V], JT [J, 3], JD [NB, 3J]) in fp64, unrounded"""
    V3 = 3 * m.V
    D = m.shapedirs.astype(np.float64).reshape(V3, m.NB).T
    if m.posedirs is not None:
        D = np.concatenate([D, m.posedirs.astype(np.float64)])
    jr = m.j_regressor.astype(np.float64)
    JT = jr @ m.v_template.astype(np.float64)
    JD = np.einsum("jv,vak->kja", jr, m.shapedirs.astype(np.float64)).reshape(m.NB, 3 * m.J)
    return D, JT, JD


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def rodrigues(r, dt):
    """[N, 3] -> [N, 9] row-major, the header's expression in dtype dt"""
    r = r.astype(dt)
    e = r + dt(1e-8)
    angle = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    x, y, z = r[:, 0] / angle, r[:, 1] / angle, r[:, 2] / angle
    s, m = np.sin(angle), dt(1) - np.cos(angle)
    o = np.zeros_like(x)
    xx, yy, zz, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
    K = [o, -z, y, z, o, -x, -y, x, o]
    KK = [-(yy + zz), xy, xz, xy, -(xx + zz), yz, xz, yz, -(xx + yy)]
    return np.stack([((dt(1) if i % 4 == 0 else dt(0)) + s * K[i]) + m * KK[i] for i in range(9)], 1).astype(dt)


def pose_stage(Jf, parents, pose, dt):
    """Jf [N, 3J] joints, pose [N, 3J] -> (xforms [N, J, 12], posefeat [N, 9 (J - 1)]) in dtype dt, the header's order"""
    N, J = pose.shape[0], len(parents)
    Jf = Jf.astype(dt).reshape(N, J, 3)
    G = np.zeros((N, J, 12), dt)
    A = np.zeros((N, J, 12), dt)
    pf = np.zeros((N, 9 * (J - 1)), dt)
    eye = np.eye(3, dtype=dt).reshape(9)
    for j in range(J):
        R = rodrigues(pose[:, 3 * j:3 * j + 3], dt)
        if j >= 1:
            pf[:, 9 * (j - 1):9 * j] = R - eye
        if j == 0:
            for a in range(3):
                G[:, 0, 4 * a:4 * a + 3] = R[:, 3 * a:3 * a + 3]
                G[:, 0, 4 * a + 3] = Jf[:, 0, a]
        else:
            p = int(parents[j])
            d = Jf[:, j] - Jf[:, p]
            Gp = G[:, p]
            for a in range(3):
                for c in range(3):
                    G[:, j, 4 * a + c] = dot3(Gp[:, 4 * a], Gp[:, 4 * a + 1], Gp[:, 4 * a + 2], R[:, c], R[:, 3 + c], R[:, 6 + c])
                G[:, j, 4 * a + 3] = dot3(Gp[:, 4 * a], Gp[:, 4 * a + 1], Gp[:, 4 * a + 2], d[:, 0], d[:, 1], d[:, 2]) + Gp[:, 4 * a + 3]
        A[:, j] = G[:, j]
        for a in range(3):
            A[:, j, 4 * a + 3] = G[:, j, 4 * a + 3] - dot3(G[:, j, 4 * a], G[:, j, 4 * a + 1], G[:, j, 4 * a + 2], Jf[:, j, 0], Jf[:, j, 1], Jf[:, j, 2])
    return A, pf


def _rows(m, inp):
    """live rows flattened: (index arrays b, t), shape per row [N, NS], expr [N, NE], pose [N, 3J]"""
    B, L = inp["pose"].shape[:2]
    bt = [(b, t) for b in range(B) for t in range(inp["frames"][b])]
    b = np.array([x[0] for x in bt], dtype=np.int64)
    t = np.array([x[1] for x in bt], dtype=np.int64)
    sh = inp["shape"][b if inp["shape"].shape[0] > 1 else np.zeros_like(b)]
    return b, t, sh, inp["expr"][b, t], inp["pose"][b, t]


def fma32(a, b, c):
    """float32 fused multiply-add through fp64 (the product is exact there; the sum is rounded twice)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def restate(m, inp, dt):
    """dict(xforms [N, J, 12], posefeat [N, P], joints [N, 3J], verts [N, V, 3], lmk [N, NL, 3] | None) over the LIVE rows in
    (clip, frame) order, in dtype dt (see the module docstring)."""
    b, t, sh, ex, ps = _rows(m, inp)
    N, V3, NS, NE, P = len(b), 3 * m.V, sh.shape[1], ex.shape[1], 9 * (m.J - 1)
    D64, JT64, JD64 = tables64(m)
    vt = m.v_template.reshape(-1)
    xt = None if inp["extra"] is None else inp["extra"][b, t]
    tr = None if inp["transl"] is None else inp["transl"][b, t]
    w = m.lbs_weights
    if dt is np.float64:
        v = vt.astype(dt)[None] + sh.astype(dt) @ D64[:NS] + ex.astype(dt) @ D64[m.expr_at:m.expr_at + NE]          # v_shaped
        Jf = np.einsum("jv,nva->nja", m.j_regressor.astype(dt), v.reshape(N, m.V, 3)).reshape(N, 3 * m.J)
        A, pf = pose_stage(Jf, m.parents, ps, dt)
        v = v + pf @ D64[m.NB:]
        if xt is not None:
            v = v + xt.astype(dt)
        T = np.einsum("vj,nje->nve", w.astype(dt), A)
    else:
        D, JT, JD = (a.astype(np.float32) for a in (D64, JT64, JD64))
        Jf = np.broadcast_to(JT.reshape(1, -1), (N, 3 * m.J)).copy()
        for k in range(NS):
            Jf = Jf + sh[:, k:k + 1] * JD[k][None]
        for k in range(NE):
            Jf = Jf + ex[:, k:k + 1] * JD[m.expr_at + k][None]
        A, pf = pose_stage(Jf, m.parents, ps, dt)
        v = np.broadcast_to(vt[None], (N, V3)).copy()
        for k in range(NS):
            v = fma32(sh[:, k:k + 1], D[k][None], v)
        for k in range(NE):
            v = fma32(ex[:, k:k + 1], D[m.expr_at + k][None], v)
        for p in range(P):
            v = fma32(pf[:, p:p + 1], D[m.NB + p][None], v)
        if xt is not None:
            v = v + xt
        T = w[None, :, 0, None] * A[:, None, 0]
        for j in range(1, m.J):
            T = fma32(np.broadcast_to(w[None, :, j, None], T.shape), np.broadcast_to(A[:, None, j], T.shape), T)
    v = v.reshape(N, m.V, 3)
    out = np.zeros((N, m.V, 3), dt)
    for c in range(3):
        if dt is np.float64:
            out[..., c] = T[..., 4 * c] * v[..., 0] + T[..., 4 * c + 1] * v[..., 1] + T[..., 4 * c + 2] * v[..., 2] + T[..., 4 * c + 3]
        else:
            out[..., c] = fma32(T[..., 4 * c + 2], v[..., 2], fma32(T[..., 4 * c + 1], v[..., 1], T[..., 4 * c] * v[..., 0])) + T[..., 4 * c + 3]
        if tr is not None:
            out[..., c] = out[..., c] + tr[:, c:c + 1].astype(dt)
    lmk = None
    if inp["lv"] is not None:
        lb = inp["lb"].astype(dt)
        lmk = sum(lb[None, :, c, None] * out[:, inp["lv"][:, c]] for c in range(3))
    return dict(xforms=A, posefeat=pf, joints=Jf, verts=out, lmk=lmk)


def pose_error(m, inp):
    """(E, largest |joint coordinate|): the float32 restatement's max-abs error against fp64 over xforms and posefeat"""
    r64, r32 = restate(m, inp, np.float64), restate(m, inp, np.float32)
    if r64["xforms"].shape[0] == 0:
        return 0.0, 0.0
    e = float(np.abs(r32["xforms"].astype(np.float64) - r64["xforms"]).max())
    if r64["posefeat"].size:
        e = max(e, float(np.abs(r32["posefeat"].astype(np.float64) - r64["posefeat"]).max()))
    return e, float(np.abs(r64["joints"]).max())


def pose_bound(m, inp):
    """4 E floored at 2^-22 x the largest joint coordinate"""
    e, jmax = pose_error(m, inp)
    return max(4 * e, 2.0 ** -22 * jmax), e


def blend_skin64(m, D, inp, xforms, posefeat):
    """Stage B in fp64 from fp32 inputs: D [NB + P, 3V] float32 (fdm_flame_tables_host: the library's own table is a fair input here only
    because tests/test_flame_out_cpu.py::test_tables_against_numpy pins it bit for bit against numpy's transposition), xforms [N, J, 12] and posefeat [N, P] float32 over
    the live rows -> (out [N, V, 3], S [N, V, 3], n, parts) with parts = (|v| [N, V, 3], |T| [N, V, 12]) for the propagated bound."""
    b, t, sh, ex, _ = _rows(m, inp)
    f = np.float64
    N, NS, NE, P = len(b), sh.shape[1], ex.shape[1], 9 * (m.J - 1)
    D = D.astype(f)
    co = np.concatenate([sh.astype(f), ex.astype(f), posefeat.astype(f)], 1)
    Dr = np.concatenate([D[:NS], D[m.expr_at:m.expr_at + NE], D[m.NB:]])
    vt = m.v_template.reshape(1, -1).astype(f)
    v, va = vt + co @ Dr, np.abs(vt) + np.abs(co) @ np.abs(Dr)
    if inp["extra"] is not None:
        x = inp["extra"][b, t].astype(f)
        v, va = v + x, va + np.abs(x)
    w = m.lbs_weights.astype(f)
    T, Ta = np.einsum("vj,nje->nve", w, xforms.astype(f)), np.einsum("vj,nje->nve", np.abs(w), np.abs(xforms.astype(f)))
    v, va = v.reshape(N, m.V, 3), va.reshape(N, m.V, 3)
    out, S = np.zeros((N, m.V, 3)), np.zeros((N, m.V, 3))
    for c in range(3):
        out[..., c] = (T[..., 4 * c:4 * c + 3] * v).sum(-1) + T[..., 4 * c + 3]
        S[..., c] = (Ta[..., 4 * c:4 * c + 3] * va).sum(-1) + Ta[..., 4 * c + 3]
    n = (1 + NS + NE + P + (inp["extra"] is not None)) + m.J + 4
    if inp["transl"] is not None:
        tr = inp["transl"][b, t].astype(f)
        out, S, n = out + tr[:, None], S + np.abs(tr)[:, None], n + 1
    return out, S, n, (va, Ta)


def propagated(m, D, e, parts):
    """What an error e in every transform and pose-feature entry moves a vertex by, at most: e (sum_j |w_j|) (sum_a |v|_a + 1) through
    the transforms plus e sum_a |T|_ca sum_p |D[NB + p]|_a through the pose correctives.  [N, V, 3]"""
    va, Ta = parts
    W = np.abs(m.lbs_weights.astype(np.float64)).sum(1)                       # [V]
    Dp = np.abs(D[m.NB:].astype(np.float64)).sum(0).reshape(m.V, 3)           # [V, 3]
    out = np.zeros(va.shape)
    for c in range(3):
        out[..., c] = e * W[None] * (va.sum(-1) + 1) + e * (Ta[..., 4 * c:4 * c + 3] * Dp[None]).sum(-1)
    return out


def live(x, frames):
    """the live rows of a [B, L, ...] array in (clip, frame) order, after checking that every other row is zero"""
    for b, n in enumerate(frames):
        assert np.all(x[b, n:] == 0)
    return np.concatenate([x[b, :n] for b, n in enumerate(frames)])
