"""The recurrences of the time filter hand-off restated in numpy float32 (include/fdm_hip.h, fdm_tfilter_create_recur; DESIGN.md section
2 item 28), from the definition and not from the kernel: a loop over frames in which every line is ONE float32 array operation (numpy
rounds each float32 result on its own and does not contract; np.sqrt and the division of float32 arrays are correctly rounded, as
__fsqrt_rn and __fdiv_rn are).  The causal and the zero-phase direction, the strength rule and the carried state."""
import numpy as np

F32 = np.float32


def coeffs(kind, fps, cutoff=None, min_cutoff=None, beta=0.0, d_cutoff=1.0):
    """(k, c0, be, cd, fr, ad, a0, 0) as float32: k = (float)(fps / 2 pi) with the division in float64; the rest in float32"""
    k = F32(float(fps) / (2.0 * np.pi))
    if kind == "ema":
        c0, be, cd, ad = F32(cutoff), F32(0), F32(0), F32(0)
    else:
        c0, be, cd = F32(min_cutoff), F32(beta), F32(d_cutoff)
        ad = F32(cd / F32(cd + k))
    a0 = F32(c0 / F32(c0 + k))
    return np.array([k, c0, be, cd, F32(fps), ad, a0, 0], dtype=F32)


def fresh_state(N):
    """seen = 0 and (y_prev, x_prev, dh) = 0"""
    return dict(seen=0, st=np.zeros((3, N), F32))


def causal(x, kind, q, state=None):
    """One clip x [L, N] (N = 3 V) -> f [L, N], the unblended recurrence.  state (fresh_state, or what an earlier call left) is
    continued and updated in place; L = 0 leaves it as it is."""
    x = np.asarray(x, dtype=F32)
    L, N = x.shape
    k, c0, be, cd, fr, ad, a0 = (F32(v) for v in q[:7])
    st = fresh_state(N) if state is None else state
    y, xp, dh = st["st"][0].copy(), st["st"][1].copy(), st["st"][2].copy()
    f = np.zeros((L, N), F32)
    for t in range(L):
        xt = x[t]
        if st["seen"] + t == 0:
            y, dh = xt.copy(), np.zeros(N, F32)
        else:
            if kind == "one_euro":
                d = xt - xp
                dx = d * fr
                e = dx - dh
                g = ad * e
                dh = dh + g
                d3 = dh.reshape(-1, 3)
                xx, yy, zz = d3[:, 0] * d3[:, 0], d3[:, 1] * d3[:, 1], d3[:, 2] * d3[:, 2]
                s2 = xx + yy
                s2 = s2 + zz
                s = np.sqrt(s2)
                bs = be * s
                fc = c0 + bs
                den = fc + k
                a = np.repeat(fc / den, 3)
            else:
                a = a0
            d = xt - y
            m = a * d
            y = y + m
        xp = xt.copy()
        assert y.dtype == F32 and dh.dtype == F32
        f[t] = y
    if L > 0:
        if kind == "one_euro":
            st["st"][0], st["st"][1], st["st"][2] = y, xp, dh
        else:
            st["st"][0] = y
        st["seen"] += L
    return f


def blend(x, f, strength):
    """out = f without a strength; x where s_v == 0; else x + s_v (f - x), three rounded operations"""
    if strength is None:
        return f
    x = np.asarray(x, dtype=F32)
    s = np.repeat(np.asarray(strength, dtype=F32), 3)[None, :]
    d = f - x
    m = s * d
    return np.where(s == 0, x, x + m).astype(F32)


def filter_clip(x, kind, q, direction="causal", strength=None, state=None):
    """One clip x [L, N] -> out [L, N]"""
    x = np.asarray(x, dtype=F32)
    if direction == "causal":
        return blend(x, causal(x, kind, q, state), strength)
    assert state is None, "zero_phase carries no state"
    f = causal(x, kind, q)
    f = causal(f[::-1], kind, q)[::-1]
    return blend(x, f, strength)


def filter_batch(x, lens, kind, q, direction="causal", strength=None, states=None):
    """x [B, L_max, N] with L per clip (None: L_max) -> out: each clip over its own frames (rows past them are never read), zeros after"""
    x = np.asarray(x)
    out = np.zeros(x.shape, F32)
    for b in range(x.shape[0]):
        L = x.shape[1] if lens is None else lens[b]
        out[b, :L] = filter_clip(x[b, :L], kind, q, direction, strength, None if states is None else states[b])
    return out


def clip(L, N, seed, scale=1.0):
    """A [L, N] float32 clip of offsets-like numbers: a smooth path plus jitter, both signs, a few decades"""
    g = np.random.default_rng(seed)
    amp = scale * np.exp(g.uniform(-3.0, 1.0, (1, N)))
    t = np.arange(L, dtype=np.float64)[:, None]
    return (amp * (np.sin(0.2 * t + g.uniform(0, 6.0, (1, N))) + 0.2 * g.standard_normal((L, N)))).astype(F32)
