"""The time filter hand-off restated in numpy (include/fdm_hip.h, fdm_tfilter_*), twice: in float32 in the
header's order, every operation rounded on its own (numpy float32 array operations round each result to float32 and do not contract),
which the device matches bit for bit; and in float64.  Plus the taps in float64, the cases and the tolerances, derived here once.

THE TOLERANCE OF THE FILTER.  With u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms,
Lemma 3.1: a product of n factors (1 + d_i), |d_i| <= u, is 1 + theta_n with |theta_n| <= gamma_n).  The chain is
    acc_0 = fl(h0 x_t),  acc_k = fl(acc_{k-1} + fl(h_k fl(x_{t-k} + x_{t+k}))),  k = 1 .. R.
The term of tap k is rounded by its pair sum, its product and the R - k + 1 sums that follow: at most R + 2 roundings, the centre term
at most R + 1.  So f32 = sum_k h_k (x_{t-k} + x_{t+k}) (1 + theta^(k)) with every |theta^(k)| <= gamma_{R+2} <= gamma_{2R+2}: the count the
definition names, 2 R + 2 rounded operations (more than R + 2, which only loosens it), is kept as stated.  The float64 evaluation of the
SAME float32 taps and inputs obeys the same analysis at u64 = 2^-53, so with g_n = gamma_n(2^-24) + gamma_n(2^-53):
    |f32 - f64| <= g_{2R+2} S,   S = |h0| |x_t| + sum_{k=1..R} |h_k| (|x_{e(t-k)}| + |x_{e(t+k)}|).
With a strength s: y32 = fl(x + fl(s fl(f32 - x))), three more roundings.  y32 = x (1 + d3) + s f32 (1 + theta_3) - s x (1 + theta_3), so
    |y32 - y64| <= g_{2R+5} (|x| (1 + s) + s S).
Nothing here is tuned to what the device returns.

THE TOLERANCE OF THE TAPS (float64, u64 = 2^-53), C function against the restatement below; both sides are float64 programs, so the
bound is twice one side's.  Gaussian: w_k = exp(-a), a = k^2 / (2 sigma^2) from 3 rounded operations, so w_k carries a relative error
3 a u64 from its argument plus one u64 of exp itself: an absolute error <= (3 a e^-a + w_k) u64 <= 2.2 u64 (a e^-a <= 1 / e, w_k <= 1).
The sum W = w_0 + 2 sum w_k >= 1 of R + 1 terms carries <= (2 R + 1) 2.2 u64 + (R + 1) u64 W, and h_k = w_k / W <= 1 one more rounding:
    |dh_k| <= u64 (2.2 + 2.2 (2 R + 1) + R + 2) = u64 (2.2 (2 R + 2) + R + 2)      per side.
Savitzky-Golay: h_k = sum_{j <= order} p_j(0) p_j(k) / <p_j, p_j> over the window's orthogonal polynomials; every term is an entry of an
orthogonal projector, so |term| <= 1.  The C function builds p_j from the monomial ((i - R) / R)^j by two Gram-Schmidt passes against
the j earlier polynomials -- 2 j projections of 4 n + 1 operations each, n = 2 R + 1 -- then a norm of 2 n operations and 3 more for the
term.  To first order a term's relative error is at most the operations on that longest chain times u64:
    |dh_k| <= (order + 1) (2 order (4 n + 1) + 2 n + 3) u64      per side
(the restatement solves the same least-squares problem by an SVD pseudo-inverse of the same scaled monomials, whose condition number
is below 100 for order <= 5 on any window; it is given the same allowance).  The exact rational for order 2,
    h_k = 3 (3 m^2 + 3 m - 1 - 5 k^2) / ((2 m - 1) (2 m + 1) (2 m + 3)),  m = R      (Savitzky & Golay 1964; Madden 1978, eq. 8),
evaluated with fractions, has no error of its own: one side's allowance.
Measured on the host (tests/test_time_filter_cpu.py prints them): Gaussian gap <= 5.6e-17, Savitzky-Golay gap to the restatement
<= 6.7e-16 and to the rational <= 2.3e-16 over the cases below -- two to four orders inside the bounds."""
from fractions import Fraction

import numpy as np

F32 = np.float32
U32, U64 = 2.0 ** -24, 2.0 ** -53
FRAME_TILE, COLUMN_CHUNK, RADIUS_MAX = 128, 96, 32      # csrc/tfilter.hpp: TF_TILE, TF_CHUNK, TF_RMAX (tests read them from fdm_amd.tfilter)


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


def edge_index(i, L, edge="mirror"):
    """e(i) of the header for a clip of L frames; i: an int array"""
    i = np.asarray(i, dtype=np.int64)
    if edge == "nearest":
        return np.minimum(np.maximum(i, 0), L - 1)
    if L == 1:
        return np.zeros_like(i)
    p = 2 * (L - 1)
    m = ((i % p) + p) % p
    return np.where(m < L, m, p - m)


def _filter(x, h, edge, strength, dt):
    """One clip x [L, N] -> y [L, N] in the header's order, every array operation in dtype dt"""
    x = np.asarray(x, dtype=dt)
    h = np.asarray(h, dtype=F32).astype(dt)
    L, N = x.shape
    t = np.arange(L)
    acc = h[0] * x
    for k in range(1, len(h)):
        pair = x[edge_index(t - k, L, edge)] + x[edge_index(t + k, L, edge)]
        acc = acc + h[k] * pair
    assert acc.dtype == dt
    if strength is None:
        return acc
    s = np.repeat(np.asarray(strength, dtype=F32).astype(dt), 3)[None, :]
    y = x + s * (acc - x)
    return np.where(s == 0, x, y).astype(dt)


def filter_f32(x, h, edge="mirror", strength=None):
    return _filter(x, h, edge, strength, F32)


def filter_f64(x, h, edge="mirror", strength=None):
    return _filter(x, h, edge, strength, np.float64)


def filter_batch(x, lens, h, edge="mirror", strength=None, fn=filter_f32):
    """x [B, L_max, N] with L per clip -> y: each clip filtered along its own frames (rows past them are never read), zeros after"""
    x = np.asarray(x)
    y = np.zeros(x.shape, dtype=F32 if fn is filter_f32 else np.float64)
    for b, L in enumerate(lens):
        y[b, :L] = fn(x[b, :L], h, edge, strength)
    return y


def bound(x, h, edge="mirror", strength=None):
    """The derived bound on |f32 - f64| per element of one clip x [L, N] (module docstring)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    h = np.abs(np.asarray(h, dtype=F32).astype(np.float64))
    L, R = x.shape[0], len(h) - 1
    t = np.arange(L)
    S = h[0] * x
    for k in range(1, R + 1):
        S = S + h[k] * (x[edge_index(t - k, L, edge)] + x[edge_index(t + k, L, edge)])
    g = lambda n: gamma(n, U32) + gamma(n, U64)  # noqa: E731
    if strength is None:
        return g(2 * R + 2) * S
    s = np.repeat(np.asarray(strength, dtype=np.float64), 3)[None, :]
    return g(2 * R + 5) * (x * (1.0 + s) + s * S)


# ---- taps in float64
def gaussian_taps(sigma, R):
    k = np.arange(R + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return w / (w[0] + 2.0 * w[1:].sum())


def savgol_taps(R, order):
    """The centre row of the least-squares polynomial fit over -R .. R: row R of A pinv(A), A the scaled monomials"""
    i = np.arange(-R, R + 1, dtype=np.float64) / max(R, 1)
    A = np.stack([i ** j for j in range(order + 1)], axis=1)
    return (A @ np.linalg.pinv(A))[R, R:]


def savgol2_exact(R):
    """Order 2 (and 3) as exact rationals"""
    m = R
    den = Fraction((2 * m - 1) * (2 * m + 1) * (2 * m + 3))
    return [Fraction(3 * (3 * m * m + 3 * m - 1 - 5 * k * k)) / den for k in range(R + 1)]


def gaussian_tol(R):
    return 2.0 * U64 * (2.2 * (2 * R + 2) + R + 2)


def savgol_tol(R, order, sides=2):
    n = 2 * R + 1
    return sides * U64 * (order + 1) * (2 * order * (4 * n + 1) + 2 * n + 3)


GAUSSIAN_CASES = [(0.5, 2), (1.0, 3), (1.5, 5), (2.5, 8), (4.0, 12), (10.0, 32), (0.3, 32), (50.0, 32), (1.0, 0)]      # (sigma, R)
SAVGOL_CASES = [(1, 2), (2, 2), (2, 3), (2, 4), (3, 5), (4, 2), (5, 4), (8, 3), (16, 5), (32, 2), (32, 5)]               # (R, order)


# ---- inputs
def clip(L, N, seed, scale=1.0):
    """A [L, N] float32 clip of offsets-like numbers: both signs, a few decades"""
    g = np.random.default_rng(seed)
    return (g.standard_normal((L, N)) * scale * np.exp(g.uniform(-3.0, 1.0, (1, N)))).astype(F32)


def taps_for(R, seed=0):
    """Float32 half-taps for radius R: a Gaussian of sigma = max(R, 1) / 2.5 rounded to float32 (any taps would do)"""
    return gaussian_taps(max(R, 1) / 2.5, R).astype(F32)
