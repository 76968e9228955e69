"""The kernels that search or reduce to a scalar behind fdm_op_* (csrc/elementwise.hpp: vq_quant_body, vq_stats_partial_body /
vq_stats_final_kernel, argmax_rows_rep_kernel, diff_partial / diff_final_kernel, vertex_err_kernel / vertex_err_final_kernel,
motion_partial / motion_final_kernel, linear_interp_kernel): host models in numpy, the case tables and the bounds shared by
tests/test_reduce_cpu.py and tests/test_reduce_gpu.py.  Plain helper module (pytest does not collect it), host only.

Exact cases
-----------
Integer-valued fp32 operands whose every partial sum stays below 2^24 (fp32) are summed exactly in ANY order, with or without fused
multiply-add: the host states the result once and the GPU file asks for equal bits.  The limits are asserted by the CPU file
(vq_is_exact, stats_expected's own assertions, diff_exact_inputs), not assumed.

Bounds (u = 2^-24, U = 2^-53; the library is compiled with -ffp-contract=off: every +, * and / rounds once; -fhip-fp32-correctly-
rounded-divide-sqrt is the default).  Each is a first-order count through the kernel's stated operations, times SLACK = 2 for what
first order leaves out (as tests/norm_cases.py and tests/epilogue_cases.py do), except the summation bounds, which are the rigorous
any-order ones: n values summed in any order by n - 1 rounded additions err by at most gamma(n - 1) sum |v|, gamma(k) = k e / (1 - k e).

  perplexity (vq_stats_final_kernel)   p_k = float(hist[k]) / float(rows) in fp32: the reference takes the same fp32 p_k, so the
      division is not part of the error.  a = fl(p_k + c), c = 1e-10f: ln a = ln(p_k + c) + d, |d| <= u.  l = logf(a): relative R.
      t = fl(p_k l): relative u.  |t - p_k ln(p_k + c)| <= p_k (u + (R + u) |ln(p_k + c)|).  The K terms are summed in double
      (gamma64(K) sum |t|), the sum is rounded to fp32 (u |H|):
          dH = SLACK [ sum_k p_k (u + (R + u) |ln(p_k + c)|) + u |H| + gamma64(K) sum_k |t_k| ]
      out = expf(-H^) = exp(-H) exp(H - H^) (1 + R'):  |out - exp(-H)| <= exp(-H) (expm1(dH) + R exp(dH)).
      R = R_T = 4u: two ulps of the result for logf and expf.  HIP's documentation gives 1 ulp for each; the allowance of two is the
      one tests/epilogue_cases.py makes for the same functions (a result may sit one ulp from the rounding of the true value).
  mean_diff, randn data   d = fl(a - b): relative u; |d| exact, fl(d d): one more rounding, and d^2 carries 2u from d: the term is
      within TERM u of the true one (TERM = 1 for l1, 3 for l2).  n terms in any order: gamma(n - 1) sum |term|.  scale = fl(1 / n)
      (n < 2^24 is exact as a float): u; the last product: u.
          |out - mean| <= (gamma(n - 1) + (TERM + 2) u) (1 + 4u) mean |term|
  vertex_err sums   d2 (fp32, the same bits as the host's) is summed in double: R terms per frame in any order, then F frames in
      any order, one division: gamma64(R + F) sum d2 / (F R).  sum sqrt: the radicand dx dx + dy dy + dz dz in double (3 products,
      2 additions, all terms positive: 3 U relative, halved by the root) and the root itself (U): 3 U per term on top.
          |out[1] - ref| <= SLACK gamma64(R + F) ref,  |out[2] - ref| <= SLACK (gamma64(R + F) + 3 U) ref
      out[0] = mean_f frame_max: F doubles in any order and a division: SLACK gamma64(F + 1) ref.  The references are math.fsum's
      exactly rounded sums, so numpy's own summation error is not in the comparison.
  motion_std   s (fp32) is the same bits as the host's; s s is exact in double (24 x 24 bits).  Per region vertex, with
      m2 = mean_f s^2 >= mu^2:  s2 / F: F - 1 additions and the division: F U m2.  mu = s1 / F: F U mu, so mu mu: (2 F + 1) U mu^2
      <= (2 F + 1) U m2.  The subtraction: U var <= U m2.  Together
          dv = (3 F + 2) U m2        -- absolute in the variance, and NOT relative to it: var << m2 when the motion is small
      std^ = sqrt(max(var + e, 0)), |e| <= dv:  |std^ - std| <= min(sqrt(dv), dv / std) (the first is the floor that holds at
      var = 0, the second is e / (sqrt(var + e) + sqrt(var))), + U std for the root.  The mean over R vertices: gamma64(R + 1) mean.
          bound_r = SLACK (min(sqrt(dv_r), dv_r / std_r) + U std_r),   bound_mean = mean_r bound_r + SLACK gamma64(R + 1) mean_r std_r
      The chunking (FC = F below 64 frames, 64 chunks from there on) only reorders the F additions: the same bound.

Nothing here is fitted to what a kernel returns.  Measured on the MI355X against these bounds (tests/test_reduce_gpu.py prints them):
perplexity reaches 0.12 of its bound, the vertex_err sums 0.14, motion_std 0.006 (worst-case roundings of F additions do not line
up) and the randn mean_diff 0.0009 (an any-order bound of 300000 additions against a tree of depth ~ 20).
"""
import math
from collections import namedtuple

import numpy as np

import mesh_cases as MC

U = 2.0 ** -24
U64 = 2.0 ** -53
R_T = 4.0 * U
SLACK = 2.0
F32, F64 = np.float32, np.float64
EXACT_LIMIT = 2 ** 24


def gamma(k, e=U):
    return k * e / (1.0 - k * e)


def gen(*key):
    return np.random.default_rng([int(k) for k in key])


def bits(a):
    """The bits of an fp32 / fp64 array as integers (equal bits, not equal values: -0.0 is not +0.0)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(got, want):
    """Equal bits where `want` is a number; a NaN (any payload) where it is NaN."""
    got, want = np.atleast_1d(np.asarray(got)), np.atleast_1d(np.asarray(want))
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


# ---------------------------------------------------------------------------------------------------------------------
# A. the quantiser on exactly representable data
# ---------------------------------------------------------------------------------------------------------------------
N_BOOKS = 3
VQ_LIM = 8
VQ_CK = [(1, 1), (3, 5), (64, 63), (64, 64), (64, 65), (65, 130), (128, 256)]
VQ_BR = [(1, 1), (1, 3), (2, 5), (3, 4)]


def clip_books(B):
    """book[b] of the per-clip form: every slice, never in clip order"""
    return ((2 * np.arange(B) + 1) % N_BOOKS).astype(np.int32)


def row_books(rows, out_of_range=False):
    """book[row] of the per-row form: neighbouring rows (of one workgroup) in different slices; out_of_range: the first row names
    -1 and the last N_BOOKS (both read slice 0, the rule stated above vq_quant_body)."""
    bk = ((2 * np.arange(rows) + 1) % N_BOOKS).astype(np.int32)
    if out_of_range:
        bk[0] = -1
        bk[-1] = N_BOOKS
    return bk


def book_slice(bk):
    """The slice a per-row entry reads."""
    bk = np.asarray(bk).astype(np.int64)
    return np.where((bk < 0) | (bk >= N_BOOKS), 0, bk)


def vq_inputs(c, K, B, R):
    """Integer-valued latents z [B, R, c] and codebook [N_BOOKS * K, c], |v| <= VQ_LIM."""
    g = gen(11, c, K, B, R)
    return (g.integers(-VQ_LIM, VQ_LIM + 1, size=(B, R, c)).astype(F32), g.integers(-VQ_LIM, VQ_LIM + 1, size=(N_BOOKS * K, c)).astype(F32))


def vq_is_exact(z, codebook):
    """Whether z2, e2, dot and d_k are integers below 2^24 in every order: |v| <= VQ_LIM integers, 4 c VQ_LIM^2 < 2^24
    (z2 + e2 + 2 |dot| <= 4 c VQ_LIM^2 bounds every intermediate of d_k = (z2 + e2) - 2 dot)."""
    fin = z[np.isfinite(z)]
    ok = all(bool((np.abs(v) <= VQ_LIM).all() and (v == np.round(v)).all()) for v in (fin, codebook))
    return ok and 4 * z.shape[-1] * VQ_LIM * VQ_LIM < EXACT_LIMIT


def vq_distances(zr, E):
    """d_k of one latent row against the K rows of E in fp64: (z2 + e2) - 2 dot, the kernel's expression (exact on the integer
    data; on a row with NaN or inf it gives NaN or +inf where the kernel's does: inf e_i is NaN for e_i = 0, inf - inf is NaN)."""
    zr, E = zr.astype(F64), E.astype(F64)
    with np.errstate(all="ignore"):
        return ((zr * zr).sum() + (E * E).sum(1)) - 2.0 * (E * zr[None]).sum(1)


def first_min(d):
    """The kernel's rule: the first k whose d_k is below everything before it, starting from +inf; none (every d_k NaN or +inf) ->
    bk = 0x7fffffff >= K -> 0."""
    d = np.where(d < np.inf, d, np.inf)
    return int(np.argmin(d)) if bool((d < np.inf).any()) else 0


def vq_expected(z, codebook, K, slices):
    """slices [B * R]: the codebook slice of each row -> (idx int64 [B * R], z_q fp32 [B, c, R] = z + (e - z) transposed)."""
    B, R, c = z.shape
    zr = z.reshape(B * R, c)
    idx = np.zeros(B * R, dtype=np.int64)
    zq = np.zeros((B * R, c), dtype=F32)
    for r in range(B * R):
        E = codebook[slices[r] * K:(slices[r] + 1) * K]
        idx[r] = first_min(vq_distances(zr[r], E))
        with np.errstate(all="ignore"):
            zq[r] = zr[r] + (E[idx[r]] - zr[r])
    return idx, np.ascontiguousarray(zq.reshape(B, R, c).transpose(0, 2, 1))


def vq_wave_twin(d, defect=None):
    """vq_quant_body's search on one row of distances d [K]: the lane scan (lane l takes k = l, l + 64, ..), the xor-butterfly merge,
    `bk >= K -> 0`; what lane 0 writes.  defect: 'scan_le' (the scan's < as <=), 'merge_no_tiebreak' (the merge without ok < bk),
    'merge_le' (the merge's < as <=)."""
    K, big = len(d), 0x7fffffff
    best, bk = np.full(64, np.inf), np.full(64, big, dtype=np.int64)
    for k in range(K):
        l = k % 64
        if (d[k] <= best[l]) if defect == "scan_le" else (d[k] < best[l]):
            best[l], bk[l] = d[k], k
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ob, ok = best[lane ^ o], bk[lane ^ o]
        if defect == "merge_le":
            take = ob <= best
        elif defect == "merge_no_tiebreak":
            take = ob < best
        else:
            take = (ob < best) | ((ob == best) & (ok < bk))
        best, bk = np.where(take, ob, best), np.where(take, ok, bk)
    return 0 if bk[0] >= K else int(bk[0])


VQ_DEFECTS = ("scan_le", "merge_no_tiebreak", "merge_le")

# Duplicated codebook rows, one list of (lower, higher) pairs per slice (disjoint within a slice).  Both rows of a pair hold one
# vector, and a latent equal to that vector has them as its only nearest codes (distance 0): the lower index must win.
#   (k, k + 1) neighbouring lanes (63, 64: lanes 63 and 0);  (k, k + 64), (k, k + 128) one lane;  (5, 70) lanes 5 and 6, the lower index in
#   the earlier lane;  (70, 133), (6, 69) lanes 6 and 5, the lower index in the later lane;  (0, K - 1).
VQ_TIES = {
    (3, 5): [[(1, 2), (0, 4)], [(0, 1), (3, 4)], [(2, 3), (0, 4)]],
    (65, 130): [[(10, 11), (20, 84), (5, 70), (0, 129), (63, 64), (1, 65), (127, 128)],
                [(11, 12), (6, 69), (31, 32), (40, 104), (64, 128), (2, 66), (7, 8)],
                [(3, 4), (13, 14), (33, 97), (62, 126), (0, 129), (65, 128), (21, 22)]],
    (128, 256): [[(10, 11), (20, 84), (30, 158), (5, 70), (0, 255), (63, 64), (127, 128)],
                 [(11, 12), (70, 133), (31, 32), (100, 228), (40, 104), (191, 192), (1, 254)],
                 [(6, 69), (12, 13), (64, 128), (0, 255), (129, 193), (33, 34), (3, 131)]],
}


def vq_tie_inputs(c, K, rowbook):
    """-> (z [N_BOOKS, R, c], codebook, slices [N_BOOKS * R], pairs [N_BOOKS * R] of (lower, higher)).  Per-clip form: clip b is in
    slice clip_books(N_BOOKS)[b]; per-row form: row r in slice row_books(..)[r].  Row j of a clip holds pair j of its slice."""
    sets = VQ_TIES[(c, K)]
    R = len(sets[0])
    g = gen(13, c, K)
    cb = g.integers(-VQ_LIM, VQ_LIM + 1, size=(N_BOOKS * K, c)).astype(F32)
    for s, pairs in enumerate(sets):
        for lo, hi in pairs:
            cb[s * K + hi] = cb[s * K + lo]
    slices = book_slice(row_books(N_BOOKS * R)) if rowbook else np.repeat(clip_books(N_BOOKS).astype(np.int64), R)
    z = np.zeros((N_BOOKS * R, c), dtype=F32)
    pairs = []
    for r in range(N_BOOKS * R):
        lo, hi = sets[slices[r]][r % R]
        z[r] = cb[slices[r] * K + lo]
        pairs.append((lo, hi))
    return z.reshape(N_BOOKS, R, c), cb, slices, pairs


def vq_nonfinite_inputs(c, K):
    """B, R = 2, 5: row 3 has a NaN and row 4 +inf in the latent, in the middle of finite neighbours (rows 0-3: one workgroup)."""
    z, cb = vq_inputs(c, K, 2, 5)
    z = z.copy()
    z.reshape(10, c)[3, c // 2] = np.nan
    z.reshape(10, c)[4, 0] = np.inf
    return z, cb


# ---------------------------------------------------------------------------------------------------------------------
# B. vq_stats
# ---------------------------------------------------------------------------------------------------------------------
StatsCase = namedtuple("StatsCase", "B R c K idx_kind")
STATS_CASES = ([StatsCase(B, R, c, K, "random") for (B, R) in ((1, 1), (1, 3), (2, 2), (1, 5))
                for (c, K) in ((1, 1), (5, 63), (65, 256), (130, 257))]
               + [StatsCase(1, 4096, 4, 7, "random"), StatsCase(1, 4099, 4, 7, "random"),
                  StatsCase(1, 5, 5, 63, "one_code"), StatsCase(1, 4099, 4, 7, "one_code"), StatsCase(2, 2, 65, 256, "one_code")])


def stats_id(s):
    return f"B{s.B}-R{s.R}-c{s.c}-K{s.K}-{s.idx_kind}"


def stats_blocks(rows):
    """Workgroups of the partial kernel = the doubles of `partial` the call writes (fdm_op_vq_stats: 4 rows each, at most 1024)."""
    return min(1024, (rows + 3) // 4)


def stats_inputs(case, seed=0):
    """Integer data as in A; idx: any code in [0, K) (the statistics take the indices as given)."""
    g = gen(17, case.B, case.R, case.c, case.K, seed)
    rows = case.B * case.R
    z = g.integers(-VQ_LIM, VQ_LIM + 1, size=(case.B, case.R, case.c)).astype(F32)
    cb = g.integers(-VQ_LIM, VQ_LIM + 1, size=(N_BOOKS * case.K, case.c)).astype(F32)
    idx = np.full(rows, (5 + seed) % case.K, dtype=np.int64) if case.idx_kind == "one_code" else g.integers(0, case.K, size=rows).astype(np.int64)
    return z, cb, idx


def perplexity_reference(hist, rows):
    """(exp(-sum p_k ln(p_k + 1e-10f)) in fp64 of the kernel's fp32 p_k, its bound) -- the derivation is in the module docstring."""
    K = len(hist)
    pk = (hist.astype(F32) / F32(rows)).astype(F64)
    lg = np.log(pk + F64(F32(1e-10)))
    t = pk * lg
    H = -float(t.sum())
    dH = SLACK * (float((pk * (U + (R_T + U) * np.abs(lg))).sum()) + U * abs(H) + gamma(K, U64) * float(np.abs(t).sum()))
    perp = math.exp(H)
    return perp, perp * (math.expm1(dH) + R_T * math.exp(dH))


def perplexity_twin(hist, rows):
    """The kernel's evaluation with numpy's fp32 log and exp: p_k, fl(p_k + c), log, the product in fp32; the sum in double; exp in
    fp32."""
    pk = hist.astype(F32) / F32(rows)
    with np.errstate(all="ignore"):
        t = pk * np.log(pk + F32(1e-10))
    return float(np.exp(F32(-F32(t.astype(F64).sum()))))


def stats_expected(z, cb, K, slices, idx, beta):
    """-> dict(hist int32 [K], onehot fp32 [rows, K], loss fp32 (exact), perp, perp_bound).  sq = sum (e - z)^2 is an exact integer:
    every row's sum stays below 2^24 (fp32, any order) and the total below 2^53 (double); m = float(sq / (rows c)), then
    beta m + m in fp32 as two rounded steps."""
    B, R, c = z.shape
    rows = B * R
    e = cb[slices * K + idx].astype(F64)
    d = e - z.reshape(rows, c).astype(F64)
    row_sq = (d * d).sum(1)
    assert bool((row_sq < EXACT_LIMIT).all()) and float(row_sq.sum()) < 2.0 ** 53 and bool((d == np.round(d)).all())
    sq = int(row_sq.sum())
    m = F32(sq / (rows * c))                     # int / int: the correctly rounded quotient, as the kernel's double division
    loss = F32(F32(F32(beta) * m) + m)
    hist = np.bincount(idx, minlength=K).astype(np.int32)
    onehot = np.zeros((rows, K), dtype=F32)
    onehot[np.arange(rows), idx] = 1.0
    perp, bound = perplexity_reference(hist, rows)
    return dict(hist=hist, onehot=onehot, loss=loss, perp=perp, perp_bound=bound)


# ---------------------------------------------------------------------------------------------------------------------
# C. argmax_rows
# ---------------------------------------------------------------------------------------------------------------------
ARGMAX_ROWS = (1, 63, 64, 65, 130)
ARGMAX_N = (1, 2, 7)
ARGMAX_REP = (1, 16)
NAN = float("nan")
# (row, the first maximum by the kernel's rule)
ARGMAX_EDGE_ROWS = [([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 0), ([0.0, 1.0, 4.0, 2.0, 3.0, 4.0, 1.0], 2), ([-0.0, 0.0, -1.0], 0), ([0.0, -0.0, -1.0], 0),
                    ([NAN, 5.0, 3.0], 0), ([1.0, NAN, 3.0], 2), ([NAN, NAN, NAN], 0), ([3.0, NAN, 1.0], 0), ([-np.inf, -np.inf], 0),
                    ([1.0, np.inf, np.inf], 1)]


def argmax_first(x):
    """x [rows, n] -> int32 [rows]: best = 0, then every column i >= 1 in order takes over on x[i] > x[best] alone (a NaN compares
    false both ways: in column 0 it is never beaten, elsewhere it never wins)."""
    x = np.asarray(x, dtype=F32)
    best = np.zeros(x.shape[0], dtype=np.int32)
    bv = x[:, 0].copy()
    for i in range(1, x.shape[1]):
        with np.errstate(invalid="ignore"):
            take = x[:, i] > bv
        bv = np.where(take, x[:, i], bv)
        best = np.where(take, np.int32(i), best)
    return best


def argmax_inputs(rows, n):
    """Small integers (many ties) with -0.0 for some zeros and a NaN in one element in nine."""
    g = gen(19, rows, n)
    x = g.integers(-2, 3, size=(rows, n)).astype(F32)
    x = np.where((x == 0) & (g.random((rows, n)) < 0.5), F32(-0.0), x)
    return np.where(g.random((rows, n)) < 1.0 / 9.0, F32(NAN), x).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# D. mean_diff
# ---------------------------------------------------------------------------------------------------------------------
DIFF_TRIP = 1024 * 256                  # elements of one trip of the partial kernel's loop: the grid is capped at 1024 x 256
DIFF_EXACT_N = (1, 63, 64, 255, 256, 257, DIFF_TRIP, DIFF_TRIP + 1, DIFF_TRIP + 257)
DIFF_RANDN_N = (1000, 300001)


def diff_blocks(n):
    """Workgroups of diff_partial_kernel = the floats of `partial` the call writes."""
    return min(1024, (n + 255) // 256)


def diff_exact_inputs(n):
    """a - b integer-valued in [-3, 3]: sum |d| <= 3 n and sum d^2 <= 9 n stay below 2^24 for every n of DIFF_EXACT_N."""
    assert 9 * n < EXACT_LIMIT
    g = gen(23, n)
    b = g.integers(-4, 5, size=n).astype(F32)
    d = g.integers(-3, 4, size=n).astype(F32)
    return b + d, b


def diff_exact_expected(a, b, l1):
    """float(sum) * (1.0f / float(n)), the launcher's scale and the final kernel's product."""
    d = a.astype(F64) - b.astype(F64)
    total = int((np.abs(d) if l1 else d * d).sum())
    assert total < EXACT_LIMIT
    return F32(total) * (F32(1.0) / F32(len(a)))


def diff_randn_inputs(n):
    g = gen(29, n)
    return g.standard_normal(n).astype(F32), g.standard_normal(n).astype(F32)


def diff_reference(a, b, l1):
    """(fp64 mean, bound) -- module docstring."""
    n = len(a)
    d = a.astype(F64) - b.astype(F64)
    term = np.abs(d) if l1 else d * d
    mean = math.fsum(term.tolist()) / n
    return mean, (gamma(n - 1) + ((1 if l1 else 3) + 2) * U) * (1.0 + 4.0 * U) * mean + 1e-45


def diff_twin(a, b, l1):
    """fp32 evaluation in one fixed order (numpy's pairwise sum over the fp32 terms): some order, inside the any-order bound."""
    d = a - b
    term = np.abs(d) if l1 else d * d
    return F32(term.sum(dtype=F32)) * (F32(1.0) / F32(len(a)))


# ---------------------------------------------------------------------------------------------------------------------
# E. vertex_err
# ---------------------------------------------------------------------------------------------------------------------
VerrCase = namedtuple("VerrCase", "name F V R region plant")


def _region(name, V, R):
    g = gen(31, V, R)
    if name == "none":
        return None
    if name == "descending":
        return np.sort(g.choice(V, size=R, replace=False))[::-1].astype(np.int32).copy()
    if name == "repeated":
        return g.integers(0, max(V // 8, 1), size=R).astype(np.int32)
    return g.permutation(V)[:R].astype(np.int32) if R <= V else g.integers(0, V, size=R).astype(np.int32)


VERR_CASES = ([VerrCase(f"R{R}", 3, 300, R, "random", None) for R in (1, 63, 255, 256, 257)]
              + [VerrCase(f"all-V{V}", 3, V, V, "none", None) for V in (1, 257)]
              + [VerrCase("descending", 3, 300, 257, "descending", None), VerrCase("repeated", 3, 300, 257, "repeated", None)]
              + [VerrCase(f"max-at-{p}", 3, 300, 257, "random", p) for p in (0, 255, 256)]
              + [VerrCase(f"F{F}", F, 4, 4, "none", None) for F in (1, 255, 256, 257)])


def verr_inputs(case):
    """gt, pred [F, V, 3] fp32 of face size (coordinates of order 0.1, errors of order 1e-3), region int32 [R] or None.  plant: the
    region entry that holds every frame's largest error."""
    g = gen(37, case.F, case.V, case.R, sum(map(ord, case.name)))
    gt = (0.1 * g.standard_normal((case.F, case.V, 3))).astype(F32)
    pred = (gt.astype(F64) + 1e-3 * g.standard_normal((case.F, case.V, 3))).astype(F32)
    region = _region(case.region, case.V, case.R)
    if case.plant is not None:
        pred[:, region[case.plant]] = gt[:, region[case.plant]] + F32(0.05)
    return gt, pred, region


def verr_expected(gt, pred, region):
    """-> dict(frame_max fp32 [F] (exact: numpy's float32 ((dx dx + dy dy) + dz dz).max()), out fp64 [3], out_bound [3],
    frame_sum fp64 [F, 2], frame_sum_bound [F, 2])."""
    F, V = gt.shape[:2]
    sel = np.arange(V) if region is None else region.astype(np.int64)
    R = len(sel)
    with np.errstate(all="ignore"):
        d = gt[:, sel] - pred[:, sel]                                     # fp32 [F, R, 3]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz                                  # fp32, numpy's order over axis 2
        fmax = np.array([np.max(d2[f]) for f in range(F)], dtype=F32)       # np.max propagates NaN
        dd = d.astype(F64)
        nrm = np.sqrt(dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1] + dd[..., 2] * dd[..., 2])
    fs = np.array([[math.fsum(d2[f].astype(F64).tolist()), math.fsum(nrm[f].tolist())] for f in range(F)])
    out = np.array([math.fsum(fmax.astype(F64).tolist()) / F, math.fsum(fs[:, 0].tolist()) / (F * R), math.fsum(fs[:, 1].tolist()) / (F * R)])
    g = gamma(R + F, U64)
    ob = SLACK * np.array([gamma(F + 1, U64), g, g + 3.0 * U64]) * np.abs(out) + 1e-300
    fb = SLACK * np.array([gamma(R, U64), gamma(R, U64) + 3.0 * U64])[None] * np.abs(fs) + 1e-300
    return dict(frame_max=fmax, out=out, out_bound=ob, frame_sum=fs, frame_sum_bound=fb)


def verr_twin(gt, pred, region, defect=None):
    """frame_max as the kernel folds it: a running maximum from 0 over the region.  defect 'fmax_drops_nan': through fmaxf, which
    returns its other operand for a NaN (the kernel before the NaN fix)."""
    F, V = gt.shape[:2]
    sel = np.arange(V) if region is None else region.astype(np.int64)
    out = np.zeros(F, dtype=F32)
    with np.errstate(all="ignore"):
        d = gt[:, sel] - pred[:, sel]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    for f in range(F):
        mx = F32(0.0)
        for v in d2[f]:
            if defect == "fmax_drops_nan":
                mx = mx if np.isnan(v) else (v if np.isnan(mx) else max(mx, v))
            else:
                mx = mx if np.isnan(mx) else (v if np.isnan(v) else max(mx, v))
        out[f] = mx
    return out


# ---------------------------------------------------------------------------------------------------------------------
# F. motion_std
# ---------------------------------------------------------------------------------------------------------------------
MOTION_F = (1, 2, 63, 64, 65, 130)
MOTION_R = (1, 255, 256, 257)
MOTION_V = 300
MOTION_KINDS = ("motion", "near_one", "micro")
MotionCase = namedtuple("MotionCase", "kind F R with_region")
# every size on ordinary motion; the two cancellation kinds at the frame-chunk switch and at both ends, on one vertex and on 257
MOTION_CASES = ([MotionCase("motion", F, R, wr) for F in MOTION_F for R in MOTION_R for wr in (True, False)]
                + [MotionCase(kind, F, R, True) for kind in ("near_one", "micro") for F in (2, 63, 64, 65, 130) for R in (1, 257)])


def motion_id(m):
    return f"{m.kind}-F{m.F}-R{m.R}-{'region' if m.with_region else 'all'}"


def motion_chunks(F):
    """Frame chunks of the launch (fdm_op_motion_std): `partial` holds 2 * motion_chunks(F) * R doubles."""
    return F if F < 64 else 64


def motion_inputs(kind, F, R, with_region, V=MOTION_V):
    """verts [F, V, 3], tmpl [V, 3] fp32, region int32 [R] or None (then V = R).
    'motion': offsets from the template of the template's own size (std of s of the order of its mean);
    'near_one': s about 1 +- 1e-4 (the vertex sits 1 from the template and moves by 5e-5);
    'micro': s about 1e-6 (1 +- 1e-3)."""
    if not with_region:
        V = R
    g = gen(41, F, R, V, MOTION_KINDS.index(kind), int(with_region))
    tmpl = (0.1 * g.standard_normal((V, 3))).astype(F32)
    if kind == "motion":
        off = 0.01 * g.standard_normal((F, V, 3))
    else:
        length, rel = (1.0, 5e-5) if kind == "near_one" else (1e-3, 5e-4)
        axis = g.standard_normal((V, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        off = length * axis[None] * (1.0 + rel * g.standard_normal((F, V, 1)))
    verts = (tmpl.astype(F64)[None] + off).astype(F32)
    region = g.permutation(V)[:R].astype(np.int32) if with_region else None
    return verts, tmpl, region


def motion_s(verts, tmpl, region):
    """s [F, R] fp32, the kernel's expression: ((dx dx + dy dy) + dz dz) of d = verts - tmpl, every operation rounded."""
    sel = np.arange(tmpl.shape[0]) if region is None else region.astype(np.int64)
    d = verts[:, sel] - tmpl[sel][None]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def motion_reference(s):
    """s [F, R] fp32 -> (std_r fp64 [R] two-pass population std, bound_r [R], mean, bound_mean) -- module docstring."""
    F, R = s.shape
    s = s.astype(F64)
    mu = s.mean(0)
    dev = s - mu
    dev = dev - dev.mean(0)                       # the mean in two steps, as tests/norm_cases.py stats64
    std = np.sqrt((dev * dev).mean(0))
    dv = (3.0 * F + 2.0) * U64 * (s * s).mean(0)
    with np.errstate(all="ignore"):
        by_std = np.where(std > 0, dv / std, np.inf)
    bound = SLACK * (np.minimum(np.sqrt(dv), by_std) + U64 * std) + 1e-300
    mean = math.fsum(std.tolist()) / R
    return std, bound, mean, math.fsum(bound.tolist()) / R + SLACK * gamma(R + 1, U64) * mean


def motion_twin(s, chunks=None):
    """The kernel's one pass in double: per chunk (frames F fc / FC .. F (fc + 1) / FC) s1 += s, s2 += s s; the chunks folded in
    order; sqrt(max(s2 / F - mu mu, 0)) -> (std_r [R], mean)."""
    F, R = s.shape
    FC = motion_chunks(F) if chunks is None else chunks
    s = s.astype(F64)
    t1, t2 = np.zeros(R), np.zeros(R)
    for fc in range(FC):
        p1, p2 = np.zeros(R), np.zeros(R)
        for f in range(F * fc // FC, F * (fc + 1) // FC):
            p1 = p1 + s[f]
            p2 = p2 + s[f] * s[f]
        t1, t2 = t1 + p1, t2 + p2
    mu = t1 / F
    std = np.sqrt(np.maximum(t2 / F - mu * mu, 0.0))
    return std, float(std.sum() / R)


# ---------------------------------------------------------------------------------------------------------------------
# G. linear_interp: the host model is mesh_cases.positions, the one restatement of interp_taps (csrc/handoff.hpp)
# ---------------------------------------------------------------------------------------------------------------------
INTERP_T = [(1, 1), (1, 5), (5, 1), (2, 7), (7, 2), (50, 30), (30, 50), (33, 33)]
INTERP_BC = [(1, 1), (3, 5), (1, 1024), (3, 1024)]
INTERP_STRIDE = (1, 30, 513, 1024)      # B, Tin, Tout, C: B Tout C = 525312 > 2048 x 256 = 524288, the grid-stride loop takes a second trip
INTERP_GRID = 2048 * 256


def interp_inputs(B, Tin, C):
    return gen(43, B, Tin, C).standard_normal((B, Tin, C)).astype(F32)


def interp_expected(x, Tout):
    """x [B, Tin, C] -> [B, Tout, C]: l0 x[i0] + l1 x[i1], two products and a sum rounded separately, with the taps of the frame-rate
    rule.  mesh_cases.positions resamples a clip of L frames at fps (a, b) to int(L / a * b) frames: (Tin, Tout) gives Tout exactly,
    and equal rates are the identity there as equal lengths are here."""
    B, Tin, C = x.shape
    assert MC.frames_out(Tin, (Tin, Tout)) == Tout
    return np.stack(MC.positions(x, None, [Tin] * B, (Tin, Tout), dt=np.float32))
