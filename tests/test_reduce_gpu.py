"""GPU: the kernels that search or reduce to a scalar (csrc/elementwise.hpp: the VQ nearest-code search, its statistics, the row
argmax, mean_diff, vertex_err, motion_std, linear_interp), called through fdm_amd.ops, against the host models of
tests/reduce_cases.py: indices, one-hots, histograms, the exact losses and means, frame_max and the interpolation on every element
bit for bit; perplexity, the randn means, the metric sums and the motion std inside the bounds derived there.  Every output buffer is
pre-filled with NaN (floats) or -1 (integers) between two guards of 64 sentinel elements (the twin of tests/test_norm_edges_gpu.py's
Out for any dtype): no guard may change.  tests/test_reduce_cpu.py shows the cases are exact where they claim to be and see the
mistakes these kernels invite."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import reduce_cases as RC  # noqa: E402
from fdm_amd import ops  # noqa: E402
from fdm_amd._lib import FdmError  # noqa: E402

DEV = "cuda:0"
GUARD, SENT = 64, -7.0
F32, F64 = np.float32, np.float64
WORST = {}


class Buf:
    """An output of `shape` and torch `dtype`, NaN (floats) or -1 (integers) all over, 64 sentinel elements on each side."""

    def __init__(self, shape, dtype=torch.float32):
        self.n = n = math.prod(shape)
        self.raw = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=DEV)
        self.raw[GUARD:GUARD + n] = float("nan") if dtype.is_floating_point else -1
        self.t = self.raw[GUARD:GUARD + n].view(shape)

    def np(self, what=""):
        """The written region on the host, after a synchronize and the guard check."""
        torch.cuda.synchronize()
        g = torch.cat([self.raw[:GUARD], self.raw[GUARD + self.n:]])
        assert bool((g == SENT).all()), f"{what}: a guard element was written"
        return self.t.cpu().numpy()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ratio(op, err, bound, what):
    r = float(np.max(np.where(np.isfinite(err), err / bound, np.inf)))
    WORST[op] = max(WORST.get(op, 0.0), r)
    print(f"REDUCE_RATIO {op} {what} {r:.4f} (worst so far: {WORST[op]:.4f})")
    assert r <= 1.0, f"{op} {what}: error / bound = {r:.4g} (error {float(np.max(err)):.4g}, bound {float(np.max(bound)):.4g})"


# ---------------------------------------------------------------------------------------------------------------------
# A. the quantiser on exactly representable data
# ---------------------------------------------------------------------------------------------------------------------
def vq_launch(z, cb, K, book, rowbook):
    """-> (idx int64 [B R], z_q fp32 [B, c, R]) of ops.vq_quant (book [B]) or ops.vq_quant_rows (book [B R])."""
    B, R, c = z.shape
    zq, idx = Buf((B, c, R)), Buf((B * R,), torch.int64)
    zd, cd, bd = dev(z), dev(cb), dev(book)
    if rowbook:
        ops.vq_quant_rows(zd, cd, bd, RC.N_BOOKS, B, R, c, K, zq.t, idx.t)
    else:
        ops.vq_quant(zd, cd, bd, B, R, c, K, zq.t, idx.t)
    return idx.np("idx"), zq.np("z_q")


def vq_check(z, cb, K, book, rowbook, tag):
    slices = RC.book_slice(book) if rowbook else np.repeat(book.astype(np.int64), z.shape[1])
    want_idx, want_zq = RC.vq_expected(z, cb, K, slices)
    idx, zq = vq_launch(z, cb, K, book, rowbook)
    bad = np.nonzero(idx != want_idx)[0]
    assert len(bad) == 0, f"{tag}: rows {bad[:8].tolist()} took codes {idx[bad[:8]].tolist()}, the first minimum is {want_idx[bad[:8]].tolist()}"
    assert RC.same_bits(zq, want_zq), f"{tag}: z_q is not the chosen code row"
    return idx


@pytest.mark.parametrize("c,K", RC.VQ_CK)
def test_vq_quant_exact_data_indices_and_zq_bit_for_bit(c, K):
    """Integer data: every distance is exact in any order, so the index is the first minimum of the fp64 distance matrix and z_q the
    chosen code row, for the per-clip book (n_books = 3, a different slice per clip) and the per-row book (a different slice on
    neighbouring rows of one workgroup; entries -1 and n_books read slice 0).  An out-of-range PER-CLIP book is not passed:
    fdm_op_vq_quant has no n_books argument and no clamp, so such an entry is an out-of-bounds read of the codebook."""
    for B, R in RC.VQ_BR:
        z, cb = RC.vq_inputs(c, K, B, R)
        vq_check(z, cb, K, RC.clip_books(B), False, f"vq_quant c{c} K{K} B{B} R{R}")
        vq_check(z, cb, K, RC.row_books(B * R), True, f"vq_quant_rows c{c} K{K} B{B} R{R}")
        vq_check(z, cb, K, RC.row_books(B * R, True), True, f"vq_quant_rows (entries -1, n_books) c{c} K{K} B{B} R{R}")


def test_vq_quant_without_a_book_reads_slice_0():
    z, cb = RC.vq_inputs(64, 65, 2, 5)
    want_idx, want_zq = RC.vq_expected(z, cb, 65, np.zeros(10, dtype=np.int64))
    idx, zq = vq_launch(z, cb, 65, None, False)
    assert np.array_equal(idx, want_idx) and RC.same_bits(zq, want_zq)


@pytest.mark.parametrize("c,K", sorted(RC.VQ_TIES))
@pytest.mark.parametrize("rowbook", [False, True], ids=["clip", "rows"])
def test_vq_quant_equal_distances_take_the_lower_index(c, K, rowbook):
    """Duplicated codebook rows that are the only nearest codes of their latents (distance 0): neighbouring lanes, one lane (k and
    k + 64, k + 128), the lower index in the earlier and in the later lane, (0, K - 1).  The lower index wins every time."""
    z, cb, slices, pairs = RC.vq_tie_inputs(c, K, rowbook)
    book = RC.row_books(len(slices)) if rowbook else RC.clip_books(RC.N_BOOKS)
    idx = vq_check(z, cb, K, book, rowbook, f"ties c{c} K{K}")
    assert idx.tolist() == [lo for lo, _ in pairs]


@pytest.mark.parametrize("c,K", [(3, 5), (64, 65)])
@pytest.mark.parametrize("rowbook", [False, True], ids=["clip", "rows"])
def test_vq_quant_row_without_a_finite_distance_takes_code_0(c, K, rowbook):
    """A NaN in the latent makes every distance NaN, +inf makes every distance NaN or +inf: no `d < best` holds, bk stays
    0x7fffffff and the documented rule `bk >= K -> 0` gives code 0; the finite rows beside them are untouched."""
    z, cb = RC.vq_nonfinite_inputs(c, K)
    book = RC.row_books(10) if rowbook else RC.clip_books(2)
    idx = vq_check(z, cb, K, book, rowbook, f"non-finite c{c} K{K}")
    assert idx[3] == 0 and idx[4] == 0


# ---------------------------------------------------------------------------------------------------------------------
# B. vq_stats
# ---------------------------------------------------------------------------------------------------------------------
class StatsBufs:
    def __init__(self, rows, K, min_enc=True):
        self.me = Buf((rows, K)) if min_enc else None
        self.partial = Buf((RC.stats_blocks(rows),), torch.float64)
        self.hist = Buf((K,), torch.int32)
        self.out = Buf((2,))


def stats_launch(case, z, cb, book, rowbook, idx, beta, bufs):
    args = (case.B, case.R, case.c, case.K, beta, bufs.me.t if bufs.me else None, bufs.partial.t, bufs.hist.t, bufs.out.t)
    if rowbook:
        ops.vq_stats_rows(z, cb, book, RC.N_BOOKS, idx, *args)
    else:
        ops.vq_stats(z, cb, book, idx, *args)
    out = bufs.out.np("out")
    assert bool(np.isfinite(bufs.partial.np("partial")).all()), "a partial the final kernel reads was not written"
    return out, bufs.hist.np("hist"), (bufs.me.np("min_encodings") if bufs.me else None)


@pytest.mark.parametrize("case", RC.STATS_CASES, ids=RC.stats_id)
@pytest.mark.parametrize("rowbook", [False, True], ids=["clip", "rows"])
def test_vq_stats_histogram_onehot_loss_exact_perplexity_bounded(case, rowbook):
    """hist = bincount, min_encodings = the one-hot matrix on every element, loss = beta m + m bit for bit (sq is an exact integer on
    this data), perplexity inside the bound of reduce_cases.perplexity_reference -- also past one grid trip (4096 rows: exactly one
    trip of 1024 workgroups x 4 rows; 4099: a second trip of three rows), for K past the final kernel's k += 256 loop, with and
    without min_encodings (the other outputs keep their bits), and on a second call over the SAME hist / partial buffers with other
    indices (equal to a call on fresh buffers)."""
    rows = case.B * case.R
    z, cb, idx = RC.stats_inputs(case)
    _, _, idx2 = RC.stats_inputs(case, seed=1)
    book = RC.row_books(rows, True) if rowbook else RC.clip_books(case.B)
    slices = RC.book_slice(book) if rowbook else np.repeat(book.astype(np.int64), case.R)
    zd, cd, bd = dev(z), dev(cb), dev(book)
    tag = f"{'vq_stats_rows' if rowbook else 'vq_stats'} {RC.stats_id(case)}"
    beta = 0.25
    shared = StatsBufs(rows, case.K)
    for k, ix in enumerate((idx, idx2)):                       # the second pass reuses hist and partial as the first left them
        want = RC.stats_expected(z, cb, case.K, slices, ix, beta)
        shared.out, shared.me = Buf((2,)), Buf((rows, case.K))
        out, hist, me = stats_launch(case, zd, cd, bd, rowbook, dev(ix), beta, shared)
        assert np.array_equal(hist, want["hist"]), f"{tag} call {k}: histogram"
        assert RC.same_bits(me, want["onehot"]), f"{tag} call {k}: min_encodings"
        assert RC.same_bits(out[0], want["loss"]), f"{tag} call {k}: loss {out[0]!r}, exact value {want['loss']!r}"
        ratio("perplexity", np.abs(np.array([float(out[1]) - want["perp"]])), np.array([want["perp_bound"]]), f"{tag} call {k}")
        if case.idx_kind == "one_code":
            assert abs(float(out[1]) - 1.0) <= want["perp_bound"], f"{tag}: one code, perplexity {out[1]!r}"
        fresh, fhist, _ = stats_launch(case, zd, cd, bd, rowbook, dev(ix), beta, StatsBufs(rows, case.K))
        assert RC.same_bits(fresh, out) and np.array_equal(fhist, hist), f"{tag} call {k}: reused buffers differ from fresh ones"
        bare, bhist, _ = stats_launch(case, zd, cd, bd, rowbook, dev(ix), beta, StatsBufs(rows, case.K, min_enc=False))
        assert RC.same_bits(bare, out) and np.array_equal(bhist, hist), f"{tag} call {k}: outputs depend on min_encodings"
    for b2 in (0.3,):                                          # a beta that is not a power of two: beta m rounds
        want = RC.stats_expected(z, cb, case.K, slices, idx, b2)
        out, _, _ = stats_launch(case, zd, cd, bd, rowbook, dev(idx), b2, StatsBufs(rows, case.K, min_enc=False))
        assert RC.same_bits(out[0], want["loss"]), f"{tag} beta {b2}"


# ---------------------------------------------------------------------------------------------------------------------
# C. argmax_rows and the per-clip argmax
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", RC.ARGMAX_ROWS)
@pytest.mark.parametrize("n", RC.ARGMAX_N)
@pytest.mark.parametrize("rep", RC.ARGMAX_REP)
def test_argmax_rows_is_the_first_maximum(rows, n, rep):
    """The kernel's rule, restated by reduce_cases.argmax_first: from column 0, a later column takes over on v > best alone (ties: the
    first; a NaN in column 0 stays, elsewhere never wins), written rep times per row."""
    x = RC.argmax_inputs(rows, n)
    want = np.repeat(RC.argmax_first(x), rep)
    for n_books in (n, n + 2):
        out = Buf((rows * rep,), torch.int32)
        ops.argmax_rows(dev(x), out.t, rows, n, rep, n_books)
        assert np.array_equal(out.np(f"argmax rows {rows} n {n} rep {rep}"), want), f"rows {rows} n {n} rep {rep} n_books {n_books}"


def test_argmax_rows_ties_signed_zeros_and_nan():
    for row, want in RC.ARGMAX_EDGE_ROWS:
        x = np.array([row] * 3, dtype=F32)
        out = Buf((6,), torch.int32)
        ops.argmax_rows(dev(x), out.t, 3, len(row), 2, len(row))
        assert out.np(str(row)).tolist() == [want] * 6, row


def test_argmax_rows_refusals():
    x, out = dev(np.zeros((4, 3), dtype=F32)), Buf((4,), torch.int32)
    with pytest.raises(FdmError):
        ops.argmax_rows(x, out.t, 4, 3, 1, 2)                  # n > n_books: the argmax could name a book outside the codebook
    with pytest.raises(FdmError):
        ops.argmax_rows(x, out.t, 4, 3, 0, 3)                  # rep = 0
    assert bool((out.np("refused") == -1).all())


def test_per_clip_argmax_of_the_vq_plan():
    """argmax_rows_kernel (csrc/encoders.hip) through VQPlan.quant on the mead preset: all zeros -> book 0, two equal maxima -> the
    lower, a soft vector -> its argmax; each with the bits of the same call given the equivalent one-hot vector."""
    from fdm_amd._lib import F32 as KF32
    from fdm_amd.vq import VQPlan
    from oracle import weights as W
    p = W.PRESETS["mead"]
    plan = VQPlan("mead", W.make_vq_weights("mead"), KF32, DEV)
    z = torch.randn(3, 2 * p["G"], p["c"], generator=torch.Generator().manual_seed(5)) * (1.5 / 256)
    emo = torch.zeros(3, p["n_books"])
    emo[1, 2] = emo[1, 5] = 0.7
    emo[1, 0] = 0.1
    emo[2] = torch.tensor([0.05, 0.1, 0.05, 0.1, 0.45, 0.2, 0.05])
    books = [0, 2, 4]
    zq, idx = plan.quant(z, emo)
    zq1, idx1 = plan.quant(z, torch.eye(p["n_books"])[books])
    assert torch.equal(idx, idx1) and torch.equal(zq.view(torch.int32), zq1.view(torch.int32))
    assert not torch.equal(idx, plan.quant(z, torch.eye(p["n_books"])[[0, 5, 4]])[1])      # (the books do tell: the other maximum differs)


# ---------------------------------------------------------------------------------------------------------------------
# D. mean_diff
# ---------------------------------------------------------------------------------------------------------------------
def diff_launch(a, b, l1):
    n = a.numel()
    partial, out = Buf((RC.diff_blocks(n),)), Buf((1,))       # guarded at exactly the block count the launcher uses
    got = ops.mean_diff(a, b, l1=l1, partial=partial.t, out=out.t)
    assert got.data_ptr() == out.t.data_ptr()
    v = out.np(f"mean_diff n {n} out")
    assert bool(np.isfinite(partial.np(f"mean_diff n {n} partial")).all()), "a partial the final kernel reads was not written"
    return v[0]


@pytest.mark.parametrize("n", RC.DIFF_EXACT_N)
def test_mean_diff_exact_cases_bit_for_bit(n):
    """a - b integer-valued in [-3, 3]: every partial and the total are exact, the result is float(sum) * (1.0f / float(n)) -- past
    the grid cap of 1024 x 256 elements as well, where a workgroup takes a second trip."""
    a, b = RC.diff_exact_inputs(n)
    ad, bd = dev(a), dev(b)
    for l1 in (False, True):
        got, want = diff_launch(ad, bd, l1), RC.diff_exact_expected(a, b, l1)
        assert RC.same_bits(got, want), f"n {n} l1 {l1}: {got!r}, exact value {want!r}"
        zero = diff_launch(ad, ad.clone(), l1)
        assert RC.bits(zero) == 0, f"n {n} l1 {l1}: a == b gave {zero!r}, not +0.0"
    assert float(ops.mean_diff(ad, bd)[0]) == float(RC.diff_exact_expected(a, b, False))      # the wrapper's own scratch


@pytest.mark.parametrize("n", RC.DIFF_RANDN_N)
@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_mean_diff_randn_within_the_any_order_bound(n, l1):
    a, b = RC.diff_randn_inputs(n)
    ref, bound = RC.diff_reference(a, b, l1)
    got = diff_launch(dev(a), dev(b), l1)
    ratio("mean_diff", np.array([abs(float(got) - ref)]), np.array([bound]), f"n {n} {'l1' if l1 else 'l2'}")
    assert RC.same_bits(diff_launch(dev(a), dev(b), l1), got)                                   # deterministic


# ---------------------------------------------------------------------------------------------------------------------
# E. vertex_err
# ---------------------------------------------------------------------------------------------------------------------
def verr_launch(gt, pred, region, tag):
    F, V = gt.shape[:2]
    R = V if region is None else len(region)
    fmax, fsum, out = Buf((F,)), Buf((F, 2), torch.float64), Buf((3,), torch.float64)
    ops.vertex_err(dev(gt), dev(pred), dev(region), R, F, V, fmax.t, fsum.t, out.t)
    return fmax.np(tag + " frame_max"), fsum.np(tag + " frame_sum"), out.np(tag + " out")


@pytest.mark.parametrize("case", RC.VERR_CASES, ids=lambda c: c.name)
def test_vertex_err_frame_max_bit_for_bit_sums_bounded(case):
    """frame_max[f] is numpy's float32 ((dx dx + dy dy) + dz dz).max() over the region, bit for bit -- at R around the 256 threads of
    a workgroup, without a region, for a descending and a repeating region, with the maximum at the first, the 256th and the last
    region entry, and for F around the final kernel's f += 256 loop; the double sums and the three outputs inside their bounds."""
    gt, pred, region = RC.verr_inputs(case)
    want = RC.verr_expected(gt, pred, region)
    fmax, fsum, out = verr_launch(gt, pred, region, case.name)
    assert RC.same_bits(fmax, want["frame_max"]), f"{case.name}: frame_max"
    ratio("vertex_err", np.abs(fsum - want["frame_sum"]), want["frame_sum_bound"], case.name + " frame_sum")
    ratio("vertex_err", np.abs(out - want["out"]), want["out_bound"], case.name + " out")


def test_vertex_err_nan_in_the_region_is_reported_outside_it_ignored():
    """One NaN coordinate of a region vertex in one frame of three: that frame's maximum and all three outputs are NaN (numpy's max
    propagates it; a metric must not score a clean lip error for a model that emits NaN on the lips), the other frames' maxima keep
    their bits.  A NaN at a vertex outside the region changes nothing."""
    for case, at in ((RC.VERR_CASES[2], 100), (RC.VERR_CASES[4], 256), (RC.VERR_CASES[0], 0)):       # R = 255, 257 (second trip), 1
        gt, pred, region = RC.verr_inputs(case)
        clean = verr_launch(gt, pred, region, case.name)
        for coord in range(3):
            inside = pred.copy()
            inside[1, region[at], coord] = np.nan
            want = RC.verr_expected(gt, inside, region)
            fmax, fsum, out = verr_launch(gt, inside, region, case.name + " NaN")
            assert bool(np.isnan(fmax[1])) and RC.same_bits(fmax, want["frame_max"]), f"{case.name}: frame_max {fmax.tolist()}"
            assert RC.same_bits(fmax[[0, 2]], clean[0][[0, 2]])
            assert bool(np.isnan(out).all()) and bool(np.isnan(fsum[1]).all()) and RC.same_bits(fsum[[0, 2]], clean[1][[0, 2]])
        outside = pred.copy()
        outside[1, sorted(set(range(case.V)) - set(region.tolist()))[0]] = np.nan
        got = verr_launch(gt, outside, region, case.name + " NaN outside")
        assert all(RC.same_bits(g, c) for g, c in zip(got, clean))
    gt, pred, _ = RC.verr_inputs(RC.VERR_CASES[6])                                                     # no region, V = 257
    pred[2, 256, 1] = np.nan
    fmax, _, out = verr_launch(gt, pred, None, "all NaN")
    assert np.isnan(fmax).tolist() == [False, False, True] and bool(np.isnan(out).all())


def test_vertex_err_equal_sequences_give_exact_zeros():
    gt, _, region = RC.verr_inputs(RC.VERR_CASES[4])
    for got in verr_launch(gt, gt.copy(), region, "equal"):
        assert int(np.count_nonzero(RC.bits(got))) == 0


# ---------------------------------------------------------------------------------------------------------------------
# F. motion_std
# ---------------------------------------------------------------------------------------------------------------------
def motion_launch(verts_d, tmpl_d, region, R, F, V, tag):
    partial, out = Buf((2 * RC.motion_chunks(F) * R,), torch.float64), Buf((1,), torch.float64)      # exactly what the launch writes
    ops.motion_std(verts_d, tmpl_d, dev(region), R, F, V, partial.t, out.t)
    v = out.np(tag + " out")
    assert bool(np.isfinite(partial.np(tag + " partial")).all()), "a partial the final kernel reads was not written"
    return float(v[0])


@pytest.mark.parametrize("case", RC.MOTION_CASES, ids=RC.motion_id)
def test_motion_std_within_the_one_pass_bound(case):
    """Against the fp64 two-pass population std of the fp32 s values: the mean over the region inside bound_mean, and single region
    vertices (R = 1 regions: the first, the middle, the last, the one with the smallest std) inside their own bound -- F on both
    sides of the switch from FC = F to 64 frame chunks, R around the 256 threads of a workgroup, and the two kinds of data on which
    s2 / F - mu mu cancels.  F = 1 gives exactly 0."""
    verts, tmpl, region = RC.motion_inputs(*case)
    V = tmpl.shape[0]
    std, bound, mean, bound_mean = RC.motion_reference(RC.motion_s(verts, tmpl, region))
    vd, td = dev(verts), dev(tmpl)
    tag = RC.motion_id(case)
    got = motion_launch(vd, td, region, case.R, case.F, V, tag)
    if case.F == 1:
        assert got == 0.0 and not math.copysign(1.0, got) < 0, f"{tag}: one frame gave {got!r}"
    ratio("motion_std", np.array([abs(got - mean)]), np.array([bound_mean]), tag + " mean")
    if case.with_region:
        picks = sorted({0, case.R // 2, case.R - 1, int(np.argmin(std))})
        one = np.array([motion_launch(vd, td, region[r:r + 1], 1, case.F, V, f"{tag} vertex {r}") for r in picks])
        ratio("motion_std", np.abs(one - std[picks]), bound[picks], tag + " single vertices")


def test_motion_std_constant_vertex_gives_zero_or_the_floor():
    """No motion at all: s is constant over the frames, the variance is 0 and s2 / F - mu mu is rounding alone; fmax(.., 0) takes
    what falls below zero and what stays above is inside the bound's floor sqrt(dv)."""
    for F in (1, 2, 63, 65):
        verts, tmpl, region = RC.motion_inputs("motion", F, 257, True)
        verts[:] = verts[0][None]
        std, bound, mean, bound_mean = RC.motion_reference(RC.motion_s(verts, tmpl, region))
        assert mean == 0.0
        got = motion_launch(dev(verts), dev(tmpl), region, 257, F, tmpl.shape[0], f"constant F {F}")
        assert 0.0 <= got <= bound_mean, (F, got, bound_mean)


# ---------------------------------------------------------------------------------------------------------------------
# G. linear_interp
# ---------------------------------------------------------------------------------------------------------------------
def interp_check(B, Tin, Tout, C):
    x = RC.interp_inputs(B, Tin, C)
    want = RC.interp_expected(x, Tout)
    y = Buf((B, Tout, C))
    ops.linear_interp(dev(x), y.t, B, Tin, Tout, C)
    got = y.np(f"linear_interp B{B} {Tin}->{Tout} C{C}")
    assert RC.same_bits(got, want), f"B{B} {Tin}->{Tout} C{C}: {int((RC.bits(got) != RC.bits(want)).sum())} elements differ"
    if Tin == Tout:
        assert RC.same_bits(got, x)                            # equal lengths: the identity


@pytest.mark.parametrize("Tin,Tout", RC.INTERP_T)
def test_linear_interp_every_element_bit_for_bit(Tin, Tout):
    """l0 x[i0] + l1 x[i1] with the taps of interp_taps, two products and a sum rounded separately: the host model is
    mesh_cases.positions, the restatement the mesh tests use."""
    for B, C in RC.INTERP_BC:
        interp_check(B, Tin, Tout, C)


def test_linear_interp_past_one_grid():
    interp_check(*RC.INTERP_STRIDE)                            # (B, Tin, Tout, C) with B Tout C > 2048 x 256


def test_worst_ratios_are_reported():
    """Not a check of its own: prints the largest error / bound each operator reached in this session (pytest -s)."""
    for op, r in sorted(WORST.items()):
        print(f"REDUCE_WORST {op} {r:.4f}")
    assert all(r <= 1.0 for r in WORST.values())
