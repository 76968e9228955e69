"""CPU: the host models, case tables and bounds of tests/reduce_cases.py are known good before a GPU sees them.  The exact cases are
exact (every sum below 2^24 is asserted here, not assumed); each host model agrees with torch on the CPU; for every inexact case a
plain evaluation of the kernel's operation order sits inside the stated bound of the fp64 reference; and the cases see the mistakes
the kernels invite (the twins' defects), where a mistake can be seen in values at all."""
import math

import numpy as np
import pytest
import torch

import reduce_cases as RC

F32, F64 = np.float32, np.float64


# ---- A. quantiser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,K", RC.VQ_CK)
def test_vq_cases_are_exact_and_the_model_is_torchs_first_minimum(c, K):
    for B, R in RC.VQ_BR:
        z, cb = RC.vq_inputs(c, K, B, R)
        assert RC.vq_is_exact(z, cb)
        for slices in (np.repeat(RC.clip_books(B).astype(np.int64), R), RC.book_slice(RC.row_books(B * R)), RC.book_slice(RC.row_books(B * R, True))):
            idx, zq = RC.vq_expected(z, cb, K, slices)
            zt, ct = torch.from_numpy(z).double().reshape(B * R, c), torch.from_numpy(cb).double()
            for r in range(B * R):
                E = ct[slices[r] * K:(slices[r] + 1) * K]
                d = ((zt[r][None] - E) ** 2).sum(1)                                   # |z - e|^2, the definition
                assert float(d.max()) < RC.EXACT_LIMIT and int(torch.argmin(d)) == idx[r]
                assert np.array_equal(RC.vq_distances(z.reshape(B * R, c)[r], cb[slices[r] * K:(slices[r] + 1) * K]), d.numpy())
                assert RC.vq_wave_twin(d.numpy()) == idx[r]                            # the lane scan and merge state the same rule
                assert np.array_equal(zq[r // R, :, r % R], cb[slices[r] * K + idx[r]])  # z + (e - z) is the code row itself
    assert int(RC.book_slice(RC.row_books(7, True))[0]) == 0 and int(RC.book_slice(RC.row_books(7, True))[-1]) == 0
    assert len(set(RC.row_books(8)[:4].tolist())) > 1                                # different slices inside one workgroup


@pytest.mark.parametrize("c,K", sorted(RC.VQ_TIES))
@pytest.mark.parametrize("rowbook", [False, True], ids=["clip", "rows"])
def test_vq_tie_cases_have_two_nearest_codes_and_see_a_wrong_tie_rule(c, K, rowbook):
    z, cb, slices, pairs = RC.vq_tie_inputs(c, K, rowbook)
    assert RC.vq_is_exact(z, cb)
    idx, _ = RC.vq_expected(z, cb, K, slices)
    flipped = {d: 0 for d in RC.VQ_DEFECTS}
    zr = z.reshape(-1, c)
    for r, (lo, hi) in enumerate(pairs):
        d = RC.vq_distances(zr[r], cb[slices[r] * K:(slices[r] + 1) * K])
        assert sorted(np.nonzero(d == d.min())[0].tolist()) == [lo, hi] and d.min() == 0.0, (r, lo, hi)
        assert idx[r] == lo and RC.vq_wave_twin(d) == lo
        for defect in RC.VQ_DEFECTS:
            flipped[defect] += RC.vq_wave_twin(d, defect) != lo
    if K <= 64:
        assert flipped.pop("scan_le") == 0                                              # one code per lane: the scan has no tie to break
    assert all(n > 0 for n in flipped.values()), flipped
    kinds = {"neighbours": any(hi == lo + 1 for lo, hi in pairs), "ends": (0, K - 1) in pairs}
    if K > 64:
        kinds["one lane"] = any(hi == lo + 64 for lo, hi in pairs)
        kinds["lower index in the later lane"] = any(lo % 64 > hi % 64 for lo, hi in pairs)
        kinds["lower index in the earlier lane"] = any(lo % 64 < hi % 64 and hi > lo + 1 for lo, hi in pairs)
    if K > 133:
        kinds["one lane, two trips apart"] = any(hi == lo + 128 for lo, hi in pairs)
        assert (5, 70) in pairs and (70, 133) in pairs
    assert all(kinds.values()), kinds


@pytest.mark.parametrize("c,K", [(3, 5), (64, 65)])
def test_vq_rows_without_a_finite_distance_take_code_0(c, K):
    z, cb = RC.vq_nonfinite_inputs(c, K)
    slices = np.repeat(RC.clip_books(2).astype(np.int64), 5)
    idx, zq = RC.vq_expected(z, cb, K, slices)
    zr = z.reshape(10, c)
    for r in (3, 4):
        d = RC.vq_distances(zr[r], cb[slices[r] * K:(slices[r] + 1) * K])
        assert not bool((d < np.inf).any()) and idx[r] == 0 and RC.vq_wave_twin(d) == 0
    assert bool(np.isnan(d).any() or np.isinf(d).all())
    clean_idx, clean_zq = RC.vq_expected(RC.vq_inputs(c, K, 2, 5)[0], cb, K, slices)
    keep = [r for r in range(10) if r not in (3, 4)]
    assert np.array_equal(idx[keep], clean_idx[keep])                                   # finite neighbours untouched
    assert bool(np.isnan(zq[0, c // 2, 3])) and bool(np.isnan(zq[0, 0, 4])) and int(np.isnan(zq).sum()) == 2


# ---- B. vq_stats ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.STATS_CASES, ids=RC.stats_id)
def test_vq_stats_model_against_torch_and_the_perplexity_bound(case):
    z, cb, idx = RC.stats_inputs(case)
    rows = case.B * case.R
    for slices in (np.repeat(RC.clip_books(case.B).astype(np.int64), case.R), RC.book_slice(RC.row_books(rows, True))):
        for beta in (0.25, 0.3):
            want = RC.stats_expected(z, cb, case.K, slices, idx, beta)                  # (asserts its own exactness)
            e = torch.from_numpy(cb).double()[torch.from_numpy(slices * case.K + idx)]
            mse = float(torch.nn.functional.mse_loss(e, torch.from_numpy(z).double().reshape(rows, case.c)))
            assert abs(float(want["loss"]) - (1.0 + beta) * mse) <= 4.0 * RC.U * (1.0 + beta) * mse
        assert np.array_equal(want["hist"], torch.bincount(torch.from_numpy(idx), minlength=case.K).numpy())
        oh = torch.nn.functional.one_hot(torch.from_numpy(idx), case.K).float().numpy()
        assert np.array_equal(want["onehot"], oh)
        p = torch.from_numpy(oh).double().mean(0)
        perp = float(torch.exp(-(p * torch.log(p + 1e-10)).sum()))
        assert abs(want["perp"] - perp) <= 1e-6 * perp                                  # (torch's p_k and 1e-10 are fp64: the fp32 p_k differ by u)
        twin = RC.perplexity_twin(want["hist"], rows)
        assert abs(twin - want["perp"]) <= want["perp_bound"], (twin, want["perp"], want["perp_bound"])
        assert want["perp_bound"] <= 2e-5 * want["perp"]                                # a bound, not a licence
        if case.idx_kind == "one_code":
            assert abs(1.0 - want["perp"]) <= want["perp_bound"] and twin == 1.0


def test_vq_stats_sizes_reach_the_second_grid_trip_and_the_final_kernels_second_loop():
    assert RC.stats_blocks(4096) == 1024 and 4 * RC.stats_blocks(4096) == 4096            # exactly one trip
    assert RC.stats_blocks(4099) == 1024 and 4099 - 4096 == 3                            # a second trip of three rows
    assert {s.K for s in RC.STATS_CASES} >= {1, 63, 256, 257} and {s.B * s.R for s in RC.STATS_CASES} >= {1, 3, 4, 5, 4096, 4099}
    z, cb, i0 = RC.stats_inputs(RC.StatsCase(1, 5, 5, 63, "random"), seed=0)
    _, _, i1 = RC.stats_inputs(RC.StatsCase(1, 5, 5, 63, "random"), seed=1)
    assert not np.array_equal(i0, i1)                                                  # the histogram-reuse test has two index sets


# ---- C. argmax --------------------------------------------------------------------------------------------------------------
def test_argmax_model_is_torchs_first_maximum_and_states_the_nan_rule():
    for rows in RC.ARGMAX_ROWS:
        for n in RC.ARGMAX_N:
            x = RC.argmax_inputs(rows, n)
            got = RC.argmax_first(x)
            clean = ~np.isnan(x).any(1)
            assert np.array_equal(got[clean], torch.argmax(torch.from_numpy(x[clean]), dim=1).numpy().astype(np.int32))
    assert bool(np.isnan(RC.argmax_inputs(130, 7)).any()) and bool((RC.argmax_inputs(130, 7) == 0).any())
    for row, want in RC.ARGMAX_EDGE_ROWS:
        assert int(RC.argmax_first(np.array([row], dtype=F32))[0]) == want, row
    nan_rows = [(r, w) for r, w in RC.ARGMAX_EDGE_ROWS if np.isnan(r).any()]
    torch_says = [int(torch.argmax(torch.tensor(r))) for r, _ in nan_rows]
    assert [w for _, w in nan_rows] != torch_says                                      # the rule is not torch's on NaN: it is stated, not inherited


# ---- D. mean_diff -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RC.DIFF_EXACT_N)
def test_mean_diff_exact_cases_are_exact(n):
    a, b = RC.diff_exact_inputs(n)
    d = a.astype(F64) - b.astype(F64)
    assert bool((d == np.round(d)).all()) and float(np.abs(d).max()) <= 3.0 and bool(((a - b).astype(F64) == d).all())
    assert 9 * n < RC.EXACT_LIMIT and float((d * d).sum()) < RC.EXACT_LIMIT and float(np.abs(d).sum()) < RC.EXACT_LIMIT
    ta, tb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
    for l1, ref in ((False, float(torch.nn.functional.mse_loss(ta, tb))), (True, float(torch.nn.functional.l1_loss(ta, tb)))):
        want = RC.diff_exact_expected(a, b, l1)
        assert want.dtype == F32 and abs(float(want) - ref) <= 2.0 * RC.U * ref        # 1 / n and the product: two roundings
    assert float(RC.diff_exact_expected(a, a, False)) == 0.0
    assert RC.diff_blocks(n) == min(1024, -(-n // 256))


def test_mean_diff_sizes_cross_the_grid_cap():
    assert RC.DIFF_TRIP == 1024 * 256 and RC.diff_blocks(RC.DIFF_TRIP) == 1024 and RC.diff_blocks(RC.DIFF_TRIP + 1) == 1024
    assert RC.diff_blocks(RC.DIFF_TRIP - 1) == 1024 and RC.diff_blocks(257) == 2 and RC.diff_blocks(256) == 1


@pytest.mark.parametrize("n", RC.DIFF_RANDN_N)
@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
def test_mean_diff_bound_holds_for_a_plain_fp32_evaluation(n, l1):
    a, b = RC.diff_randn_inputs(n)
    ref, bound = RC.diff_reference(a, b, l1)
    ta, tb = torch.from_numpy(a).double(), torch.from_numpy(b).double()
    tref = float(torch.nn.functional.l1_loss(ta, tb) if l1 else torch.nn.functional.mse_loss(ta, tb))
    assert abs(ref - tref) <= 1e-12 * ref
    assert abs(float(RC.diff_twin(a, b, l1)) - ref) <= bound
    seq = F32(0.0)                                                                     # the worst order a kernel could take: one running sum
    for t in (np.abs(a - b) if l1 else (a - b) * (a - b))[:20000]:
        seq = F32(seq + t)
    ref20k, bound20k = RC.diff_reference(a[:20000], b[:20000], l1) if n > 20000 else (ref, bound)
    assert abs(float(seq * (F32(1.0) / F32(min(n, 20000)))) - ref20k) <= bound20k
    assert bound <= 0.04 * ref                                                         # gamma(300000) = 0.018: an any-order bound is wide


# ---- E. vertex_err ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.VERR_CASES, ids=lambda c: c.name)
def test_vertex_err_model_against_torch(case):
    gt, pred, region = RC.verr_inputs(case)
    want = RC.verr_expected(gt, pred, region)
    sel = torch.arange(case.V) if region is None else torch.from_numpy(region).long()
    assert len(sel) == case.R
    d = torch.from_numpy(gt)[:, sel] - torch.from_numpy(pred)[:, sel]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert RC.same_bits(want["frame_max"], d2.max(1).values.numpy())
    assert RC.same_bits(want["frame_max"], RC.verr_twin(gt, pred, region))
    dd = d.double()
    ref = [float(d2.max(1).values.double().mean()), float(d2.double().mean()), float(dd.pow(2).sum(-1).sqrt().mean())]
    assert bool((np.abs(want["out"] - np.array(ref)) <= 1e-12 * np.abs(want["out"])).all())
    assert bool((want["out_bound"] <= 1e-12 * np.abs(want["out"]) + 1e-299).all())
    if case.plant is not None:
        where = np.argmax(np.where(True, (gt[:, region] - pred[:, region]).astype(F64) ** 2, 0).sum(-1), axis=1)
        assert bool((where == case.plant).all())
    if case.region == "descending":
        assert bool((np.diff(region) < 0).all())
    if case.region == "repeated":
        assert len(set(region.tolist())) < len(region)


def test_vertex_err_nan_cases_see_a_maximum_that_drops_nan():
    case = RC.VERR_CASES[2]                                                             # R = 255 of V = 300
    gt, pred, region = RC.verr_inputs(case)
    clean = RC.verr_expected(gt, pred, region)
    inside = pred.copy()
    inside[1, region[100], 2] = np.nan
    want = RC.verr_expected(gt, inside, region)
    assert bool(np.isnan(want["frame_max"][1])) and bool(np.isnan(want["out"]).all())
    assert RC.same_bits(want["frame_max"][[0, 2]], clean["frame_max"][[0, 2]])
    assert RC.same_bits(RC.verr_twin(gt, inside, region), want["frame_max"])
    dropped = RC.verr_twin(gt, inside, region, "fmax_drops_nan")
    assert bool(np.isfinite(dropped).all()) and not RC.same_bits(dropped, want["frame_max"])
    outside = pred.copy()
    outside[1, sorted(set(range(case.V)) - set(region.tolist()))[0]] = np.nan
    assert RC.same_bits(RC.verr_expected(gt, outside, region)["frame_max"], clean["frame_max"])


# ---- F. motion_std ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.MOTION_CASES, ids=RC.motion_id)
def test_motion_std_one_pass_in_double_stays_inside_the_bound(case):
    verts, tmpl, region = RC.motion_inputs(*case)
    s = RC.motion_s(verts, tmpl, region)
    assert s.dtype == F32 and s.shape == (case.F, case.R)
    std, bound, mean, bound_mean = RC.motion_reference(s)
    tstd = torch.from_numpy(s).double().std(0, unbiased=False).numpy() if case.F > 1 else np.zeros(case.R)
    assert bool((np.abs(std - tstd) <= 1e-6 * std + 1e-30).all())                      # (torch's own two-pass std loses digits to the offset)
    for chunks in (None, 1, min(case.F, 7)):                                           # whatever the chunking, the same bound
        tw, tw_mean = RC.motion_twin(s, chunks)
        assert bool((np.abs(tw - std) <= bound).all()), float((np.abs(tw - std) / bound).max())
        assert abs(tw_mean - mean) <= bound_mean
    if case.F == 1:
        assert float(np.abs(RC.motion_twin(s)[0]).max()) == 0.0 and float(std.max()) == 0.0
    if case.kind == "near_one":
        assert bool((np.abs(s - 1.0) < 1e-3).all()) and bool((std < 1e-3).all())
    if case.kind == "micro":
        assert bool((np.abs(s / 1e-6 - 1.0) < 2e-2).all())
    if case.kind != "motion" and case.F >= 63:                                         # small motion: the bound is far from relative to u^2 ..
        assert float((bound / std).max()) > 100.0 * RC.U64
    assert bound_mean < 1e-4 * mean or case.F == 1                                     # .. and still tells a std from a wrong one


def test_motion_std_constant_vertex_gives_zero_or_the_floor():
    verts, tmpl, region = RC.motion_inputs("motion", 65, 5, True)
    verts[:] = verts[0][None]                                                           # no motion at all
    s = RC.motion_s(verts, tmpl, region)
    std, bound, mean, bound_mean = RC.motion_reference(s)
    assert float(std.max()) == 0.0 and mean == 0.0
    tw, tw_mean = RC.motion_twin(s)
    floor = RC.SLACK * np.sqrt((3.0 * 65 + 2.0) * RC.U64 * (s.astype(F64) ** 2).mean(0))
    assert bool((tw <= bound).all()) and bool((bound <= floor + 1e-299).all()) and tw_mean <= bound_mean


def test_motion_std_sizes_cross_the_chunk_switch():
    assert [RC.motion_chunks(F) for F in RC.MOTION_F] == [1, 2, 63, 64, 64, 64]
    assert {(m.F, m.R) for m in RC.MOTION_CASES if m.kind == "motion"} == {(F, R) for F in RC.MOTION_F for R in RC.MOTION_R}


# ---- G. linear_interp -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tin,Tout", RC.INTERP_T)
def test_linear_interp_model_against_torch(Tin, Tout):
    for B, C in ((1, 1), (3, 5)):
        x = RC.interp_inputs(B, Tin, C)
        want = RC.interp_expected(x, Tout)
        assert want.dtype == F32 and want.shape == (B, Tout, C)
        ref = torch.nn.functional.interpolate(torch.from_numpy(x).double().transpose(1, 2), size=Tout, mode="linear", align_corners=True).transpose(1, 2).numpy()
        assert bool((np.abs(want - ref) <= 64.0 * RC.U * np.abs(x).max()).all())        # fl((Tin - 1) / (Tout - 1)) t errs by <= 2u Tin
        if Tin == Tout:
            assert RC.same_bits(want, x)
        if Tin == 1 or Tout == 1:
            assert RC.same_bits(want, np.repeat(x[:, :1], Tout, axis=1))


def test_linear_interp_stride_case_is_past_one_grid():
    B, Tin, Tout, C = RC.INTERP_STRIDE
    assert B * Tout * C > RC.INTERP_GRID and B * Tout * C < 2 * RC.INTERP_GRID
    assert {(1, 1), (3, 5)} <= set(RC.INTERP_BC) and {c for _, c in RC.INTERP_BC} == {1, 5, 1024} and {b for b, _ in RC.INTERP_BC} == {1, 3}


def test_bounds_are_made_of_the_stated_constants():
    assert RC.U == 2.0 ** -24 and RC.U64 == 2.0 ** -53 and RC.R_T == 4.0 * RC.U and RC.SLACK == 2.0
    assert math.isclose(RC.gamma(300000), 300000 * RC.U / (1 - 300000 * RC.U))
