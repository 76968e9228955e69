"""Host: the twins and the bounds of tests/epilogue_cases.py.  The clean twins (fp32 torch in the kernel's order of operations) sit
inside every bound over the full case list; every seeded defect pushes at least one case over its bound; gelu_erf_fast's formula
error is re-measured; the bound stays a small stated fraction of the reference, so that a loose bound cannot hide a failure."""
import itertools

import pytest
import torch

import epilogue_cases as EC
import gemm_cases as GC
import norm_cases as NC
from epilogue_cases import ACT_GELU_ERF, ACT_LEAKY02, ACT_RELU, BF16, F32  # noqa: E402

KIND_IDS = lambda k: EC.KIND_NAMES[k]  # noqa: E731
ACT_IDS = lambda a: EC.ACT_NAMES[a]  # noqa: E731
LAUNCHES = list(itertools.product(EC.SHAPES, ("grid", "special"), (False, True)))


def gemm_ratio(kind, act, shape, launch, resid, defect=None, ulps=None):
    """Worst error-to-bound ratio of the twin over both outputs of one launch (a non-finite value counts as infinite)."""
    got = EC.gemm_twin(kind, act, shape, launch, resid, defect, ulps)
    return max(EC.worst(got[out], *EC.gemm_reference(kind, act, shape, launch, resid, out))[0] for out in ("f32", "t"))


@pytest.mark.parametrize("act", EC.HEAVY, ids=ACT_IDS)
@pytest.mark.parametrize("kind", EC.KINDS, ids=KIND_IDS)
def test_clean_gemm_twin_is_inside_every_bound(kind, act):
    top = 0.0
    for shape, launch, resid in LAUNCHES:
        got = EC.gemm_twin(kind, act, shape, launch, resid)
        for out in ("f32", "t"):
            ref, bnd = EC.gemm_reference(kind, act, shape, launch, resid, out)
            assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bnd).all()) and bool((bnd > 0).all())
            r, idx, err, b = EC.worst(got[out], ref, bnd)
            assert r <= 1.0, f"{shape} {launch} resid={resid} out_{out}: twin / bound = {r:.4g} at {idx}: error {err:.4g}, bound {b:.4g}"
            top = max(top, r)
    print(f"EPI_TWIN_RATIO gemm {EC.ACT_NAMES[act]} {EC.KIND_NAMES[kind]} ({EC.kind_class(kind)}) {top:.4f}")


@pytest.mark.parametrize("act", (ACT_RELU, ACT_LEAKY02), ids=ACT_IDS)
def test_exact_controls(act):
    """ReLU and LeakyReLU(0.2) are exact: the twin equals the fp64 reference rounded once, in every kind; ReLU's bound is the floor."""
    for kind, launch in itertools.product(EC.KINDS, ("grid", "special")):
        _, _, v, _ = EC.act_problem(kind, "ragged", launch)
        assert torch.equal(EC.act_twin(kind, act, v).double(), EC.act64(v, act).float().double())
        if act == ACT_RELU:
            assert float(EC.act_bound(EC.fast_kind(kind), act, v).max()) <= 1e-30


@pytest.mark.parametrize("act", EC.ALL_ACTS, ids=ACT_IDS)
def test_clean_flat_twins_are_inside_every_bound(act):
    top = 0.0
    vs = [EC.bias_act_problem(size, vec)[2] for size in ("small", "large") for vec in (False, True)]
    vs += [EC.small_linear_problem(size, K)[3] for size in ("small", "large") for K in (1, 8)]
    for v in vs:
        r, idx, err, b = EC.worst(EC.act_twin(F32, act, v), *EC.flat_reference(act, v))
        assert r <= 1.0, f"twin / bound = {r:.4g} at {idx} (v = {float(v[idx])!r}): error {err:.4g}, bound {b:.4g}"
        top = max(top, r)
    print(f"EPI_TWIN_RATIO flat {EC.ACT_NAMES[act]} f32 {top:.4f}")


def test_value_lists_hold_what_they_claim():
    vals = EC.flat_values()
    sp = set(EC.specials().tolist())
    for x in (0.0, 2.0 ** -126, -2.0 ** -126, 20.0, -20.0, 44.0, -45.0, 88.0, -89.0, 100.0, -1e4, 65504.0, -65520.0, 65520.0):
        assert x in sp
    for x in (1e-30, 7e4, 1e13, 3e38):
        assert float(torch.tensor(x, dtype=torch.float32)) in sp and -float(torch.tensor(x, dtype=torch.float32)) in sp
    assert bool((EC.specials().view(torch.int32) == torch.tensor(-0.0).view(torch.int32)).any())                     # -0 itself
    assert EC.dense_grid().numel() == 48 * 64 + 1 and float(EC.dense_grid()[0]) == -24.0 and float(EC.dense_grid()[-1]) == 24.0
    for size, vec in itertools.product(("small", "large"), (False, True)):
        x, w, v = EC.bias_act_problem(size, vec)
        assert (x.numel() < 256) == (size == "small") and x.shape[1] % 4 != 0
        if size == "large":
            assert set(vals.tolist()) <= set(x.reshape(-1).tolist())
    for size, K in itertools.product(("small", "large"), (1, 8)):
        x, W, bias, v = EC.small_linear_problem(size, K)
        assert (v.numel() < 256) == (size == "small") and v.shape[1] % 4 != 0 and x.shape[1] == K
        if size == "large":
            assert set(EC.dense_grid()[:-1].tolist()) <= set(v.reshape(-1).tolist())
        else:
            assert torch.equal(v[0].view(torch.int32)[2:], bias.view(torch.int32)[2:])                               # row I = 0: the specials themselves
    for kind, shape in itertools.product(EC.KINDS, EC.SHAPES):
        _, _, v, _ = EC.act_problem(kind, shape, "grid")
        assert set(EC.dense_grid().tolist()) <= set(v.reshape(-1).tolist())
        p, bias, v, _ = EC.act_problem(kind, shape, "special")
        assert int((torch.arange(p.M) % 3 == 0).sum()) >= 20 and torch.equal(v[0, 2:].view(torch.int32), bias[2:].view(torch.int32))


DEFECT_CASES = [(d, a, k) for d, (acts, kinds) in EC.DEFECTS.items() for a in acts for k in kinds]


@pytest.mark.parametrize("defect,act,kind", DEFECT_CASES, ids=lambda x: x if isinstance(x, str) else None)
def test_every_defect_leaves_a_bound(defect, act, kind):
    top = max(gemm_ratio(kind, act, shape, launch, resid, defect) for shape, launch, resid in LAUNCHES)
    print(f"EPI_DEFECT {defect} {EC.ACT_NAMES[act]} {EC.KIND_NAMES[kind]}: worst ratio {top:.4g}")
    assert top > 1.0


@pytest.mark.parametrize("kind", EC.KINDS, ids=KIND_IDS)
def test_missing_softplus_threshold_is_benign(kind):
    """Recorded, not wished for: without the threshold the form still returns v beyond 20 (IEEE infinities, the overflow-safe tanh)."""
    (acts, _), = EC.BENIGN.values()
    top = max(gemm_ratio(kind, acts[0], shape, launch, resid, "softplus_no_threshold") for shape, launch, resid in LAUNCHES)
    print(f"EPI_BENIGN softplus_no_threshold {EC.KIND_NAMES[kind]}: worst ratio {top:.4g}")
    assert top <= 1.0


def test_perturbed_hardware_primitives_move_the_ratio():
    """The protocol for an allowance the GPU exceeds works: an exp / log that is off by more ulps than HW_ULPS shows in the ratio."""
    base = max(gemm_ratio(BF16, EC.ACT_MISH, "interior", "grid", False), 1e-3)
    far = gemm_ratio(BF16, EC.ACT_MISH, "interior", "grid", False, ulps=(64.0, 64.0))
    print(f"EPI_ULPS mish bf16: clean {base:.4f}, exp and log off by 64 ulp {far:.4f}")
    assert far > 1.0 > base


def test_gelu_fast_formula_error_is_the_recorded_constant():
    e = NC.gelu_fast_formula_error()
    assert 0.5 * NC.GELU_FAST_FORMULA_ERR < e <= NC.GELU_FAST_FORMULA_ERR
    v = EC.flat_values().double()                                  # and it holds over this module's values, which reach beyond [-8, 8]
    e2 = float((NC.gelu_fast_formula(v) - EC.gelu_erf64(v)).abs().max())
    print(f"EPI_GELU_FAST formula error {e:.4g} on norm_cases' grid, {e2:.4g} over the epilogue values")
    assert e2 <= NC.GELU_FAST_FORMULA_ERR
    w = torch.linspace(-8.0, 8.0, 4001, dtype=torch.float64)
    assert float((EC.gelu_erf64(w) - NC.gelu64(w)).abs().max()) < 1e-14
    assert float((EC.gelu_tanh64(w) - torch.nn.functional.gelu(w, approximate="tanh")).abs().max()) < 1e-12
    assert float((EC.mish64(w) - torch.nn.functional.mish(w)).abs().max()) < 1e-12


@pytest.mark.parametrize("act", EC.HEAVY, ids=ACT_IDS)
def test_bound_is_a_small_fraction_of_the_reference(act):
    """Over the dense grid: bound <= SANITY (|ref| + 1) for fp32 outputs, (u_T + SANITY) (|ref| + 1) for out_t."""
    top = 0.0
    for kind, shape, resid in itertools.product(EC.KINDS, EC.SHAPES, (False, True)):
        for out in ("f32", "t"):
            ref, bnd = EC.gemm_reference(kind, act, shape, "grid", resid, out)
            frac = float((bnd / (ref.abs() + 1.0)).max())
            lim = EC.SANITY + (NC.u_out(kind, "t") + 2.0 ** -25 if out == "t" else 0.0)
            assert frac <= lim, (EC.KIND_NAMES[kind], shape, resid, out, frac, lim)
            if out == "f32":
                top = max(top, frac)
    print(f"EPI_BOUND_FRACTION {EC.ACT_NAMES[act]}: bound / (|ref| + 1) <= {top / EC.U:.1f} u on the dense grid (limit {EC.SANITY / EC.U:.0f} u)")


def test_operands_are_exact_in_every_kind():
    for kind, shape, launch in itertools.product(EC.KINDS, EC.SHAPES, ("grid", "special")):
        GC.assert_exact(kind, EC.act_case(shape, launch))
        p, bias, v, r = EC.act_problem(kind, shape, launch)
        assert bias.dtype == v.dtype == r.dtype == torch.float32 and v.shape == (p.M, p.N)


# ---------------------------------------------------------------------------------------------------------------------
# the LayerNorm fold
# ---------------------------------------------------------------------------------------------------------------------
FOLD_CASES = list(itertools.product(EC.NPARTS, EC.FOLD_M))


def fold_ratios(kind, nparts, M, defect=None):
    """Worst twin-to-bound ratio of (colsum over both N and both outputs, rln over both outputs) of one (nparts, M)."""
    p = EC.fold_problem(kind, nparts, M)
    st = EC.partials_twin(p.x)
    cs = max(EC.worst(EC.colsum_twin(kind, p, N, st, defect)[out], *EC.colsum_reference(kind, out, p, N, st))[0]
             for N in EC.FOLD_N for out in ("f32", "t"))
    rl = max(EC.worst(EC.rln_twin(kind, p, st, defect)[out], *EC.rln_reference(kind, out, p, st))[0] for out in ("f32", "t"))
    return cs, rl


@pytest.mark.parametrize("kind", EC.KINDS, ids=KIND_IDS)
def test_clean_fold_twins_are_inside_every_bound(kind):
    top = {"producer": 0.0, "producer-real": 0.0, "colsum": 0.0, "rln": 0.0}
    for nparts, M in FOLD_CASES:
        for real in (False, True):
            p = EC.fold_problem(kind, nparts, M, real)
            r, idx, err, b = EC.worst(EC.partials_twin(p.x), *EC.producer_reference(p.x))
            assert r <= 1.0, f"producer nparts={nparts} M={M} real={real}: twin / bound = {r:.4g} at {idx}"
            top["producer-real" if real else "producer"] = max(top["producer-real" if real else "producer"], r)
        cs, rl = fold_ratios(kind, nparts, M)
        assert cs <= 1.0 and rl <= 1.0, (nparts, M, cs, rl)
        top["colsum"], top["rln"] = max(top["colsum"], cs), max(top["rln"], rl)
    for form, r in top.items():
        print(f"EPI_TWIN_RATIO fold {form} {EC.KIND_NAMES[kind]} {r:.4f}")


def test_exact_producer_partials_are_exact_and_rows_are_what_they_claim():
    for nparts, M in FOLD_CASES:
        p = EC.fold_problem(F32, nparts, M)
        st = EC.partials_twin(p.x)
        assert torch.equal(st.double(), EC.producer_reference(p.x)[0])             # integer sums below 2^24
        s = EC.rowstats64(st, p.D)
        for m in range(M):
            k = EC.row_kind(m, nparts)
            row = p.x[m].double()
            if k < 4:
                assert abs(float(row.mean()) - 2.0 * EC.RATIOS[k]) < 0.5 and float(row.max() - row.min()) <= 4.0
            elif k == 4:
                assert float(row.max()) == float(row.min()) and float(s["var"][m]) == 0.0
            else:
                assert float(row[0]) == float(row[1]) + 1.0 and float(row[1:].max()) == float(row[1:].min())
        if p.D in (768, 1088, 1024, 2048):
            assert EC._clamp_constant(p.D)[1] < -EC.EPS32                        # the fp32 variance of the kind-5 row is negative beyond eps


@pytest.mark.parametrize("defect", EC.FOLD_DEFECTS)
def test_every_fold_defect_leaves_a_bound(defect):
    top = max(max(fold_ratios(F32, nparts, M, defect)) for nparts, M in FOLD_CASES)
    print(f"EPI_DEFECT fold {defect}: worst ratio {top:.4g}")
    assert top > 1.0


def test_what_the_fold_gives_up_per_offset_ratio():
    """Reported, not asserted: the colsum consumer's bound relative to the magnitude of its reference, per offset-to-spread ratio
    (nparts = 32, the widest row), next to the bound a two-pass LayerNorm of the same row would have (norm_cases.e_z, s = 17)."""
    p = EC.fold_problem(F32, 32, 65)
    st = EC.partials_twin(p.x)
    ref, bnd = EC.colsum_reference(F32, "f32", p, 64, st)
    z = NC.stats64(p.x, 1, EC.EPS32)
    two_pass = 2.0 * (NC.e_z(z, 17, EC.EPS32).abs() @ p.W1[:64].abs().double().t())
    for k, ratio in enumerate(EC.RATIOS):
        rows = (p.rk == k).nonzero().view(-1)
        frac = float((bnd[rows] / ref[rows].abs().mean()).max())
        frac2 = float((two_pass[rows] / ref[rows].abs().mean()).max())
        print(f"EPI_FOLD_COST offset / spread = {ratio}: fold bound / mean |ref| = {frac:.3g} (a two-pass LayerNorm's: {frac2:.3g})")
        assert frac > 0.0
