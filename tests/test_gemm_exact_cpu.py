"""CPU: the case list of tests/gemm_cases.py proven before a GPU is involved.  Every (kind, case) satisfies the conditions that
make bit equality legitimate; the CPU twin of the GEMM contract (gemm_cases.model: flat offsets, k-tiles, fp32 arithmetic)
reproduces the fp64 reference exactly; and every mistake these kernels invite, switched on in the twin, is seen by at least one
case the GPU file runs -- so an identical slip in a kernel cannot stay green there."""
import pytest
import torch

import gemm_cases as GC

KIND_IDS = lambda k: GC.KIND_NAMES[k]  # noqa: E731


@pytest.mark.parametrize("kind", GC.KINDS, ids=KIND_IDS)
def test_every_case_is_exact(kind):
    for case in GC.CASES:
        try:
            GC.assert_exact(kind, case)
        except AssertionError as e:
            raise AssertionError(f"{GC.KIND_NAMES[kind]} {case.id}: {e}") from e


@pytest.mark.parametrize("kind", GC.KINDS, ids=KIND_IDS)
def test_model_equals_reference(kind):
    for case in GC.CASES:
        want, got = GC.expected(kind, case), GC.model(kind, case)
        assert sorted(want) == sorted(got) == sorted(GC.outputs_of(GC.problem(kind, case)))
        for name in want:
            assert GC.identical(got[name], want[name]), f"{GC.KIND_NAMES[kind]} {case.id}: the twin's {name} differs from the reference"


def test_case_list_covers_the_forms():
    """The table of the case list: every tile-edge row count, column count, k depth and form is present."""
    cs = GC.CASES
    assert {1, 63, 64, 65, 79, 81, 129, 257} <= {c.M for c in cs}
    assert {4, 60, 64, 68, 132, 200, 67, 1} <= {c.N for c in cs}
    assert {1, 2, 3, 4, 5, 9} <= {c.ku for c in cs if not c.K} and any(c.K == 2048 for c in cs)
    assert {"gap", "overlap"} <= {c.lda for c in cs} and any(c.ldo for c in cs) and any(c.ldr for c in cs)
    assert {1, 7} <= {c.rmod for c in cs} and all(c.M % c.rmod for c in cs if c.rmod > 1)
    assert {(True, True), (True, False), (False, True), (False, False)} <= {(c.bias, c.resid) for c in cs}
    assert {GC.ACT_NONE, GC.ACT_RELU, GC.ACT_LEAKY02} <= {c.act for c in cs} and {"f32", "t", "both"} <= {c.out for c in cs}
    assert {1, 3, 8} <= {c.G for c in cs if not c.C}
    assert {1, 3} <= {c.C for c in cs} and {4, 8} <= {c.G for c in cs if c.C} and all(c.M % 64 for c in cs if c.C)
    assert {2, 4} <= {c.S for c in cs}
    assert {33, 47} <= {c.kv[2] for c in cs if c.kv} and {64, 128} <= {c.kv[3] for c in cs if c.kv} and all(c.kv[0] == 2 for c in cs if c.kv) and any(c.kv[1] == 2 for c in cs if c.kv)
    assert any(c.stat and c.M % 16 for c in cs) and any(c.lo == "zero" and not c.stat for c in cs)


@pytest.mark.parametrize("mistake", sorted(GC.MISTAKES))
def test_every_mistake_is_seen(mistake):
    """For every kind the mistake can show in: some case's buffers differ from the reference once the twin makes it."""
    for kind in GC.MISTAKES[mistake]:
        caught = None
        for case in sorted(GC.CASES, key=lambda c: not GC.can_show(mistake, c)):      # (stable: the likely cases first, then all the others)
            want, got = GC.expected(kind, case), GC.model(kind, case, mistake)
            if any(not GC.identical(got[n], want[n]) for n in want):
                caught = case
                break
        assert caught is not None, f"{mistake} ({GC.KIND_NAMES[kind]}): no case sees it -- a case is missing"
        print(f"GEMM_MISTAKE {mistake} {GC.KIND_NAMES[kind]}: caught by {caught.id}")


def test_truncation_needs_the_rounding_case():
    """The ordinary cases' outputs are small integers, exact in bf16 and fp16: only the "round" case can tell round-to-nearest
    from truncation, and it does so away from ties as well (an odd multiple of half an ulp would hide a round-half-up)."""
    case = next(c for c in GC.CASES if c.values == "round")
    for kind in (GC.BF16, GC.F16):
        ref = GC.reference(kind, case)
        x, t = ref.f32[0], ref.t[0]
        inexact = x != t
        assert bool(inexact.any())
        ulp = 2.0 ** (torch.floor(torch.log2(x.abs().clamp_min(1.0))) - (7 if kind == GC.BF16 else 10))
        assert bool(((x - t).abs()[inexact] < ulp[inexact] / 2).any()), "only ties: add a value off the midpoint"
