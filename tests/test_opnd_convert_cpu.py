"""CPU: the host model of the fp32 -> operand-kind conversion (tests/opnd_cases.py) is right and its value set sees the mistakes
this code invites.  The model is integer arithmetic on bit patterns; here it meets three statements it shares no code with --
torch's CPU casts, NC.round_kind and attn_cases.split_host -- and must agree with each wherever they are defined.  Then the
split kind's precision claim, the twins, the layouts, and the float32 restatements the GPU file compares the movers with."""
import numpy as np
import pytest
import torch

import mesh_cases as MC
import norm_cases as NC
import opnd_cases as OC
import reduce_cases as RC
from attn_cases import split_host
from opnd_cases import BF16, F16, F16X3, F32

KIND_IDS = lambda k: OC.KIND_NAMES[k]  # noqa: E731
INTERP_T = [(1, 1), (1, 4), (5, 1), (7, 7), (2, 5), (101, 61), (61, 101)]
U = 2.0 ** -24


def u16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def values_f32():
    return torch.from_numpy(OC.f32_of(OC.VALUES).copy())


def exact64(kind, planes):
    """fp64 value of stored planes of a 16-bit kind."""
    dt = torch.bfloat16 if kind == BF16 else torch.float16
    p = [torch.from_numpy(pl.view(np.int16).copy()).view(dt).double().numpy() for pl in planes]
    return p[0] + p[1] / 2048.0 if kind == F16X3 else p[0]


# ---------------------------------------------------------------------------------------------------------------------
# the value set
# ---------------------------------------------------------------------------------------------------------------------
def test_value_set_holds_the_classes_it_names():
    v = set(int(x) for x in OC.VALUES)
    assert len(v) == OC.NV == 65536 * 6
    named = {"+0": 0x00000000, "-0": 0x80000000, "smallest fp32 subnormal": 0x00000001, "largest fp32 subnormal": 0x007FFFFF,
             "-subnormal": 0x807FFFFF, "+inf": 0x7F800000, "-inf": 0xFF800000, "quiet NaN": 0x7FC00000, "-quiet NaN": 0xFFC00000,
             "signalling NaN": 0x7F800001, "-signalling NaN": 0xFF800001, "signalling NaN, low word": 0x7F80FFFF,
             "65408, below the clamp": 0x477F8000, "65535.996, above it": 0x477FFFFF, "65536": 0x47800000, "2^-14": 0x38800000, "just below 2^-14": 0x387FFFFF, "2^-24": 0x33800000, "2^-25": 0x33000000,
             "just above 2^-25": 0x33000001, "just below 2^-25": 0x32FFFFFF, "bf16 overflow edge": 0x7F7F8000,
             "just below it": 0x7F7F7FFF, "fp32 max": 0x7F7FFFFF, "bf16 tie, even": 0x3F808000, "bf16 tie, odd": 0x3F818000,
             "bf16 near-tie below": 0x3F807FFF, "bf16 near-tie above": 0x3F808001}
    for name, bits in named.items():
        assert bits in v, name
    for e in range(256):                                     # every exponent with the all-zero and the all-one mantissa
        assert (e << 23) in v and ((e << 23) | 0x7FFFFF) in v and (0x80000000 | (e << 23)) in v
    # fp16 ties: none in the normal range (13 bits dropped, none of the lower halves has the low 13 bits 0x1000) -- TIES_F16 has
    # them; 65504 and 65520 themselves: EDGES_F16
    low13 = {lo & 0x1FFF for lo in OC.LOWER}
    assert 0x1000 not in low13 and 0x477FE000 not in v and 0x477FF000 not in v
    assert {0x477FE000, 0x477FF000, 0xC77FE000, 0xC77FF000} <= set(int(x) for x in OC.EDGES_F16)
    assert len(OC.EXTRA) == len(OC.TIES_F16) + len(OC.EDGES_F16) and not (set(int(x) for x in OC.EXTRA) & v)
    t = OC.TIES_F16
    assert len(set(int(x) for x in t)) == len(t) == 2 * 30 * 4 * 3
    assert {int(x) & 0x1FFF for x in t} == {0x0FFF, 0x1000, 0x1001}
    e = (t.astype(np.int64) >> 23) & 0xFF
    assert int(e.min()) == 127 - 14 and int(e.max()) == 127 + 15


def test_tiled_shifts_by_the_repeat_number():
    n = 2 * OC.GRID + 1
    t = OC.tiled(n)
    assert np.array_equal(t[:OC.NV], OC.VALUES)
    assert np.array_equal(t[OC.NV:2 * OC.NV - 1], OC.VALUES[1:]) and t[2 * OC.NV - 1] == OC.VALUES[0]
    for step in (1, OC.GRID, OC.NV):                         # a neighbour, a grid stride on, a repeat on: another value
        same = t[:-step] == t[step:]
        assert float(same.mean()) < 1e-3, step
    for kind in OC.SIXTEEN:                                  # ... and, in all but a sliver, another stored word
        s = OC.stored_tiled(kind, OC.GRID + 257)[:OC.GRID + 257]
        assert float((s[:-OC.GRID] == s[OC.GRID:]).mean()) < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# agreement with the other statements of the rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", ["VALUES", "EXTRA"])
def test_model_agrees_with_torch_round_kind_and_split_host(values):
    bits = getattr(OC, values)
    x = torch.from_numpy(OC.f32_of(bits).copy())
    ok = OC.in_f16_range(bits)
    assert int(ok.sum()) > 0.4 * len(bits)
    want = {BF16: u16(x.bfloat16())[None], F16: u16(x.half())[None], F16X3: u16(split_host(x))}
    for kind in OC.SIXTEEN:
        got = OC.convert(kind, bits)
        assert got.dtype == np.uint16 and got.shape == want[kind].shape
        for pl in range(got.shape[0]):
            msg = OC.first_mismatch(kind, got[pl][ok], want[kind][pl][ok], bits[ok], f"{values} plane {pl} vs torch")
            assert msg is None, msg
        # NC.round_kind returns the VALUE of what is stored: compare as fp64 values, zeros by their sign too
        rk = NC.round_kind(kind, x).double().numpy()[ok]
        mine = exact64(kind, [pl[ok] for pl in got])
        assert np.array_equal(mine, rk) and np.array_equal(np.signbit(mine), np.signbit(rk)), OC.KIND_NAMES[kind]
    # bf16 beyond fp16's range: every finite value, overflow to inf included; inf stays inf; a NaN stays a NaN
    fin = (bits.astype(np.int64) & 0x7FFFFFFF) <= 0x7F800000
    got, ref = OC.convert(BF16, bits)[0], u16(x.bfloat16())
    assert np.array_equal(got[fin], ref[fin])
    assert np.array_equal(OC.is_nan16(got, OC.FMT_BF16), ~fin)
    assert np.array_equal(OC.convert(F32, bits)[0], bits)


def test_model_outside_fp16_range_follows_the_stated_rule():
    """What no other host statement covers: the clamp's edges, the infinities and the NaNs of the fp16 kinds."""
    x = np.array([0x477FE000, 0x477FE001, 0x477FEFFF, 0x477FF000, 0x47800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0xC77FE001,
                  0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF80FFFF, 0x80000000, 0x00000001, 0x807FFFFF], np.uint32)
    hi = [0x7BFF] * 7 + [0xFBFF] * 2 + [0xFBFF] * 2 + [0x7BFF] * 2 + [0x8000, 0x0000, 0x8000]      # quiet NaNs: the lower bound; signalling: the upper
    assert [int(v) for v in OC.convert(F16, x)[0]] == hi
    p = OC.convert(F16X3, x)
    assert [int(v) for v in p[0]] == hi
    assert [int(v) for v in p[1]] == [0] * 13 + [0x0000, 0x0000, 0x8000]      # -0 -> (-0, +0); -subnormal -> (-0, -0)
    b = OC.convert(BF16, x)[0]
    assert [int(v) for v in b[:9]] == [0x4780, 0x4780, 0x4780, 0x4780, 0x4780, 0x7F80, 0x7F80, 0xFF80, 0xC780]
    assert bool(OC.is_nan16(b[9:13], OC.FMT_BF16).all()) and [int(v) for v in b[13:]] == [0x8000, 0x0000, 0x8080]
    assert int(OC.convert(BF16, np.array([0x7F7F8000], np.uint32))[0, 0]) == 0x7F80      # the overflow edge is a tie to even: inf
    assert int(OC.convert(BF16, np.array([0x7F7F7FFF], np.uint32))[0, 0]) == 0x7F7F


# ---------------------------------------------------------------------------------------------------------------------
# the split kind's precision
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", ["VALUES", "EXTRA"])
def test_split_kind_holds_22_bits(values):
    """|x - (hi + lo / 2048)| <= 2^-22 |x| + 2^-36 for every finite |x| <= 65504, in fp64 (where hi + lo / 2048 is exact).

    r = x - float(hi) is exact in fp32: where hi is normal, r is a multiple of x's last place and |r| <= half a last place of hi
    = 2^-11 2^e <= 2^-11 |x| (e the exponent of x), which is 2^12 last places of x: it fits; below 2^-14, hi is a multiple of
    2^-24, |r| <= 2^-25 and |r| <= |x| (hi = 0, or |x| >= 2^-25), and r is a multiple of x's last place again.  The scaling by
    2^11 only moves the exponent up: exact.  lo = fp16(2048 r) is the one rounding: where 2048 |r| >= 2^-14 it is relative,
    |2048 r - lo| <= 2^-11 2048 |r|, so |r - lo / 2048| <= 2^-11 |r| <= 2^-22 |x| (and <= 2^-11 2^-25 = 2^-36 below fp16's normal
    range); where 2048 |r| < 2^-14 it is absolute, half of 2^-24: 2^-25 / 2048 = 2^-36.  Either term alone covers its case, the sum
    covers both: the constants of the issue are the derived ones.  2048 |r| <= |x| <= 65504: lo never overflows."""
    bits = getattr(OC, values)
    ok = OC.in_f16_range(bits)
    b = bits[ok]
    x = OC.f32_of(b).astype(np.float64)
    hi, lo = OC.convert(F16X3, b)
    for pl in (hi, lo):
        assert not bool((OC.decode(pl, OC.FMT_F16)[3] != OC.FINITE).any()), "a plane holds inf or NaN"
    # the two fp32 operations are exact, as claimed: the exact difference is an fp32 number, and so is its 2048-fold
    h64 = exact64(F16, [hi])
    r = x - h64                                              # (exact in fp64: both are fp32 numbers at most 2^12 last places apart, or hi = 0)
    assert np.array_equal(r.astype(np.float32).astype(np.float64), r)
    assert np.array_equal((r * 2048.0).astype(np.float32).astype(np.float64), r * 2048.0)
    assert bool((np.abs(r) <= np.maximum(2.0 ** -11 * np.abs(x), 2.0 ** -25)).all())
    err = np.abs(x - exact64(F16X3, [hi, lo]))
    bound = 2.0 ** -22 * np.abs(x) + 2.0 ** -36
    i = int((err / bound).argmax())
    print(f"SPLIT_QUALITY {values}: worst error / bound {float(err[i] / bound[i]):.4f} at input {int(b[i]):#010x}")
    assert bool((err <= bound).all()), (hex(int(b[i])), float(err[i]), float(bound[i]))
    # one plane alone does not meet it: the bound asserts the lo plane's work
    assert float((np.abs(x - h64) / bound).max()) > 1000.0


# ---------------------------------------------------------------------------------------------------------------------
# the twins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake,kind", [(m, k) for m, kinds in OC.MISTAKES.items() for k in kinds],
                         ids=lambda v: v if isinstance(v, str) else OC.KIND_NAMES[v])
def test_every_mistake_is_caught_by_the_value_set(mistake, kind):
    """The model with one mistake switched on differs from the model on VALUES, at the element named for it."""
    n = OC.NV
    want = OC.stored(kind, OC.VALUES, fill=0xFFFF)
    got = OC.stored(kind, OC.VALUES, fill=0xFFFF, mistake=mistake)
    if mistake in ("lo_at_n_minus_1", "lo_at_n_plus_1"):
        # one element early: lo[0] lands on hi[n - 1] (and the last word of the lo plane keeps the fill it had); one late: word n
        # keeps its fill and lo[n - 1] lands behind the destination.  The GPU test holds the destination between guards.
        at = n - 1 if mistake == "lo_at_n_minus_1" else n
        m = min(len(got), len(want))
        assert got[at] != want[at], (mistake, at)
        assert len(got) != len(want) or got[2 * n - 1] != want[2 * n - 1]
        k = int((got[:m] != want[:m]).sum())
        print(f"MISTAKE {mistake} {OC.KIND_NAMES[kind]}: caught at word {at} of the destination (got {int(got[at]):#06x}, "
              f"want {int(want[at]):#06x}); {k} words differ")
        return
    w = OC.WITNESS[(mistake, kind)]
    at = np.nonzero(OC.VALUES == w)[0]
    assert len(at) == 1, f"{w:#010x} is not an element of VALUES"
    i = int(at[0])
    planes = [i, n + i] if kind == F16X3 else [i]
    assert any(got[j] != want[j] for j in planes), (mistake, OC.KIND_NAMES[kind], hex(w))
    assert not bool(OC.same_stored(kind, got, want).all())
    k = int((~OC.same_stored(kind, got, want)).sum())
    print(f"MISTAKE {mistake} {OC.KIND_NAMES[kind]}: caught at element {i}, input {w:#010x}: twin "
          f"{[hex(int(got[j])) for j in planes]}, model {[hex(int(want[j])) for j in planes]}; {k} words differ")


def test_the_comparison_takes_any_bf16_nan_and_nothing_else():
    want = np.array([0x7FC0, 0x3F80, 0x7F80], np.uint16)
    assert bool(OC.same_stored(BF16, np.array([0xFFFF, 0x3F80, 0x7F80], np.uint16), want).all())
    assert list(OC.same_stored(BF16, np.array([0x7F80, 0x3F81, 0x7FC0], np.uint16), want)) == [False, False, False]
    assert list(OC.same_stored(F16, np.array([0x7E00, 0x7E01], np.uint16), np.array([0x7E00, 0x7E00], np.uint16))) == [True, False]
    msg = OC.first_mismatch(F16, np.array([1, 2], np.uint16), np.array([1, 3], np.uint16), np.array([7, 9], np.uint32), "t")
    assert "word 1" in msg and "0x00000009" in msg and "got 0x0002" in msg and "want 0x0003" in msg


# ---------------------------------------------------------------------------------------------------------------------
# the movers' host expressions
# ---------------------------------------------------------------------------------------------------------------------
def test_mover_expectations_are_the_index_arithmetic_they_claim():
    d = 5
    x = np.arange(4 * d, dtype=np.float32)
    assert np.array_equal(OC.bias_act_expected(x, np.arange(d, dtype=np.float32) * 100)[6:8], [106.0, 207.0])
    x3 = np.arange(2 * 3 * 2, dtype=np.float32).reshape(2, 3, 2)
    rep, zer = OC.pad_rows_expected(x3, 2, False), OC.pad_rows_expected(x3, 2, True)
    assert rep.shape == (2, 7, 2) and np.array_equal(rep[1, :, 0], [6, 6, 6, 8, 10, 10, 10]) and np.array_equal(zer[1, :, 0], [0, 0, 6, 8, 10, 0, 0])
    x4 = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    g = OC.group_pad_expected(x4, 2, 1)
    assert g.shape == (2, 2, 5, 2) and np.array_equal(g[1, 1, :, 0], [0, 14, 18, 22, 0]) and np.array_equal(g[0, 0, :, 1], [0, 1, 5, 9, 0])
    m = OC.masked_expected(np.full((3, 4), np.nan, np.float32), [0, 1, 4])
    assert np.array_equal(np.isnan(m), [[False] * 4, [True, False, False, False], [True] * 4]) and not np.signbit(m[0]).any()
    M = 3 * 101 * 7 * 11
    a, b, c = (np.arange(mod, dtype=np.float32)[:, None] * s for (_, mod), s in zip(OC.ADD_ROWS_MAPS, (1.0, 1000.0, 1e6)))
    want = OC.add_rows_expected(M, a, b, c)[:, 0]
    for m_ in (0, 1, 3, 50, 101, 549, M - 1):
        assert want[m_] == (m_ % 101) + 1000.0 * ((m_ // 3) % 7) + 1e6 * ((m_ // 50) % 11)
    assert len({(m_ % 101, (m_ // 3) % 7, (m_ // 50) % 11) for m_ in range(M)}) > 101 * 7      # three maps, out of phase


@pytest.mark.parametrize("Tin,Tout", INTERP_T)
def test_interp_restatement_against_fp64(Tin, Tout):
    """The float32 restatement of interp_taps the GPU file uses (mesh_cases.positions through reduce_cases.interp_expected)
    against the same expression in fp64.  src = fl(fl((Tin - 1) / (Tout - 1)) t) carries two roundings, 2u (Tin - 1) at most; it
    moves l1 (the subtraction is exact) and, through l1, the result by 2u (Tin - 1) |x[i1] - x[i0]| <= 4u (Tin - 1) max|x| -- the
    interpolant is continuous, so a floor that falls on the other side of an integer changes nothing in this; the two products
    and the sum add 3u max|x|.  End frames: t = 0 takes 1 x[0] + 0 x[1]; the last frame is exact whenever src reaches Tin - 1
    exactly, which these cases do (asserted)."""
    for C in (3, 67):
        x = RC.interp_inputs(2, Tin, C)
        want = RC.interp_expected(x, Tout)
        fps = (Tin, Tout)
        ref = np.stack(MC.positions(x.astype(np.float64), None, [Tin] * 2, fps, dt=np.float64))
        assert want.dtype == np.float32 and want.shape == ref.shape == (2, Tout, C)
        assert bool((np.abs(want - ref) <= (4.0 * (Tin - 1) + 3.0) * U * np.abs(x).max()).all())
        assert RC.same_bits(want[:, 0], x[:, 0])
        if Tout > 1:
            assert RC.same_bits(want[:, -1], x[:, -1])
        if Tin == Tout:
            assert RC.same_bits(want, x)
