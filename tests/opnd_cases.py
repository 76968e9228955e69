"""The fp32 -> operand-kind conversion (csrc/common.hpp: clamp_f16, store_opnd1, store_opnd4; fdm_op_cast and every out_t copy go
through them): a host model in integer arithmetic, the value set it is held to, the mistakes it can be switched to, and the index
arithmetic of the plain movers (csrc/elementwise.hpp), shared by tests/test_opnd_convert_cpu.py and tests/test_opnd_convert_gpu.py.
Plain helper module (pytest does not collect it); host only: nothing here touches a device or loads the library.

The rule, per kind (include/fdm_hip.h at fdm_op_cast says the same)
-------------------------------------------------------------------
  FDM_F32    the 32 bits are copied (signalling NaNs and subnormals included).
  FDM_BF16   round to nearest, ties to even, on the 16 bits that are dropped; fp32 subnormals become bf16 subnormals (same exponent
             range, gradual); inf stays inf; a finite value at or above 2^128 - 2^119 rounds to inf.  A NaN stores a NaN.
  FDM_F16    c = clamp(x, -65504, 65504) first (-0 stays -0, +-inf become +-65504), then round to nearest even with gradual
             underflow: below 2^-14 the result is a multiple of 2^-24, at or below 2^-25 it is a zero of x's sign.  A NaN stores
             a bound, never a NaN: a QUIET NaN of either sign the LOWER bound, -65504 (0xFBFF), a SIGNALLING NaN of either sign the
             UPPER bound, +65504 (0x7BFF).  clamp_f16 is one v_med3_f32, which for a NaN operand returns min(min(x, lo), hi) in the
             kernels' IEEE mode: min drops a quiet NaN (min(x, lo) = lo, then min(lo, hi) = lo) but quiets and RETURNS a signalling
             one (min(x, lo) = quiet x, then min(quiet x, hi) = hi).  Found by these tests on the MI355X and pinned as the rule
             (csrc/common.hpp, include/fdm_hip.h): either way the stored value is finite, which is what the clamp is for, and no
             arithmetic of the device produces a signalling NaN -- only fdm_op_cast can meet one, in data that came from the host.
  FDM_F16X3  hi = fp16(c) as above; lo = fp16((c - float(hi)) * 2048), every fp32 operation rounded once (both are exact, see
             test_opnd_convert_cpu.py), stored lo_off elements after hi (fdm_op_cast: n).  c - float(hi) is +0 when c is exactly an
             fp16 value (round to nearest: x - x = +0), so lo is then +0 whatever the sign of x; a NaN stores (+-65504, +0).

The model works on the bit pattern: decode() turns a pattern of any format into (sign, integer significand, exponent of its last
bit, class), sub() is an fp32 subtraction carried out on those integers, encode() rounds such a triple into a format.  No value is
ever held in a floating-point variable, and no torch or numpy cast takes part: tests/test_opnd_convert_cpu.py then compares the
model with torch's CPU casts, NC.round_kind and split_host wherever those are defined -- two independent statements that must agree.

bf16 NaNs: what `(bf16)v` stores for a NaN depends on how the compiler lowers the conversion (a hardware convert on gfx950, an
integer sequence on older targets; neither is derivable from the source), so a bf16 NaN is compared by NaN-ness, not by payload:
same_stored() accepts any NaN where the model has one.  (Observed on the MI355X, not asserted: the upper half of the input with
the quiet bit set.)  Everything else, in every kind, is compared bit for bit.

The value set
-------------
VALUES: every 16-bit upper half of an fp32 word crossed with the lower halves 0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, the
upper half varying slowest: 393 216 patterns, one pass of a grid of 2048 x 256 lanes.  Both zeros, every fp32 subnormal binade, every
exponent with an all-zero and an all-one mantissa, both infinities, quiet and signalling NaNs of both signs; every tie and near-tie of
bf16 (the lower half IS what bf16 drops); values on both sides of 65504 and 65520 (65408, 65535.996, 65536); 2^-14, 2^-24, 2^-25;
bf16's overflow edge 0x7F7F8000.
What it does NOT hold: fp16 drops 13 bits in its normal range and none of the six lower halves is a tie there (their low 13 bits are
0x0000, 0x0001 or 0x1FFF); fp16 ties appear in VALUES only below 2^-16, where 16 or more bits are dropped.  Nor does it hold 65504
(0x477FE000) or 65520 (0x477FF000, the tie between 65504 and fp16's overflow) themselves.  EXTRA adds both: TIES_F16 -- for every
exponent of fp16's normal range, both signs, four kept-mantissa patterns (even and odd last bits, the carry into the next binade)
and the dropped 13 bits 0x0FFF, 0x1000, 0x1001 -- and EDGES_F16, +-65504 and +-65520 with their two fp32 neighbours each.
tiled(n): the set repeated to n elements with the repeat number added to the index before the lookup, so the element one grid
stride on (or one element on, or n on) holds another value."""
import functools

import numpy as np

from fdm_amd._lib import BF16, F16, F16X3, F32

I64 = np.int64
FMT_F32, FMT_F16, FMT_BF16 = (8, 23), (5, 10), (8, 7)      # (exponent bits, stored mantissa bits)
FINITE, INF, NAN = 0, 1, 2
GRID = 2048 * 256                                           # lanes of the capped 1-D grid (csrc/host.hpp grid_for)
SIXTEEN = (BF16, F16, F16X3)
KIND_NAMES = {F32: "f32", BF16: "bf16", F16: "f16", F16X3: "f16x3"}
F16_MAX_BITS = 0x477FE000                                   # 65504.0f
F16_LOWEST_BITS = 0xC77FE000                                # -65504.0f


# ---------------------------------------------------------------------------------------------------------------------
# integer floating point
# ---------------------------------------------------------------------------------------------------------------------
def _bitlen(v):
    """Bits needed to write v >= 0 (0 for 0)."""
    v = v.copy()
    n = np.zeros(v.shape, I64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (v >> s) != 0
        n += m * s
        v = np.where(m, v >> s, v)
    return n + (v != 0)


def decode(bits, fmt):
    """Pattern of format fmt -> (sign, sig, q, cls): the value is (-1)^sign * sig * 2^q (sig an integer) when cls == FINITE."""
    eb, tm = fmt
    b = np.asarray(bits).astype(I64)
    emax, bias = (1 << eb) - 1, (1 << (eb - 1)) - 1
    s, e, m = (b >> (eb + tm)) & 1, (b >> tm) & emax, b & ((1 << tm) - 1)
    cls = np.where(e == emax, np.where(m == 0, INF, NAN), FINITE)
    sig = np.where(cls == FINITE, np.where(e == 0, m, m | (1 << tm)), 0)
    return s, sig, np.maximum(e, 1) - bias - tm, cls


def encode(num, fmt, rounding="nearest_even", flush_subnormals=False):
    """(sign, sig, q, cls) -> pattern of format fmt: one rounding (to nearest, ties to even), gradual underflow, overflow to inf.
    rounding / flush_subnormals: the mistakes of the twins."""
    s, sig, q, cls = num
    eb, tm = fmt
    emax, bias = (1 << eb) - 1, (1 << (eb - 1)) - 1
    ex = _bitlen(sig) - 1 + q                                # exponent of the leading bit
    et = np.maximum(ex, 1 - bias)                            # ... of the binade the result is rounded in
    shift = et - tm - q                                      # bits of sig below the result's last place
    sh, lsh = np.clip(shift, 0, 62), np.clip(-shift, 0, 62)
    half = np.where(sh > 0, I64(1) << np.maximum(sh - 1, 0), 0)
    if rounding == "nearest_even":
        r = (sig + half - 1 + ((sig >> sh) & 1)) >> sh
    elif rounding == "truncate":
        r = sig >> sh
    elif rounding == "ties_away":
        r = (sig + half) >> sh
    else:
        raise ValueError(rounding)
    r = np.where(sh > 0, r, sig << lsh)
    mag = np.where(sig == 0, 0, ((et + bias - 1) << tm) + r)  # a carry out of the mantissa lands in the exponent, where it belongs
    mag = np.minimum(mag, emax << tm)
    if flush_subnormals:
        mag = np.where(mag < (1 << tm), 0, mag)
    mag = np.where(cls == INF, emax << tm, np.where(cls == NAN, (emax << tm) | (1 << (tm - 1)), mag))
    return (s << (eb + tm)) | mag


def sub(a, b):
    """a - b of two DECODED fp32 numbers as an exact integer difference (the caller's encode(.., FMT_F32) is the one rounding).
    An operand more than 2^28 last-places below the other only decides the rounding's direction: it enters as one sticky unit."""
    (sa, siga, qa, ca), (sb, sigb, qb, cb) = a, b
    sb = 1 - sb                                              # a + (-b)
    cap = 28
    gap = qa - qb
    hi_a, hi_b = gap > cap, gap < -cap
    A = np.where(hi_b, (siga != 0).astype(I64), siga << np.clip(gap, 0, cap))
    B = np.where(hi_a, (sigb != 0).astype(I64), sigb << np.clip(-gap, 0, cap))
    q = np.where(hi_a, qa - cap, np.where(hi_b, qb - cap, np.minimum(qa, qb)))
    v = (1 - 2 * sa) * A + (1 - 2 * sb) * B
    s = np.where(v == 0, sa & sb, (v < 0).astype(I64))      # an exact zero is +0 unless both addends are negative zeros
    cls = np.where((ca == NAN) | (cb == NAN) | ((ca == INF) & (cb == INF) & (sa != sb)), NAN,
                   np.where((ca == INF) | (cb == INF), INF, FINITE))
    s = np.where(cls == INF, np.where(ca == INF, sa, sb), s)
    return s, np.abs(v), q, cls


def scale2(num, k):
    """num * 2^k (exact; the caller's encode is the rounding)."""
    s, sig, q, cls = num
    return s, sig, q + k, cls


def is_nan16(bits, fmt):
    eb, tm = fmt
    b = np.asarray(bits).astype(I64) & ((1 << (eb + tm)) - 1)
    return b > (((1 << eb) - 1) << tm)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
# name -> the kinds it can show in.  The two layout mistakes are stored()'s, the others convert()'s.
MISTAKES = {
    "truncate": SIXTEEN,                      # round toward zero instead of to nearest even
    "ties_away": SIXTEEN,                     # ties away from zero
    "no_clamp": (F16, F16X3),                 # fp16 overflows to inf
    "lo_unclamped": (F16X3,),                 # hi from the clamped x, lo from x itself
    "lo_unscaled": (F16X3,),                  # lo = half(x - hi)
    "lo_reversed": (F16X3,),                  # lo = half((hi - x) * 2048)
    "flush_f16_subnormals": (F16, F16X3),     # fp16 results below 2^-14 become zeros
    "nan_passed": (F16, F16X3),               # a NaN reaches the fp16 conversion
    "lo_at_n_minus_1": (F16X3,),              # the lo plane one element early / late
    "lo_at_n_plus_1": (F16X3,),
}
# (mistake, kind) -> the input pattern of VALUES at which the twin must differ (layout mistakes: see test_opnd_convert_cpu.py)
WITNESS = {
    ("truncate", BF16): 0x3F80FFFF, ("truncate", F16): 0x3F80FFFF, ("truncate", F16X3): 0x3F80FFFF,      # just below 1 + one last place
    ("ties_away", BF16): 0x3F808000,          # 1 + half a bf16 last place, kept mantissa even
    ("ties_away", F16): 0x37008000, ("ties_away", F16X3): 0x37008000,      # 128.5 * 2^-24: a tie of the fp16 subnormals
    ("no_clamp", F16): 0x47800000, ("no_clamp", F16X3): 0x47800000,        # 65536
    ("lo_unclamped", F16X3): 0x47800000,      # (65536 - 65504) * 2048 = 65536: lo overflows
    ("lo_unscaled", F16X3): 0x3F800001, ("lo_reversed", F16X3): 0x3F800001,      # 1 + 2^-23: lo = 2^-12
    ("flush_f16_subnormals", F16): 0x33800000, ("flush_f16_subnormals", F16X3): 0x33800000,      # 2^-24
    ("nan_passed", F16): 0x7FC00000, ("nan_passed", F16X3): 0x7FC00000,
}


def clamp_bits(bits, nan_passed=False):
    """clamp_f16 on fp32 patterns: |x| above 65504 (infinities included) -> +-65504, a quiet NaN -> -65504, a signalling NaN
    (mantissa bit 22 clear) -> +65504, everything else as it is."""
    b = np.asarray(bits).astype(I64)
    mag = b & 0x7FFFFFFF
    out = np.where(mag > F16_MAX_BITS, (b & 0x80000000) | F16_MAX_BITS, b)
    nan_to = np.where((b & 0x00400000) != 0, F16_LOWEST_BITS, F16_MAX_BITS)
    return np.where(mag > 0x7F800000, b if nan_passed else nan_to, out)


def convert(kind, x_bits, mistake=None):
    """fp32 patterns [n] -> the stored plane(s) [planes, n]: uint16 patterns (FDM_F32: uint32, one plane)."""
    assert mistake is None or mistake in MISTAKES
    x = np.asarray(x_bits).astype(I64)
    if kind == F32:
        return x.astype(np.uint32)[None]
    mode = dict(rounding=mistake if mistake in ("truncate", "ties_away") else "nearest_even")
    if kind == BF16:
        return encode(decode(x, FMT_F32), FMT_BF16, **mode).astype(np.uint16)[None]
    mode["flush_subnormals"] = mistake == "flush_f16_subnormals"
    c = x if mistake == "no_clamp" else clamp_bits(x, nan_passed=mistake == "nan_passed")
    hi = encode(decode(c, FMT_F32), FMT_F16, **mode)
    if kind == F16:
        return hi.astype(np.uint16)[None]
    hi32 = decode(encode(decode(hi, FMT_F16), FMT_F32), FMT_F32)      # float(hi): exact
    xl = decode(x if mistake == "lo_unclamped" else c, FMT_F32)
    d = encode(sub(hi32, xl) if mistake == "lo_reversed" else sub(xl, hi32), FMT_F32)
    p = encode(scale2(decode(d, FMT_F32), 0 if mistake == "lo_unscaled" else 11), FMT_F32)
    lo = encode(decode(p, FMT_F32), FMT_F16, **mode)
    return np.stack([hi, lo]).astype(np.uint16)


def stored(kind, x_bits, lo_off=None, fill=0, mistake=None):
    """What a destination of the kind holds after the conversion of n values: [n] words (split kind: [lo_off + n], hi at 0, lo at
    lo_off, `fill` in between; lo_off = n when not given, as fdm_op_cast places it)."""
    p = convert(kind, x_bits, mistake if mistake not in ("lo_at_n_minus_1", "lo_at_n_plus_1") else None)
    n = p.shape[1]
    if kind != F16X3:
        return p[0]
    lo_off = n if lo_off is None else lo_off
    at = lo_off + {"lo_at_n_minus_1": -1, "lo_at_n_plus_1": 1}.get(mistake, 0)
    out = np.full(max(lo_off, at) + n, fill, np.uint16)
    out[:n] = p[0]
    out[at:at + n] = p[1]
    return out


def same_stored(kind, got, want):
    """Mask of the words that agree: bit for bit, except that a bf16 NaN of the model is matched by any bf16 NaN."""
    got, want = np.asarray(got), np.asarray(want)
    ok = got == want
    if kind == BF16:
        ok |= is_nan16(got, FMT_BF16) & is_nan16(want, FMT_BF16)
    return ok


def first_mismatch(kind, got, want, x_bits=None, what=""):
    """None, or the message naming the first word that differs: index, input bits, bits got, bits wanted."""
    bad = np.nonzero(~same_stored(kind, got, want))[0]
    if not len(bad):
        return None
    i = int(bad[0])
    src = ""
    if x_bits is not None:
        n = len(x_bits)
        src = f" input {int(x_bits[i % n]):#010x}" + (" (lo plane)" if i >= n else "")
    w = 8 if kind == F32 else 4
    return (f"{what} {KIND_NAMES[kind]}: word {i}{src}: got {int(got[i]):#0{w + 2}x}, want {int(want[i]):#0{w + 2}x} "
            f"({len(bad)} of {len(got)} words differ)")


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------
LOWER = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
VALUES = ((np.arange(65536, dtype=np.uint32)[:, None] << 16) | np.array(LOWER, np.uint32)[None, :]).reshape(-1)
VALUES.setflags(write=False)
NV = len(VALUES)
assert NV == 393216 and NV <= GRID


def _ties_f16():
    e = np.arange(127 - 14, 127 + 16, dtype=np.uint32)                       # fp32 exponent fields of fp16's normal range
    kept = np.array([0x000, 0x001, 0x3FE, 0x3FF], np.uint32)                 # the 10 mantissa bits fp16 keeps
    drop = np.array([0x0FFF, 0x1000, 0x1001], np.uint32)                     # the 13 it drops: below, at and above the tie
    sign = np.array([0, 1], np.uint32)
    return ((sign[:, None, None, None] << 31) | (e[None, :, None, None] << 23) | (kept[None, None, :, None] << 13)
            | drop[None, None, None, :]).reshape(-1)


TIES_F16 = _ties_f16()
_edges = np.array([0x477FDFFF, 0x477FE000, 0x477FE001, 0x477FEFFF, 0x477FF000, 0x477FF001], np.uint32)
EDGES_F16 = np.concatenate([_edges, _edges | np.uint32(0x80000000)])
EXTRA = np.concatenate([TIES_F16, EDGES_F16])
for _a in (TIES_F16, EDGES_F16, EXTRA):
    _a.setflags(write=False)


def tiled(n):
    """[n] uint32: VALUES repeated, the repeat number added to the index before the lookup."""
    i = np.arange(n, dtype=I64)
    return VALUES[(i + i // NV) % NV]


def f32_of(bits):
    """uint32 patterns -> the float32 array holding them (no conversion: the same bytes)."""
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def in_f16_range(bits):
    """Mask: finite with |x| <= 65504."""
    return (np.asarray(bits).astype(I64) & 0x7FFFFFFF) <= F16_MAX_BITS


@functools.lru_cache(maxsize=None)
def stored_tiled(kind, n):
    """stored(kind, tiled(n)) with lo_off = n: built once per (kind, n), never modified."""
    out = stored(kind, tiled(n))
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the movers (csrc/elementwise.hpp): index arithmetic on the host, float32 numpy.  Every case has a little over GRID elements: the
# grid-stride loop takes a second trip, and d = 67 keeps i % d and the row maps out of phase with the stride.
# ---------------------------------------------------------------------------------------------------------------------
MOVER_D = 67


def position_values(n, seed):
    """[n] fp32, another value at every position: a seeded normal plus a slow ramp (no two grid strides alike)."""
    g = np.random.default_rng(seed)
    return (g.standard_normal(n) + np.arange(n) * 2.0 ** -12).astype(np.float32)


def bias_act_expected(x, vec):
    """ACT_NONE: out[i] = in[i] + vec[i % d]."""
    n, d = len(x), len(vec)
    return x + vec[np.arange(n) % d]


ADD_ROWS_MAPS = ((1, 101), (3, 7), (50, 11))                # (div, mod) of a, b, c: three distinct row maps


def add_rows_expected(M, a, b, c):
    """out[m] = (a[(m / div) % mod] + b[..]) + c[..]: the kernel's order, one fp32 rounding per addition."""
    m = np.arange(M)
    rows = [(m // div) % mod for div, mod in ADD_ROWS_MAPS]
    return (a[rows[0]] + b[rows[1]]) + c[rows[2]]


def pad_rows_expected(x, pad, zero):
    """x [B, L, d] -> [B, L + 2 pad, d]: replicate (row clamp(k - pad, 0, L - 1)) or zeros outside."""
    B, L, d = x.shape
    src = np.arange(L + 2 * pad) - pad
    out = x[:, np.clip(src, 0, L - 1)]
    if zero:
        out = np.where(((src < 0) | (src >= L))[None, :, None], np.float32(0), out)
    return np.ascontiguousarray(out)


def group_pad_expected(x, groups, pad):
    """x [B, T, d] -> [groups, B, T + 2 pad, d / groups], zeros in the padding."""
    B, T, d = x.shape
    dg = d // groups
    out = np.zeros((groups, B, T + 2 * pad, dg), np.float32)
    out[:, :, pad:pad + T] = x.reshape(B, T, groups, dg).transpose(2, 0, 1, 3)
    return out


def masked_expected(x, lens):
    """x [B, L, ...] with everything at or beyond lens[b] along axis 1 replaced by +0 (zero_pad_rows, mask_samples)."""
    out = x.copy()
    for b, n in enumerate(lens):
        out[b, n:] = 0.0
    return out


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
