"""GPU: the fp32 -> operand-kind conversion and the plain movers, every stored word against the host model of tests/opnd_cases.py.

A. fdm_op_cast over VALUES (every 16-bit upper half of an fp32 word x six lower halves: zeros, subnormals, ties, the clamp, the
   infinities, NaNs) and over EXTRA (fp16's normal-range ties, 65504 and 65520 themselves) in all four kinds; at n = 1, 255, 256, 257
   with the destination 1 and 3 elements into its buffer (the kernel stores scalars and include/fdm_hip.h asks for no alignment);
   over the grid-stride boundary (n = 524 288 + 257 and 2 x 524 288 + 1: the second and third trip of the loop).
B. store_opnd4 / store_opnd1 through the GEMM epilogue: W = 0, no bias, resid = the value set, out = both: out_f32 = +0 + resid (so
   -0 becomes +0 and a NaN a NaN; everything else, fp32 subnormals included, keeps its bits) and out_t = the model applied to the
   out_f32 the launch wrote.  N = 64 (vector stores) and N = 67 in rows of 68 (vector stores and the scalar column tail), on tile
   1, the heuristic's tile and the general kernel.  Not covered: the packed K / V stores and the LayerNorm, time-norm and scheduler
   copies call the same two functions but cannot be fed arbitrary values (their inputs are normalised, or drawn); their own tests
   check them on the values they can produce.
C. The movers over the grid-stride boundary (a little over 524 288 elements each, d = 67), torch.equal against index arithmetic.
D. fdm_op_set_ints: the values travel with the launch.
E. fdm_op_linear_interp bit for bit against the float32 restatement of interp_taps (mesh_cases.positions).

Everything is bit for bit; the one exception is the payload of a bf16 NaN (tests/opnd_cases.py says why).  Every output sits
between 64-element guards that must stay (the Buf of tests/test_sched_noise_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import opnd_cases as OC  # noqa: E402
import reduce_cases as RC  # noqa: E402
from opnd_cases import BF16, F16, F16X3, F32  # noqa: E402
from test_gemm_exact_gpu import TILE_GENERAL  # noqa: E402
from test_sched_noise_gpu import GUARD, SENT, Buf  # noqa: E402
from fdm_amd import ops  # noqa: E402
from fdm_amd._lib import check, lib  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
KINDS = [F32, BF16, F16, F16X3]
KIND_IDS = lambda k: OC.KIND_NAMES[k]  # noqa: E731


def dev_f32(bits):
    """uint32 patterns -> a device fp32 tensor holding exactly those bits."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32).to(DEV)


def dev_np(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def words(t):
    """The bit patterns of a device tensor, on the host: uint16 for the 16-bit types, uint32 for fp32 / int32."""
    t = t.detach().cpu().contiguous()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


def fill_of(kind):
    """What an unwritten word shows: NaN where the model never stores one (the fp16 kinds), the sentinel elsewhere."""
    return NAN if kind in (F16, F16X3) else SENT


def fill_word(kind):
    return int(words(torch.full((1,), fill_of(kind), dtype=ops.tdtype(kind)))[0])


def cast_into(kind, src_bits, off=0, tail=0):
    """fdm_op_cast of src_bits into a guarded destination that starts `off` elements into its buffer and has `tail` spare
    elements behind it -> the bit patterns of everything between the guards."""
    n = len(src_bits)
    total = off + (2 * n if kind == F16X3 else n) + tail
    out = Buf(total, fill=fill_of(kind), dtype=ops.tdtype(kind))
    dst = ops.Split(out.buf.view(1, 1, -1), F16X3, 0, GUARD + off) if kind == F16X3 else out.arg[off:]
    ops.cast(dev_f32(src_bits), dst)
    torch.cuda.synchronize()
    assert out.guards_intact(), f"{OC.KIND_NAMES[kind]} n={n} off={off}: a guard element was written"
    return words(out.arg)


def cast_check(kind, src_bits, want, off=0, tail=0, what=""):
    got = cast_into(kind, src_bits, off, tail)
    fw = fill_word(kind)
    n = len(want)
    assert bool((got[:off] == fw).all()) and bool((got[off + n:] == fw).all()), f"{what}: written outside the destination"
    msg = OC.first_mismatch(kind, got[off:off + n], want, src_bits, what)
    assert msg is None, msg


# ---------------------------------------------------------------------------------------------------------------------
# A. fdm_op_cast
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", ["VALUES", "EXTRA"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_cast_over_the_value_set(kind, values):
    """Every stored word equals the model; the split kind's lo plane sits exactly n elements after hi."""
    bits = getattr(OC, values)
    cast_check(kind, bits, OC.stored(kind, bits), tail=2, what=f"cast {values}")


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_cast_sizes_and_unaligned_destinations(kind, n, off):
    """One element, one block less one, one block, one block and one; the destination 0, 1 and 3 elements into its buffer (an odd
    2-byte, 4-byte or, split kind with odd n, lo-plane address).  Values: a stretch of VALUES that crosses 65504."""
    i0 = int(np.nonzero(OC.VALUES == 0x477F8000)[0][0]) - n // 2
    bits = OC.VALUES[i0:i0 + n]
    cast_check(kind, bits, OC.stored(kind, bits), off=off, tail=3, what=f"cast n={n} off={off}")


@pytest.mark.parametrize("n", [OC.GRID + 257, 2 * OC.GRID + 1])
@pytest.mark.parametrize("kind", OC.SIXTEEN, ids=KIND_IDS)
def test_cast_over_the_grid_stride_boundary(kind, n):
    """More elements than the capped grid has lanes: the elements from 524 288 on are the second (and third) trip of the loop,
    and every one of them holds another value than the element one stride before it."""
    assert n > OC.GRID
    cast_check(kind, OC.tiled(n), OC.stored_tiled(kind, n), tail=2, what=f"cast tiled({n})")


# ---------------------------------------------------------------------------------------------------------------------
# B. the operand copy of the GEMM epilogue
# ---------------------------------------------------------------------------------------------------------------------
def _opnd(kind, t):
    """Host [rows, K] fp32 of values exact in the kind -> the device operand (split kind: lo plane zeros)."""
    dt = ops.tdtype(kind)
    if kind == F16X3:
        return ops.Split(torch.stack([t.to(dt), torch.zeros_like(t, dtype=dt)]).to(DEV), F16X3)
    return t.to(dt).to(DEV)


@pytest.mark.parametrize("N,ld", [(64, 64), (67, 68)], ids=["n64", "n67"])
@pytest.mark.parametrize("kind", OC.SIXTEEN, ids=KIND_IDS)
def test_gemm_epilogue_copy_over_the_value_set(kind, N, ld):
    """acc = +0 exactly (W = 0, A finite), so out_f32 = +0 + resid and out_t = the conversion of that.  M rows cover the whole
    set; N = 64: 6144 x 64 is VALUES itself; N = 67 in rows of 68: the 64 vector columns and a 3-column scalar tail, column 67 of
    every row untouched."""
    K = 64
    M = -(-OC.NV // N)
    n = M * ld
    src = OC.tiled(n)
    resid = dev_f32(src)
    A, W = _opnd(kind, torch.ones(M, K)), _opnd(kind, torch.zeros(N, K))
    col = np.arange(n) % ld
    live = col < N
    x = src.astype(np.int64)
    isnan = (x & 0x7FFFFFFF) > 0x7F800000
    want32 = np.where(x == 0x80000000, 0, x).astype(np.uint32)                    # +0 + -0 = +0
    sent32 = int(words(torch.full((1,), SENT))[0])
    fw = fill_word(kind)
    seen = None                                              # (out_f32 words, their conversion): the tiles write the same bits
    for tile in (1, 0, 1 | TILE_GENERAL):
        o32 = Buf(n, fill=SENT)
        ot = Buf(2 * n if kind == F16X3 else n, fill=fill_of(kind), dtype=ops.tdtype(kind))
        out_t = ops.Split(ot.buf.view(1, 1, -1), F16X3, 0, GUARD) if kind == F16X3 else ot.arg
        if kind == F16X3:
            out_t.lo_off = n
        ops.gemm(A, W, M, N, K, resid=resid, ldr=ld, out_f32=o32.arg, ldo_f32=ld, out_t=out_t, ldo_t=ld, tile=tile)
        torch.cuda.synchronize()
        what = f"gemm {OC.KIND_NAMES[kind]} N={N} tile {tile:#x}"
        assert o32.guards_intact() and ot.guards_intact(), what
        g32, gt = words(o32.arg), words(ot.arg)
        assert bool((g32[~live] == sent32).all()) and bool((gt.reshape(-1, n)[:, ~live] == fw).all()), f"{what}: a column at or past N was written"
        # out_f32: the input's bits (-0 -> +0), a NaN for a NaN
        gnan = (g32.astype(np.int64) & 0x7FFFFFFF) > 0x7F800000
        bad = np.nonzero(live & ((gnan != isnan) | (~isnan & (g32 != want32))))[0]
        assert not len(bad), (f"{what}: out_f32 element {int(bad[0])} (row {int(bad[0]) // ld}, column {int(bad[0]) % ld}), input "
                              f"{int(src[bad[0]]):#010x}: got {int(g32[bad[0]]):#010x}, want {int(want32[bad[0]]):#010x}; {len(bad)} differ")
        # out_t: the model applied to what out_f32 holds
        if seen is None or not np.array_equal(seen[0], g32):
            seen = (g32, OC.stored(kind, g32[live]))
        want = seen[1]
        msg = OC.first_mismatch(kind, gt.reshape(-1, n)[:, live].reshape(-1), want, g32[live], what + " out_t (live elements in row order)")
        assert msg is None, msg


# ---------------------------------------------------------------------------------------------------------------------
# C. the movers over the grid-stride boundary
# ---------------------------------------------------------------------------------------------------------------------
D = OC.MOVER_D


def _equal(out, want, what):
    torch.cuda.synchronize()
    assert out.guards_intact(), f"{what}: a guard element was written"
    got = out.cpu()
    want = torch.from_numpy(np.ascontiguousarray(want)).reshape(-1)
    assert got.shape == want.shape and got.numel() > OC.GRID
    if not torch.equal(got, want) or not np.array_equal(words(got), words(want)):
        i = int(np.nonzero(words(got) != words(want))[0][0])
        raise AssertionError(f"{what}: element {i} ({'second' if i >= OC.GRID else 'first'} trip): got {float(got[i])!r}, want {float(want[i])!r}")


def test_bias_act_second_trip():
    rows = 7826                                              # 7826 x 67 = 524 342
    x, vec = OC.position_values(rows * D, 1), OC.position_values(D, 2) * 8.0
    out = Buf(rows * D)
    ops.bias_act(dev_np(x), dev_np(vec), out.arg, rows, D, ops.ACT_NONE)
    _equal(out, OC.bias_act_expected(x, vec), "bias_act")


def test_add_rows_second_trip():
    M = 7826
    a, b, c = (OC.position_values(mod * D, 3 + i).reshape(mod, D) * 4.0 ** i for i, (_, mod) in enumerate(OC.ADD_ROWS_MAPS))
    (ad, am), (bd, bm), (cd, cm) = OC.ADD_ROWS_MAPS
    out = Buf(M * D)
    ops.add_rows(out.arg, M, D, dev_np(a), ad, am, dev_np(b), bd, bm, dev_np(c), cd, cm)
    _equal(out, OC.add_rows_expected(M, a, b, c), "add_rows")


def test_zero_pad_rows_second_trip():
    """In place: rows at or beyond lens[b] hold NaN going in and +0 coming out; every other element keeps its bits."""
    B, L = 4, 1957                                           # 4 x 1957 x 67 = 524 476
    lens = [0, 1, L, 1000]
    x = OC.position_values(B * L * D, 6).reshape(B, L, D)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    buf = Buf(B * L * D, fill=dev_np(x.reshape(-1)))
    ops.zero_pad_rows(buf.arg, B, L, D, dev_np(np.array(lens, np.int32)))
    _equal(buf, OC.masked_expected(x, lens), "zero_pad_rows")


def test_mask_samples_second_trip():
    B, n = 4, 131100                                         # 4 x 131 100 = 524 400
    lens = [0, 1, n, 70001]
    wav = OC.position_values(B * n, 7).reshape(B, n)
    for b, k in enumerate(lens):
        wav[b, k:] = np.nan
    out = Buf(B * n)
    wav_d, lens_d = dev_np(wav), dev_np(np.array(lens, np.int32))
    check(lib().fdm_op_mask_samples(wav_d.data_ptr(), out.arg.data_ptr(), B, n, lens_d.data_ptr(), ops.stream()))
    _equal(out, OC.masked_expected(wav, lens), "mask_samples")


@pytest.mark.parametrize("zero", [False, True], ids=["replicate", "zero"])
def test_pad_rows_second_trip(zero):
    B, L, pad = 2, 3900, 7                                   # 2 x 3914 x 67 = 524 476
    x = OC.position_values(B * L * D, 8).reshape(B, L, D)
    out = Buf(B * (L + 2 * pad) * D)
    ops.pad_rows(dev_np(x), out.arg, B, L, D, pad, zero=zero)
    _equal(out, OC.pad_rows_expected(x, pad, zero), f"pad_rows zero={zero}")


def test_group_pad_second_trip():
    B, T, d, groups, pad = 2, 3800, 69, 3, 2                 # 3 x 2 x 3804 x 23 = 524 952 (d = 67 has no groups to split into)
    x = OC.position_values(B * T * d, 9).reshape(B, T, d)
    out = Buf(B * (T + 2 * pad) * d)
    ops.group_pad(dev_np(x), out.arg, B, T, d, groups, pad)
    _equal(out, OC.group_pad_expected(x, groups, pad), "group_pad")


# ---------------------------------------------------------------------------------------------------------------------
# D. fdm_op_set_ints
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_set_ints_values_travel_with_the_launch(n):
    """The host array is overwritten as soon as the call returns, before anything is synchronised: the device must still
    receive the values it held during the call (64 per launch: n = 65 and 130 take two and three)."""
    vals = (np.arange(n, dtype=np.int64) * 2654435761 % 2 ** 31 - 2 ** 30).astype(np.int32)
    host = vals.copy()
    out = Buf(n, fill=-1, dtype=torch.int32)
    check(lib().fdm_op_set_ints(out.arg.data_ptr(), host.ctypes.data_as(C.c_void_p), n, ops.stream()))
    host[:] = 0x5A5A5A5A
    torch.cuda.synchronize()
    assert out.guards_intact()
    assert np.array_equal(out.cpu().numpy(), vals)


# ---------------------------------------------------------------------------------------------------------------------
# E. fdm_op_linear_interp
# ---------------------------------------------------------------------------------------------------------------------
def _interp_check(B, Tin, Tout, Cn):
    x = RC.interp_inputs(B, Tin, Cn)
    want = RC.interp_expected(x, Tout)
    y = Buf(B * Tout * Cn)
    ops.linear_interp(dev_np(x), y.arg, B, Tin, Tout, Cn)
    torch.cuda.synchronize()
    assert y.guards_intact()
    got = y.cpu().numpy().reshape(B, Tout, Cn)
    assert RC.same_bits(got, want), f"B{B} {Tin}->{Tout} C{Cn}: {int((RC.bits(got) != RC.bits(want)).sum())} elements differ"
    assert RC.same_bits(got[:, 0], x[:, 0]) and (Tout == 1 or RC.same_bits(got[:, -1], x[:, -1]))      # the end frames, exactly


@pytest.mark.parametrize("Cn", [3, 67])
@pytest.mark.parametrize("Tin,Tout", [(1, 1), (1, 4), (5, 1), (7, 7), (2, 5), (101, 61), (61, 101)])
def test_linear_interp_bit_for_bit(Tin, Tout, Cn):
    """l0 x[i0] + l1 x[i1] with the taps of interp_taps (csrc/handoff.hpp), two rounded products and one rounded sum: the host
    model is mesh_cases.positions, the one restatement of the taps (tests/test_opnd_convert_cpu.py holds it to fp64)."""
    _interp_check(2, Tin, Tout, Cn)


def test_linear_interp_second_trip():
    B, Tin, Tout, Cn = 2, 40, 3914, 67                       # 2 x 3914 x 67 = 524 476
    assert B * Tout * Cn > OC.GRID
    _interp_check(B, Tin, Tout, Cn)
