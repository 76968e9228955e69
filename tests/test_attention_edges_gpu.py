"""GPU: the fused attention kernel on its own (Q, Kp, Vp packed on the host and uploaded, no GEMM in front) against an fp64
reference of what it reads, element by element inside the bound derived in tests/attn_cases.py, at tile, mask and layout edges;
and the contract forms no other test visits: pad keys holding non-zero values, ldq != d, ldo != d, fp32 attention writing a
split plane pair, slopes without the causal mask.  tests/test_attention_edges_cpu.py shows that the cases see the mistakes this
kernel invites."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_cases as AC  # noqa: E402
from attn_cases import BF16, F16, F16X3, F32  # noqa: E402
from fdm_amd import ops  # noqa: E402

DEV = "cuda:0"
KIND_IDS = lambda k: AC.KIND_NAMES[k]  # noqa: E731


@functools.lru_cache(maxsize=None)
def prepared(kind, case):
    """Operands, reference and bound of one (kind, case): computed once, shared among the tests, never modified."""
    opnd = AC.operands(kind, *case.inputs(), device=DEV)
    ref = AC.reference(opnd.q, opnd.k, opnd.v, case.scale, case.causal, case.slope_values(), case.period)
    return opnd, ref, AC.bound(kind, ref, case.hd)


def new_output(kind, rows, cols, fill=0.0):
    if kind == F16X3:
        return ops.Split(torch.full((2, rows, cols), fill, device=DEV, dtype=torch.float16), F16X3)
    return torch.full((rows, cols), fill, device=DEV, dtype=AC.plane_dtype(kind))


def bits(t):
    return t.planes if isinstance(t, ops.Split) else t


def run(kind, opnd, case, pad_fill=0.0, causal=None, slopes="case", period=None):
    """One launch on host-packed operands -> the output object ([B*L, d], or the plane pair)."""
    B, H, L, hd = opnd.B, opnd.H, opnd.L, opnd.hd
    d = H * hd
    Q, Kp, Vp, Lpad = opnd.device_inputs(DEV, pad_fill)
    sl = case.slope_values() if isinstance(slopes, str) else slopes
    O = new_output(kind, B * L, d)
    ops.attention(Q, Kp, Vp, O, B=B, H=H, L=L, hd=hd, ldq=d, ldo=d, Lpad=Lpad, scale=case.scale,
                  causal=case.causal if causal is None else causal, slopes=sl.to(DEV) if sl is not None else None,
                  period=case.period if period is None else period)
    torch.cuda.synchronize()
    return O


def values(O, opnd):
    """Output object -> fp64 [B, H, L, hd]."""
    return AC.unrows(O.float().double().cpu(), opnd.B, opnd.H, opnd.L, opnd.hd)


def check(kind, case, O, what=""):
    opnd, ref, bnd = prepared(kind, case)
    r, idx, err, b = AC.worst(values(O, opnd), ref, bnd)
    print(f"ATTN_RATIO {AC.KIND_NAMES[kind]} {what}{case.id} {r:.4f}")
    assert r <= 1.0, (f"{AC.KIND_NAMES[kind]} {what}{case.id}: error / bound = {r:.4g} at (b, h, i, e) = {idx}: |gpu - ref| = {err:.4g}, "
                      f"bound = {b:.4g}, ref = {float(ref.o[idx]):.6g}")


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.id)
@pytest.mark.parametrize("kind", AC.KINDS, ids=KIND_IDS)
def test_attention_within_per_element_bound(kind, case):
    opnd, _, _ = prepared(kind, case)
    check(kind, case, run(kind, opnd, case))


PAD_CASES = [AC.Case("gaussian", 1, 3, L, hd, c, 9, "pow2" if c else "none") for c in (True, False)
             for (L, hd) in ((33, 64), (47, 128), (16, 64), (17, 256), (31, 64))]


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("kind", AC.KINDS, ids=KIND_IDS)
def test_pad_keys_are_never_seen(kind, causal):
    """'Pad keys must hold finite values': the same inputs packed with pads of 0, 64 and -64 give the same bits (L % 32 of
    1, 15, 16, 17, 31: the fp32 kind's 16-key tiles meet a half-empty and a whole pad tile)."""
    for case in (c for c in PAD_CASES if c.causal == causal):
        opnd, _, _ = prepared(kind, case)
        base = run(kind, opnd, case, 0.0)
        check(kind, case, base, "pads ")
        for fill in (64.0, -64.0):
            assert torch.equal(bits(run(kind, opnd, case, fill)), bits(base)), f"{case.id}: pads of {fill} changed the output"


STRIDED = AC.Case("gaussian", 2, 3, 33, 64, True, 9, "pow2")


@pytest.mark.parametrize("kind", AC.KINDS, ids=KIND_IDS)
def test_strided_q_and_o(kind):
    """ldq = 3d (Q the first d columns of a QKV-wide buffer whose other columns hold a sentinel) and O written into the middle
    of a [B*L + 8, d + 64] sentinel buffer (ldo = d + 64): the bits of the dense call, nothing else touched.  L = 33: the last
    query tile is ragged."""
    case = STRIDED
    opnd, _, _ = prepared(kind, case)
    B, H, L, hd = opnd.B, opnd.H, opnd.L, opnd.hd
    d, R0, C0, SENT = H * hd, 4, 32, 7.0
    dense = run(kind, opnd, case)
    check(kind, case, dense, "dense ")
    Q, Kp, Vp, Lpad = opnd.device_inputs(DEV, 0.0, ldq=3 * d, sentinel=1e4)
    buf = new_output(kind, B * L + 8, d + 64, SENT)
    O = ops.Split(buf.planes, F16X3, R0, C0) if kind == F16X3 else buf[R0:, C0:]
    ops.attention(Q, Kp, Vp, O, B=B, H=H, L=L, hd=hd, ldq=3 * d, ldo=d + 64, Lpad=Lpad, scale=case.scale, causal=True,
                  slopes=case.slope_values().to(DEV), period=case.period)
    torch.cuda.synchronize()
    got = bits(buf)
    inside = got[..., R0:R0 + B * L, C0:C0 + d]
    assert torch.equal(inside, bits(dense))
    outside = torch.ones_like(got, dtype=torch.bool)
    outside[..., R0:R0 + B * L, C0:C0 + d] = False
    assert bool((got[outside] == SENT).all()), "a sentinel column or guard row was written"


@pytest.mark.parametrize("wide", [0, 64], ids=["ldo=d", "ldo>d"])
def test_fp32_attention_writes_split_output(wide):
    """fdm_attn_args.o_split = FDM_F16X3: fp32 attention writes the next GEMM's split operand.  The planes are those of the
    library's cast of the fp32 output, bit for bit (one store helper), with ldo = d and inside a wider sentinel buffer."""
    case = AC.Case("gaussian", 3, 3, 33, 64, True, 9, "pow2")
    opnd, _, _ = prepared(F32, case)
    B, H, L, hd = opnd.B, opnd.H, opnd.L, opnd.hd
    d = H * hd
    o32 = run(F32, opnd, case)
    check(F32, case, o32, "o_split ")
    want = ops.to_operand(o32, F16X3).planes
    Q, Kp, Vp, Lpad = opnd.device_inputs(DEV, 0.0)
    O = ops.Split(torch.full((2, B * L, d + wide), 7.0, device=DEV, dtype=torch.float16), F16X3)
    ops.attention(Q, Kp, Vp, O, B=B, H=H, L=L, hd=hd, ldq=d, ldo=d + wide, Lpad=Lpad, scale=case.scale, causal=True,
                  slopes=case.slope_values().to(DEV), period=case.period)
    torch.cuda.synchronize()
    assert torch.equal(O.planes[:, :, :d], want)
    assert bool((O.planes[:, :, d:] == 7.0).all())
    assert float((O.float()[:, :d] - o32).abs().max()) <= 2.0 ** -21 * float(o32.abs().max())      # and they hold the fp32 result


@pytest.mark.parametrize("period", [7, 9])
@pytest.mark.parametrize("kind", AC.KINDS, ids=KIND_IDS)
def test_alibi_without_causal_mask(kind, period):
    """slopes with causal = 0 (include/fdm_hip.h, fdm_attn_args): every key is visible and the bias is the same floor formula on
    both sides of the diagonal, -slope_h * floor((i - j) / period), positive for j > i.  Period 7 takes the per-key floor, period
    9 the compare / select form (negative D, negative f0)."""
    case = AC.Case("steep_alibi", 1, 3, 47, 64, False, period, "steep")
    opnd, ref, _ = prepared(kind, case)
    O = run(kind, opnd, case)
    check(kind, case, O)
    # the bias is really applied above the diagonal: without it the first row would be a flat average of V
    flat = opnd.v[:, :, :, :].mean(2)
    assert float((ref.o[:, :, 0] - flat).abs().max()) > 0.1


@pytest.mark.parametrize("builder", sorted(AC.BUILDERS))
@pytest.mark.parametrize("kind", AC.KINDS, ids=KIND_IDS)
def test_attention_is_repeatable(kind, builder):
    """Three launches of each builder's largest case give the same bits (the merge of the four waves goes through LDS)."""
    case = AC.largest_case(builder)
    opnd, _, _ = prepared(kind, case)
    first = bits(run(kind, opnd, case))
    for _ in range(2):
        assert torch.equal(bits(run(kind, opnd, case)), first)
