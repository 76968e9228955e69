"""The GEMM on exactly representable operands: operand builders, an exact fp64 reference, the conditions that make equality
legitimate, a CPU twin with switchable mistakes and the case list shared by tests/test_gemm_exact_cpu.py and
tests/test_gemm_exact_gpu.py.  Plain helper module (pytest does not collect it); host only: nothing here touches a device or
loads the library.

Why equality
------------
A entries are small integers, W entries are in {-1, 0, 1} (split kind: hi planes as above, lo planes integers in [-2, 2], value
hi + lo / 2048), bias and residual are integers in [-8, 8].  Every product and every partial sum of a k loop, in ANY association
order, is then an integer far below 2^24: fp32 accumulation is exact whatever the tile, the ring depth or the MFMA shape.  The
split kind's documented evaluation (csrc/common.hpp, "Operand kinds") is sum hi.hi + (sum hi.lo + sum lo.hi) / 2048 with two
accumulators and one scaling after the loop, the lo.lo term dropped by design: both sums are integers, the scaling by a power of
two is exact, and with |sum hi.hi| < 2^12 and |cross| < 2^12 the total has at most 12 integer and 11 fraction bits, so bias and
residual still fit 24 bits.  The fp64 value of that expression is therefore also the exact fp32 answer, and a dropped,
duplicated or misplaced term shows as an integer-sized difference (1 / 2048 for a lo-plane term) at a named element.
assert_exact() checks these conditions for every (kind, case); nothing in them comes from what a kernel returns.

The epilogue forms kept exact: bias add, ReLU, LeakyReLU(0.2) (one fp32 product float32(0.2) * v, the same single rounding on
both sides; leaky cases carry no residual, so no second rounding and no fused multiply-add can differ), residual add, the
operand-kind copy (round to nearest even: torch's CPU casts; the split kind as store_opnd4 does it: hi = half(x),
lo = half((x - hi) * 2048)), packed K / V (attn_cases.pack_host of the exact values), stat_out (integer sums and sums of
squares below 2^24) and ksplit planes.  Mish and the GELUs are not exact arithmetic: tests/epilogue_cases.py bounds them per
element on these operands, and the LayerNorm folds on exact rows of their own.  The fused scheduler is compared bit for bit
with GEMM + fdm_op_sched_step in tests/test_ops_gpu.py (modes 0, 1 and 3)."""
import functools
import zlib
from collections import namedtuple
from types import SimpleNamespace

import torch

from attn_cases import KIND_NAMES, KINDS, SPLIT_SCALE, kv_pad, pack_host, plane_dtype  # noqa: F401  (re-exported)
from fdm_amd._lib import ACT_LEAKY02, ACT_NONE, ACT_RELU, BF16, F16, F16X3, F32

GAP = 3.0          # what the columns between K and lda / ldw hold: exact in every kind, visible in any sum that reads it
SENT16 = -77.0     # sentinel of 16-bit outputs and of the packed K / V buffers (pad keys must stay finite); fp32 outputs: NaN
R0 = 2             # guard rows above and below every output window
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LEAKY02: "leaky"}


def _one_thread(fn):
    """The tensors here are tiny and there are tens of thousands of operations on them: torch's intra-op thread pool costs a
    hundred times what it saves.  Run `fn` on one thread and put the caller's setting back."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        n = torch.get_num_threads()
        if n == 1:
            return fn(*a, **kw)
        torch.set_num_threads(1)
        try:
            return fn(*a, **kw)
        finally:
            torch.set_num_threads(n)
    return wrapped


def k_unit(kind):
    """Elements of K per k-tile (128 bytes of a row)."""
    return 32 if kind == F32 else 64


def epc(kind):
    """Elements per 16-byte chunk."""
    return 4 if kind == F32 else 8


def planes_of(kind):
    return 2 if kind == F16X3 else 1


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case(namedtuple("Case", "name M N ku K bias resid act out lda ldo ldr rmod G C S kv stat wden lo values")):
    """M, N: rows and columns of one problem (kv: taken from the QKV geometry).  K = `K` if given, else ku k-units of the kind.
    out: "f32" | "t" | "both".  lda: "dense" | "gap" (lda = ldw = K + 8 chunks, GAP in between) | "overlap" (lda = one k-unit
    < K: overlapping rows, the strided-conv form).  ldo / ldr: extra columns of the output / residual rows (ldo > 0: the window
    starts 8 columns into the row).  rmod: resid_row_mod.  G: batch (0 = unbatched), column groups.  C: batch2 (0 = none).
    S: ksplit.  kv: (B, H, L, hd) of a QKV projection with packed K / V.  stat: stat_out.  wden: one W entry in wden is
    non-zero.  lo: "rand" | "zero" (split kind's lo planes).  values: "random" | "unique" (A holds position-dependent values
    and every W row one 1: each output is a copy of one A element) | "round" (outputs of thousands: the operand-kind copy has
    to round) | "rowcol" / "row" (acc[m, n] = I_m + J_n / = I_m: the known pre-activation values of tests/epilogue_cases.py)."""

    @property
    def id(self):
        return self.name


def mk(name, M=0, N=0, ku=2, **kw):
    d = dict(K=0, bias=True, resid=True, act=ACT_NONE, out="both", lda="dense", ldo=0, ldr=0, rmod=0, G=0, C=0, S=0, kv=None,
             stat=False, wden=1, lo="rand", values="random")
    d.update(kw)
    return Case(name, M, N, ku, **d)


CASES = [
    # rows across the edges of the 32-, 64-, 80-, 128- and 256-row tiles; columns across 64 / 128, 67 and 1 through the scalar tail
    mk("edge-1x4", 1, 4), mk("edge-63x60", 63, 60), mk("edge-64x64", 64, 64), mk("edge-65x68", 65, 68),
    mk("edge-79x132", 79, 132), mk("edge-81x200", 81, 200), mk("edge-129x67", 129, 67), mk("edge-257x1", 257, 1),
    mk("edge-257x132", 257, 132), mk("edge-1x67", 1, 67), mk("edge-80x128", 80, 128), mk("edge-129x4", 129, 4),
    # k loop: fewer, as many and more k-tiles than every ring depth (2, 3, 4 stages); one tile: prologue == tail
    mk("k1", 65, 68, 1), mk("k2", 33, 132, 2), mk("k3", 65, 68, 3), mk("k4", 65, 68, 4), mk("k5", 65, 68, 5), mk("k9", 65, 68, 9),
    mk("k2048-round", 65, 68, K=2048, wden=4, values="round"),
    # strides
    mk("lda-gap", 65, 68, 3, lda="gap"),
    mk("lda-overlap", 70, 64, 3, lda="overlap", values="unique"),
    mk("ldo-wide", 65, 68, ldo=16), mk("ldo-odd", 63, 60, ldo=13), mk("ldr-wide", 65, 68, ldr=4), mk("ldr-odd", 65, 64, ldr=3),
    mk("rmod1", 65, 68, rmod=1), mk("rmod7", 65, 64, rmod=7), mk("rmod7-ragged", 37, 67, rmod=7, ldr=5),
    # epilogue families
    mk("epi-bias", 65, 68, resid=False), mk("epi-resid", 65, 68, bias=False), mk("epi-neither", 65, 68, bias=False, resid=False),
    mk("epi-relu", 65, 68, act=ACT_RELU), mk("epi-relu-plain", 64, 64, act=ACT_RELU, bias=False, resid=False),
    mk("epi-leaky", 65, 68, act=ACT_LEAKY02, resid=False), mk("epi-leaky-64", 64, 128, act=ACT_LEAKY02, resid=False, bias=False),
    mk("epi-f32-only", 65, 68, out="f32"), mk("epi-t-only", 65, 68, out="t"), mk("epi-t-only-64", 64, 64, out="t", resid=False),
    mk("lo-zero", 65, 68, 3, lo="zero"),
    # batch: column groups
    mk("batch1", 50, 60, G=1, values="unique"), mk("batch3", 50, 68, G=3, values="unique"), mk("batch8", 33, 64, G=8, values="unique"),
    mk("batch3-random", 65, 64, G=3, act=ACT_RELU),
    # batch2: C clips over G groups, T not a multiple of 64
    mk("batch2-1x4", 70, 64, G=4, C=1, values="unique"), mk("batch2-3x8", 37, 64, G=8, C=3, values="unique"),
    mk("batch2-3x4-48", 70, 48, G=4, C=3, values="unique", act=ACT_RELU),
    # ksplit
    mk("ksplit2", 65, 64, 4, S=2, out="f32"), mk("ksplit4", 37, 128, 4, S=4, out="f32"), mk("ksplit4-k8", 64, 64, 8, S=4, out="f32", resid=False),
    # packed K / V: a row tile straddles the clip boundary; L = 40: whole packed chunks (the transposed-tile V path)
    mk("kv-33-hd64", kv=(2, 2, 33, 64), values="unique", resid=False, out="t"),
    mk("kv-47-hd128", kv=(2, 2, 47, 128), values="unique", resid=False, out="t"),
    mk("kv-40-hd64", kv=(2, 2, 40, 64), values="unique", resid=False, out="both"),
    mk("kv-33-random", kv=(2, 2, 33, 64), resid=False, out="t"),
    mk("kv-33-one-head", kv=(2, 1, 33, 64), values="unique", resid=False, out="t"),      # d = 64: a 128-column tile spans Q | K and V | nothing
    # stat_out (integer outputs: the split kind with lo = 0)
    mk("stat-65x64", 65, 64, stat=True, lo="zero"), mk("stat-81x192", 81, 192, 3, stat=True, lo="zero"),
]
assert len({c.name for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# operands and geometry
# ---------------------------------------------------------------------------------------------------------------------
def _randint(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


@functools.lru_cache(maxsize=None)
@_one_thread
def problem(kind, case):
    """Everything one launch needs, on the host: flat operand buffers (fp32 tensors holding values exact in `kind`, one row per
    plane), strides in elements, and the flat offset of every output element.  Never modified after it is built."""
    p = SimpleNamespace(kind=kind, case=case)
    ku, e, P = k_unit(kind), epc(kind), planes_of(kind)
    K = case.K or case.ku * ku
    M, N = case.M, case.N
    if case.kv:
        p.B, p.H, p.L, p.hd = case.kv
        p.d, p.Lpad = p.H * p.hd, kv_pad(p.L)
        M, N = p.B * p.L, 3 * p.d
    G, C, S = max(case.G, 1), max(case.C, 1), max(case.S, 1)
    if case.lda == "gap":
        lda = ldw = K + 8 * e
    elif case.lda == "overlap":
        lda, ldw = ku, K
        assert K > ku and case.values == "unique"
    else:
        lda = ldw = K
    a_blk = (max((M - 1) * lda + K, M * K) + e - 1) // e * e      # one (clip, group) block; room for rows read at stride K
    p.M, p.N, p.K, p.G, p.C, p.S, p.P = M, N, K, G, C, S, P
    p.lda, p.ldw, p.a_bs2, p.a_bs, p.w_bs = lda, ldw, a_blk, C * a_blk, N * ldw
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) * 8 + kind)
    na, nw = G * C * a_blk, G * N * ldw
    p.a_idx = torch.as_strided(torch.arange(na), (C, G, M, K), (p.a_bs2, p.a_bs, lda, 1))
    p.w_idx = torch.as_strided(torch.arange(nw), (G, N, K), (p.w_bs, ldw, 1))
    A, W = torch.full((2, na), GAP), torch.full((2, nw), GAP)
    if case.values == "unique":
        # A: a function of the flat position (consistent where rows overlap); W: one 1 per row, another column per group
        A[0, p.a_idx] = ((p.a_idx * 37) % 251 - 125).float()
        A[1, p.a_idx] = ((p.a_idx * 3) % 5 - 2).float()
        W[:, p.w_idx] = 0.0
        n = torch.arange(N).view(1, N).expand(G, N)
        g = torch.arange(G).view(G, 1).expand(G, N)
        W[0, p.w_idx[g, n, (5 * n + 3 * g) % K]] = 1.0
    elif case.values == "round":
        # out[m, n] = a_m * count_n: column 0 has K (split kind: 1500, to stay below its 2^12) non-zeros, so outputs reach
        # +-4096 (+-3000) + bias + residual: beyond 2^8, 2^11 and 2^12, where bf16 and fp16 hold every second, fourth ... integer
        s = torch.where(torch.rand(K, generator=gen) < 0.5, -1.0, 1.0)
        am = torch.tensor([1.0, 2.0, -1.0, -2.0])[torch.arange(M) % 4]
        mask = (torch.rand(N, K, generator=gen) * case.wden < 1.0).float()
        mask[0] = (torch.randperm(K, generator=gen) < (min(K, 1500) if P == 2 else K)).float()
        A[0, p.a_idx] = (am.view(M, 1) * s.view(1, K)).expand(C, G, M, K)
        W[0, p.w_idx] = (mask * s.view(1, K)).expand(G, N, K)
        A[1, p.a_idx] = _randint(gen, -2, 2, (C, G, M, K))
        W[1, p.w_idx] = _randint(gen, -2, 2, (G, N, K))
    elif case.values in ("rowcol", "row"):
        # acc[m, n] = I_m + J_n (tests/epilogue_cases.py): the first half of K carries I_m against one 1 per W row (at another k
        # per row), the second half ones against W in {-1, 0, 1} whose row sum is J_n ("row": +1 -1 pairs, J_n = 0, products live)
        assert case.lo == "zero" and K % 4 == 0
        h = K // 2
        i_m = (torch.arange(M) % 49 - 24).float()
        if case.values == "row":
            i_m = torch.where(torch.arange(M) % 3 == 0, torch.zeros(M), i_m)
        A[0, p.a_idx] = torch.cat([i_m.view(M, 1).expand(M, h), torch.ones(M, K - h)], 1).expand(C, G, M, K)
        wv = torch.zeros(G, N, K)
        wv[:, torch.arange(N), (5 * torch.arange(N)) % h] = 1.0
        if case.values == "row":
            wv[:, :, h:] = torch.tensor([1.0, -1.0]).repeat((K - h) // 2)
        else:
            wv[:, :, h:] = _randint(gen, -1, 1, (G, N, K - h))
        W[0, p.w_idx] = wv
    else:
        A[0, p.a_idx] = _randint(gen, -2, 2, (C, G, M, K))
        wv = _randint(gen, -1, 1, (G, N, K))
        if case.wden > 1:
            wv = wv * (torch.rand(G, N, K, generator=gen) * case.wden < 1.0).float()
        W[0, p.w_idx] = wv
        A[1, p.a_idx] = _randint(gen, -2, 2, (C, G, M, K))
        W[1, p.w_idx] = _randint(gen, -2, 2, (G, N, K))
    if case.lo == "zero":
        A[1, p.a_idx] = 0.0
        W[1, p.w_idx] = 0.0
    p.A, p.W = A[:P].contiguous(), W[:P].contiguous()
    p.a = [p.A[pl][p.a_idx].double() for pl in range(P)]      # logical operands [C, G, M, K], [G, N, K]
    p.w = [p.W[pl][p.w_idx].double() for pl in range(P)]
    p.bias_bs = N
    p.bias = _randint(gen, -8, 8, (G * N,)) if case.bias else None
    # outputs: C*M rows of G column groups inside guard rows (and, ldo > 0, guard columns)
    p.No = p.d if case.kv else N                                  # columns that reach out_f32 / out_t (the Q range of a QKV launch)
    p.ldo = G * p.No + case.ldo
    p.C0 = 8 if case.ldo else 0
    assert case.ldo == 0 or case.ldo >= 8
    p.out_bs, p.out_bs2 = p.No, M * p.ldo
    p.base = R0 * p.ldo + p.C0
    if S > 1:
        p.ks_stride = M * p.ldo + 8
        p.total = p.base + (S + 1) * p.ks_stride                  # a whole guard plane behind plane S - 1
    else:
        p.ks_stride = 0
        p.total = (R0 + C * M + R0) * p.ldo
    c_, g_, m_, n_ = torch.meshgrid(torch.arange(C), torch.arange(G), torch.arange(M), torch.arange(p.No), indexing="ij")
    p.off = p.base + c_ * p.out_bs2 + g_ * p.out_bs + m_ * p.ldo + n_
    # residual: rows of its own stride; always C*M rows (rows >= resid_row_mod are there to be never read)
    p.ldr = G * p.No + case.ldr
    assert C == 1 or p.ldr == p.ldo                               # out_batch_stride2 moves outputs and residual alike
    p.resid = _randint(gen, -8, 8, (C * M * p.ldr,)) if case.resid else None
    rrow = m_ % case.rmod if case.rmod else m_
    p.r_idx = c_ * p.out_bs2 + g_ * p.out_bs + rrow * p.ldr + n_
    if case.kv:
        p.kv_total = p.B * p.H * p.Lpad * p.hd + 16
    if case.stat:
        assert N % 64 == 0 and G == 1 and C == 1
        p.stat_base, p.stat_total = 4, 4 + (N // 64) * M * 2 + 8
    return p


def outputs_of(p):
    """Names of the buffers a launch of p writes."""
    names = [n for n in ("f32", "t") if p.case.out in (n, "both")]
    if p.case.kv:
        names += ["kp", "vp"]
    if p.case.stat:
        names.append("stat")
    return names


def buffer_dtype(kind, name):
    return torch.float32 if name in ("f32", "stat") else plane_dtype(kind)


def blank(p):
    """Sentinel-filled output buffers [planes, elements]: NaN for fp32 outputs, SENT16 for 16-bit ones and for packed K / V."""
    out = {}
    for name in outputs_of(p):
        dt = buffer_dtype(p.kind, name)
        P = 1 if name in ("f32", "stat") else p.P
        n = {"f32": p.total, "t": p.total, "stat": getattr(p, "stat_total", 0)}.get(name, getattr(p, "kv_total", 0))
        fill = SENT16 if (name in ("kp", "vp") or dt != torch.float32) else float("nan")
        out[name] = torch.full((P, n), fill, dtype=dt)
    return out


def to_kind(kind, x32, trunc=False):
    """fp32 values -> [planes, ...] in the kind's storage type: round to nearest even (torch's CPU cast), the split kind as
    store_opnd4 does.  trunc: the mistake of rounding toward zero instead."""
    def cast(x, dt):
        r = x.to(dt)
        if not trunc:
            return r
        over = r.float().abs() > x.abs()
        return torch.where(over, r.view(torch.int16) - 1, r.view(torch.int16)).view(dt)
    x32 = x32.float()
    if kind == F32:
        return x32.unsqueeze(0)
    if kind == BF16:
        return cast(x32, torch.bfloat16).unsqueeze(0)
    if kind == F16:
        return cast(x32, torch.float16).unsqueeze(0)
    hi = cast(x32, torch.float16)
    lo = ((x32 - hi.float()) * SPLIT_SCALE).half()
    return torch.stack([hi, lo])


def differing(a, b):
    """Mask of the elements that differ: equal values are equal (torch.equal's sense, +0 == -0); a NaN equals only the very
    same bit pattern, so the NaN sentinel matches itself and no other NaN, and no number."""
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return (a.view(it) != b.view(it)) & ~(a == b)


def identical(a, b):
    """torch.equal over whole sentinel-filled buffers (differing(): the NaN sentinel compares by its bits)."""
    return a.shape == b.shape and a.dtype == b.dtype and not bool(differing(a, b).any())


# ---------------------------------------------------------------------------------------------------------------------
# exact reference
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
@_one_thread
def _stages(kind, case):
    """fp64 evaluation of the documented expression, stage by stage, per K slice: lists over s of [C, G, M, N] tensors."""
    p = problem(kind, case)
    per = p.K // p.S
    st = SimpleNamespace(hh=[], cross=[], mag=[], acc=[], biased=[], act=[], v=[])
    mm = lambda x, y, k0, k1: torch.einsum("cgmk,gnk->cgmn", x[..., k0:k1], y[..., k0:k1])  # noqa: E731
    for s in range(p.S):
        k0, k1 = s * per, (s + 1) * per
        hh = mm(p.a[0], p.w[0], k0, k1)
        mag = mm(p.a[0].abs(), p.w[0].abs(), k0, k1)
        cross = torch.zeros_like(hh)
        if p.P == 2:
            cross = mm(p.a[0], p.w[1], k0, k1) + mm(p.a[1], p.w[0], k0, k1)
            mag = torch.maximum(mag, mm(p.a[0].abs(), p.w[1].abs(), k0, k1) + mm(p.a[1].abs(), p.w[0].abs(), k0, k1))
        acc = hh + cross / SPLIT_SCALE
        v = acc
        if p.bias is not None and s == 0:
            v = v + p.bias.double().view(1, p.G, 1, p.N)
            mag = mag + p.bias.double().abs().view(1, p.G, 1, p.N)
        biased = v
        if case.act == ACT_RELU:
            v = v.clamp_min(0.0)
        elif case.act == ACT_LEAKY02:
            v32 = v.float()                                        # (exact: assert_exact checks the round trip)
            v = torch.where(v32 > 0, v32, torch.tensor(0.2, dtype=torch.float32) * v32).double()
        act = v
        if p.resid is not None and s == 0:
            assert p.No == p.N
            r = p.resid.double()[p.r_idx]
            v = v + r
            mag = mag + r.abs()
        for k_, x in zip(("hh", "cross", "mag", "acc", "biased", "act", "v"), (hh, cross, mag, acc, biased, act, v)):
            getattr(st, k_).append(x)
    return st


@functools.lru_cache(maxsize=None)
@_one_thread
def reference(kind, case):
    """Exact outputs as fp64 tensors: f32 [S, C, G, M, No] (S K-slice planes; S = 1 otherwise), t [planes, C, G, M, No] (the
    operand-kind copy), kp / vp [planes, B*H, Lpad*hd] (pad keys = SENT16), stat [N/64, M, 2]."""
    p = problem(kind, case)
    v = torch.stack(_stages(kind, case).v)                         # [S, C, G, M, N]
    ref = SimpleNamespace(f32=v[..., :p.No], t=to_kind(kind, v[0, ..., :p.No].float()).double())
    if case.kv:
        heads = lambda x: to_kind(kind, x.reshape(p.B, p.L, p.H, p.hd).permute(0, 2, 1, 3).float())  # noqa: E731
        k, vv = heads(v[0, 0, 0][:, p.d:2 * p.d]), heads(v[0, 0, 0][:, 2 * p.d:])
        if p.P == 1:
            k, vv = k[0], vv[0]
        kp, vp = pack_host(k, vv, p.Lpad, kind, SENT16)
        ref.kp, ref.vp = kp.double().view(p.P, p.B * p.H, -1), vp.double().view(p.P, p.B * p.H, -1)
    if case.stat:
        x = v[0, 0, 0].view(p.M, p.N // 64, 64)
        ref.stat = torch.stack([x.sum(-1), (x * x).sum(-1)], -1).transpose(0, 1).contiguous()      # [(n / 64), m, {sum, sum of squares}]
    return ref


@functools.lru_cache(maxsize=None)
@_one_thread
def expected(kind, case):
    """reference() laid into the sentinel buffers of blank(): name -> [planes, elements] in the storage type.  Built once per
    (kind, case) and shared: never modified."""
    p, ref = problem(kind, case), reference(kind, case)
    out = blank(p)
    if "f32" in out:
        for s in range(p.S):
            out["f32"][0, p.off + s * p.ks_stride] = ref.f32[s].float()
    if "t" in out:
        for pl in range(p.P):
            out["t"][pl, p.off] = ref.t[pl].to(out["t"].dtype)
    for name in ("kp", "vp"):
        if name in out:
            out[name][:, :p.kv_total - 16] = getattr(ref, name).reshape(p.P, -1).to(out[name].dtype)
    if "stat" in out:
        out["stat"][0, p.stat_base:p.stat_base + ref.stat.numel()] = ref.stat.reshape(-1).float()
    return out


@_one_thread
def assert_exact(kind, case):
    """The conditions under which the fp64 reference is the exact fp32 answer in any accumulation order (module docstring)."""
    p, st = problem(kind, case), _stages(kind, case)
    dt = plane_dtype(kind)
    for name, x in (("A", p.A), ("W", p.W), ("the 16-bit sentinel", torch.tensor([SENT16, GAP]))):
        assert torch.equal(x.to(dt).float(), x), f"{name} does not survive the cast to the kind's storage type"
    for name, x in (("bias", p.bias), ("resid", p.resid)):
        assert x is None or (torch.equal(x, x.round()) and float(x.abs().max()) <= 8.0), f"{name} is not integers in [-8, 8]"
    rt = lambda x: torch.equal(x.float().double(), x) and bool(torch.isfinite(x).all())  # noqa: E731
    for s in range(p.S):
        assert float(st.mag[s].max()) < 2.0 ** 24, "sum |a||w| + |bias| + |resid| reaches 2^24"
        assert torch.equal(st.hh[s], st.hh[s].round()) and torch.equal(st.cross[s], st.cross[s].round())
        if p.P == 2:
            assert float(st.hh[s].abs().max()) < 2.0 ** 12 and float(st.cross[s].abs().max()) < 2.0 ** 12
        for x in (st.acc[s], st.biased[s], st.act[s], st.v[s]):
            assert rt(x), "a stage of the reference does not survive fp32"
        if case.act == ACT_LEAKY02:
            assert p.resid is None, "leaky cases carry no residual (a second rounding, or a fused multiply-add, could differ)"
    if case.stat:
        v = st.v[0]
        assert torch.equal(v, v.round()), "stat_out cases need integer outputs (squares of k / 2048 do not fit fp32)"
        assert float((v * v).view(p.M, p.N // 64, 64).sum(-1).max()) < 2.0 ** 24
    ref = reference(kind, case)
    for x in (ref.f32, ref.t) + ((ref.kp, ref.vp) if case.kv else ()) + ((ref.stat,) if case.stat else ()):
        assert rt(x)


# ---------------------------------------------------------------------------------------------------------------------
# CPU twin: the GEMM contract (include/fdm_hip.h, fdm_gemm_args) restated with flat offsets and k-tiles, each slip switchable
# ---------------------------------------------------------------------------------------------------------------------
ALL, SPLIT, SIXTEEN = tuple(KINDS), (F16X3,), (BF16, F16, F16X3)
MISTAKES = {                       # name -> kinds it can show in
    "last_ktile_dropped": ALL, "last_chunk_dropped": ALL, "first_ktile_twice": ALL, "last_col_unwritten": ALL, "last_row_unwritten": ALL,
    "bias_tile_relative": ALL, "bias_ragged_prev_group": ALL, "resid_row_unwrapped": ALL, "ldr_as_n": ALL, "lda_as_k": ALL,
    "batch_ignored_w": ALL, "batch_ignored_bias": ALL, "batch_ignored_out": ALL, "out_bs2_omitted": ALL,
    "ksplit_bias_every_slice": ALL, "ksplit_ranges_swapped": ALL, "kp_row_without_clip": ALL, "vp_head_zero": ALL,
    "split_cross_unscaled": SPLIT, "split_lo_ignored": SPLIT, "out_t_truncated": SIXTEEN,
}


def can_show(mistake, case):
    """Whether the form of `case` can show `mistake` at all (the CPU test tries these cases first; it does not rely on it)."""
    return {"first_ktile_twice": case.ku == 1 and not case.K, "bias_tile_relative": case.bias and case.N > 64,
            "bias_ragged_prev_group": case.bias and case.N % 4 != 0 and case.N > 4, "resid_row_unwrapped": case.rmod > 0,
            "ldr_as_n": case.ldr > 0, "lda_as_k": case.lda != "dense", "batch_ignored_w": case.G > 1, "batch_ignored_bias": case.G > 1,
            "batch_ignored_out": case.G > 1, "out_bs2_omitted": case.C > 1, "ksplit_bias_every_slice": case.S > 1,
            "ksplit_ranges_swapped": case.S > 1, "kp_row_without_clip": bool(case.kv), "vp_head_zero": bool(case.kv),
            "out_t_truncated": case.values == "round"}.get(mistake, True)


def _kp_off(l, e, hd, E):
    """csrc/common.hpp kp_offset."""
    KT = 4 * E
    nsub, nks = KT // 16, hd // (4 * E)
    kt, w = l // KT, l % KT
    s, r = (((w >> 2) & 1), (((w >> 3) << 2) | (w & 3))) if nsub == 2 else (torch.zeros_like(w), w)
    ch = e // E
    return ((((kt * nsub + s) * nks + (ch >> 2)) * 4 + (ch & 3)) * 16 + r) * E + e % E


def _vp_off(l, e, hd, E):
    """csrc/common.hpp vp_offset."""
    KT = 4 * E
    kt, w = l // KT, l % KT
    return (((kt * (hd >> 4) + (e >> 4)) * 4 + w // E) * 16 + (e & 15)) * E + w % E


@_one_thread
def model(kind, case, mistake=None):
    """name -> buffer, as blank(): what the contract writes, in fp32 arithmetic over k-tiles; `mistake` switches one slip on."""
    assert mistake is None or mistake in MISTAKES
    p = problem(kind, case)
    mis = lambda name: mistake == name  # noqa: E731
    out = blank(p)
    ku, E, M, N, K, No = k_unit(kind), epc(kind), p.M, p.N, p.K, p.No
    nk, ar = K // ku, torch.arange
    per = nk // p.S
    m_, n_ = ar(M).view(M, 1), ar(N).view(1, N)
    wmask = torch.ones(M, N, dtype=torch.bool)
    if mis("last_col_unwritten"):
        wmask[:, N - 1] = False
    if mis("last_row_unwritten"):
        wmask[M - 1, :] = False
    for c in range(p.C):
        for g in range(p.G):
            lda = K if mis("lda_as_k") else p.lda
            ai = g * p.a_bs + c * p.a_bs2 + m_ * lda + ar(K).view(1, K)
            wi = (0 if mis("batch_ignored_w") else g) * p.w_bs + ar(N).view(N, 1) * p.ldw + ar(K).view(1, K)
            a, w = [p.A[pl][ai] for pl in range(p.P)], [p.W[pl][wi] for pl in range(p.P)]
            for s in range(p.S):
                src = p.S - 1 - s if mis("ksplit_ranges_swapped") else s
                tiles = list(range(src * per, (src + 1) * per))
                if mis("last_ktile_dropped") and tiles[-1] == nk - 1:
                    tiles = tiles[:-1]
                if mis("first_ktile_twice") and nk == 1:
                    tiles = tiles + tiles
                acc, accl = torch.zeros(M, N), torch.zeros(M, N)
                for kt in tiles:
                    k0, k1 = kt * ku, (kt + 1) * ku - (E if mis("last_chunk_dropped") and kt == nk - 1 else 0)
                    acc += a[0][:, k0:k1] @ w[0][:, k0:k1].t()
                    if p.P == 2 and not mis("split_lo_ignored"):
                        accl += a[0][:, k0:k1] @ w[1][:, k0:k1].t()
                        accl += a[1][:, k0:k1] @ w[0][:, k0:k1].t()
                if p.P == 2:
                    acc = acc + accl * (1.0 if mis("split_cross_unscaled") else 1.0 / SPLIT_SCALE)
                v = acc
                if p.bias is not None and (s == 0 or mis("ksplit_bias_every_slice")):
                    bn = n_.clone()
                    if mis("bias_tile_relative"):
                        bn = bn % 64
                    if mis("bias_ragged_prev_group") and N % 4 and N > 4:
                        bn = torch.where(bn >= N // 4 * 4, bn - 4, bn)
                    v = v + p.bias[(0 if mis("batch_ignored_bias") else g) * p.bias_bs + bn]
                if case.act == ACT_RELU:
                    v = torch.relu(v)
                elif case.act == ACT_LEAKY02:
                    v = torch.where(v > 0, v, torch.tensor(0.2, dtype=torch.float32) * v)
                zoff = (0 if mis("batch_ignored_out") else g) * p.out_bs + (0 if mis("out_bs2_omitted") else c) * p.out_bs2
                if p.resid is not None and s == 0:
                    rrow = m_ % case.rmod if (case.rmod and not mis("resid_row_unwrapped")) else m_
                    v = v + p.resid[zoff + rrow * (N if mis("ldr_as_n") else p.ldr) + n_]
                # stores: columns below No to out_f32 / out_t, the K and V ranges of a QKV launch to the packed buffers
                dst = (p.base + s * p.ks_stride + zoff + m_ * p.ldo + n_)[:, :No]
                wm, vq = wmask[:, :No], v[:, :No]
                if "f32" in out:
                    out["f32"][0, dst[wm]] = vq[wm]
                if "t" in out and s == 0:
                    tk = to_kind(kind, vq, trunc=mis("out_t_truncated"))
                    for pl in range(p.P):
                        out["t"][pl, dst[wm]] = tk[pl][wm]
                if case.kv:
                    blk = p.Lpad * p.hd
                    b, l = m_ // p.L, m_ % p.L
                    cc = ar(p.d).view(1, p.d)
                    h, e = cc // p.hd, cc % p.hd
                    kd = ((0 if mis("kp_row_without_clip") else b) * p.H + h) * blk + _kp_off(l, e, p.hd, E)
                    vd = (b * p.H + (0 if mis("vp_head_zero") else h)) * blk + _vp_off(l, e, p.hd, E)
                    for name, d_, c0 in (("kp", kd, p.d), ("vp", vd, 2 * p.d)):
                        tk, wm = to_kind(kind, v[:, c0:c0 + p.d], trunc=mis("out_t_truncated")), wmask[:, c0:c0 + p.d]
                        for pl in range(p.P):
                            out[name][pl, d_[wm]] = tk[pl][wm]
                if case.stat:
                    x = torch.where(wmask, v, torch.zeros_like(v)).view(M, N // 64, 64)
                    sd = p.stat_base + ar(N // 64).view(1, -1) * 2 * M + 2 * m_
                    out["stat"][0, sd] = x.sum(-1)
                    out["stat"][0, sd + 1] = (x * x).sum(-1)
    return out
