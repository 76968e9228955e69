"""Attention on its own: host packing, exact operands, an fp64 reference, a per-element error bound, input builders and the
case list shared by tests/test_attention_edges_cpu.py and tests/test_attention_edges_gpu.py.  Plain helper module (pytest does
not collect it); nothing here needs a device except the split-kind branch of operands(..., device=...).

The bound
---------
For query i of one (clip, head), with visible keys j (n_i of them), s_ij the fp64 score and p = softmax(s):

    |o_gpu - o_ref|_ie <= 2 * [ u_P + u_O + 2*delta_i + (n_i + 4) * 2^-24 ] * A_ie + tiny_ie
    delta_i = ((hd + 2) * 2^-24 + u_ll) * T_i + 2^-22 * M_i
    A_ie = sum_j p_ij |v_je|      T_i = max_j scale * sum_e |q_ie||k_je|      M_i = max_j |s_ij|

Derivation, following csrc/attention.hpp:
  * the score is an fp32-accumulated dot product of hd terms (error <= (hd + 2) * 2^-24 * T_i; the split kind also drops the
    lo.lo product, <= 2^-22 * T_i = u_ll * T_i), multiplied by the scale, biased and (16-bit kinds) carried in the log2 domain:
    two fp32 roundings of a number of size <= M_i plus a 1-2 ulp exp / exp2 whose argument has size <= 2 M_i: 2^-22 * M_i;
  * an absolute score error delta is a relative error delta of exp(s - m); it enters the numerator and the denominator: 2*delta_i;
  * the probabilities are rounded to the kind for the second product (u_P) and summed in fp32 over n_i keys, the row sums as
    well ((n_i + 4) * 2^-24, the 4 for the rescales and the merge), the result is rounded to the kind (u_O);
  * the four waves' partial states are merged with one more exp and one more fp32 product each: the leading 2.
  unit roundoffs       u_P = u_O      u_ll
    fp32               2^-24          0
    bf16               2^-8           0
    fp16               2^-11          0
    split fp16         2^-21          2^-22
  * tiny_ie (added to the issue's formula; it is the only term that is not relative to A_ie).  fp16 has a narrow exponent range:
    a probability below 2^-14 (relative to its wave's running maximum, so p~ <= 1) or an output below 2^-14 is rounded to a
    SUBNORMAL fp16 with absolute error <= 2^-25 instead of relative error 2^-11.  The later rescales, the merge weights and
    1 / l are all <= 1 (l >= 1: the row maximum itself contributes 1), so a key adds at most 2^-25 |v_je| and the store at
    most 2^-25:   tiny_ie = 2^-25 * (1 + 2 * V1_ie),  V1_ie = sum over visible j of |v_je|   (fp16; the 2 is the merge's)
    The split kind rounds its lo plane, (x - hi) * 2^11, the same way: 2^-25 / 2^11 = 2^-36 in place of 2^-25.
    fp32 and bf16 share fp32's exponent range: tiny = 1e-30.
Nothing in the bound is fitted to what the kernel returns."""
import math
from collections import namedtuple

import torch

from fdm_amd._lib import BF16, F16, F16X3, F32

KINDS = [F32, BF16, F16, F16X3]
KIND_NAMES = {F32: "f32", BF16: "bf16", F16: "f16", F16X3: "f16x3"}
SPLIT_SCALE = 2048.0
_U = {F32: (2.0 ** -24, 0.0), BF16: (2.0 ** -8, 0.0), F16: (2.0 ** -11, 0.0), F16X3: (2.0 ** -21, 2.0 ** -22)}
_TINY = {F32: None, BF16: None, F16: 2.0 ** -25, F16X3: 2.0 ** -36}


def kv_pad(L):
    return (L + 31) // 32 * 32


def plane_dtype(kind):
    return {BF16: torch.bfloat16, F16: torch.float16, F16X3: torch.float16}.get(kind, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
def pack_host(k, v, Lpad, kind, pad_fill=0.0):
    """Host restatement of the fragment-packed K / V layouts (include/fdm_hip.h, fdm_attn_args).
    k, v: [B, H, L, hd] -> two [B*H, Lpad*hd] tensors, pad keys = pad_fill (any finite value).  A split kind is packed plane by
    plane: k, v are then [2, B, H, L, hd] (hi, lo) and the results [2, B*H, Lpad*hd], both planes' pads = pad_fill."""
    if k.dim() == 5:
        pk, pv = zip(*(pack_host(k[p], v[p], Lpad, kind, pad_fill) for p in range(k.shape[0])))
        return torch.stack(pk), torch.stack(pv)
    B, H, L, hd = k.shape
    epc = 8 if kind in (BF16, F16, F16X3) else 4
    kt_keys = 4 * epc
    nsub, nks = kt_keys // 16, hd // (4 * epc)
    l = torch.arange(L).view(L, 1)
    e = torch.arange(hd).view(1, hd)
    kt, w = l // kt_keys, l % kt_keys
    if nsub == 2:
        sub, r = (w >> 2) & 1, ((w >> 3) << 2) | (w & 3)
    else:
        sub, r = torch.zeros_like(w), w
    ch = e // epc
    koff = (((((kt * nsub + sub) * nks + (ch >> 2)) * 4 + (ch & 3)) * 16 + r) * epc + e % epc).reshape(-1)
    voff = ((((kt * (hd // 16) + (e >> 4)) * 4 + w // epc) * 16 + (e & 15)) * epc + w % epc).reshape(-1)
    assert koff.unique().numel() == L * hd and voff.unique().numel() == L * hd
    kp = torch.full((B * H, Lpad * hd), pad_fill, dtype=k.dtype)
    vp = torch.full((B * H, Lpad * hd), pad_fill, dtype=v.dtype)
    kp[:, koff] = k.reshape(B * H, L * hd)
    vp[:, voff] = v.reshape(B * H, L * hd)
    return kp, vp


def rows(x):
    """[B, H, L, hd] -> the row-major [B*L, H*hd] matrix the kernel takes for Q and writes for O."""
    B, H, L, hd = x.shape
    return x.transpose(1, 2).reshape(B * L, H * hd)


def unrows(x, B, H, L, hd):
    return x.reshape(B, L, H, hd).transpose(1, 2)


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def split_host(x):
    """fp32 -> (hi, lo) fp16 planes, x ~= hi + lo / 2^11 (the arithmetic of the library's cast, on the host)."""
    x = x.float().clamp(-65504.0, 65504.0)
    hi = x.half()
    lo = ((x - hi.float()) * SPLIT_SCALE).half()
    return torch.stack([hi, lo])


def exact(kind, planes):
    """fp64 value of what the kernel reads."""
    if kind == F16X3:
        return planes[0].double() + planes[1].double() / SPLIT_SCALE
    return planes.double()


class Operands:
    """planes: (q, k, v), each [B, H, L, hd] in the kind's storage type ([2, B, H, L, hd] for the split kind);
    q, k, v: their exact fp64 values."""

    def __init__(self, kind, planes):
        self.kind, self.planes = kind, planes
        self.q, self.k, self.v = (exact(kind, p) for p in planes)
        self.B, self.H, self.L, self.hd = self.q.shape

    def device_inputs(self, device, pad_fill=0.0, ldq=None, sentinel=0.0):
        """(Q, Kp, Vp, Lpad) on the device.  ldq > H*hd: Q is the first H*hd columns of a [B*L, ldq] buffer whose other
        columns hold `sentinel`."""
        from fdm_amd import ops
        Lpad, d = kv_pad(self.L), self.H * self.hd
        qp, kp, vp = self.planes
        Kp, Vp = pack_host(kp, vp, Lpad, self.kind, pad_fill)
        if self.kind == F16X3:
            qm = torch.stack([rows(qp[0]), rows(qp[1])])
        else:
            qm = rows(qp)
        if ldq is not None and ldq != d:
            wide = torch.full(qm.shape[:-1] + (ldq,), sentinel, dtype=qm.dtype)
            wide[..., :d] = qm
            qm = wide
        qm, Kp, Vp = qm.contiguous().to(device), Kp.to(device), Vp.to(device)
        if self.kind == F16X3:
            return ops.Split(qm, F16X3), ops.Split(Kp, F16X3), ops.Split(Vp, F16X3), Lpad
        return qm, Kp, Vp, Lpad


def operands(kind, q, k, v, device=None):
    """fp32 q, k, v [B, H, L, hd] -> Operands of `kind`: rounded to bf16 / fp16 on the host, split by the library's own cast
    when a device is given (split_host otherwise), so that the reference starts from what the kernel actually reads."""
    if kind == F32:
        planes = tuple(t.float().clone() for t in (q, k, v))
    elif kind == BF16:
        planes = tuple(t.float().bfloat16() for t in (q, k, v))
    elif kind == F16:
        planes = tuple(t.float().clamp(-65504.0, 65504.0).half() for t in (q, k, v))
    elif device is None:
        planes = tuple(split_host(t) for t in (q, k, v))
    else:
        from fdm_amd import ops
        planes = tuple(ops.to_operand(t.float().contiguous().to(device), F16X3).planes.cpu() for t in (q, k, v))
    return Operands(kind, planes)


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "o A T M n V1")


def reference(qh, kh, vh, scale, causal, slopes, period):
    """fp64 attention of exact operands [B, H, L, hd].  s_ij = scale * q_i.k_j - slope_h * floor((i - j) / period), the same
    floor formula for j > i when not causal, -inf for j > i when causal.  Returns o and the scale quantities of bound()."""
    B, H, L, hd = qh.shape
    qh, kh, vh = qh.double(), kh.double(), vh.double()
    i = torch.arange(L).view(L, 1)
    j = torch.arange(L).view(1, L)
    s = torch.einsum("bhid,bhjd->bhij", qh, kh) * scale
    if slopes is not None:
        fl = torch.div(i - j, period, rounding_mode="floor").double()
        s = s - slopes.double().view(1, H, 1, 1) * fl
    vis = (j <= i) if causal else torch.ones(L, L, dtype=torch.bool)
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.softmax(s, -1)
    o = torch.einsum("bhij,bhjd->bhid", p, vh)
    A = torch.einsum("bhij,bhjd->bhid", p, vh.abs())
    T = (torch.einsum("bhid,bhjd->bhij", qh.abs(), kh.abs()) * scale).masked_fill(~vis, 0.0).amax(-1)
    M = s.abs().masked_fill(~vis, 0.0).amax(-1)
    n = vis.sum(-1).double().view(1, 1, L).expand(B, H, L)
    V1 = torch.einsum("ij,bhjd->bhid", vis.double(), vh.abs())
    return Ref(o, A, T, M, n, V1)


def bound(kind, ref, hd):
    """Per-element bound [B, H, L, hd] on |o_kernel - ref.o| (module docstring)."""
    u, u_ll = _U[kind]
    delta = ((hd + 2) * 2.0 ** -24 + u_ll) * ref.T + 2.0 ** -22 * ref.M
    rel = 2.0 * (u + u + 2.0 * delta + (ref.n + 4.0) * 2.0 ** -24)
    tiny = 1e-30 if _TINY[kind] is None else _TINY[kind] * (1.0 + 2.0 * ref.V1)
    return rel.unsqueeze(-1) * ref.A + tiny


def worst(o, ref, bnd):
    """(ratio, (b, h, i, e), error, bound) of the element with the largest |o - ref| / bound; NaN counts as infinite."""
    err = (o.double() - ref.o).abs()
    ratio = torch.where(torch.isfinite(err), err / bnd, torch.full_like(err, float("inf")))
    flat = int(ratio.argmax())
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(flat), ratio.shape))
    return float(ratio.reshape(-1)[flat]), idx, float(err.reshape(-1)[flat]), float(bnd.reshape(-1)[flat])


# ---------------------------------------------------------------------------------------------------------------------
# inputs (all seeded, all [B, H, L, hd] fp32)
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed, B, H, L, hd):
    return torch.Generator().manual_seed(seed * 1000003 + ((B * 31 + H) * 1009 + L) * 521 + hd)


def gaussian(B, H, L, hd, seed=0):
    g = _gen(seed, B, H, L, hd)
    return tuple(torch.randn(B, H, L, hd, generator=g) for _ in range(3))


def _peaked(B, H, L, hd, seed, late):
    """q_i ~ u, k_j ~ c_j u with |u_e| = 1: with scale hd^-0.5 the score is about c_j sqrt(hd), ramped over the key index from
    60 / L to 60 (late: the row maximum moves in every key tile, up to the last visible one) or from 60 down (early: it sits in
    the first tile).  |k| <= 60 / sqrt(hd) + noise: far inside fp16."""
    g = _gen(seed, B, H, L, hd)
    u = torch.where(torch.rand(B, H, 1, hd, generator=g) < 0.5, -1.0, 1.0)
    pos = torch.arange(L, dtype=torch.float32)
    ramp = ((pos + 1) if late else (L - pos)) / L
    c = (60.0 / math.sqrt(hd)) * ramp.view(1, 1, L, 1)
    q = u + 0.25 * torch.randn(B, H, L, hd, generator=g)
    k = c * u + 0.25 * torch.randn(B, H, L, hd, generator=g)
    v = torch.randn(B, H, L, hd, generator=g)
    return q, k, v


def peaked_late(B, H, L, hd, seed=0):
    return _peaked(B, H, L, hd, seed + 1, True)


def peaked_early(B, H, L, hd, seed=0):
    return _peaked(B, H, L, hd, seed + 2, False)


def skewed_v(B, H, L, hd, seed=0):
    """V columns 5 and hd - 3 of magnitude 1e3 beside columns of 1e-3: only a per-element bound checks the small ones."""
    q, k, v = gaussian(B, H, L, hd, seed + 3)
    col = torch.full((hd,), 1e-3)
    col[5] = col[hd - 3] = 1e3
    return q, k, v * col


def steep_alibi(B, H, L, hd, seed=0):
    """q, k near zero: the bias alone (STEEP slopes, up to 2.0) decides the distribution."""
    q, k, v = gaussian(B, H, L, hd, seed + 4)
    return 1e-3 * q, 1e-3 * k, v


BUILDERS = {"gaussian": gaussian, "peaked_late": peaked_late, "peaked_early": peaked_early, "skewed_v": skewed_v,
            "steep_alibi": steep_alibi}


def slopes_of(name, H):
    if name == "none":
        return None
    if name == "pow2":
        return torch.tensor([2.0 ** -(h + 1) for h in range(H)])
    if name == "steep":
        return torch.tensor([2.0 * 0.75 ** h for h in range(H)])
    raise ValueError(name)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case(namedtuple("Case", "builder B H L hd causal period slopes")):
    @property
    def id(self):
        return f"{self.builder}-{self.B}x{self.H}x{self.L}x{self.hd}-{'causal' if self.causal else 'full'}-p{self.period}-{self.slopes}"

    @property
    def scale(self):
        return 1.0 / math.sqrt(self.hd)

    def inputs(self):
        return BUILDERS[self.builder](self.B, self.H, self.L, self.hd)

    def slope_values(self):
        return slopes_of(self.slopes, self.H)


_C, _N = True, False
# Hand-picked, not the product: head dims 64 / 128 / 256; L around one fp32 (16) and one 16-bit (32) key tile, two tiles, and
# several per wave; the switch to two query sub-tiles (383 / 384 / 385, 415) with one (clip, head); B*H of 1, 3, 9 (the grid pads to
# rounds of 8) and 16; the periodic step's fast form (period >= 8: 8, 9, 25, 30, 1000 > L) and slow form (1, 3, 7); slopes
# without the causal mask; every builder.  Every kind runs every case.
CASES = [
    Case("gaussian", 1, 1, 1, 64, _C, 30, "pow2"),
    Case("gaussian", 1, 3, 15, 128, _C, 3, "pow2"),
    Case("gaussian", 3, 3, 16, 64, _N, 1, "none"),
    Case("gaussian", 2, 8, 17, 128, _C, 7, "pow2"),
    Case("gaussian", 1, 1, 31, 256, _C, 8, "pow2"),
    Case("gaussian", 1, 3, 32, 64, _C, 9, "pow2"),
    Case("gaussian", 3, 3, 33, 128, _C, 25, "pow2"),
    Case("gaussian", 2, 8, 47, 64, _C, 30, "pow2"),
    Case("gaussian", 1, 3, 65, 256, _C, 1000, "pow2"),
    Case("gaussian", 2, 8, 130, 128, _C, 1, "pow2"),
    Case("gaussian", 1, 1, 1, 128, _N, 1, "none"),
    Case("gaussian", 1, 3, 15, 64, _N, 1, "none"),
    Case("gaussian", 1, 1, 16, 256, _N, 1, "none"),
    Case("gaussian", 1, 1, 17, 256, _N, 1, "none"),
    Case("gaussian", 3, 3, 31, 128, _N, 1, "none"),
    Case("gaussian", 1, 3, 33, 64, _N, 1, "none"),
    Case("peaked_late", 1, 3, 47, 128, _C, 30, "pow2"),
    Case("peaked_late", 3, 3, 65, 64, _N, 1, "none"),
    Case("peaked_late", 2, 8, 130, 64, _C, 9, "pow2"),
    Case("peaked_late", 1, 1, 130, 256, _C, 25, "pow2"),
    Case("peaked_early", 1, 3, 65, 128, _C, 8, "pow2"),
    Case("peaked_early", 2, 8, 130, 128, _N, 1, "none"),
    Case("peaked_early", 1, 1, 33, 256, _N, 1, "none"),
    Case("skewed_v", 3, 3, 47, 64, _C, 7, "pow2"),
    Case("skewed_v", 1, 3, 130, 128, _N, 1, "none"),
    Case("skewed_v", 1, 1, 65, 256, _C, 30, "pow2"),
    Case("steep_alibi", 1, 3, 33, 64, _C, 1, "steep"),
    Case("steep_alibi", 3, 3, 65, 128, _C, 3, "steep"),
    Case("steep_alibi", 1, 3, 47, 128, _C, 7, "steep"),
    Case("steep_alibi", 2, 8, 130, 64, _C, 8, "steep"),
    Case("steep_alibi", 1, 3, 130, 128, _C, 9, "steep"),
    Case("steep_alibi", 1, 1, 65, 256, _C, 25, "steep"),
    Case("steep_alibi", 1, 3, 32, 128, _C, 1000, "steep"),
    Case("steep_alibi", 1, 3, 17, 64, _N, 9, "steep"),
    Case("steep_alibi", 1, 1, 31, 128, _N, 7, "steep"),
    # the switch to two query sub-tiles per workgroup (single-plane kinds, head dim <= 128), one (clip, head)
    Case("gaussian", 1, 1, 383, 128, _C, 30, "pow2"),
    Case("gaussian", 1, 1, 384, 128, _C, 30, "pow2"),
    Case("gaussian", 1, 1, 385, 128, _C, 30, "pow2"),
    Case("gaussian", 1, 1, 384, 64, _N, 1, "none"),
    Case("peaked_late", 1, 1, 415, 64, _C, 25, "pow2"),
    Case("peaked_early", 1, 1, 385, 64, _N, 1, "none"),
    Case("skewed_v", 1, 1, 383, 64, _C, 9, "pow2"),
    Case("steep_alibi", 1, 1, 415, 128, _C, 8, "steep"),
    Case("peaked_late", 1, 1, 385, 256, _C, 30, "pow2"),
]


def largest_case(builder):
    """The case of `builder` with the most score elements."""
    return max((c for c in CASES if c.builder == builder), key=lambda c: c.B * c.H * c.L * c.L * c.hd)
