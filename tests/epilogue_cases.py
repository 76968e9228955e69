"""The GEMM's inexact epilogue forms -- Mish, GELU(erf), GELU(tanh) through gemm_act<HEAVY, T> (csrc/gemm.hpp) -- and act_apply's
two other callers (ops.bias_act, ops.small_linear): case lists, fp64 references of exactly what the kernel reads, per-element
bounds counted from the kernel's arithmetic and a CPU twin of each form with a defect= switch, shared by
tests/test_gemm_epilogue_cpu.py and tests/test_gemm_epilogue_gpu.py.  Plain helper module (pytest does not collect it), host only.

The pre-activation value is known bit for bit
---------------------------------------------
Operands are exact in every kind (gemm_cases.assert_exact): values "rowcol" gives acc[m, n] = I_m + J_n, I_m = m % 49 - 24,
J_n a small integer; "row" gives J_n = 0 (from +1 -1 pairs: the products are live) and I_m = 0 in every third row.  The fp32
bias carries the grid: the value entering the activation is v = fl32(acc + bias[n]), one fp32 addition, the same on the host.
  grid launch      bias[n] = (n % 64) / 64 - J_n: v = I_m + (n % 64) / 64, every multiple of 1 / 64 in [-24, 24.98]
  special launch   bias[n] = SPECIALS[n]: the rows with I_m = 0 carry the special value itself, the other rows its neighbours
                   I_m + special (the values around +-20, +-44, +-88 move across the thresholds; the large ones absorb I_m)
-0 cannot enter the GEMM's activation (the accumulator is +0 and +0 + -0 = +0); ops.bias_act reaches it (in = -0, no vector).

Bounds (u = 2^-24; -ffp-contract=off: every +, * and / rounds once, u relative)
---------------------------------------------------------------------------
A first-order count through the expression, times SLACK = 2 for what first order leaves out (products of the terms, 1-ulp
rather than half-ulp divides), as tests/norm_cases.py does.  Transcendentals: R = 4u relative (2 ulp of the result), the allowance
of norm_cases.py, for the hardware __expf / __logf and for libm's expf, log1pf and tanhf alike (HIP documents 1, 1 and 2 ulp).
  Mish, libm (fp32 and split kinds; act_apply): e = expf(v) (R); sp = log1pf(e): d_sp = e R / (1 + e) + R sp (v > 20: sp = v, which is
      softplus(v) - log1p(e^-v)); t = tanhf(sp): d_t = (1 - t^2) d_sp + R t; out = v t: |v| d_t + u |out|.  No cancellation: relative.
  Mish, hardware (bf16, fp16): e = __expf(v) (R); a = 1 + e: d_a = e R + u a; sp = __logf(a): d_sp = d_a / a + R sp;
      E = __expf(2 sp): relative R + 2 d_sp; b = 1 + E: d_b = E rel(E) + u b; q = 2 / b: d_q = q (d_b / b + u); t = 1 - q: d_t = d_q + u t;
      out = v t: |v| d_t + u |out|.  On the negative tail a rounds to 1 and t cancels: the bound there is absolute, ~ 3u |v|.
  GELU(tanh): c = k (v + 0.044715 v v v): three products, the sum, the product by k and the two fp32 constants: d_c = 7u |c| (the
      terms have one sign).  libm: th = tanhf(c): d_th = (1 - th^2) d_c + R |th|; s = 1 + th: d_s = d_th + u s; out = v (0.5 s):
      0.5 |v| d_s + u |out| (s cancels for c << 0: absolute, ~ 2u |v|).  Hardware: E = __expf(2c): relative R + 2 d_c; b = 1 + E;
      q = 2 / b; t = 2 - q: d_t = d_q + u t; out = v (0.5 t).
  GELU(erf): norm_cases.act_bound (6u |v| + 2u |GELU|; the 16-bit kinds' gelu_erf_fast: GELU_FAST_FORMULA_ERR + 12u |v| + 2u |GELU|).
  then  + u |out + r| for the residual add, + u_T |y_t| + tiny for out_t (fp16 planes: of the value clamped to +-65504), + 1e-30
  (a flushed subnormal).  Nothing here is fitted to what a kernel returns; tests/test_gemm_epilogue_gpu.py prints the measured
  error-to-bound ratios.
  HW_ULPS: the allowance of __expf / __logf in ulps and what the GPU run measured against it are recorded beside the constant.

Bound sanity: over the dense grid the bound never exceeds SANITY = 2^-15 of |reference| + 1 for fp32 outputs, and
u_T + 2^-25 + 2^-15 for out_t (2^-25: fp16's subnormal floor).  The widest bound is gelu_erf_fast's 12u |v| + 2.1e-7 at v = -24,
292u where the reference is 0 (Mish: 240u; libm GELU(erf): 144u); the clean twins reach 0.5 - 1.0 of their bounds where one final
rounding is all there is (the residual add, out_t) and 0.1 - 0.9 elsewhere, so the next power of two above 292u is the fraction: a
wrong branch or a dead term errs by the size of the output, thousands of times that.

Defects of the twins (DEFECTS): each pushes at least one case over its bound.  "softplus_no_threshold" is NOT among them: with
IEEE infinities log(1 + exp(v)) and tanh's overflow-safe form give v for v > 88.7 as well, and between 20 and 88 the logarithm
returns v to an ulp, so leaving the threshold out stays inside the bound (BENIGN; the CPU test asserts that too).  The reverse of
"fast_in_f32" (libm forms in a 16-bit kind) is more accurate than what it replaces and cannot leave a bound either, and
"fast_in_f32" itself is seeded in Mish only: the hardware GELU(tanh) errs by ~ 2u |v| on its tail exactly as libm's 1 + tanhf does,
and gelu_erf_fast's 2.1e-7 lies inside libm GELU(erf)'s 6u |v| wherever it is reached -- bounds cannot tell those apart."""
import functools

import torch

import gemm_cases as GC
import norm_cases as NC
from attn_cases import _TINY, _U, KIND_NAMES, KINDS  # noqa: F401  (re-exported)
from fdm_amd._lib import ACT_GELU_ERF, ACT_GELU_TANH, ACT_LEAKY02, ACT_MISH, ACT_NONE, ACT_RELU, BF16, F16, F16X3, F32

U = 2.0 ** -24
HW_ULPS = 2                    # __expf / __logf: ulps of the result allowed.  Measured on the MI355X with this allowance (never raised): the
                               # hardware Mish reaches 0.35 of its bound, GELU(tanh) 0.34, gelu_erf_fast 0.16 (out_f32, no residual)
R_T = 2.0 * HW_ULPS * U        # the same 2 ulp for libm's expf / log1pf / tanhf
SLACK = 2.0
SANITY = 2.0 ** -15
F64, F32T = torch.float64, torch.float32
HEAVY = (ACT_MISH, ACT_GELU_ERF, ACT_GELU_TANH)
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_MISH: "mish", ACT_GELU_ERF: "gelu_erf", ACT_GELU_TANH: "gelu_tanh", ACT_LEAKY02: "leaky"}
K_TANH, C_TANH = 0.7978845608028654, 0.044715


def fast_kind(kind):
    """is_fast16<T> of csrc/common.hpp: the kinds whose GEMM epilogue takes the hardware forms."""
    return kind in (BF16, F16)


def kind_class(kind):
    return "16-bit" if fast_kind(kind) else "f32-class"


# ---------------------------------------------------------------------------------------------------------------------
# the values
# ---------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return torch.tensor(x, dtype=F32T)


def specials():
    """The fp32 special values, 68 of them (one per column of the widest launch)."""
    t20 = _f32(20.0)
    up, dn = torch.nextafter(t20, _f32(float("inf"))), torch.nextafter(t20, _f32(float("-inf")))
    v = [0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 1e-30, -1e-30, 20.0, float(up), float(dn), -20.0,
         44.0, -44.0, 45.0, -45.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4, 65504.0, -65504.0, 65520.0, -65520.0, 7e4, -7e4,
         1e13, -1e13, 3e38, -3e38,
         # more of the same kind: around the thresholds the forms have (1 + e^v rounds to 1 below -16.6; exp(2 sp) overflows at 44.36;
         # expf at 88.72 and flushes below -87.3; v v v overflows at 6.98e12; GELU(tanh)'s exp(2c) overflows at v = 9.6)
         -16.5, -16.75, -17.0, 16.6, 44.25, 44.375, 44.5, -44.375, 88.5, 88.75, -87.25, -87.5, -103.0, -104.0, 6.9e12, 7.0e12, -6.9e12, -7.0e12,
         9.5, 9.75, -9.5, -9.75, 5.5, -5.5, 3.3e38, -3.3e38, 1e-20, -1e-20, 2.0 ** -24, -2.0 ** -24, 32752.0, -32752.0, 65519.0, -65519.0, 1e5, -1e5]
    t = _f32(v)
    assert t.numel() == 68 and bool(torch.isfinite(t).all())
    return t


def dense_grid():
    """[-24, 24] at a step of 1 / 64."""
    return torch.arange(-24 * 64, 24 * 64 + 1, dtype=F32T) / 64.0


def flat_values():
    """Every value of the issue's list once: what ops.bias_act and ops.small_linear run over."""
    return torch.cat([dense_grid(), specials()])


SHAPES = {"interior": (64, 64), "ragged": (65, 68)}


@functools.lru_cache(maxsize=None)
def act_case(shape, launch):
    """The gemm_cases.Case of one launch: shape 'interior' | 'ragged', launch 'grid' | 'special'.  One k-unit (the lean epilogue on
    the interior shape), no bias and no residual of gemm_cases' own (this module brings them)."""
    M, N = SHAPES[shape]
    return GC.mk(f"epi-act-{shape}-{launch}", M, N, 1, bias=False, resid=False, lo="zero", values="rowcol" if launch == "grid" else "row")


@functools.lru_cache(maxsize=None)
def act_problem(kind, shape, launch):
    """(gemm_cases problem, bias [N] fp32, v [M, N] fp32 = the value entering the activation, resid [M, N] fp32 integers)."""
    case = act_case(shape, launch)
    GC.assert_exact(kind, case)
    p = GC.problem(kind, case)
    acc = GC._stages(kind, case).acc[0][0, 0]                      # [M, N] fp64, exact
    assert torch.equal(acc, acc.round()) and float(acc.abs().max()) < 2 ** 10 and float(acc.abs().max()) > 0
    n = torch.arange(p.N)
    if launch == "grid":
        i_m = (torch.arange(p.M) % 49 - 24).double().view(-1, 1)
        j_n = acc[0:1] - i_m[0:1]
        assert torch.equal(acc, i_m + j_n)
        bias = ((n % 64).double() / 64.0 - j_n[0]).float()
        assert torch.equal(bias.double(), (n % 64).double() / 64.0 - j_n[0])
    else:
        bias = specials()[:p.N].clone()
    v = acc.float() + bias.view(1, -1)                             # the kernel's one fp32 addition
    if launch == "grid":
        assert torch.equal(v.double(), acc + bias.double().view(1, -1))        # (exact here: v is on the grid)
        assert set(dense_grid().tolist()) <= set(v.reshape(-1).tolist())
    else:
        hit = v[(torch.arange(p.M) % 3 == 0)]
        assert all(bool((hit[:, j].view(torch.int32) == bias[j:j + 1].view(torch.int32)).all()) or float(bias[j]) == 0.0 for j in range(p.N))
    g = torch.Generator().manual_seed(1234 + p.M)
    resid = torch.randint(-8, 9, (p.M, p.N), generator=g).float()
    return p, bias, v, resid


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------
def softplus64(v):
    return torch.where(v > 30.0, v, torch.log1p(torch.exp(v.clamp_max(30.0))))


def mish64(v):
    return v * torch.tanh(softplus64(v))


def gelu_erf64(v):
    return 0.5 * v * torch.erfc(-v * 0.7071067811865476)           # 1 + erf(x) = erfc(-x): no cancellation on the negative tail


def _c64(v):
    return K_TANH * (v + C_TANH * v * v * v)


def gelu_tanh64(v):
    return v * (1.0 / (1.0 + torch.exp((-2.0 * _c64(v)).clamp(-700.0, 700.0))))      # 0.5 (1 + tanh c) = 1 / (1 + e^-2c)


def act64(v, act):
    v = v.double()
    if act == ACT_MISH:
        return mish64(v)
    if act == ACT_GELU_ERF:
        return gelu_erf64(v)
    if act == ACT_GELU_TANH:
        return gelu_tanh64(v)
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    if act == ACT_LEAKY02:
        return torch.where(v > 0, v, float(_f32(0.2)) * v)
    return v


def act_bound(fast, act, v):
    """Bound on |act_gpu(v) - act64(v)| for fp32 v (module docstring); fast: the hardware forms."""
    v = v.double()
    a = v.abs()
    ref = act64(v, act)
    if act == ACT_GELU_ERF:
        return NC.act_bound(BF16 if fast else F32, v, torch.zeros_like(v), ACT_GELU_ERF) + 1e-30
    if act == ACT_MISH:
        e = torch.exp(v.clamp_max(80.0))
        sp = softplus64(v)
        if fast:
            one_e = 1.0 + e
            d_sp = (e * R_T + U * one_e) / one_e + R_T * sp
        else:
            d_sp = e * R_T / (1.0 + e) + R_T * sp
        d_sp = torch.where(v > 20.0, torch.exp(-v.clamp_min(0.0)), d_sp)
        t = torch.tanh(sp)
        if fast:
            E = torch.exp((2.0 * sp).clamp_max(700.0))
            b = 1.0 + E
            d_b = E * (R_T + 2.0 * d_sp) + U * b
            q = 2.0 / b
            d_t = q * (d_b / b + U) + U * t
        else:
            d_t = (1.0 - t * t) * d_sp + R_T * t
        return SLACK * (a * d_t + U * ref.abs()) + 1e-30
    if act == ACT_GELU_TANH:
        c = _c64(v)
        d_c = 7.0 * U * c.abs()
        if fast:
            E = torch.exp((2.0 * c).clamp(-700.0, 700.0))
            b = 1.0 + E
            d_b = E * (R_T + 2.0 * d_c) + U * b
            q = 2.0 / b
            d_s = q * (d_b / b + U) + U * (2.0 - q)
        else:
            th = torch.tanh(c)
            d_s = (1.0 - th * th).clamp_min(0.0) * d_c + R_T * th.abs() + U * (1.0 + th)
        d_s = torch.where(torch.isfinite(d_s), d_s, 2.0 * U * torch.ones_like(d_s))      # |c| beyond fp64's exp: the form has saturated
        return SLACK * (0.5 * a * d_s + U * ref.abs()) + 1e-30
    if act == ACT_LEAKY02:
        return U * ref.abs() + 1e-30                               # one product by float32(0.2), which the reference holds exactly
    return torch.full_like(v, 1e-30)                               # exact forms


def clamp_kind(kind, y):
    return y.clamp(-65504.0, 65504.0) if kind in (F16, F16X3) else y


@functools.lru_cache(maxsize=None)
def gemm_reference(kind, act, shape, launch, resid, out):
    """(ref, bound) [M, N] fp64 of output `out` ('f32' | 't') of one launch."""
    _, _, v, r = act_problem(kind, shape, launch)
    return finish(kind, out, act_bound(fast_kind(kind), act, v), act64(v, act), r if resid else None)


def finish(kind, out, bound, ref, resid=None):
    if resid is not None:
        ref = ref + resid.double()
        bound = bound + U * ref.abs()
    if out == "t":
        ref = clamp_kind(kind, ref)
        bound = bound + NC.u_out(kind, "t") * ref.abs() + NC.tiny_out(kind, "t")
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------
# CPU twins: fp32 torch in the kernel's order of operations
# ---------------------------------------------------------------------------------------------------------------------
DEFECTS = {      # name -> (activations, kinds) it is seeded in
    "softplus_wrong_side": ((ACT_MISH,), tuple(KINDS)),
    "tanh_naive": ((ACT_MISH, ACT_GELU_TANH), (BF16, F16)),
    "fast_in_f32": ((ACT_MISH,), (F32, F16X3)),
    "out_t_unclamped": ((ACT_MISH, ACT_GELU_ERF, ACT_GELU_TANH), (F16, F16X3)),
}
BENIGN = {"softplus_no_threshold": ((ACT_MISH,), tuple(KINDS))}


def act_twin(kind, act, v, defect=None, ulps=None):
    """gemm_act<HEAVY, T> (fast kinds) / act_apply in fp32 torch.  ulps = (exp, log): multiply the hardware exp / log results by
    1 + ulps * 2^-23 (the protocol for an allowance that the GPU exceeds)."""
    assert v.dtype == F32T
    one, two, half = _f32(1.0), _f32(2.0), _f32(0.5)
    fast = fast_kind(kind) != (defect == "fast_in_f32")
    xexp = (lambda x: torch.exp(x) * _f32(1.0 + ulps[0] * 2.0 ** -23)) if ulps else torch.exp
    xlog = (lambda x: torch.log(x) * _f32(1.0 + ulps[1] * 2.0 ** -23)) if ulps else torch.log
    if act == ACT_MISH:
        soft = xlog(one + xexp(v)) if fast else torch.log1p(torch.exp(v))
        if defect == "softplus_wrong_side":
            sp = torch.where(v < 20.0, v, soft)
        elif defect == "softplus_no_threshold":
            sp = soft
        else:
            sp = torch.where(v > 20.0, v, soft)
        if fast:
            E = xexp(two * sp)
            return v * ((E - one) / (E + one)) if defect == "tanh_naive" else v * (one - two / (one + E))
        return v * torch.tanh(sp)
    if act == ACT_GELU_TANH:
        c = _f32(K_TANH) * (v + _f32(C_TANH) * v * v * v)
        if fast:
            E = xexp(two * c)
            return v * (half * ((E - one) / (E + one) + one)) if defect == "tanh_naive" else v * (half * (two - two / (one + E)))
        return v * (half * (one + torch.tanh(c)))
    if act == ACT_GELU_ERF:
        return NC.gelu_fast_formula(v) if fast else half * v * (one + torch.erf(v * _f32(0.70710678118654752440)))
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LEAKY02:
        return torch.where(v > 0, v, _f32(0.2) * v)
    return v


def store_twin(kind, y, defect=None):
    """fp32 -> the fp32 value of out_t (store_opnd4 / store_opnd1)."""
    if defect == "out_t_unclamped" and kind in (F16, F16X3):
        hi = y.half()
        return hi.float() if kind == F16 else hi.float() + ((y - hi.float()) * GC.SPLIT_SCALE).half().float() / GC.SPLIT_SCALE
    return NC.round_kind(kind, y)


def gemm_twin(kind, act, shape, launch, resid, defect=None, ulps=None):
    """-> {'f32': [M, N] fp32, 't': fp32 value of out_t}."""
    _, _, v, r = act_problem(kind, shape, launch)
    y = act_twin(kind, act, v, defect, ulps)
    if resid:
        y = y + r
    return {"f32": y, "t": store_twin(kind, y, defect)}


# ---------------------------------------------------------------------------------------------------------------------
# ops.bias_act and ops.small_linear: fp32 kernels on act_apply
# ---------------------------------------------------------------------------------------------------------------------
ALL_ACTS = (ACT_NONE, ACT_RELU, ACT_MISH, ACT_GELU_ERF, ACT_GELU_TANH, ACT_LEAKY02)
D_ODD = 67                     # not a multiple of 4


@functools.lru_cache(maxsize=None)
def bias_act_problem(size, vec):
    """size 'small' (3 x 67 = 201 elements: below one 256-thread block) | 'large' (47 x 67: above); vec: with the per-column vector
    (small integers; without it v = in, which lets -0 and the subnormals through).  -> (in [rows, d], vec [d] | None, v)."""
    vals = flat_values()
    if size == "small":
        rows = 3
        pick = torch.cat([specials(), dense_grid()[::23]])[:rows * D_ODD]
    else:
        rows = 47
        pick = torch.cat([vals, vals])[:rows * D_ODD]
    assert pick.numel() == rows * D_ODD and (size == "small" or vals.numel() <= rows * D_ODD)
    x = pick.view(rows, D_ODD).clone()
    w = ((torch.arange(D_ODD) % 5) - 2).float() if vec else None
    v = x + w if vec else x + _f32(0.0)
    return x, w, v


@functools.lru_cache(maxsize=None)
def small_linear_problem(size, K):
    """out[b, j] = act(bias[j] + sum_k W[j, k] x[b, k]) with acc[b, j] = I_b + J_j exact (fmaf of integers): x[b, 0] = I_b,
    x[b, k > 0] = 1, W[j, 0] = 1, W[j, k > 0] in {-1, 0, 1}.  'large': 49 x 67, bias = the 1 / 64 grid minus J_j; 'small': 3 x 67 = 201
    outputs, I = (0, 1, -1), J_j = 0 (+1 -1 pairs), bias = the specials.  -> (x [B, K], W [d, K], bias [d], v [B, d])."""
    d = D_ODD
    g = torch.Generator().manual_seed(55 + K)
    if size == "large":
        B = 49
        i_b = (torch.arange(B) - 24).float()
        wk = torch.randint(-1, 2, (d, K - 1), generator=g).float()
        bias = ((torch.arange(d) % 64).float() / 64.0 - wk.sum(1))
    else:
        B = 3
        i_b = _f32([0.0, 1.0, -1.0])
        wk = torch.tensor([1.0, -1.0]).repeat(K // 2 + 1)[:K - 1].expand(d, K - 1).clone()
        if (K - 1) % 2:
            wk[:, -1] = 0.0
        bias = specials()[:d].clone()
    x = torch.cat([i_b.view(B, 1), torch.ones(B, K - 1)], 1).contiguous()
    W = torch.cat([torch.ones(d, 1), wk], 1).contiguous()
    acc = x.double() @ W.double().t()
    assert torch.equal(acc, acc.round()) and float(acc.abs().max()) < 2 ** 10
    v = acc.float() + bias.view(1, d)
    return x, W, bias, v


def flat_reference(act, v):
    """(ref, bound) of an fp32 kernel on act_apply."""
    return act64(v, act), act_bound(False, act, v)


def worst(got, ref, bnd):
    return NC.worst(got, ref, bnd)


# ---------------------------------------------------------------------------------------------------------------------
# the LayerNorm fold: producer (GEMM + stat_out), consumers (ln_colsum; rln_gamma / rln_beta on the residual)
# ---------------------------------------------------------------------------------------------------------------------
# Rows of x [M, D = 64 nparts]: x[m, k] = off_m + d[m, k], d integers in [-2, 2] (spread 2), off_m = 2 * ratio, ratio = 0, 1, 8, 64
# by (m + nparts) % 6, a constant row 100 + m % 7 (kind 4) and a row c + 1, c, c, .. (kind 5, _clamp_constant: fp32's
# q / n - mu mu is negative there): every value is an integer below 256, exact in every kind,
# so the 16-bit operand copy x_t the consumer multiplies is x itself and its accumulator is exact.  "real" producers add randn to the
# residual instead: x is then whatever fp32 the launch wrote, and only what is compared with sums of THAT is checked on them
# (the partials, and the F32 / F16X3 chain).
#
# Bounds, counted from gemm_epilogue and gemm_load_rowstats (csrc/gemm.hpp):
#   producer   a value passes (v0 + v1) + (v2 + v3) (2 additions), rows_sum (2) and the four fragments in column order (3): S_PROD = 7.
#              |sum^ - sum| <= 7u sum |x|,  |sq^ - sq| <= 8u sum x^2  (the square's own rounding)            [no leading factor: exact count]
#   statistics s = sum_i s_i and q = sum_i q_i in order (np - 1 additions), inv = 1 / ln_dim (1), the product (1):
#              dmu = (np + 1) u sum |s_i| / n;   E2 = q / n: (np + 1) u E2;   var = max(E2 - mu mu, 0): dvar = (np + 1) u E2 + 2 |mu| dmu
#              + u mu^2 + u var  -- the conditioning factor E2 / (var + eps) of the issue: the subtraction is formed in fp32.
#              rs = 1 / sqrtf(var + eps): not first order when dvar ~ var + eps (a constant row), so an interval:
#              rs_hi = 1 / sqrt(max(var - dvar, 0) + eps), rs_lo = 1 / sqrt(var + dvar + eps), drs = max(rs_hi - rs, rs - rs_lo) + 3u rs_hi
#   colsum     out = ((acc - mu cs) rs) + bias, acc exact:   2 [ rs_hi (u |mu cs| + 2u |acc - mu cs| + dmu |cs|) + |acc - mu cs| drs + u |out| ]
#   rln        out = (acc + bias) + ((((x - mu) rs) g) + b):  2 [ |g| (rs_hi (dmu + 3u |x - mu|) + |x - mu| drs) + u |t| + u |acc + bias| + u |out| ]
#   chain      (F32, F16X3; a real producer) against fp64 LN(x) W^T + b of the fp32 x the producer wrote: the colsum bound with the
#              producer's partial bounds added to the sums (dS = 7u sum |x|, dQ = 8u sum x^2 per row: what norm_cases' P_z carries for
#              a perturbed mean and variance) and the accumulator's own error ((D + 2) u + u_T + u_ll) sum |x| |w| times rs_hi.
#   The leading 2 is norm_cases' (products of first-order terms, 1-ulp divides); + u_T |y_t| + tiny for out_t.
S_PROD = 7
NPARTS = (1, 4, 12, 16, 17, 32)
FOLD_M = (1, 63, 65)
FOLD_N = (64, 68)
RATIOS = (0, 1, 8, 64)
EPS32 = float(_f32(1e-5))
FOLD_DEFECTS = ("partial17_dropped", "ln_dim_less_one_partial", "stats_of_next_row", "variance_unclamped", "mu_colsum_left_out",
                "rln_gamma_beta_swapped")


def _clamp_constant(D):
    """c in [128, 253] for the row (c + 1, c, c, ...): the one whose fp32 q / n - mu mu is most negative at n = D, from the arithmetic
    of gemm_load_rowstats alone (the sums of such a row are exact integers).  An exactly constant row of integers never needs the
    clamp (mu rounds to c, q / n to c c: the difference is 0), so this is the row that does: its true variance is ~ 1 / D."""
    c = torch.arange(128.0, 254.0)
    inv = _f32(1.0) / _f32(float(D))
    S, Q = c * D + 1.0, c * c * D + 2.0 * c + 1.0
    var = Q * inv - (S * inv) * (S * inv)
    return float(c[int(var.argmin())]), float(var.min())


def row_kind(m, nparts):
    """0..3: index into RATIOS; 4: the constant row; 5: the constant row with one element off by one (the clamp)."""
    return (m + nparts) % 6


@functools.lru_cache(maxsize=None)
def fold_problem(kind, nparts, M, real=False):
    """Everything the three launches read, on the host (fp32 tensors of values exact in `kind`)."""
    from types import SimpleNamespace
    D, ku = 64 * nparts, GC.k_unit(kind)
    g = torch.Generator().manual_seed(9000 + nparts * 131 + M * 7 + (1 if real else 0))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
    p = SimpleNamespace(kind=kind, nparts=nparts, M=M, D=D, K0=ku, real=real)
    rk = torch.tensor([row_kind(m, nparts) for m in range(M)])
    p.rk = rk
    off = torch.where(rk == 4, 100.0 + (torch.arange(M) % 7).float(), 2.0 * torch.tensor(RATIOS + (0, 0), dtype=F32T)[rk])
    off = torch.where(rk == 5, torch.full((M,), _clamp_constant(D)[0]), off)
    # producer: acc0[m, n] = off_m + j_n (A0 = [off_m, 1, 0 ..], W0 = [1, j_n, 0 ..]); resid: integers in [-1, 1] (constant rows: -j_n)
    p.A0 = torch.zeros(M, ku)
    p.A0[:, 0], p.A0[:, 1] = off, 1.0
    p.W0 = torch.zeros(D, ku)
    j = ri(-1, 1, (D,))
    p.W0[:, 0], p.W0[:, 1] = 1.0, j
    r = ri(-1, 1, (M, D))
    r = torch.where((rk >= 4).view(M, 1), -j.view(1, D).expand(M, D), r)
    r[:, 0] += (rk == 5).float()
    if real:
        r = r + torch.randn(M, D, generator=g)
    p.R0 = r.contiguous()
    acc0 = p.A0.double() @ p.W0.double().t()
    assert float(acc0.abs().max()) < 256 and torch.equal(acc0, acc0.round())
    p.x = acc0.float() + p.R0                                       # the launch's one fp32 addition (no bias): out_f32, bit for bit
    if not real:
        assert torch.equal(p.x, p.x.round()) and float(p.x.abs().max()) < 256 and torch.equal(p.x.to(GC.plane_dtype(kind)).float(), p.x)
        assert bool((p.x[rk == 4] == off[rk == 4].view(-1, 1)).all())
    # consumers: W' in {-1, 0, 1} [68, D] (the first N rows are used), its exact column sums, real biases; rln: K = one k-unit
    p.W1 = ri(-1, 1, (68, D))
    p.cs = p.W1.sum(1)
    assert float((p.x.abs().double() @ p.W1.abs().double().t()).max()) < 2.0 ** 24
    p.b1 = torch.randn(68, generator=g)
    p.A2, p.W2 = ri(-2, 2, (M, ku)), ri(-1, 1, (D, ku))
    p.b2 = torch.randn(D, generator=g)
    p.gamma, p.beta = 1.0 + 0.5 * torch.randn(D, generator=g), 0.5 * torch.randn(D, generator=g)
    return p


def partials_twin(x):
    """stat_out [nparts, M, 2] of x [M, 64 nparts] in the epilogue's order (fp32)."""
    M, D = x.shape

    def red(t):
        q = t.view(M, D // 64, 4, 4, 4)                            # [m, part, fragment, lane group, column]
        lane = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
        f = (lane[..., 0] + lane[..., 1]) + (lane[..., 2] + lane[..., 3])
        return ((f[..., 0] + f[..., 1]) + f[..., 2]) + f[..., 3]
    q4 = x.view(M, D // 64, 4, 4, 4)
    sq = q4 * q4
    lane_q = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
    fq = (lane_q[..., 0] + lane_q[..., 1]) + (lane_q[..., 2] + lane_q[..., 3])
    qq = ((fq[..., 0] + fq[..., 1]) + fq[..., 2]) + fq[..., 3]
    return torch.stack([red(x), qq], -1).transpose(0, 1).contiguous()


def producer_reference(x):
    """fp64 sums of the fp32 x the launch wrote -> (ref [nparts, M, 2], bound)."""
    M, D = x.shape
    q = x.double().view(M, D // 64, 64)
    s1, s2, a1 = q.sum(-1), (q * q).sum(-1), q.abs().sum(-1)
    ref = torch.stack([s1, s2], -1).transpose(0, 1).contiguous()
    bnd = torch.stack([S_PROD * U * a1, (S_PROD + 1) * U * s2], -1).transpose(0, 1).contiguous() + 1e-30
    return ref, bnd


def rowstats_twin(stats, ln_dim, defect=None):
    """gemm_load_rowstats in fp32: stats [nparts, M, 2] -> (mu [M, 1], rs [M, 1])."""
    nparts, M = stats.shape[:2]
    s, q = torch.zeros(M), torch.zeros(M)
    for i in range(nparts):
        if defect == "partial17_dropped" and i == 16:
            continue
        s, q = s + stats[i, :, 0], q + stats[i, :, 1]
    n = ln_dim - 64 if defect == "ln_dim_less_one_partial" else ln_dim
    inv = _f32(1.0) / _f32(float(n))
    mu = s * inv
    var = q * inv - mu * mu
    if defect != "variance_unclamped":
        var = var.clamp_min(0.0)
    rs = _f32(1.0) / torch.sqrt(var + _f32(1e-5))
    if defect == "stats_of_next_row":
        nxt = (torch.arange(M) + 1).clamp_max(M - 1)
        mu, rs = mu[nxt], rs[nxt]
    return mu.view(M, 1), rs.view(M, 1)


def rowstats64(stats, ln_dim, dS=None, dQ=None):
    """fp64 statistics of the partials as read, with their error terms: dict of [M, 1] tensors."""
    st = stats.double()
    nparts = st.shape[0]
    n = float(ln_dim)
    S, Q, A = st[..., 0].sum(0), st[..., 1].sum(0), st[..., 0].abs().sum(0)
    mu, E2 = S / n, Q / n
    var = (E2 - mu * mu).clamp_min(0.0)
    rs = 1.0 / torch.sqrt(var + EPS32)
    dmu = (nparts + 1.0) * U * A / n + (dS / n if dS is not None else 0.0)
    dvar = (nparts + 1.0) * U * E2 + (dQ / n if dQ is not None else 0.0) + 2.0 * mu.abs() * dmu + U * mu * mu + U * var
    rs_hi = 1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + EPS32)
    rs_lo = 1.0 / torch.sqrt(var + dvar + EPS32)
    drs = torch.maximum(rs_hi - rs, rs - rs_lo) + 3.0 * U * rs_hi
    v = lambda t: t.view(-1, 1)  # noqa: E731
    return dict(mu=v(mu), rs=v(rs), dmu=v(dmu), rs_hi=v(rs_hi), drs=v(drs), var=v(var), E2=v(E2))


def colsum_reference(kind, out, p, N, stats, x=None, chain=False):
    """(ref, bound) [M, N] of the ln_colsum consumer reading `stats` (as read) and the operand copy of x."""
    xx = (p.x if x is None else x).double()
    W, cs, b = p.W1[:N].double(), p.cs[:N].double().view(1, N), p.b1[:N].double().view(1, N)
    acc = xx @ W.t()
    acc_err = 0.0
    if chain:
        a1, a2 = xx.abs().view(p.M, p.nparts, 64).sum(-1), (xx * xx).view(p.M, p.nparts, 64).sum(-1)
        s = rowstats64(stats, p.D, dS=(S_PROD * U * a1).sum(1), dQ=((S_PROD + 1) * U * a2).sum(1))
        st = NC.stats64(xx, 1, EPS32)
        s["mu"], s["rs"] = st.mean, st.r                           # the reference's statistics: of x itself
        acc_err = ((p.D + 2.0) * U + _U[kind][0] + _U[kind][1]) * (xx.abs() @ W.abs().t())
    else:
        s = rowstats64(stats, p.D)
    c = acc - s["mu"] * cs
    ref = s["rs"] * c + b
    bnd = 2.0 * (s["rs_hi"] * (U * (s["mu"] * cs).abs() + 2.0 * U * c.abs() + s["dmu"] * cs.abs() + acc_err) + c.abs() * s["drs"] + U * ref.abs())
    return finish(kind, out, bnd + 1e-30, ref)


def colsum_twin(kind, p, N, stats, defect=None):
    mu, rs = rowstats_twin(stats, p.D, defect)
    acc = (p.x.double() @ p.W1[:N].double().t()).float()           # exact
    v = acc if defect == "mu_colsum_left_out" else acc - mu * p.cs[:N].view(1, N)
    y = v * rs + p.b1[:N].view(1, N)
    return {"f32": y, "t": store_twin(kind, y)}


def rln_reference(kind, out, p, stats):
    s = rowstats64(stats, p.D)
    acc = p.A2.double() @ p.W2.double().t() + p.b2.double().view(1, -1)
    g, b = p.gamma.double().view(1, -1), p.beta.double().view(1, -1)
    c = p.x.double() - s["mu"]
    t = c * s["rs"] * g + b
    ref = acc + t
    bnd = 2.0 * (g.abs() * (s["rs_hi"] * (s["dmu"] + 3.0 * U * c.abs()) + c.abs() * s["drs"]) + U * t.abs() + U * acc.abs() + U * ref.abs())
    return finish(kind, out, bnd + 1e-30, ref)


def rln_twin(kind, p, stats, defect=None):
    mu, rs = rowstats_twin(stats, p.D, defect)
    v = (p.A2.double() @ p.W2.double().t()).float() + p.b2.view(1, -1)
    g, b = (p.beta, p.gamma) if defect == "rln_gamma_beta_swapped" else (p.gamma, p.beta)
    y = v + ((p.x - mu) * rs * g.view(1, -1) + b.view(1, -1))
    return {"f32": y, "t": store_twin(kind, y)}
