"""The kernels that compute a mean and a variance (csrc/elementwise.hpp: ln_row_kernel, conv0_kernel / conv0_ln_gelu_kernel,
leaky_instnorm[_lens]_kernel, time_groupnorm_kernel with its chunked pair and their _lens forms, adain_kernel): fp64 references of
exactly what each kernel reads, a per-element error bound counted from the kernel's arithmetic, seeded value builders, a CPU twin of
each kernel (fp32 torch in the kernel's summation order, with a defect= switch) and the case lists shared by
tests/test_norm_edges_cpu.py and tests/test_norm_edges_gpu.py.  Plain helper module (pytest does not collect it), host only.

The bound
---------
u = 2^-24.  A row x_1..x_n (after its addends) is normalised: mean, c_i = x_i - mean, var = sum c_i^2 / div, r = 1 / sqrt(var + eps),
z_i = c_i r, y_i = g_i z_i + b_i.  a1 = mean_i |x_i|.  The library is compiled with -ffp-contract=off: every * and + rounds.

  mean     n values pass through s fp32 additions (s per kernel below) and one multiplication by 1/n (or division by n):
           |mean^ - mean| <= (s + 1) u a1 =: dm.  The error is common to every c_i: the conditioning term, r dm per element.
  c_i      one subtraction: u |c_i| (+ dm).
  var      squares (1 rounding each) through s additions, one scaling, + eps: (s + 3) u relative, + 2u from the c_i it was formed
           from, + n dm^2 / (div (var + eps)) from the shift of every c_i by dm (second order, but it grows with a1^2).
  r        half of that, + sqrtf + the reciprocal (1 rounding each: -fhip-fp32-correctly-rounded-divide-sqrt is the default):
           (s + 9) / 2 u + (n / div) dm^2 / (2 (var + eps)).
  z_i      c_i (u) * r (one product): relative (s + 13) / 2 u                                  [the (s + 13) / 2 of the issue]
  y_i      * g_i and + b_i: u |g_i z_i| + u |y_i| <= covered by the 2u |y_i| term and the leading factor 2 (see below)

    E_z,i = r (s + 1) u a1 + |c_i| r [ (s + 13) / 2 u + (n / div) dm^2 / (2 (var + eps)) ]
    |y_gpu - y_ref|_i <= 2 [ |g_i| (E_z,i + P_z,i) + 2u |y_i| ] + u_T |y_i| + tiny

  The leading 2 pays for what a first-order count leaves out: products of the terms above, the g_i product's own rounding
  (u |g_i z_i| <= |g_i| |c_i| r u, a thirteenth of the bracket at the smallest s), and a 1-ulp rather than half-ulp sqrtf / divide.
  A clean kernel sits at 0.05 - 0.3 of the bound; nothing in it is fitted to what a kernel returns.

  P_z: a perturbation delta of the row (roundings of the sums that FORM the row, or a whole earlier stage's error) enters at first
  order as   P_z,i = r ( |delta_i| + mean|delta| + |c_i| r rms(delta) )     (through c_i, through the mean, through r).

  s, from the loops:
    ln_row_kernel           3 in-thread ((v0 + v1) + (v2 + v3): 2 levels, counted as 3 additions a value can meet with its slot sum),
                            6 in wave_sum (4 DPP steps + (r0 + r1) + (r2 + r3)), NV in the fixed-order sum of red[slot][w]: 9 + NV
    conv0_ln_gelu_kernel    7 in-thread (8 channels) + 6 (wave_sum): 13
    leaky_instnorm*, time_groupnorm* (three-pass)   ceil(L / 16) in the time-lane's strided loop + 16 over red[i][cl]
    adain_kernel            ceil(L / 64) + 6
  row-forming roundings (delta_i = count * u * A_i, A_i = sum of the |terms| of element i):
    ln_row_kernel           x_planes - 1 plane additions; e = em + et (1, when both are given); v += e (1)
    leaky kernels           0.2f * x for x < 0: u |x_i| / 5, and 0.2f itself is 0.2 (1 + 2^-26): together <= 1.25 u |leaky(x_i)|
    conv0 kernels           ten fmaf and + bias: gamma_11 (sum_k |w_k x_k| + |bias|), gamma_11 = 11u / (1 - 11u)
  two stages (gamma2): the first stage's bound (without u_T, without activation) + 2 roundings of h + e is the delta of the second.
  AdaIN: out = z_c * ss + sm, z_c = (c - cm) / cs (content half: E_z with g = 1, unbiased div = Lc - 1),
    ss = sqrt(var_s + eps): relative (s_s + 7) / 2 u + (Ls / (Ls - 1)) dm_s^2 / (2 (var_s + eps)); sm: dm_s = (s_s + 1) u a1_s:
    |out_gpu - out_ref|_i <= 2 [ ss E_z,i + |z_i| ss * rel(ss) + dm_s + 2u (|z_i ss| + |out_i|) ]
  chunked group norm (time_stats_kernel + time_norm_apply_kernel): one-pass sums in fp64 over s64 = ceil(chunk / 16) + 16 + nch
    additions (+ the product), mean and r rounded to fp32 once; U = 2^-53:
    dm = u |mean| + (s64 + 1) U a1;   rel(r) = u + (s64 + 4) U (E[x^2] + eps) / (var + eps)   [q / T - mean^2 cancels in fp64]
    |y_gpu - y_ref|_i <= 2 [ |g_i| ( r dm + |c_i| r (2u + rel(r)) ) + 2u |y_i| ] + u_T |y_i| + tiny
  activations: RELU and LEAKY are 1-Lipschitz and exact; GELU(erf) is L-Lipschitz with L = 1.13 (max |GELU'| = 1.1289) and
    act_apply's 0.5f * v * (1.f + erff(v * c)) errs by <= 6u |v| + 2u |GELU(v)| (erff within 4 ulp, the argument's rounding
    through z erf'(z) <= 0.49, the 1 + erf rounding; two products).  The bf16 and fp16 kinds evaluate gelu_erf_fast
    (csrc/common.hpp: Abramowitz-Stegun 7.1.26 on the hardware exp): its FORMULA error is the one number here that is measured,
    not counted: GELU_FAST_FORMULA_ERR = max over GELU_FAST_GRID of |formula in fp64 - GELU|, recorded below and re-measured by
    the CPU test; its fp32 evaluation adds <= 12u |v| (five Horner steps, the reciprocal, __expf within 2 ulp of a value <= 1,
    all on numbers <= 1.5: 24u on erf) + 2u |GELU(v)|.
  u_T (0 for y_f32) and the subnormal floors `tiny` are those of tests/attn_cases.py: fp32 2^-24, bf16 2^-8, fp16 2^-11,
    split 2^-21; tiny = 2^-25 (fp16), 2^-36 (split), 1e-30 otherwise.
"""
from collections import namedtuple

import torch

from attn_cases import _TINY, _U, KIND_NAMES, KINDS, SPLIT_SCALE, split_host
from fdm_amd._lib import ACT_GELU_ERF, ACT_NONE, ACT_RELU, BF16, F16, F16X3, F32

U = 2.0 ** -24
U64 = 2.0 ** -53
EPS = 1e-5
GELU_LIP = 1.13
# measured by gelu_fast_formula_error(): the maximum over GELU_FAST_GRID = 16 * 2^16 + 1 equally spaced points of [-8, 8] of
# |gelu_erf_fast's formula evaluated in fp64 - 0.5 v (1 + erf(v / sqrt 2))|; the CPU test re-measures it.
GELU_FAST_GRID = (-8.0, 8.0, 16 * 65536 + 1)
GELU_FAST_FORMULA_ERR = 2.12e-7
F64, F32T = torch.float64, torch.float32


def u_out(kind, out):
    """Unit roundoff of the output: out = 'f32' (y_f32: none) or 't' (y_t of `kind`)."""
    return 0.0 if out == "f32" else _U[kind][0]


def tiny_out(kind, out):
    return 1e-30 if out == "f32" or _TINY[kind] is None else _TINY[kind]


def round_kind(kind, y):
    """fp32 -> the fp32 value of what a y_t of `kind` holds (the rounding of store_opnd* / from_f32 in csrc/common.hpp: round to
    nearest even; fp16 planes clamp at +-65504; split = hi + lo / 2^11)."""
    if kind == BF16:
        return y.bfloat16().float()
    if kind == F16:
        return y.clamp(-65504.0, 65504.0).half().float()
    if kind == F16X3:
        p = split_host(y)
        return p[0].float() + p[1].float() / SPLIT_SCALE
    return y


def fast_gelu_kind(kind):
    return kind in (BF16, F16)


# ---------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------
def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))


def gelu_fast_formula(v):
    """gelu_erf_fast of csrc/common.hpp restated in the dtype of v (fp64: the formula error; fp32: the twin)."""
    x = v.abs() * 0.70710678118654752440
    t = 1.0 / (1.0 + 0.3275911 * x)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    e = 1.0 - poly * torch.exp(-x * x)
    return 0.5 * v * (1.0 + torch.where(v < 0, -e, e))


def gelu_fast_formula_error():
    v = torch.linspace(*GELU_FAST_GRID, dtype=F64)
    return float((gelu_fast_formula(v) - gelu64(v)).abs().max())


def act64(y, act):
    if act == ACT_RELU:
        return y.clamp_min(0.0)
    if act == ACT_GELU_ERF:
        return gelu64(y)
    return y


def act_bound(kind, y_pre, e_pre, act):
    """Bound after the activation: Lipschitz constant * bound before it + the activation's own evaluation error."""
    if act != ACT_GELU_ERF:
        return e_pre
    ya = gelu64(y_pre)
    if fast_gelu_kind(kind):
        return GELU_LIP * e_pre + GELU_FAST_FORMULA_ERR + 12.0 * U * y_pre.abs() + 2.0 * U * ya.abs()
    return GELU_LIP * e_pre + 6.0 * U * y_pre.abs() + 2.0 * U * ya.abs()


def act32(kind, y, act):
    """The twin's activation (fp32)."""
    if act == ACT_RELU:
        return y.clamp_min(0.0)
    if act == ACT_GELU_ERF:
        if fast_gelu_kind(kind):
            return gelu_fast_formula(y)
        return 0.5 * y * (1.0 + torch.erf(y * 0.70710678118654752440))
    return y


# ---------------------------------------------------------------------------------------------------------------------
# the statistics of a row, its bound terms
# ---------------------------------------------------------------------------------------------------------------------
Stat = namedtuple("Stat", "mean c var r z a1 n div")


def stats64(x, dim, eps, unbiased=False):
    """fp64 statistics of x over `dim` (kept)."""
    x = x.double()
    n = x.shape[dim]
    div = n - 1 if unbiased else n
    m0 = x.sum(dim, keepdim=True) / n
    c0 = x - m0
    corr = c0.sum(dim, keepdim=True) / n          # the mean in two steps: exact to fp64 rounding of c, whatever the offset
    mean, c = m0 + corr, c0 - corr
    var = (c * c).sum(dim, keepdim=True) / div
    r = 1.0 / torch.sqrt(var + eps)
    return Stat(mean, c, var, r, c * r, x.abs().mean(dim, keepdim=True), n, div)


def e_z(st, s, eps):
    """E_z of the module docstring (no leading 2)."""
    dm = (s + 1.0) * U * st.a1
    second = (st.n / st.div) * dm * dm / (2.0 * (st.var + eps))
    return st.r * dm + st.c.abs() * st.r * ((s + 13.0) / 2.0 * U + second)


def p_z(st, delta, dim):
    """P_z: first-order effect on z of a perturbation |delta| of the row."""
    rms = torch.sqrt((delta * delta).mean(dim, keepdim=True))
    return st.r * (delta + delta.mean(dim, keepdim=True) + st.c.abs() * st.r * rms)


def finish(kind, out, y_pre, e_pre, act):
    """-> (y_ref, bound) after the activation and the output rounding."""
    y = act64(y_pre, act)
    return y, act_bound(kind, y_pre, e_pre, act) + u_out(kind, out) * y.abs() + tiny_out(kind, out)


def worst(got, ref, bnd):
    """(ratio, index, error, bound) of the element with the largest |got - ref| / bound; a non-finite value counts as infinite."""
    err = (got.double() - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / bnd, torch.full_like(err, float("inf")))
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    return float(ratio.reshape(-1)[flat]), idx, float(err.reshape(-1)[flat]), float(bnd.reshape(-1)[flat])


# ---------------------------------------------------------------------------------------------------------------------
# value builders: [R rows, n values to reduce over] fp32, seeded; `slices` [n] names the partial sum each position belongs to
# (LayerNorm: the wave, col // 256; time kernels: the time-lane, l % 16; AdaIN: the lane, i % 64)
# ---------------------------------------------------------------------------------------------------------------------
def _gen(name, R, n, seed):
    return torch.Generator().manual_seed(seed * 1000003 + (sum(map(ord, name)) * 1009 + R) * 65537 + n)


def build(name, R, n, slices=None, seed=0):
    g = _gen(name, R, n, seed)
    z = torch.randn(R, n, generator=g)
    row = torch.arange(R, dtype=F32T).view(R, 1)
    if name == "centred":
        return z
    if name == "offset100":                       # mean = 100 * std
        return 100.0 + z
    if name == "offset1000":
        return 1000.0 + z
    if name == "tiny":                            # std 1e-4: var 1e-8, far below eps
        return 1e-4 * z
    if name == "constant":                        # variance exactly 0 (a different value per row)
        return (3.7 - 1.3 * row).expand(R, n).contiguous()
    if name == "outlier":
        z[:, 7 % n] = 1e4
        return z
    if name == "wave_skew":                       # each partial sum has its own mean and scale
        sl = slices if slices is not None else torch.zeros(n, dtype=torch.long)
        mean = 10.0 * (sl + 1).float() * torch.where(sl % 2 == 0, 1.0, -1.0)
        scale = 2.0 ** ((sl % 5).float() - 2.0)
        return mean.view(1, n) + scale.view(1, n) * z
    if name == "row_scales":                      # 1e-3, 1, 1e3 in one launch
        return z * (10.0 ** (3.0 * ((row + 1) % 3 - 1)))
    if name == "negative_heavy":                  # nine values in ten below zero
        return z - 1.3
    raise ValueError(name)


BUILDERS = ["centred", "offset100", "offset1000", "tiny", "constant", "outlier", "wave_skew", "row_scales", "negative_heavy"]


def _affine(d, seed):
    g = torch.Generator().manual_seed(77 + seed * 131 + d)
    return 1.0 + 0.5 * torch.randn(d, generator=g), 0.5 * torch.randn(d, generator=g)


def time_major(rows, B, d):
    """[B * d, L] builder rows -> the kernels' channels-last [B, L, d]."""
    return rows.view(B, d, -1).transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
LN_FORMS = ["plain", "addends", "shared", "two", "two_add", "planes2", "planes3", "planes4", "clip"]
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_GELU_ERF: "gelu"}


class LnCase(namedtuple("LnCase", "builder M d form act")):
    @property
    def id(self):
        return f"{self.builder}-{self.M}x{self.d}-{self.form}-{ACT_NAMES[self.act]}"

    @property
    def planes(self):
        return int(self.form[6:]) if self.form.startswith("planes") else 0

    @property
    def plane_stride(self):
        return self.M * self.d + 64               # above M * d, a multiple of 4

    def inputs(self):
        """dict of CPU tensors / ints: what ops.layernorm takes (tensors fp32 / int32)."""
        M, d = self.M, self.d
        sl = torch.arange(d) // 256
        npl = max(self.planes, 1)
        x = torch.stack([build(self.builder, M, d, sl, seed=p) for p in range(npl)])      # [npl, M, d]
        if npl > 1:                                # partial planes: the first carries the offset, the others are O(1) partials
            x[1:] = torch.stack([build("centred", M, d, sl, seed=10 + p) for p in range(1, npl)])
        inp = {"x": x, "eps": EPS}
        inp["gamma"], inp["beta"] = _affine(d, 1)
        g = _gen("ln" + self.form, M, d, 3)
        if self.form in ("addends", "two_add", "clip"):
            inp["add_tab"] = 2.0 * torch.randn(7, d, generator=g) + 1.0
            inp["tab_index"] = torch.tensor([3, 5, 0, 6, 2, 1, 4, 3, 0, 6], dtype=torch.int32)        # tab_index[k] != k
        if self.form in ("addends", "two_add"):
            inp["add_mat"] = 3.0 * torch.randn(M, d, generator=g) - 2.0
            inp["tab_step"] = torch.tensor([4], dtype=torch.int32)
        if self.form == "shared":                  # rows m share add_mat rows (m' / group) * L + m' % L, m' = m % wrap
            inp.update(add_mat_L=3, add_mat_group=6, add_mat_wrap=12)
            inp["add_mat"] = 3.0 * torch.randn(6, d, generator=g) - 2.0
        if self.form == "clip":                    # the table row of clip (m % wrap) / rows: clip_step[clip * stride]
            inp.update(clip_rows=2, clip_wrap=6, clip_step_stride=2)
            inp["clip_step"] = torch.tensor([4, 0, 9, 0, 1, 0], dtype=torch.int32)      # (odd words: a stride of 1 would take row tab_index[0])
        if self.form in ("two", "two_add"):
            inp["gamma2"], inp["beta2"] = _affine(d, 2)
        return inp


def ln_addend_rows(case, inp, defect=None):
    """(add_mat row per output row or None, add_tab row per output row or None)."""
    M = case.M
    m = torch.arange(M)
    amat = atab = None
    if "add_mat" in inp:
        if case.form == "shared":
            L, grp, wrap = inp["add_mat_L"], inp["add_mat_group"], inp["add_mat_wrap"]
            mm = m % wrap
            amat = (mm // grp) * L + (mm % grp if defect == "addend_row_mod_group" else mm % L)
            amat = amat % inp["add_mat"].shape[0]
        else:
            amat = m
    if "add_tab" in inp:
        if case.form == "clip":
            k = inp["clip_step"][((m % inp["clip_wrap"]) // inp["clip_rows"]) * inp["clip_step_stride"]].long()
        else:
            k = inp["tab_step"].long().expand(M)
        atab = (k if defect == "table_row_k" else inp["tab_index"].long()[k]) % inp["add_tab"].shape[0]
    return amat, atab


def _ln_row_terms(case, inp, dtype):
    amat, atab = ln_addend_rows(case, inp)
    em = inp["add_mat"].to(dtype)[amat] if amat is not None else None
    et = inp["add_tab"].to(dtype)[atab] if atab is not None else None
    return em, et


def ln_reference(kind, out, case, inp):
    """(y_ref, bound) [M, d] fp64 for output `out` ('f32' | 't') of `kind`."""
    d = case.d
    s = 9 + d // 256
    x = inp["x"].double()
    em, et = _ln_row_terms(case, inp, F64)
    e = (em if em is not None else 0.0) + (et if et is not None else 0.0)
    has_e = em is not None or et is not None
    n_e = (1 if (em is not None and et is not None) else 0) + (1 if has_e else 0)
    A_e = (em.abs() if em is not None else 0.0) + (et.abs() if et is not None else 0.0)
    two = "gamma2" in inp
    g1, b1 = inp["gamma"].double(), inp["beta"].double()
    row = x.sum(0)
    A = x.abs().sum(0)
    nr = x.shape[0] - 1
    if not two and has_e:
        row, A, nr = row + e, A + A_e, nr + n_e
    st = stats64(row, 1, inp["eps"])
    y = g1 * st.z + b1
    err = 2.0 * (g1.abs() * (e_z(st, s, inp["eps"]) + p_z(st, nr * U * A, 1)) + 2.0 * U * y.abs())
    if two:
        g2, b2 = inp["gamma2"].double(), inp["beta2"].double()
        row2 = y + e if has_e else y
        delta = err + (n_e * U * (y.abs() + A_e) if has_e else 0.0)
        st = stats64(row2, 1, inp["eps"])
        y = g2 * st.z + b2
        err = 2.0 * (g2.abs() * (e_z(st, s, inp["eps"]) + p_z(st, delta, 1)) + 2.0 * U * y.abs())
    return finish(kind, out, y, err, case.act)


def wave_sum32(v):
    """wave_sum of csrc/common.hpp on [..., 64]: four DPP steps (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror),
    then (r0 + r1) + (r2 + r3) of lanes 0, 16, 32, 48."""
    lane = torch.arange(64)
    for perm in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
        v = v + v[..., perm]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def _ln_block_sum(t, NV, defect):
    """t [M, d] -> [M, 1]: (t0 + t1) + (t2 + t3) per thread, wave_sum, the NV slots in order."""
    M = t.shape[0]
    q = t.view(M, NV, 64, 4)
    w = wave_sum32((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))      # [M, NV]
    tot = torch.zeros(M)
    for i in range(NV):
        if defect == "third_wave_dropped" and i == 2:
            continue
        tot = tot + w[:, i]
    return tot.view(M, 1)


def _ln_stage32(v, g, b, NV, eps, defect):
    d = 256 * NV
    inv_d = torch.tensor(1.0 / d, dtype=F32T)
    if defect == "one_pass_var":
        mean = _ln_block_sum(v, NV, defect) * inv_d
        var = _ln_block_sum(v * v, NV, defect) * inv_d - mean * mean
        v = v - mean
    else:
        mean = _ln_block_sum(v, NV, defect) * inv_d
        v = v - mean
        var = _ln_block_sum(v * v, NV, defect) * inv_d
    eps = torch.tensor(eps, dtype=F32T)
    if defect == "eps_left_out":
        rstd = 1.0 / torch.sqrt(var)
    elif defect == "eps_outside_sqrt":
        rstd = 1.0 / (torch.sqrt(var) + eps)
    else:
        rstd = 1.0 / torch.sqrt(var + eps)
    return v * rstd * g + b


def ln_twin(kind, case, inp, defect=None):
    """ln_row_kernel in fp32 torch -> the fp32 y before the output rounding (y_f32); round_kind(kind, .) is y_t."""
    NV = case.d // 256
    x = inp["x"]
    amat, atab = ln_addend_rows(case, inp, defect)
    em = inp["add_mat"][amat] if amat is not None else None
    et = inp["add_tab"][atab] if atab is not None else None
    has_e = em is not None or et is not None
    e = (em + et) if (em is not None and et is not None) else (em if em is not None else et)
    v = x[0]
    for p in range(1, x.shape[0]):
        v = v + x[p]
    two = "gamma2" in inp
    if has_e and (not two or defect == "addend_before_stage1"):
        v = v + e
    v = _ln_stage32(v, inp["gamma"], inp["beta"], NV, inp["eps"], defect)
    if two:
        if has_e and defect != "addend_before_stage1":
            v = v + e
        v = _ln_stage32(v, inp["gamma2"], inp["beta2"], NV, inp["eps"], defect)
    return act32(kind, v, case.act)


def _ln_cases():
    cs = [LnCase(b, M, d, "plain", ACT_NONE) for d in (256, 512, 768, 1024) for M in (1, 5) for b in BUILDERS]
    N, R, G = ACT_NONE, ACT_RELU, ACT_GELU_ERF
    cs += [LnCase("offset100", 5, 256, "addends", N), LnCase("centred", 5, 768, "addends", G), LnCase("row_scales", 5, 1024, "addends", R),
           LnCase("centred", 24, 256, "shared", N), LnCase("offset100", 24, 768, "shared", N), LnCase("wave_skew", 24, 512, "shared", R),
           LnCase("centred", 5, 512, "two", N), LnCase("offset100", 5, 1024, "two", G), LnCase("wave_skew", 5, 768, "two", R),
           LnCase("centred", 5, 256, "two_add", N), LnCase("offset100", 5, 768, "two_add", G), LnCase("outlier", 1, 1024, "two_add", N),
           LnCase("centred", 5, 256, "planes2", N), LnCase("offset100", 5, 768, "planes3", N), LnCase("wave_skew", 5, 1024, "planes4", G),
           LnCase("centred", 1, 512, "planes3", R),
           LnCase("centred", 12, 256, "clip", N), LnCase("offset100", 12, 768, "clip", R), LnCase("tiny", 12, 1024, "clip", N),
           LnCase("centred", 5, 768, "plain", G), LnCase("wave_skew", 5, 768, "plain", R), LnCase("negative_heavy", 5, 256, "plain", G),
           LnCase("offset1000", 5, 512, "plain", G), LnCase("row_scales", 5, 1024, "plain", R), LnCase("tiny", 1, 768, "plain", G)]
    return cs


LN_CASES = _ln_cases()


# ---------------------------------------------------------------------------------------------------------------------
# conv0 (Conv1d(1, 512, k = 10, stride 5) + bias), alone and followed by LayerNorm(512) + GELU(erf)
# ---------------------------------------------------------------------------------------------------------------------
class ConvCase(namedtuple("ConvCase", "T0 extra bias")):
    B = 2

    @property
    def n(self):
        return 5 * (self.T0 - 1) + 10 + self.extra

    @property
    def id(self):
        return f"T{self.T0}-n{self.n}-{'bias' if self.bias else 'nobias'}"

    def inputs(self):
        g = _gen("conv", self.T0, self.n, 5)
        inp = {"wav": torch.randn(self.B, self.n, generator=g) + 0.5,
               "w": 1.0 + 0.05 * torch.randn(512, 10, generator=g),                 # all near +1: the pre-norm row has a large mean
               "bias": 0.5 * torch.randn(512, generator=g) if self.bias else None, "eps": EPS}
        inp["gamma"], inp["beta"] = _affine(512, 4)
        return inp


CONV_CASES = [ConvCase(T0, extra, bias) for T0 in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33)
              for (extra, bias) in (((0, True), (4, False)) if T0 % 2 else ((4, True), (0, False)))]
GAMMA11 = 11.0 * U / (1.0 - 11.0 * U)


def conv_reference(case, inp, stride=5):
    """fp64 conv rows [B, T0, 512] and delta = gamma_11 (sum |w_k x_k| + |bias|)."""
    wav, w = inp["wav"].double(), inp["w"].double()
    fr = wav.unfold(1, 10, stride)[:, :case.T0]                                       # [B, T0, 10]
    y = torch.einsum("btk,ck->btc", fr, w)
    a = torch.einsum("btk,ck->btc", fr.abs(), w.abs())
    if inp["bias"] is not None:
        y, a = y + inp["bias"].double(), a + inp["bias"].double().abs()
    return y, GAMMA11 * a


def conv0_reference(case, inp):
    y, delta = conv_reference(case, inp)
    return y, delta + 1e-30


def conv_ln_reference(kind, case, inp):
    """conv0_ln_gelu writes one output of `kind`: fp32 kind -> a plain fp32 store (out = 'f32'), else y_t."""
    row, delta = conv_reference(case, inp)
    g, b = inp["gamma"].double(), inp["beta"].double()
    st = stats64(row, 2, inp["eps"])
    y = g * st.z + b
    err = 2.0 * (g.abs() * (e_z(st, 13, inp["eps"]) + p_z(st, delta, 2)) + 2.0 * U * y.abs())
    return finish(kind, "f32" if kind == F32 else "t", y, err, ACT_GELU_ERF)


def conv_twin(case, inp, defect=None):
    """conv0_kernel / the conv of conv0_ln_gelu_kernel: a = w_k x_k + a for k = 0..9 (fmaf has no fp32 torch form: the product
    rounds here, inside gamma_11), + bias."""
    stride = 4 if defect == "conv_stride_4" else 5
    fr = inp["wav"].unfold(1, 10, stride)[:, :case.T0]
    a = torch.zeros(case.B, fr.shape[1], 512)
    for k in range(10):
        a = fr[:, :, k:k + 1] * inp["w"][:, k].view(1, 1, 512) + a
    return a + inp["bias"] if inp["bias"] is not None else a


def conv_ln_twin(kind, case, inp, defect=None):
    v = conv_twin(case, inp, defect)                                                  # [B, T0, 512]: lane = c // 8 owns 8 channels
    B, T0 = v.shape[:2]

    def wsum(t):
        q = t.view(B, T0, 64, 8)
        if t is v:
            s = ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) + ((q[..., 4] + q[..., 5]) + (q[..., 6] + q[..., 7]))
        else:
            s = torch.zeros(B, T0, 64)
            for c in range(8):
                s = s + q[..., c]
        return wave_sum32(s).unsqueeze(-1)
    inv = torch.tensor(1.0 / 512.0, dtype=F32T)
    eps = torch.tensor(inp["eps"], dtype=F32T)
    mean = wsum(v) * inv
    if defect == "one_pass_var":
        var = wsum(v * v) * inv - mean * mean
        c = v - mean
    else:
        c = v - mean
        var = wsum(c * c) * inv
    rstd = 1.0 / torch.sqrt(var + eps)
    return act32(kind, c * rstd * inp["gamma"] + inp["beta"], ACT_GELU_ERF)


# ---------------------------------------------------------------------------------------------------------------------
# the time kernels: LeakyReLU(0.2) + instance norm, GroupNorm(groups = C) over time
# ---------------------------------------------------------------------------------------------------------------------
def lanes_sum32(t):
    """Sum over time of t [B, L, d] as the kernels do: time-lane tl takes l = tl, tl + 16, .. in order, the 16 lanes fold in order."""
    B, L, d = t.shape
    n = (L + 15) // 16
    pad = torch.zeros(B, n * 16, d, dtype=t.dtype)
    pad[:, :L] = t
    q = pad.view(B, n, 16, d)
    s = torch.zeros(B, 16, d, dtype=t.dtype)
    for i in range(n):
        s = s + q[:, i]
    tot = torch.zeros(B, d, dtype=t.dtype)
    for i in range(16):
        tot = tot + s[:, i]
    return tot.view(B, 1, d)


def time_norm_terms(x64, L, s, eps, delta=None):
    """stats over dim 1 of [B, L, d] -> (st, E_z + P_z)."""
    st = stats64(x64, 1, eps)
    e = e_z(st, s, eps)
    if delta is not None:
        e = e + p_z(st, delta, 1)
    return st, e


def s_time(L):
    return (L + 15) // 16 + 16


def _with_lens(fn, x, lens):
    """The _lens reference: the solo reference over the first lens[b] frames, zeros (and a zero bound) after."""
    B, L = x.shape[:2]
    y = torch.zeros(x.shape, dtype=F64)
    bnd = torch.full(x.shape, 1e-30, dtype=F64)
    for b in range(B):
        Lb = min(max(int(lens[b]), 1), L)
        y[b, :Lb], bnd[b, :Lb] = (t[0] for t in fn(x[b:b + 1, :Lb]))
    return y, bnd


class InCase(namedtuple("InCase", "builder L d lens")):
    B = 2

    @property
    def id(self):
        return f"{self.builder}-{self.L}x{self.d}" + ("-lens" + "_".join(map(str, self.lens)) if self.lens else "")

    @property
    def nb(self):
        return len(self.lens) if self.lens else self.B

    def inputs(self):
        B = self.nb
        return {"x": time_major(build(self.builder, B * self.d, self.L, torch.arange(self.L) % 16, seed=6), B, self.d), "eps": EPS}


def leaky64(x):
    return torch.where(x > 0, x, 0.2 * x)


def instnorm_reference(kind, out, case, inp):
    def solo(x):
        a = leaky64(x.double())
        st, e = time_norm_terms(a, x.shape[1], s_time(x.shape[1]), inp["eps"], 1.25 * U * a.abs())
        return finish(kind, out, st.z, 2.0 * (e + 2.0 * U * st.z.abs()), ACT_NONE)
    return _with_lens(solo, inp["x"], case.lens) if case.lens else solo(inp["x"])


def instnorm_twin(case, inp, defect=None):
    x = inp["x"]
    B, L, d = x.shape
    out = torch.zeros(B, L, d)
    slope = torch.tensor(0.2, dtype=F32T)
    eps = torch.tensor(inp["eps"], dtype=F32T)
    for b in range(B):
        Lb = min(max(case.lens[b], 1), L) if case.lens else L
        xb = x[b:b + 1, :Lb]
        a = xb if defect in ("leaky_skipped", "leaky_after_norm") else torch.where(xb > 0, xb, slope * xb)
        Ldiv = float(L if defect == "divide_by_L" else Lb)
        mean = lanes_sum32(a) / Ldiv
        if defect == "one_pass_var":
            var = lanes_sum32(a * a) / Ldiv - mean * mean
            c = a - mean
        else:
            c = a - mean
            var = lanes_sum32(c * c) / Ldiv
        if defect == "biased_unbiased_swap":
            var = var * Ldiv / max(Ldiv - 1.0, 1.0)
        if defect == "eps_left_out":
            rstd = 1.0 / torch.sqrt(var)
        elif defect == "eps_outside_sqrt":
            rstd = 1.0 / (torch.sqrt(var) + eps)
        else:
            rstd = 1.0 / torch.sqrt(var + eps)
        y = c * rstd
        if defect == "leaky_after_norm":
            y = torch.where(y > 0, y, slope * y)
        out[b, :Lb] = y[0]
    return out


IN_CASES = ([InCase(b, L, d, None) for (b, L, d) in [
    ("centred", 1, 8), ("negative_heavy", 1, 72), ("centred", 2, 64), ("offset100", 2, 72), ("negative_heavy", 15, 8), ("wave_skew", 15, 72),
    ("centred", 16, 64), ("offset1000", 16, 8), ("wave_skew", 17, 72), ("tiny", 17, 64), ("constant", 17, 8), ("negative_heavy", 33, 72),
    ("wave_skew", 33, 64), ("offset100", 33, 8), ("outlier", 33, 72), ("row_scales", 33, 64), ("offset1000", 33, 72), ("tiny", 2, 8),
    ("constant", 1, 64), ("centred", 15, 64), ("centred", 33, 8)]]
    + [InCase(b, L, d, (1, L // 2, L)) for (b, L, d) in [("negative_heavy", 33, 72), ("wave_skew", 17, 64), ("offset100", 16, 8),
                                                          ("centred", 15, 72), ("centred", 2, 8)]])


class GnCase(namedtuple("GnCase", "builder T C scratch affine act lens")):
    """scratch: 'none' | 'full' | 'small' (too small: the entry falls back to the three-pass kernel)."""
    @property
    def id(self):
        return (f"{self.builder}-{self.T}x{self.C}-{self.scratch}-{'affine' if self.affine else 'noaffine'}-{ACT_NAMES[self.act]}"
                + ("-lens" + "_".join(map(str, self.lens)) if self.lens else ""))

    @property
    def B(self):
        return len(self.lens) if self.lens else (1 if self.T > 5000 else 2)

    @property
    def chunked(self):
        return self.scratch == "full" and self.T >= 4096

    def inputs(self):
        B = self.B
        inp = {"x": time_major(build(self.builder, B * self.C, self.T, torch.arange(self.T) % 16, seed=8), B, self.C), "eps": EPS,
               "gamma": None, "beta": None}
        if self.affine:
            g = torch.Generator().manual_seed(99 + self.C)
            inp["gamma"], inp["beta"] = 1.0 + 0.5 * torch.randn(self.C, generator=g), 0.5 * torch.randn(self.C, generator=g)
        return inp


def chunks_of(T):
    """(chunk count, chunk width) of a clip of T >= 4096 frames (fdm_op_time_groupnorm / time_chunks_of)."""
    nch = min(64, (T + 1023) // 1024)
    return nch, ((T + nch - 1) // nch + 15) // 16 * 16


def scratch_bytes(B, T, C):
    return B * chunks_of(T)[0] * C * 16 if T >= 4096 else 0


def groupnorm_reference(kind, out, case, inp, chunked=None):
    """chunked: which form's bound (None: the one the case's scratch selects; per clip for a _lens case)."""
    g = inp["gamma"].double() if inp["gamma"] is not None else torch.ones(case.C, dtype=F64)
    b = inp["beta"].double() if inp["beta"] is not None else torch.zeros(case.C, dtype=F64)
    eps = inp["eps"]

    def solo(x, ch=None):
        x = x.double()
        T = x.shape[1]
        ch = (case.chunked if chunked is None else chunked) if ch is None else ch
        st = stats64(x, 1, eps)
        y = g * st.z + b
        if ch and T >= 4096:
            nch, chunk = chunks_of(T)
            s64 = (chunk + 15) // 16 + 16 + nch
            dm = U * st.mean.abs() + (s64 + 1.0) * U64 * st.a1
            ex2 = (x * x).mean(1, keepdim=True)
            rel_r = U + (s64 + 4.0) * U64 * (ex2 + eps) / (st.var + eps)
            err = 2.0 * (g.abs() * (st.r * dm + st.c.abs() * st.r * (2.0 * U + rel_r)) + 2.0 * U * y.abs())
        else:
            err = 2.0 * (g.abs() * e_z(st, s_time(T), eps) + 2.0 * U * y.abs())
        return finish(kind, out, y, err, case.act)
    if case.lens:
        return _with_lens(lambda xb: solo(xb, xb.shape[1] >= 4096), inp["x"], case.lens)
    return solo(inp["x"])


def groupnorm_twin(kind, case, inp, defect=None):
    x = inp["x"]
    B, T, C = x.shape
    g = inp["gamma"] if inp["gamma"] is not None else torch.ones(C)
    bt = inp["beta"] if inp["beta"] is not None else torch.zeros(C)
    eps = torch.tensor(inp["eps"], dtype=F32T)
    out = torch.zeros(B, T, C)
    for b in range(B):
        Tb = min(max(case.lens[b], 1), T) if case.lens else T
        xb = x[b:b + 1, :Tb]
        Tdiv = float(T if defect == "divide_by_L" else Tb)
        if (case.lens or case.chunked) and Tb >= 4096:
            nch, chunk = chunks_of(Tb)
            ss, qq = torch.zeros(1, 1, C, dtype=F64), torch.zeros(1, 1, C, dtype=F64)
            for c in range(nch):
                t0, t1 = c * chunk, min(Tb, (c + 1) * chunk)
                if defect == "chunk_frame_twice" and c + 1 < nch:
                    t1 += 1
                if defect == "chunk_frame_dropped" and c + 1 < nch:
                    t1 -= 1
                v = xb[:, t0:t1].double()
                ss, qq = ss + lanes_sum32(v), qq + lanes_sum32(v * v)
            mean64 = ss / Tdiv
            var64 = (qq / Tdiv - mean64 * mean64).clamp_min(0.0)
            mean, rstd = mean64.float(), (1.0 / torch.sqrt(var64 + float(eps))).float()
            c_ = xb - mean
        else:
            mean = lanes_sum32(xb) / Tdiv
            if defect == "one_pass_var":
                var = lanes_sum32(xb * xb) / Tdiv - mean * mean
                c_ = xb - mean
            else:
                c_ = xb - mean
                var = lanes_sum32(c_ * c_) / Tdiv
            rstd = 1.0 / torch.sqrt(var) if defect == "eps_left_out" else 1.0 / torch.sqrt(var + eps)
        out[b, :Tb] = act32(kind, c_ * rstd * g + bt, case.act)[0]
    return out


_N, _G = ACT_NONE, ACT_GELU_ERF
GN_CASES = ([GnCase(b, T, C, "none", aff, act, None) for (b, T, C, aff, act) in [
    ("centred", 1, 8, True, _N), ("centred", 1, 96, False, _G), ("wave_skew", 15, 8, True, _G), ("offset100", 15, 96, True, _N),
    ("centred", 16, 8, False, _N), ("wave_skew", 16, 96, True, _G), ("offset1000", 17, 8, True, _N), ("constant", 17, 96, True, _N),
    ("wave_skew", 300, 8, True, _G), ("offset100", 300, 96, False, _N), ("tiny", 300, 96, True, _G), ("outlier", 300, 8, True, _N),
    ("row_scales", 300, 96, True, _N)]]
    + [GnCase(b, T, 8, "full", aff, act, None) for (b, T, aff, act) in [
        ("centred", 4095, True, _N), ("wave_skew", 4096, True, _G), ("offset100", 4096, False, _N), ("wave_skew", 4097, True, _N),
        ("offset100", 4097, True, _G), ("centred", 5000, False, _G), ("offset1000", 5000, True, _N), ("wave_skew", 65537, True, _N),
        ("offset100", 65537, True, _G)]]
    + [GnCase("wave_skew", 4096, 8, "none", True, _N, None), GnCase("offset100", 4097, 8, "none", True, _G, None),
       GnCase("wave_skew", 4097, 8, "small", True, _N, None), GnCase("offset100", 65537, 8, "small", False, _N, None),
       GnCase("wave_skew", 4097, 8, "full", True, _G, (1, 4095, 4096, 4097)), GnCase("offset100", 4097, 8, "full", False, _N, (1, 4095, 4096, 4097)),
       GnCase("centred", 300, 96, "none", True, _G, (1, 150, 300))])


# ---------------------------------------------------------------------------------------------------------------------
# AdaIN
# ---------------------------------------------------------------------------------------------------------------------
class AdaCase(namedtuple("AdaCase", "content style NC Lc Ls")):
    @property
    def id(self):
        return f"{self.content}-{self.style}-{self.NC}x{self.Lc}x{self.Ls}"

    def inputs(self):
        return {"content": build(self.content, self.NC, self.Lc, torch.arange(self.Lc) % 64, seed=11),
                "style": build(self.style, self.NC, self.Ls, torch.arange(self.Ls) % 64, seed=12) * 2.0 + 1.0, "eps": EPS}


def s_adain(L):
    return (L + 63) // 64 + 6


def adain_reference(case, inp):
    eps = inp["eps"]
    sc, ss_ = stats64(inp["content"], 1, eps, unbiased=True), stats64(inp["style"], 1, eps, unbiased=True)
    s_s = s_adain(case.Ls)
    ssd = torch.sqrt(ss_.var + eps)
    y = sc.z * ssd + ss_.mean
    dm_s = (s_s + 1.0) * U * ss_.a1
    rel_ss = (s_s + 7.0) / 2.0 * U + (ss_.n / ss_.div) * dm_s * dm_s / (2.0 * (ss_.var + eps))
    zs = (sc.z * ssd).abs()
    err = 2.0 * (ssd * e_z(sc, s_adain(case.Lc), eps) + zs * rel_ss + dm_s + 2.0 * U * (zs + y.abs()))
    return y, err + 1e-30


def _lane64_sum32(t):
    """[NC, L] -> [NC, 1]: lane i takes i, i + 64, ..; wave_sum."""
    NC, L = t.shape
    n = (L + 63) // 64
    pad = torch.zeros(NC, n * 64)
    pad[:, :L] = t
    q = pad.view(NC, n, 64)
    s = torch.zeros(NC, 64)
    for i in range(n):
        s = s + q[:, i]
    return wave_sum32(s).view(NC, 1)


def adain_twin(case, inp, defect=None):
    eps = torch.tensor(inp["eps"], dtype=F32T)

    def half(t):
        L = t.shape[1]
        m = _lane64_sum32(t) / float(L)
        e = t - m
        div = float(L if defect == "biased_unbiased_swap" else L - 1)
        if defect == "one_pass_var":
            q = (_lane64_sum32(t * t) - float(L) * m * m) / div
        else:
            q = _lane64_sum32(e * e) / div
        if defect == "eps_left_out":
            return m, e, torch.sqrt(q)
        if defect == "eps_outside_sqrt":
            return m, e, torch.sqrt(q) + eps
        return m, e, torch.sqrt(q + eps)
    cm, ce, cs = half(inp["content"])
    sm, _, ss = half(inp["content"] if defect == "style_from_content" else inp["style"])
    return ce / cs * ss + sm


_L6 = (2, 9, 63, 64, 65, 130)
ADA_CASES = ([AdaCase("centred", "centred", NC, Lc, Ls) for (NC, Lc, Ls) in [
    (1, 2, 2), (5, 2, 130), (5, 9, 63), (1, 9, 9), (5, 63, 64), (1, 63, 2), (5, 64, 65), (1, 64, 9), (5, 65, 130), (1, 65, 63), (5, 130, 2),
    (1, 130, 64), (5, 130, 130), (5, 9, 65)]]
    + [AdaCase("centred", "offset100", 5, 65, 130), AdaCase("constant", "centred", 5, 64, 9), AdaCase("constant", "offset100", 1, 130, 2),
       AdaCase("offset1000", "offset1000", 5, 130, 65), AdaCase("wave_skew", "wave_skew", 5, 130, 130), AdaCase("tiny", "row_scales", 5, 9, 63),
       AdaCase("outlier", "tiny", 1, 63, 64), AdaCase("row_scales", "outlier", 5, 2, 9)])


# ---------------------------------------------------------------------------------------------------------------------
# the defects of the CPU twins: name -> the operators it is seeded in
# ---------------------------------------------------------------------------------------------------------------------
DEFECTS = {
    "one_pass_var": ("ln", "instnorm", "groupnorm", "adain"),
    "biased_unbiased_swap": ("instnorm", "adain"),
    "eps_left_out": ("ln", "instnorm", "groupnorm", "adain"),
    "eps_outside_sqrt": ("ln", "instnorm", "adain"),
    "third_wave_dropped": ("ln",),
    "divide_by_L": ("instnorm", "groupnorm"),
    "leaky_skipped": ("instnorm",),
    "leaky_after_norm": ("instnorm",),
    "addend_row_mod_group": ("ln",),
    "table_row_k": ("ln",),
    "addend_before_stage1": ("ln",),
    "chunk_frame_twice": ("groupnorm",),
    "chunk_frame_dropped": ("groupnorm",),
    "conv_stride_4": ("conv0", "conv_ln"),
    "style_from_content": ("adain",),
}
