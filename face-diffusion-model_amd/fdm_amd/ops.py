"""Thin tensor-level wrappers over the C ABI (raw pointers + the current HIP stream).

torch is used only as the owner of device memory and of the stream; every arithmetic operation on
the product path is a libfdm_hip.so kernel.  All wrappers raise if a tensor is not a contiguous
CUDA(HIP) tensor: there is no CPU fallback."""
import ctypes as C

import torch

from . import _lib
from ._lib import (ACT_GELU_ERF, ACT_GELU_TANH, ACT_LEAKY02, ACT_MISH, ACT_NONE, ACT_RELU, BF16, F16, F16X3, F32,
                   AttnArgs, GemmArgs, LnArgs, SchedArgs, check, lib)


class Split:
    """A split-precision GEMM operand (include/fdm_hip.h, FDM_F16X3): planes[0] = hi, planes[1] = lo of a
    [rows, cols] matrix held in one [2, rows, cols] 16-bit tensor.  Slicing rows ([r0:]) keeps the plane distance."""

    def __init__(self, planes, code, row0=0, col0=0):
        self.planes, self.code, self.row0, self.col0 = planes, code, row0, col0
        self.lo_off = planes[0].numel()

    @classmethod
    def empty(cls, rows, cols, code, device):
        return cls(torch.zeros(2, rows, cols, device=device, dtype=tdtype(code)), code)

    def __getitem__(self, sl):
        if not isinstance(sl, slice) or sl.stop is not None or sl.step is not None:
            raise _lib.FdmError("Split operands support [r0:] row offsets only")
        return Split(self.planes, self.code, self.row0 + (sl.start or 0), self.col0)

    @property
    def is_cuda(self):
        return self.planes.is_cuda

    @property
    def shape(self):
        return self.planes.shape[1:]

    def data_ptr(self):
        return self.planes.data_ptr() + (self.row0 * self.planes.shape[2] + self.col0) * self.planes.element_size()

    def numel(self):
        return self.lo_off

    def float(self):
        """hi + lo / SCALE as fp32 (tests)."""
        sc = 2048.0
        return (self.planes[0].float() + self.planes[1].float() / sc)[self.row0:, self.col0:]


def cols(t, c0):
    """The matrix from column c0 on (same row stride: pass lda / ldw = the full width) -- a K range of a GEMM operand."""
    return Split(t.planes, t.code, t.row0, t.col0 + c0) if isinstance(t, Split) else t[:, c0:]


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.FdmError("fdm_amd ops need device tensors (no CPU fallback on the product path)")
    return t.data_ptr()


def _lo(t):
    return t.lo_off if isinstance(t, Split) else 0


def stream():
    return torch.cuda.current_stream().cuda_stream


def tdtype(code):
    """torch dtype of the elements of operand kind `code` (split kinds: of each plane)."""
    return {BF16: torch.bfloat16, F16X3: torch.float16, F16: torch.float16}.get(code, torch.float32)


def is_split(code):
    return code == F16X3


def code_of(t):
    if isinstance(t, Split):
        return t.code
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise _lib.FdmError(f"unsupported dtype {t.dtype}")


def gemm(A, W, M, N, K, *, lda=None, ldw=None, bias=None, act=ACT_NONE, resid=None, ldr=None, resid_row_mod=0,
         out_f32=None, ldo_f32=None, out_t=None, ldo_t=None, batch=1, a_bs=0, w_bs=0, bias_bs=0, out_bs=0,
         out_kp=None, kp_col0=0, out_vp=None, vp_col0=0, kv_L=0, kv_Lpad=0, kv_hd=0,
         stat_out=None, ln_stat_in=None, ln_nparts=0, ln_dim=0, ln_eps=1e-5, ln_colsum=None, rln_gamma=None, rln_beta=None,
         incr_counter=None, incr_table=None, tile=0, sched=None, ksplit=0, ksplit_stride=0,
         batch2=0, a_bs2=0, out_bs2=0):
    a = GemmArgs()
    a.A, a.lda, a.a_batch_stride = _p(A), lda if lda is not None else K, a_bs
    a.W, a.ldw, a.w_batch_stride = _p(W), ldw if ldw is not None else K, w_bs
    a.M, a.N, a.K, a.batch, a.dtype = M, N, K, batch, code_of(A)
    if code_of(W) != a.dtype:
        raise _lib.FdmError("gemm: A and W operand kinds differ")
    a.a_lo_off, a.w_lo_off, a.out_t_lo_off = _lo(A), _lo(W), _lo(out_t)
    a.kv_lo_off = _lo(out_kp) or _lo(out_vp)
    a.bias, a.bias_batch_stride, a.act = _p(bias), bias_bs, act
    a.resid, a.ldr, a.resid_row_mod = _p(resid), (ldr if ldr is not None else N), resid_row_mod
    a.out_f32, a.ldo_f32 = _p(out_f32), (ldo_f32 if ldo_f32 is not None else N)
    a.out_t, a.ldo_t = _p(out_t), (ldo_t if ldo_t is not None else N)
    a.out_batch_stride = out_bs
    a.out_kp, a.kp_col0, a.out_vp, a.vp_col0 = _p(out_kp), kp_col0, _p(out_vp), vp_col0
    a.kv_L, a.kv_Lpad, a.kv_hd = kv_L, kv_Lpad, kv_hd
    a.stat_out, a.ln_stat_in, a.ln_nparts, a.ln_dim, a.ln_eps = _p(stat_out), _p(ln_stat_in), ln_nparts, ln_dim, ln_eps
    a.ln_colsum, a.rln_gamma, a.rln_beta = _p(ln_colsum), _p(rln_gamma), _p(rln_beta)
    a.incr_counter, a.incr_table = _p(incr_counter), _p(incr_table)
    a.tile = tile
    a.batch2, a.a_batch_stride2, a.out_batch_stride2 = batch2, a_bs2, out_bs2      # second batch level: W / bias shared (grouped conv over clips)
    a.ksplit, a.ksplit_stride = ksplit, ksplit_stride      # S K-slices -> S fp32 partial planes of out_f32 (summed by layernorm(x_planes=S))
    if sched is not None:      # fused scheduler update in the epilogue (resid = x_t, out_f32 = x_{t-1})
        a.sched_fuse, a.sched = 1, sched
    check(lib().fdm_op_gemm(C.byref(a), stream()))


def kv_pad(L):
    """Padded key count of the fragment-packed K / V buffers (whole 32-key tiles)."""
    return (L + 31) // 32 * 32


def kv_buffers(B, H, L, hd, dtype, device):
    """Zeroed fragment-packed K and V buffers ([B*H, Lpad*hd] each; pad keys must stay finite)."""
    Lpad = kv_pad(L)
    return (torch.zeros(B * H, Lpad * hd, device=device, dtype=dtype),
            torch.zeros(B * H, Lpad * hd, device=device, dtype=dtype), Lpad)


def pack_kv(K, V, Kp, Vp, *, B, H, L, Lpad, hd, ldk, ldv):
    check(lib().fdm_op_pack_kv(_p(K), ldk, _p(V), ldv, _p(Kp), _p(Vp), B, H, L, Lpad, hd, code_of(K), stream()))


def attention(Q, Kp, Vp, O, *, B, H, L, hd, ldq, ldo, Lpad, scale, causal=False, slopes=None, period=1, lens=None):
    """lens: device int32 [B], per-clip lengths inside the padded [B, L] problem (fdm_attn_args.lens; non-causal, head dim 64 / 128)."""
    a = AttnArgs()
    a.Q, a.ldq, a.Kp, a.Vp, a.Lpad = _p(Q), ldq, _p(Kp), _p(Vp), Lpad
    a.O, a.ldo, a.B, a.H, a.L, a.hd, a.dtype = _p(O), ldo, B, H, L, hd, code_of(Q)
    if isinstance(Q, Split):       # split attention: Q, K, V and O are fp16 plane pairs
        a.q_lo_off, a.kv_lo_off, a.o_lo_off = Q.lo_off, Kp.lo_off, O.lo_off
    elif isinstance(O, Split):     # fp32 attention writing the next GEMM's split operand
        a.o_split, a.o_lo_off = O.code, O.lo_off
    a.scale, a.causal, a.slopes, a.period, a.lens = scale, int(causal), _p(slopes), period, _p(lens)
    check(lib().fdm_op_attention(C.byref(a), stream()))


def layernorm(x, gamma, beta, M, d, *, add_mat=None, add_tab=None, tab_index=None, tab_step=None, eps=1e-5,
              act=ACT_NONE, y_f32=None, y_t=None, dtype=F32, gamma2=None, beta2=None, x_planes=0, x_plane_stride=0,
              clip_step=None, clip_step_stride=1, clip_rows=0, clip_wrap=0, add_mat_group=0, add_mat_wrap=0, add_mat_L=0):
    """add_mat_group > 0: rows share add_mat rows (fdm_ln_args.add_mat_group: row m reads (m' / group) * add_mat_L + m' % add_mat_L,
    m' = m % add_mat_wrap when add_mat_wrap > 0).
    clip_step (device int32 words, clip_step_stride ints apart): the add_tab row is chosen per clip of clip_rows rows
    (fdm_ln_args.clip_step: the slot program's form) instead of by the single word tab_step."""
    a = LnArgs()
    a.x, a.M, a.d, a.add_mat, a.add_tab = _p(x), M, d, _p(add_mat), _p(add_tab)
    a.tab_index, a.tab_step, a.gamma, a.beta, a.eps = _p(tab_index), _p(tab_step), _p(gamma), _p(beta), eps
    a.act, a.y_f32, a.y_t, a.dtype = act, _p(y_f32), _p(y_t), dtype
    a.gamma2, a.beta2, a.y_t_lo_off = _p(gamma2), _p(beta2), _lo(y_t)
    a.x_planes, a.x_plane_stride = x_planes, x_plane_stride
    a.add_mat_group, a.add_mat_wrap, a.add_mat_L = add_mat_group, add_mat_wrap, add_mat_L
    if clip_step is not None:
        a.clip_step, a.clip_step_stride, a.clip_rows, a.clip_wrap = _p(clip_step), clip_step_stride, clip_rows, clip_wrap
    check(lib().fdm_op_layernorm(C.byref(a), stream()))


def sched_args(mode, x0, x, x_out, n, *, x0u=None, cfg_scale=0.0, n_per_clip=0, tseq=None, step=None, advance=0,
               c1=None, c2=None, sigma=None, sra=None, srm1=None, sqrt_an=None, c_n=None, noise=None, noise_stride=0,
               seed=0, clip0=0, x_out_t=None, arrive=None, lm_a=None, lm_b=None, lm_c=None, lm_s=None, x0_hist=None, seed_dev=None):
    """fdm_sched_args for fdm_op_sched_step, or (with x0 / x / x_out None) for gemm(..., sched=...).
    seed_dev: device int64 [2] = {seed, clip0}, read by the kernel in place of seed / clip0 (fdm_sched_args.seed_dev)."""
    a = SchedArgs()
    a.x0, a.x0u, a.cfg_scale, a.x, a.x_out = _p(x0), _p(x0u), cfg_scale, _p(x), _p(x_out)
    a.n, a.n_per_clip, a.tseq, a.step, a.advance = n, n_per_clip, _p(tseq), _p(step), advance
    a.c1, a.c2, a.sigma, a.sra, a.srm1 = _p(c1), _p(c2), _p(sigma), _p(sra), _p(srm1)
    a.sqrt_an, a.c_n, a.noise, a.noise_stride = _p(sqrt_an), _p(c_n), _p(noise), noise_stride
    a.seed, a.clip0, a.mode = seed, clip0, mode
    a.x_out_t, a.out_dtype, a.arrive = _p(x_out_t), (code_of(x_out_t) if x_out_t is not None else 0), _p(arrive)
    a.x_out_t_lo_off = _lo(x_out_t)
    a.lm_a, a.lm_b, a.lm_c, a.lm_s, a.x0_hist = _p(lm_a), _p(lm_b), _p(lm_c), _p(lm_s), _p(x0_hist)      # mode 3: tables by step k
    if seed_dev is not None:
        a.seed_dev = _p(seed_dev)
    return a


def sched_step(mode, x0, x, x_out, n, **kw):
    a = sched_args(mode, x0, x, x_out, n, **kw)
    check(lib().fdm_op_sched_step(C.byref(a), stream()))


def slot_sched(mode, x0, x, x_out, n, state, keys, n_slots, **kw):
    """fdm_op_slot_sched: state int32 [n_slots, 4] = {k, t, live, run}, keys int64 [n_slots, 2] = {seed, clip id} (device);
    the other arguments as sched_step (n_per_clip = n // n_slots is required)."""
    a = sched_args(mode, x0, x, x_out, n, **kw)
    check(lib().fdm_op_slot_sched(C.byref(a), _p(state), _p(keys), n_slots, stream()))


def slot_group_sched(mode, x0, x, x_out, n, state, keys, n_slots, *, member, frames, entries, groups, x_long, hist_long=None, L, d,
                     frame0=0, frame1=None, plain=1, init=0, **kw):
    """fdm_op_slot_group_sched: slot_sched over the plain slots plus the group update over the long arena in one launch.  Device
    tables: member int32 [n_slots], frames int32 [arena_frames, 4], entries [n_entries, 4] 32-bit words {slot, start, weight
    bits, 0}, groups int32 [n_groups, 4]; x_long / hist_long fp32 [arena_frames * d]."""
    a = sched_args(mode, x0, x, x_out, n, **kw)
    g = _lib.SlotGroupArgs()
    g.member, g.frames, g.entries, g.groups, g.x_long, g.hist_long = _p(member), _p(frames), _p(entries), _p(groups), _p(x_long), _p(hist_long)
    g.arena_frames, g.n_entries, g.n_groups, g.L, g.d = frames.shape[0], entries.shape[0], groups.shape[0], L, d
    g.frame0, g.frame1, g.plain, g.init = frame0, frames.shape[0] if frame1 is None else frame1, plain, init
    check(lib().fdm_op_slot_group_sched(C.byref(a), _p(state), _p(keys), n_slots, C.byref(g), stream()))


def bank_args(req, desc, t, coef):
    """fdm_slot_bank_args: req int32 [n_slots, 4] = {sampler, cfg_scale bits, 0, 0}, desc int32 [n_samplers, 4] = {mode, n_steps, t_off,
    c_off}, t int32 [n_t], coef fp32 [n_coef] (device; the layout is in include/fdm_hip.h)."""
    b = _lib.SlotBankArgs()
    b.req, b.desc, b.t, b.coef = _p(req), _p(desc), _p(t), _p(coef)
    b.n_samplers, b.n_t, b.n_coef = desc.shape[0], t.numel(), coef.numel()
    return b


def slot_sched_bank(x0, x, x_out, n, state, keys, n_slots, *, req, desc, t, coef, **kw):
    """fdm_op_slot_sched_bank: slot_sched with every slot's mode, step tables and cfg_scale read from its request row and the bank
    (bank_args); kw carries the t-indexed tables (c1 / c2 / sigma, sra / srm1), x0u, x_out_t, x0_hist, n_per_clip."""
    a = sched_args(0, x0, x, x_out, n, **kw)
    b = bank_args(req, desc, t, coef)
    check(lib().fdm_op_slot_sched_bank(C.byref(a), _p(state), _p(keys), n_slots, C.byref(b), stream()))


def slot_group_sched_bank(x0, x, x_out, n, state, keys, n_slots, *, req, desc, t, coef, member, frames, entries, groups, x_long, hist_long=None,
                          L, d, frame0=0, frame1=None, plain=1, init=0, **kw):
    """fdm_op_slot_group_sched_bank: slot_group_sched with the bank (a group reads its leader's request row)."""
    a = sched_args(0, x0, x, x_out, n, **kw)
    g = _lib.SlotGroupArgs()
    g.member, g.frames, g.entries, g.groups, g.x_long, g.hist_long = _p(member), _p(frames), _p(entries), _p(groups), _p(x_long), _p(hist_long)
    g.arena_frames, g.n_entries, g.n_groups, g.L, g.d = frames.shape[0], entries.shape[0], groups.shape[0], L, d
    g.frame0, g.frame1, g.plain, g.init = frame0, frames.shape[0] if frame1 is None else frame1, plain, init
    b = bank_args(req, desc, t, coef)
    check(lib().fdm_op_slot_group_sched_bank(C.byref(a), _p(state), _p(keys), n_slots, C.byref(g), C.byref(b), stream()))


def cast(src, dst):
    check(lib().fdm_op_cast(_p(src), _p(dst), src.numel(), code_of(dst), stream()))


def to_operand(src_f32, dtype):
    """fp32 device matrix -> operand-kind copy (identity for fp32; a Split plane pair for the split kinds)."""
    if dtype == F32:
        return src_f32
    if is_split(dtype):
        dst = Split(torch.empty((2,) + tuple(src_f32.shape), dtype=tdtype(dtype), device=src_f32.device), dtype)
    else:
        dst = torch.empty(src_f32.shape, dtype=tdtype(dtype), device=src_f32.device)
    cast(src_f32.contiguous(), dst)
    return dst


def bias_act(inp, vec, out, rows, d, act):
    check(lib().fdm_op_bias_act(_p(inp), _p(vec), _p(out), rows, d, act, stream()))


def add_rows(out, M, d, a, a_div, a_mod, b=None, b_div=1, b_mod=1, c=None, c_div=1, c_mod=1):
    check(lib().fdm_op_add_rows(_p(a), a_div, a_mod, _p(b), b_div, b_mod, _p(c), c_div, c_mod, _p(out), M, d, stream()))


def small_linear(x, W, bias, out, B, K, d, act=ACT_NONE):
    check(lib().fdm_op_small_linear(_p(x), _p(W), _p(bias), _p(out), B, K, d, act, stream()))


def cond_rows(pe, style, emo, sw, sb, ew, eb, out, B, L, L_clip, d, *, L_track=None, uncond_off=0, act=ACT_NONE):
    """fdm_op_cond_rows: out [B*L, d] (and the uncond half uncond_off elements on) from per-frame tracks style [B, L_track, n_style],
    emo [B, L_track, n_emo] or None."""
    check(lib().fdm_op_cond_rows(_p(pe), _p(style), _p(emo), _p(sw), _p(sb), _p(ew), _p(eb), _p(out), int(uncond_off), B, L, L_clip,
                                 style.shape[-2] if L_track is None else L_track, d, style.shape[-1], emo.shape[-1] if emo is not None else 0,
                                 act, stream()))


def pad_rows(inp, out, B, L, d, pad, zero=False):
    check(lib().fdm_op_pad_rows(_p(inp), _p(out), B, L, d, pad, code_of(inp), int(zero), stream()))


def pad_rows_lens(inp, out, B, L, d, pad, lens):
    """Replicate padding of clips of unequal length (lens: device int32 [B]) inside one padded [B, L, d] batch."""
    check(lib().fdm_op_pad_rows_lens(_p(inp), _p(out), B, L, d, pad, code_of(inp), _p(lens), stream()))


def zero_pad_rows(x, B, L, d, lens):
    check(lib().fdm_op_zero_pad_rows(_p(x), B, L, d, _p(lens), stream()))


def group_pad(inp, out, B, T, d, groups, pad):
    check(lib().fdm_op_group_pad(_p(inp), _p(out), B, T, d, groups, pad, code_of(inp), stream()))


def group_pad_lens(inp, out, B, T, d, groups, pad, lens):
    """Grouped zero padding of clips of unequal length (lens: device int32 [B]): frames at or beyond lens[b] are written as zeros."""
    check(lib().fdm_op_group_pad_lens(_p(inp), _p(out), B, T, d, groups, pad, code_of(inp), _p(lens), stream()))


def conv0(wav, w, bias, out, B, n, T0):
    check(lib().fdm_op_conv0(_p(wav), _p(w), _p(bias), _p(out), B, n, T0, stream()))


def conv0_ln_gelu(wav, w, bias, gamma, beta, out, B, n, T0, eps=1e-5):
    """conv layer 0 + LayerNorm(512) + GELU(erf) of HuBERT-large in one kernel; out [B, T0, 512] fp32 or bf16."""
    check(lib().fdm_op_conv0_ln_gelu(_p(wav), _p(w), _p(bias), _p(gamma), _p(beta), _p(out), _lo(out), B, n, T0, eps, code_of(out), stream()))


def leaky_instnorm(x, B, L, d, *, y_f32=None, y_t=None, eps=1e-5, dtype=F32):
    check(lib().fdm_op_leaky_instnorm(_p(x), _p(y_f32), _p(y_t), B, L, d, eps, dtype, stream()))


def leaky_instnorm_lens(x, B, L, d, lens, *, y_f32=None, y_t=None, eps=1e-5, dtype=F32):
    check(lib().fdm_op_leaky_instnorm_lens(_p(x), _p(y_f32), _p(y_t), B, L, d, eps, dtype, _p(lens), stream()))


def time_groupnorm(x, gamma, beta, B, T, C, *, y_f32=None, y_t=None, eps=1e-5, act=ACT_NONE, dtype=F32, scratch=None):
    """scratch: an 8-byte aligned device buffer (>= B * min(64, ceil(T / 1024)) * C * 16 bytes) lets clips of >= 4096 frames run over
    time chunks (two launches, hundreds of workgroups) instead of C / 64 workgroups per clip."""
    nbytes = scratch.numel() * scratch.element_size() if scratch is not None else 0
    check(lib().fdm_op_time_groupnorm(_p(x), _p(gamma), _p(beta), _p(y_f32), _p(y_t), _lo(y_t), B, T, C, eps, act, dtype, _p(scratch), nbytes, stream()))


def time_groupnorm_lens(x, gamma, beta, B, T, C, lens, *, y_f32=None, y_t=None, eps=1e-5, act=ACT_NONE, dtype=F32, scratch=None):
    """time_groupnorm over clips of unequal length (lens: device int32 [B]): each clip is normalised as its own launch with scratch
    would be; here the scratch is required once the padded T reaches 4096 frames."""
    nbytes = scratch.numel() * scratch.element_size() if scratch is not None else 0
    check(lib().fdm_op_time_groupnorm_lens(_p(x), _p(gamma), _p(beta), _p(y_f32), _p(y_t), _lo(y_t), B, T, C, eps, act, dtype, _p(scratch), nbytes,
                                           _p(lens), stream()))


def mean_diff(a, b, l1=False, partial=None, out=None):
    """mean((a - b)^2) or mean(|a - b|) as a 1-element device tensor.  partial (scratch, min(1024, ceil(n / 256)) floats are written)
    and out (1 float) may be the caller's."""
    partial = torch.empty(1024, device=a.device) if partial is None else partial
    out = torch.empty(1, device=a.device) if out is None else out
    check(lib().fdm_op_mean_diff(_p(a), _p(b), _p(partial), _p(out), a.numel(), int(l1), stream()))
    return out


def linear_interp(x, y, B, Tin, Tout, C):
    check(lib().fdm_op_linear_interp(_p(x), _p(y), B, Tin, Tout, C, stream()))


def vertex_err(gt, pred, region, R, F, V, frame_max, frame_sum, out):
    check(lib().fdm_op_vertex_err(_p(gt), _p(pred), _p(region), R, F, V, _p(frame_max), _p(frame_sum), _p(out), stream()))


def motion_std(verts, tmpl, region, R, F, V, partial, out):
    check(lib().fdm_op_motion_std(_p(verts), _p(tmpl), _p(region), R, F, V, _p(partial), _p(out), stream()))


def adain(content, style, out, NC, Lc, Ls, eps=1e-5):
    check(lib().fdm_op_adain(_p(content), _p(style), _p(out), NC, Lc, Ls, eps, stream()))


def vq_quant(z, codebook, book, B, R, c, K, zq_bcl, idx):
    check(lib().fdm_op_vq_quant(_p(z), _p(codebook), _p(book), B, R, c, K, _p(zq_bcl), _p(idx), stream()))


def vq_stats(z, codebook, book, idx, B, R, c, K, beta, min_encodings, partial, hist, out):
    """book: int32 [B] or None.  partial: >= min(1024, ceil(B R / 4)) doubles, hist: K int32 (cleared by the call), out: 2 floats
    (loss, perplexity); min_encodings [B R, K] fp32 or None."""
    check(lib().fdm_op_vq_stats(_p(z), _p(codebook), _p(book), _p(idx), B, R, c, K, beta, _p(min_encodings), _p(partial), _p(hist), _p(out),
                                stream()))


def argmax_rows(x, book, rows, n, rep, n_books):
    """book[r * rep .. r * rep + rep) = the first maximum of x[r, :n] (int32)."""
    check(lib().fdm_op_argmax_rows(_p(x), _p(book), rows, n, rep, n_books, stream()))


def vq_quant_rows(z, codebook, book_rows, n_books, B, R, c, K, zq_bcl, idx):
    """vq_quant with one codebook slice per row: book_rows int32 [B R]."""
    check(lib().fdm_op_vq_quant_rows(_p(z), _p(codebook), _p(book_rows), n_books, B, R, c, K, _p(zq_bcl), _p(idx), stream()))


def vq_stats_rows(z, codebook, book_rows, n_books, idx, B, R, c, K, beta, min_encodings, partial, hist, out):
    check(lib().fdm_op_vq_stats_rows(_p(z), _p(codebook), _p(book_rows), n_books, _p(idx), B, R, c, K, beta, _p(min_encodings), _p(partial),
                                     _p(hist), _p(out), stream()))


PCM_FORMATS = {torch.int16: _lib.PCM_S16, torch.int32: _lib.PCM_S32, torch.uint8: _lib.PCM_U8, torch.float32: _lib.PCM_F32}


def resample_ratio(rate):
    """(up, down) of `rate` -> 16 kHz (fdm_resample_ratio_host)."""
    up, down = C.c_int(0), C.c_int(0)
    check(lib().fdm_resample_ratio_host(int(rate), C.byref(up), C.byref(down)))
    return up.value, down.value


def resample_len(rate, frames):
    """ceil(frames * up / down): the samples `frames` sample frames at `rate` give at 16 kHz (fdm_resample_len_host)."""
    n = lib().fdm_resample_len_host(int(rate), int(frames))
    if n < 0:
        check(int(n))
    return int(n)


def resample_taps(up, down):
    """The 20 max(up, down) + 1 taps of the resampler in float64 (fdm_resample_taps_host), as a numpy array."""
    import numpy as np
    taps = np.empty(20 * max(int(up), int(down), 1) + 1, dtype=np.float64)
    n = lib().fdm_resample_taps_host(int(up), int(down), taps.ctypes.data)
    if n < 0:
        check(n)
    return taps[:n]


def pcm_desc(pcm, rate):
    """fdm_pcm of an interleaved device tensor [frames] or [frames, C] of dtype int16 / int32 / uint8 / float32."""
    if pcm.dtype not in PCM_FORMATS:
        raise _lib.FdmError(f"PCM dtype {pcm.dtype} (int16, int32, uint8 or float32)")
    if pcm.dim() not in (1, 2) or not pcm.is_contiguous():
        raise _lib.FdmError(f"PCM tensor of shape {tuple(pcm.shape)} (contiguous [frames] or [frames, C])")
    return _lib.Pcm(_p(pcm), PCM_FORMATS[pcm.dtype], 1 if pcm.dim() == 1 else int(pcm.shape[1]), int(rate), int(pcm.shape[0]))


def frontend_forward(handle, pcms, rates, wav, *, pad=0, normalize=True):
    """fdm_frontend_forward over device tensors: pcms[b] at rates[b] Hz -> wav [B, n_max] fp32 (written whole); returns n_samples."""
    B = len(pcms)
    clips = (_lib.Pcm * max(B, 1))(*[pcm_desc(p, r) for p, r in zip(pcms, rates)])
    ns = (C.c_int * max(B, 1))()
    check(lib().fdm_frontend_forward(handle, clips, B, int(pad), int(bool(normalize)), _p(wav), int(wav.shape[-1]), ns, stream()))
    return list(ns)[:B]


class Program:
    """A recorded sequence of fdm_op_* launches, replayable as a hipGraph (fdm_prog_*)."""

    def __init__(self):
        h = C.c_void_p()
        check(lib().fdm_prog_create(C.byref(h)))
        self.h = h
        self.keep = []          # tensors referenced by raw pointer inside the program

    def __enter__(self):
        check(lib().fdm_prog_begin(self.h))
        return self

    def __exit__(self, et, ev, tb):
        rc = lib().fdm_prog_end(self.h)
        if et is None:
            check(rc)
        return False

    def hold(self, *tensors):
        self.keep.extend(tensors)

    @property
    def num_ops(self):
        return lib().fdm_prog_num_ops(self.h)

    def run(self):
        check(lib().fdm_prog_run(self.h, stream()))

    def instantiate(self):
        check(lib().fdm_prog_instantiate(self.h, stream()))

    def replay(self, n=1):
        check(lib().fdm_prog_replay(self.h, n, stream()))

    def __del__(self):
        try:
            if self.h:
                lib().fdm_prog_destroy(self.h)
                self.h = None
        except Exception:
            pass
