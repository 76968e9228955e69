// Device functions of the diffusion scheduler update (DDPM posterior sample / DDIM eta = 0 / table-driven linear multistep) and its
// Philox noise, shared by sched_kernel (elementwise.hpp), the GEMM epilogue's fused form (gemm.hpp), window_sched_kernel
// (window.hpp) and the slot passes (slots.hpp) so all of them produce the same bits.  The pieces of a scheduler pass around the
// update -- guidance mix, window blend, mode dispatch, operand copy -- are at the end of this file, once, for the same reason.
#pragma once
#include "common.hpp"
#include "../../include/fdm_hip.h"

namespace fdm {

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller: counter = (element/4, step, global clip, 0), key = seed.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ f32x4 philox_normal4(unsigned long long seed, unsigned quad, unsigned step, unsigned clip) {
  unsigned r[4];
  philox4x32_10(quad, step, clip, 0u, (unsigned)seed, (unsigned)(seed >> 32), r);
  const float k = 2.3283064365386963e-10f;  // 2^-32
  const float u0 = ((float)r[0] + 0.5f) * k, u1 = (float)r[1] * k;
  const float u2 = ((float)r[2] + 0.5f) * k, u3 = (float)r[3] * k;
  // hardware log2 / sin / cos (v_log_f32, v_sin_f32, v_cos_f32 take the angle in turns): the noise is a
  // sampling input, not a parity surface, and the accurate libm forms made this kernel VALU-bound
  const float ra = sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(fminf(u0, 1.f)));   // -2 ln u = -2 ln2 log2 u
  const float rb = sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(fminf(u2, 1.f)));
  const float s0 = __builtin_amdgcn_sinf(u1), c0 = __builtin_amdgcn_cosf(u1);
  const float s1 = __builtin_amdgcn_sinf(u3), c1 = __builtin_amdgcn_cosf(u3);
  return f32x4{ra * c0, ra * s0, rb * c1, rb * s1};
}

// ------------------------------------------------------------------------------------------------
// Scheduler step (DDPM posterior sample / DDIM eta=0 update / CFG mix), 16 B per lane.
// Explicit _rn operations (no FMA contraction) so the fp32 result is bit-identical to the
// reference's unfused torch expression order.
// ------------------------------------------------------------------------------------------------
// Per-step scalars of the update (k = step index, t = tseq[k]) and the update of 4 consecutive latent elements starting at
// flat element e of the x buffer.  Shared by sched_kernel and by the GEMM epilogue's fused form (fdm_gemm_args.sched_fuse),
// so both produce the same bits.
struct SchedCoef { int k, t; float c1, c2, sg, sra, srm1, san, cn; unsigned long long seed; int clip0; };
// LM = the table-driven linear multistep form (fdm_sched_args.mode 3) is compiled in; without it the DDPM / DDIM forms keep the
// code (and the registers: no x0_hist pointer, no extra table loads) they had before mode 3 existed.  sched_kernel and
// window_sched_kernel branch on the mode at run time; the GEMM epilogue's fused form is a template specialisation (GEMM_LM).
template <bool LM = false>
__device__ __forceinline__ SchedCoef sched_coef_load(const fdm_sched_args& p) {
  SchedCoef c;
  c.k = p.step ? *(volatile const int*)p.step : 0;
  c.t = p.tseq ? p.tseq[c.k] : c.k;
  c.c1 = c.c2 = c.sg = c.sra = c.san = c.cn = 0.f;
  c.srm1 = 1.f;
  c.seed = p.seed_dev ? p.seed_dev[0] : p.seed;
  c.clip0 = p.seed_dev ? (int)p.seed_dev[1] : p.clip0;
  if constexpr (LM) {
    // x' = a x + b x0 + c x0_prev + s z, tables indexed by step k.  The four scalars ride in the DDPM / DDIM slots
    // (c1 = b, c2 = a, sg = s, cn = c), so the coefficient block keeps its size.
    c.c1 = p.lm_b[c.k]; c.c2 = p.lm_a[c.k]; c.sg = p.lm_s[c.k]; c.cn = p.lm_c[c.k];
  } else {
    if (p.mode == 0) { c.c1 = p.c1[c.t]; c.c2 = p.c2[c.t]; c.sg = p.sigma[c.t]; }
    if (p.mode == 1) { c.sra = p.sra[c.t]; c.srm1 = p.srm1[c.t]; c.san = p.sqrt_an[c.k]; c.cn = p.c_n[c.k]; }
  }
  return c;
}
// z of 4 consecutive elements for step k: injected noise, or Philox keyed (seed, clip0 + clip, element, k)
__device__ __forceinline__ f32x4 sched_noise4(const fdm_sched_args& p, const SchedCoef& c, long long e) {
  if (p.noise) return *(const f32x4*)(p.noise + (size_t)c.k * (p.noise_stride > 0 ? p.noise_stride : p.n) + e);
  const int clip = (int)(e / p.n_per_clip);
  return philox_normal4(c.seed, (unsigned)((e - (long long)clip * p.n_per_clip) >> 2), (unsigned)c.k, (unsigned)(c.clip0 + clip));
}
template <bool LM = false>
__device__ __forceinline__ f32x4 sched_update4(const fdm_sched_args& p, const SchedCoef& c, f32x4 x0, f32x4 x, long long e) {
  f32x4 o;
  if constexpr (LM) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(__fmul_rn(c.c1, x0[j]), __fmul_rn(c.c2, x[j]));      // b x0 + a x
    // the previous step's x0 prediction: each lane reads, then rewrites, its own four elements of x0_hist (no hazard)
    if (c.cn != 0.f) {
      const f32x4 h = *(const f32x4*)(p.x0_hist + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(o[j], __fmul_rn(c.cn, h[j]));
    }
    *(f32x4*)(p.x0_hist + e) = x0;
    if (c.sg != 0.f) {
      const f32x4 z = sched_noise4(p, c, e);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(o[j], __fmul_rn(c.sg, z[j]));
    }
    return o;
  }
  if (p.mode == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(__fmul_rn(c.c1, x0[j]), __fmul_rn(c.c2, x[j]));
    if (c.t > 0) {
      const f32x4 z = sched_noise4(p, c, e);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(o[j], __fmul_rn(c.sg, z[j]));
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float eps = __fdiv_rn(__fsub_rn(__fmul_rn(c.sra, x[j]), x0[j]), c.srm1);
      o[j] = __fadd_rn(__fmul_rn(x0[j], c.san), __fmul_rn(c.cn, eps));
    }
  }
  return o;
}

// ------------------------------------------------------------------------------------------------
// The pieces of a scheduler pass around the update.  "A slot's bits are the solo call's bits, a group's bits are the windowed
// call's bits" holds because every pass goes through the SAME expression in the same operand order: change one here and every
// form named at it changes with it.  (Their launchers share the grid as well: grid_for of host.hpp, 256 lanes per block.)
// ------------------------------------------------------------------------------------------------
// Guidance mix of a quad, x0 <- u + scale * (x0 - u) (utiles/classifierfree.py:20-21), unfused.  Must agree: sched_kernel,
// slot_update_quad (both slot kernels, plain slots of both group kernels), the per-window mix of slot_group_sched_kernel and of
// window_sched_kernel.
__device__ __forceinline__ void sched_cfg_mix4(f32x4& x0, const f32x4& u, float scale) {
#pragma unroll
  for (int j = 0; j < 4; ++j) x0[j] = __fadd_rn(u[j], __fmul_rn(scale, __fsub_rn(x0[j], u[j])));
}
// One term of the window blend, terms taken in ascending window order.  The first term STARTS the sum (it is not added to a
// zero): one window of weight 1 passes x0 through bit for bit, -0 included.  Must agree: window_sched_kernel and the arena walk of
// slot_group_sched_kernel (a long request in slots against fdm_sample_windows).
__device__ __forceinline__ void sched_blend4(f32x4& acc, bool first, float wt, const f32x4& x0) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = first ? __fmul_rn(wt, x0[j]) : __fadd_rn(acc[j], __fmul_rn(wt, x0[j]));
}
// sched_update4 with the mode chosen at run time (p.mode 0 / 1 / 3).  Must agree: sched_kernel, window_sched_kernel and the slot
// kernels; the GEMM epilogue's fused form picks the same two specialisations at compile time (GEMM_LM).
__device__ __forceinline__ f32x4 sched_update4_rt(const fdm_sched_args& p, const SchedCoef& c, const f32x4& x0, const f32x4& x, long long e) {
  return p.mode == 3 ? sched_update4<true>(p, c, x0, x, e) : sched_update4<false>(p, c, x0, x, e);
}
// The operand-kind copy of an updated quad at flat element q of p.x_out_t (nothing when there is none): what the next step's first
// GEMM reads.  F32 = the fp32 kind is compiled in; window_sched_kernel is never given x_out_t on an fp32 plan and has no such
// store.  Must agree: sched_kernel (+ its mix-only mode, which admits and loads go through), the slot kernels, window_sched_kernel.
template <bool F32 = true>
__device__ __forceinline__ void sched_store_t4(const fdm_sched_args& p, long long q, const f32x4& o) {
  if (!p.x_out_t) return;
  if (p.out_dtype == FDM_BF16) store_opnd4<bf16>((bf16*)p.x_out_t + q, 0, o);
  else if (p.out_dtype == FDM_F16X3) store_opnd4<f16x3_t>((f16*)p.x_out_t + q, p.x_out_t_lo_off, o);
  else if (p.out_dtype == FDM_F16) store_opnd4<f16>((f16*)p.x_out_t + q, 0, o);
  else if constexpr (F32) *(f32x4*)((float*)p.x_out_t + q) = o;
}

}  // namespace fdm
