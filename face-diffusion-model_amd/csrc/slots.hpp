// In-flight batching (fdm_slots_open / fdm_slot_admit / fdm_slots_run): the slots of a plan are clips at DIFFERENT diffusion
// steps inside one step program.  Per-slot device state, advanced once per diffusion step before anything reads it, and the
// scheduler pass that updates every live slot with its own (k, t, seed, clip id) -- sched_update4 / sched_noise4 of sched.hpp, so a
// slot's bits are those of sched_kernel on the clip alone.  Vector loads and stores only; state words are written in plain C++.
#pragma once
#include "common.hpp"
#include "sched.hpp"
#include "../../include/fdm_hip.h"

namespace fdm {

// One int4 per slot.  k = step index of the slot's chain, t = tseq[k] (always a valid table row: idle and finished slots keep the
// last one, so the per-clip gathers of the LayerNorm launches stay in bounds), live = the slot is updated by this step,
// run = the chain has steps left.  A zeroed word is an idle slot.
struct SlotState { int k, t, live, run; };
constexpr int SLOT_WORDS = 4;      // ints per slot (fdm_ln_args.clip_step_stride of the slot program)
constexpr int SLOT_T_WORD = 1;     // the word the LayerNorm launches gather TT_l by

// First launch of a slot step: a running slot with k + 1 < n_steps moves on (k += 1, t = tseq[k], live), every other slot is
// parked (live = 0, t untouched).  One lane per slot.
__global__ __launch_bounds__(64) void slot_advance_kernel(SlotState* st, const int* tseq, int n_steps, int n_slots) {
  for (int s = threadIdx.x; s < n_slots; s += blockDim.x) {
    SlotState v = st[s];
    if (v.run && v.k + 1 < n_steps) {
      v.k += 1; v.t = tseq[v.k]; v.live = 1;
    } else {
      v.live = 0; v.run = 0;
    }
    st[s] = v;
  }
}

// fdm_slot_admit: one slot's state and noise key, by value (stream-ordered between steps; no host memory is read later)
__global__ void slot_set_kernel(SlotState* st, SlotState v, unsigned long long* key, unsigned long long seed, unsigned long long clip_id) {
  if (threadIdx.x == 0) { *st = v; key[0] = seed; key[1] = clip_id; }
}

// The scheduler pass of the slot program.  p: x0 (+ x0u, cfg_scale), x, x_out, x_out_t, n = n_slots * n_per_clip, mode 0 / 1 / 3 with
// its tables and x0_hist; p.step / tseq / seed / clip0 / seed_dev / arrive / noise are not read.  A slot that is not live is
// skipped whole: nothing of it is stored.
__global__ __launch_bounds__(256) void slot_sched_kernel(const fdm_sched_args p, const SlotState* st, const unsigned long long* keys) {
  const long long nq = p.n / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (long long)gridDim.x * blockDim.x) {
    const long long e = 4 * i;
    const int clip = (int)(e / p.n_per_clip);
    const SlotState s = st[clip];
    if (!s.live) continue;
    SchedCoef c;
    c.k = s.k; c.t = s.t;
    c.c1 = c.c2 = c.sg = c.sra = c.san = c.cn = 0.f;
    c.srm1 = 1.f;
    c.seed = keys[2 * clip];
    c.clip0 = (int)keys[2 * clip + 1] - clip;      // sched_noise4 keys by clip0 + (e / n_per_clip) = the slot's clip id
    if (p.mode == 3) { c.c1 = p.lm_b[c.k]; c.c2 = p.lm_a[c.k]; c.sg = p.lm_s[c.k]; c.cn = p.lm_c[c.k]; }
    else if (p.mode == 0) { c.c1 = p.c1[c.t]; c.c2 = p.c2[c.t]; c.sg = p.sigma[c.t]; }
    else { c.sra = p.sra[c.t]; c.srm1 = p.srm1[c.t]; c.san = p.sqrt_an[c.k]; c.cn = p.c_n[c.k]; }
    f32x4 x0 = *(const f32x4*)(p.x0 + e);
    if (p.x0u) {
      const f32x4 u = *(const f32x4*)(p.x0u + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) x0[j] = __fadd_rn(u[j], __fmul_rn(p.cfg_scale, __fsub_rn(x0[j], u[j])));
    }
    const f32x4 x = *(const f32x4*)(p.x + e);
    const f32x4 o = p.mode == 3 ? sched_update4<true>(p, c, x0, x, e) : sched_update4<false>(p, c, x0, x, e);
    *(f32x4*)(p.x_out + e) = o;
    if (p.x_out_t) {
      if (p.out_dtype == FDM_BF16) store_opnd4<bf16>((bf16*)p.x_out_t + e, 0, o);
      else if (p.out_dtype == FDM_F16X3) store_opnd4<f16x3_t>((f16*)p.x_out_t + e, p.x_out_t_lo_off, o);
      else if (p.out_dtype == FDM_F16) store_opnd4<f16>((f16*)p.x_out_t + e, 0, o);
      else *(f32x4*)((float*)p.x_out_t + e) = o;
    }
  }
}

static hipError_t slot_sched_launch(const fdm_sched_args& a, const int* state, const unsigned long long* keys, hipStream_t s) {
  const long long nq = a.n / 4;
  int blocks = (int)((nq + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(slot_sched_kernel, dim3(blocks), dim3(256), 0, s, a, (const SlotState*)state, keys);
  return hipGetLastError();
}

}  // namespace fdm
