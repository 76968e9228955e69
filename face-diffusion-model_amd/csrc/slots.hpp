// In-flight batching (fdm_slots_open / fdm_slot_admit / fdm_slots_run): the slots of a plan are clips at DIFFERENT diffusion
// steps inside one step program.  Per-slot device state, advanced once per diffusion step before anything reads it, and the
// scheduler pass that updates every live slot with its own (k, t, seed, clip id) -- the mix, update, noise and stores of sched.hpp,
// so a slot's bits are those of sched_kernel on the clip alone.  Vector loads and stores only; state words are written in plain C++.
// Long requests (fdm_slot_admit_long): a recording longer than a slot occupies a GROUP of slots, one window each; with long capacity
// the scheduler pass is slot_group_sched_kernel, which does the plain slots' update and, over the long arena, window_sched_kernel's
// blend + update per group at the group's own (k, t) (its own table walk, sched.hpp's blend term).
// Sampler bank (fdm_slot_sampler_add / fdm_slot_admit_as): with bank capacity every slot names ITS OWN sampler and guidance scale.
// Each pass is ONE body, slot_sched_kernel<BANK> and slot_group_sched_kernel<BANK>: the <true> instantiations read the sampler and
// the scale through fdm_slot_bank_args (behind `if constexpr (BANK)`), the <false> ones compile to the code without a bank.  The
// advance launch has two kernels (slot_advance_kernel, slot_advance_bank_kernel).  Layout of the bank, all plan-owned device memory:
//   req    [n_slots]     rows {int sampler, float cfg_scale, int 0, int 0}      -- its own array: SlotState keeps its stride
//   desc   [n_samplers]  rows {int mode (0 DDPM / 1 DDIM / 3 table-driven), int n_steps, int t_off, int c_off}; n_steps == 0 = free row
//   t      [n_t]         ints: sampler i's timesteps are t[t_off .. t_off + n_steps)
//   coef   [n_coef]      fp32, step-indexed, starting at c_off:   mode 1  sqrt_an[n_steps] | c_n[n_steps]
//                                                                   mode 3  a[n_steps] | b[n_steps] | c[n_steps] | s[n_steps]
//                                                                   mode 0  nothing (c1 / c2 / sigma are indexed by t and shared)
// The t-indexed tables (c1, c2, sigma, sra, srm1) stay in fdm_sched_args: every sampler shares them.
#pragma once
#include "common.hpp"
#include "sched.hpp"
#include "../../include/fdm_hip.h"
#include "kernels.hpp"
#include "host.hpp"      // grid_for: the 1-D launch grid of the pass

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

// One 16-byte row per slot and per bank descriptor (fdm_slot_bank_args.req / .desc)
struct SlotReq { int sampler; float cfg_scale; int pad0, pad1; };
struct BankDesc { int mode, n_steps, t_off, c_off; };
// step-indexed coefficients per step of a mode (the layout above)
__host__ __device__ __forceinline__ int bank_coefs_per_step(int mode) { return mode == 3 ? 4 : (mode == 1 ? 2 : 0); }

// The advance launch with a bank: n_steps and t = bank_t[t_off + k] come from the descriptor the slot's request row names.  A slot
// whose sampler id, offsets or t fall outside the bank sizes / [0, 1000) is parked like a finished one (live = 0, run = 0, t
// untouched): a bad value is never used as an index.
__global__ __launch_bounds__(64) void slot_advance_bank_kernel(SlotState* st, const SlotReq* req, const BankDesc* desc, const int* bank_t,
                                                               int n_samplers, int n_t, int n_slots) {
  for (int s = threadIdx.x; s < n_slots; s += blockDim.x) {
    SlotState v = st[s];
    bool go = false;
    if (v.run) {
      const int id = req[s].sampler;
      if (id >= 0 && id < n_samplers) {
        const BankDesc ds = desc[id];
        const int k = v.k + 1;
        if (k >= 0 && k < ds.n_steps && ds.t_off >= 0 && (long long)ds.t_off + ds.n_steps <= n_t) {
          const int t = bank_t[ds.t_off + k];
          if (t >= 0 && t < 1000) { v.k = k; v.t = t; v.live = 1; go = true; }
        }
      }
    }
    if (!go) { v.live = 0; v.run = 0; }
    st[s] = v;
  }
}

// fdm_slot_admit: one slot's state and noise key, by value (stream-ordered between steps; no host memory is read later)
__global__ void slot_set_kernel(SlotState* st, SlotState v, unsigned long long* key, unsigned long long seed, unsigned long long clip_id) {
  if (threadIdx.x == 0) { *st = v; key[0] = seed; key[1] = clip_id; }
}
// ... and with a bank its request row as well (fdm_slot_admit_as)
__global__ void slot_set_bank_kernel(SlotState* st, SlotState v, unsigned long long* key, unsigned long long seed, unsigned long long clip_id,
                                     SlotReq* req, SlotReq r) {
  if (threadIdx.x == 0) { *st = v; key[0] = seed; key[1] = clip_id; *req = r; }
}
// fdm_slot_read on a bank plan: the word of a slot that was read stops running, so that a sampler added later under the same
// descriptor never wakes it (k and t stay)
__global__ void slot_park_kernel(SlotState* st) {
  if (threadIdx.x == 0) { SlotState v = *st; v.live = 0; v.run = 0; *st = v; }
}

// A live slot's view of the bank: the mode and guidance scale of ITS request and where its step-indexed coefficients start.
// Every field is checked against the bank sizes (and k, t against the sampler) before it becomes an index; false = a bad row,
// the caller stores nothing.  16-byte vector loads of the two rows.
struct SlotBankView { int mode; float cfg_scale; const float* coef; int n_steps; };
__device__ __forceinline__ bool slot_bank_view(const fdm_sched_args& p, const fdm_slot_bank_args& b, int slot, const SlotState& s, SlotBankView& v) {
  const int4 rq = *((const int4*)b.req + slot);
  if (rq.x < 0 || rq.x >= b.n_samplers) return false;
  const int4 ds = *((const int4*)b.desc + rq.x);      // {mode, n_steps, t_off, c_off}
  if (ds.x != 0 && ds.x != 1 && ds.x != 3) return false;
  if (ds.y < 1 || s.k < 0 || s.k >= ds.y || s.t < 0 || s.t >= 1000) return false;
  if (ds.z < 0 || (long long)ds.z + ds.y > b.n_t) return false;
  if (ds.w < 0 || (long long)ds.w + (long long)bank_coefs_per_step(ds.x) * ds.y > b.n_coef) return false;
  if (ds.x == 0 && (!p.c1 || !p.c2 || !p.sigma)) return false;
  if (ds.x == 1 && (!p.sra || !p.srm1)) return false;
  if (ds.x == 3 && !p.x0_hist) return false;
  v.mode = ds.x; v.cfg_scale = __int_as_float(rq.y); v.coef = b.coef + ds.w; v.n_steps = ds.y;
  return true;
}

// The per-step scalars of a slot at ITS (k, t), noise keyed (seed, clip0 + clip of the element).  BANK: p.mode is the mode of the slot's
// sampler and the step-indexed tables are the slot's range of the bank (bv, checked by slot_bank_view); the t-indexed ones are p's.
template <bool BANK>
__device__ __forceinline__ SchedCoef slot_coef(const fdm_sched_args& p, const SlotState& s, unsigned long long seed, int clip0, const SlotBankView& bv) {
  SchedCoef c;
  c.k = s.k; c.t = s.t;
  c.c1 = c.c2 = c.sg = c.sra = c.san = c.cn = 0.f;
  c.srm1 = 1.f;
  c.seed = seed;
  c.clip0 = clip0;
  if constexpr (BANK) {
    const float* co = bv.coef;
    const int n = bv.n_steps;
    if (p.mode == 3) { c.c2 = co[c.k]; c.c1 = co[n + c.k]; c.cn = co[2 * n + c.k]; c.sg = co[3 * n + c.k]; }
    else if (p.mode == 0) { c.c1 = p.c1[c.t]; c.c2 = p.c2[c.t]; c.sg = p.sigma[c.t]; }
    else { c.sra = p.sra[c.t]; c.srm1 = p.srm1[c.t]; c.san = co[c.k]; c.cn = co[n + c.k]; }
    return c;
  }
  if (p.mode == 3) { c.c1 = p.lm_b[c.k]; c.c2 = p.lm_a[c.k]; c.sg = p.lm_s[c.k]; c.cn = p.lm_c[c.k]; }
  else if (p.mode == 0) { c.c1 = p.c1[c.t]; c.c2 = p.c2[c.t]; c.sg = p.sigma[c.t]; }
  else { c.sra = p.sra[c.t]; c.srm1 = p.srm1[c.t]; c.san = p.sqrt_an[c.k]; c.cn = p.c_n[c.k]; }
  return c;
}
// One plain slot's four elements starting at flat element e (the slot is live): CFG mix, update at the slot's (k, t), stores.
// BANK: the mode and guidance scale are those of the slot's request (p is a copy: the slot's view of the arguments); a bad row
// stores nothing.
template <bool BANK>
__device__ __forceinline__ void slot_update_quad(fdm_sched_args p, const fdm_slot_bank_args& b, const SlotState& s, const unsigned long long* keys,
                                                 int clip, long long e) {
  SlotBankView bv;
  if constexpr (BANK) {
    if (!slot_bank_view(p, b, clip, s, bv)) return;
    p.mode = bv.mode; p.cfg_scale = bv.cfg_scale;
  }
  // sched_noise4 keys by clip0 + (e / n_per_clip) = the slot's clip id
  const SchedCoef c = slot_coef<BANK>(p, s, keys[2 * clip], (int)keys[2 * clip + 1] - clip, bv);
  f32x4 x0 = *(const f32x4*)(p.x0 + e);
  if (p.x0u) sched_cfg_mix4(x0, *(const f32x4*)(p.x0u + e), p.cfg_scale);
  const f32x4 x = *(const f32x4*)(p.x + e);
  const f32x4 o = sched_update4_rt(p, c, x0, x, e);
  *(f32x4*)(p.x_out + e) = o;
  sched_store_t4(p, e, o);
}

// The scheduler pass of the slot program.  p: x0 (+ x0u, cfg_scale), x, x_out, x_out_t, n = n_slots * n_per_clip, mode 0 / 1 / 3 with
// its tables and x0_hist; p.step / tseq / seed / clip0 / seed_dev / arrive / noise are not read.  A slot that is not live is
// skipped whole: nothing of it is stored.
// BANK (fdm_op_slot_sched_bank): p.mode and p.cfg_scale are not read, every live slot takes them from its request row; p carries the
// t-indexed tables of every mode the bank may hold.  Without BANK, b is not read.
template <bool BANK>
__global__ __launch_bounds__(256) void slot_sched_kernel(const fdm_sched_args p, const SlotState* st, const unsigned long long* keys,
                                                         const fdm_slot_bank_args b) {
  const long long nq = p.n / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (long long)gridDim.x * blockDim.x) {
    const long long e = 4 * i;
    const int clip = (int)(e / p.n_per_clip);
    const SlotState s = st[clip];
    if (!s.live) continue;
    slot_update_quad<BANK>(p, b, s, keys, clip, e);
  }
}

// The scheduler pass of a slot plan with long capacity (fdm_slot_admit_long): ONE launch over the plain slots and the long arena.
//   plain slots   quads [0, p.n / 4) when g.plain: slot_sched_kernel's update, except that a slot that belongs to a group
//                 (g.member[slot] >= 0) is skipped -- its rows are written from the arena below
//   long arena    one quad per four elements of the arena frames [g.frame0, g.frame1).  A frame's group gives the leader slot,
//                 whose state word supplies (k, t, live) and whose key words supply (seed, clip id); the covering windows' x0 (CFG
//                 mix per window first) are blended in ascending window order, the first term starting the sum, as
//                 window_sched_kernel does; the update runs once per long-clip element with the element's index INSIDE ITS OWN long
//                 clip as noise counter and history index (groups have different L_total: sched_update4 gets a per-group view of p);
//                 the result goes to the arena and to every window row holding the frame (p.x_out + operand copy).
//                 g.init: no update -- the arena (x_T) is copied into the window rows, whatever the leader's word says.
// Every table row is checked against the sizes in g before it is used as an index; a row outside them stores nothing.
// BANK (fdm_op_slot_group_sched_bank): the same walk, a plain slot reading its own request row and a group its LEADER's.
template <bool BANK>
__global__ __launch_bounds__(256) void slot_group_sched_kernel(const fdm_sched_args p, const SlotState* st, const unsigned long long* keys,
                                                               const fdm_slot_group_args g, int n_slots, const fdm_slot_bank_args b) {
  const long long nq_plain = g.plain ? p.n / 4 : 0;
  const long long nq = nq_plain + (long long)(g.frame1 - g.frame0) * g.d / 4;
  const LongFrame* frames = (const LongFrame*)g.frames;
  const LongEnt* ents = (const LongEnt*)g.entries;
  const LongGroup* groups = (const LongGroup*)g.groups;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (long long)gridDim.x * blockDim.x) {
    if (i < nq_plain) {
      const long long e = 4 * i;
      const int clip = (int)(e / p.n_per_clip);
      const SlotState s = st[clip];
      if (!s.live || g.member[clip] >= 0) continue;
      slot_update_quad<BANK>(p, b, s, keys, clip, e);
      continue;
    }
    const long long ea = (long long)g.frame0 * g.d + 4 * (i - nq_plain);      // element of the arena
    const int f = (int)(ea / g.d), col = (int)(ea - (long long)f * g.d);
    const LongFrame fr = frames[f];
    if (fr.group < 0 || fr.group >= g.n_groups || fr.e0 < 0 || fr.e1 > g.n_entries) continue;
    const LongGroup gr = groups[fr.group];
    const int fl = f - gr.first;                                              // frame inside the long clip
    if (gr.leader < 0 || gr.leader >= n_slots || fl < 0 || fl >= gr.L_total) continue;
    const SlotState s = st[gr.leader];
    if (!g.init && !s.live) continue;
    // the group's view of the arguments: one clip of L_total frames whose history starts at its first arena frame; the element
    // index inside the long clip keys the noise (clip0 = the group's clip id) and indexes the history
    fdm_sched_args pl = p;
    pl.n_per_clip = (long long)gr.L_total * g.d;
    pl.x0_hist = g.hist_long ? g.hist_long + (long long)gr.first * g.d : nullptr;
    pl.noise = nullptr;
    SlotBankView bv;
    if constexpr (BANK) {
      // ... with the sampler and guidance scale of its leader's request; a bad row stores nothing
      bv.mode = 0; bv.cfg_scale = 0.f; bv.coef = nullptr; bv.n_steps = 0;
      if (!g.init && (!slot_bank_view(p, b, gr.leader, s, bv) || (bv.mode == 3 && !g.hist_long))) continue;
      pl.mode = bv.mode; pl.cfg_scale = bv.cfg_scale;
    }
    f32x4 o;
    if (g.init) {
      o = *(const f32x4*)(g.x_long + ea);
    } else {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j = fr.e0; j < fr.e1; ++j) {
        const LongEnt en = ents[j];
        const int r = fl - en.start;
        if (en.slot < 0 || en.slot >= n_slots || r < 0 || r >= g.L) continue;
        const long long q = ((long long)en.slot * g.L + r) * g.d + col;
        f32x4 x0 = *(const f32x4*)(p.x0 + q);
        if (p.x0u) sched_cfg_mix4(x0, *(const f32x4*)(p.x0u + q), pl.cfg_scale);      // per window, before the blend
        sched_blend4(acc, j == fr.e0, en.wt, x0);
      }
      const SchedCoef c = slot_coef<BANK>(pl, s, keys[2 * gr.leader], (int)keys[2 * gr.leader + 1], bv);
      const long long el = (long long)fl * g.d + col;
      const f32x4 x = *(const f32x4*)(g.x_long + ea);
      o = sched_update4_rt(pl, c, acc, x, el);
      *(f32x4*)(g.x_long + ea) = o;
    }
    for (int j = fr.e0; j < fr.e1; ++j) {
      const LongEnt en = ents[j];
      const int r = fl - en.start;
      if (en.slot < 0 || en.slot >= n_slots || r < 0 || r >= g.L) continue;
      const long long q = ((long long)en.slot * g.L + r) * g.d + col;
      *(f32x4*)(p.x_out + q) = o;
      sched_store_t4(p, q, o);
    }
  }
}

// b = the bank of the bank forms, null for the forms without one (their kernels get an empty struct that they do not read)
static hipError_t slot_sched_launch(const fdm_sched_args& a, const int* state, const unsigned long long* keys, const fdm_slot_bank_args* b, hipStream_t s) {
  const dim3 grid(grid_for(a.n / 4));
  if (b) hipLaunchKernelGGL(slot_sched_kernel<true>, grid, dim3(256), 0, s, a, (const SlotState*)state, keys, *b);
  else hipLaunchKernelGGL(slot_sched_kernel<false>, grid, dim3(256), 0, s, a, (const SlotState*)state, keys, fdm_slot_bank_args{});
  return hipGetLastError();
}

static hipError_t slot_group_sched_launch(const fdm_sched_args& a, const int* state, const unsigned long long* keys, const fdm_slot_group_args& g,
                                          int n_slots, const fdm_slot_bank_args* b, hipStream_t s) {
  const dim3 grid(grid_for((g.plain ? a.n / 4 : 0) + (long long)(g.frame1 - g.frame0) * g.d / 4));
  if (b) hipLaunchKernelGGL(slot_group_sched_kernel<true>, grid, dim3(256), 0, s, a, (const SlotState*)state, keys, g, n_slots, *b);
  else hipLaunchKernelGGL(slot_group_sched_kernel<false>, grid, dim3(256), 0, s, a, (const SlotState*)state, keys, g, n_slots, fdm_slot_bank_args{});
  return hipGetLastError();
}

}  // namespace fdm

