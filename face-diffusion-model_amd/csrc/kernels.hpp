// Launchers of the heavy kernel families, one translation unit per operand kind (gemm_*.hip, attn_*.hip) so that the
// library builds in parallel; fdm_hip.hip (the C ABI + the bandwidth kernels) calls them through these declarations (host-only helpers: host.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/fdm_hip.h"

namespace fdm {
int fail(int code, const char* fmt, ...);      // fdm_hip.hip: sets the thread's fdm_last_error() text, returns code
hipError_t gemm_launch_f32(const fdm_gemm_args& a, hipStream_t s);
hipError_t gemm_launch_bf16(const fdm_gemm_args& a, hipStream_t s);
hipError_t gemm_launch_f16x3(const fdm_gemm_args& a, hipStream_t s);
hipError_t gemm_launch_f16(const fdm_gemm_args& a, hipStream_t s);
hipError_t attn_launch_f32(const fdm_attn_args& a, hipStream_t s);
hipError_t attn_launch_bf16(const fdm_attn_args& a, hipStream_t s);
hipError_t attn_launch_f16x3(const fdm_attn_args& a, hipStream_t s);
hipError_t attn_launch_f16(const fdm_attn_args& a, hipStream_t s);
hipError_t pack_kv_launch_f32(const void* K, long long ldk, const void* V, long long ldv, void* Kp, void* Vp, int B, int H, int L, int Lpad, int hd, hipStream_t s);
hipError_t pack_kv_launch_bf16(const void* K, long long ldk, const void* V, long long ldv, void* Kp, void* Vp, int B, int H, int L, int Lpad, int hd, hipStream_t s);

// windowed sampling (window.hpp; tables built by fdm_audio_prepare_windows, plan.hip): frame f of a long clip is covered by the windows ent[off[f] .. off[f + 1]) in ascending
// window order, each with its start frame and normalised blend weight; one table serves every long clip of the batch
struct WinEnt { int w; int start; float wt; int pad; };
struct WinArgs {
  const int* off; const WinEnt* ent;
  float* xw;          // the plan's fp32 x, window layout [B * n_win, W * d] (x0 / x0u / x_out_t of the sched args use the same rows)
  int L_total;        // latent frames of a long clip
  int n_win;          // windows per long clip (plan clip b * n_win + w)
  int W;              // frames per window (= the plan's L)
  int d;              // elements per latent frame (G * c)
  int init;           // 1: no update -- copy the long buffer (x_T) into the window rows only
};
// fdm_hip.hip: records / launches window_sched_kernel like any fdm_op_* (p in long layout, see window.hpp)
int window_sched_op(const fdm_sched_args& p, const WinArgs& w, void* stream);

// in-flight batching (slots.hpp): advance every slot's {k, t, live, run} word once per step; set one slot's word and noise key
int slot_advance_op(int* state, const int* tseq, int n_steps, int n_slots, void* stream);
int slot_set_op(int* state, int slot, int k, int t, int live, int run, unsigned long long* keys, unsigned long long seed, int clip_id, void* stream);
// ... on a plan with a sampler bank (fdm_slot_bank_args): the advance launch reads every slot's own sampler; an admit also writes the
// slot's request row {sampler, cfg_scale}; a read parks the slot's word
int slot_advance_bank_op(int* state, const fdm_slot_bank_args& b, int n_slots, void* stream);
int slot_set_bank_op(int* state, int slot, int k, int t, int live, int run, unsigned long long* keys, unsigned long long seed, int clip_id,
                     void* req, int sampler, float cfg_scale, void* stream);
int slot_park_op(int* state, int slot, void* stream);

// long requests in slot mode (slots.hpp; tables built by fdm_slot_group_table_host, uploaded by fdm_slot_admit_long): the device rows
// fdm_slot_group_args points at.  One LongFrame per frame of the long arena, one LongEnt per (window, frame of the window), one
// LongGroup per group descriptor.
struct LongFrame { int group; int e0; int e1; int pad; };      // group < 0: the arena frame is free; its covering entries are ent[e0 .. e1)
struct LongEnt { int slot; int start; float wt; int pad; };    // member slot holding the window, the window's first frame, blend weight
struct LongGroup { int leader; int L_total; int first; int pad; };      // leader slot, frames of the long clip, its first arena frame

inline hipError_t gemm_launch(const fdm_gemm_args& a, hipStream_t s) {
  switch (a.dtype) {
    case FDM_BF16: return gemm_launch_bf16(a, s);
    case FDM_F16X3: return gemm_launch_f16x3(a, s);
    case FDM_F16: return gemm_launch_f16(a, s);
    default: return gemm_launch_f32(a, s);
  }
}
inline hipError_t attn_launch(const fdm_attn_args& a, hipStream_t s) {
  return a.dtype == FDM_BF16 ? attn_launch_bf16(a, s) : (a.dtype == FDM_F16 ? attn_launch_f16(a, s) : (a.dtype == FDM_F16X3 ? attn_launch_f16x3(a, s) : attn_launch_f32(a, s)));
}
}  // namespace fdm
