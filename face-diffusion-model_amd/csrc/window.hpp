// Windowed sampling of clips longer than the denoiser's max_len (fdm_audio_prepare_windows / fdm_sample_windows): one pass over
// the LONG layout [B, L_total * d] per diffusion step that blends the overlapping windows' x0 predictions, applies the scheduler
// update once per long-clip element (the same bits and the same Philox stream as sched_kernel) and writes the result back to the
// long buffer and to every window row that holds the frame (fp32 x + the operand-kind copy of the next step).
// The walk over the off[] CSR and WinEnt rows is this kernel's own (its host builder is trusted: no bounds checks); the per-term
// arithmetic -- guidance mix, blend term, update, operand copy -- is sched.hpp's, shared with slot_group_sched_kernel (slots.hpp),
// which walks the group tables of a long request in slots and must produce this kernel's bits.
#pragma once
#include "common.hpp"
#include "sched.hpp"
#include "../../include/fdm_hip.h"
#include "kernels.hpp"
#include "host.hpp"      // grid_for: the 1-D launch grid of the pass

namespace fdm {

// p: the scheduler arguments in LONG layout (x = x_out = the long buffer, n = B * L_total * d, n_per_clip = L_total * d, noise
// [steps, B, L_total * d], x0_hist of the table-driven mode [B, L_total * d]: it keeps the BLENDED x0); p.x0 / p.x0u / p.x_out_t
// are the plan's window-layout buffers.  Vector loads and stores only.
__global__ __launch_bounds__(256) void window_sched_kernel(const fdm_sched_args p, const WinArgs w) {
  const SchedCoef c = p.mode == 3 ? sched_coef_load<true>(p) : sched_coef_load<false>(p);
  const long long nq = p.n / 4, per_clip = (long long)w.L_total * w.d, wrows = (long long)w.W * w.d;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (long long)gridDim.x * blockDim.x) {
    const long long e = 4 * i;
    const int b = (int)(e / per_clip);
    const long long r = e - (long long)b * per_clip;
    const int f = (int)(r / w.d);
    const long long col = r - (long long)f * w.d;
    const int j0 = w.off[f], j1 = w.off[f + 1];
    const long long base = (long long)b * w.n_win * wrows + (long long)f * w.d + col;     // + window * wrows - start * d
    f32x4 o;
    if (w.init) {
      o = *(const f32x4*)(p.x + e);
    } else {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j = j0; j < j1; ++j) {
        const WinEnt en = w.ent[j];
        const long long q = base + (long long)en.w * wrows - (long long)en.start * w.d;
        f32x4 x0 = *(const f32x4*)(p.x0 + q);
        if (p.x0u) sched_cfg_mix4(x0, *(const f32x4*)(p.x0u + q), p.cfg_scale);      // per window, before the blend
        sched_blend4(acc, j == j0, en.wt, x0);
      }
      const f32x4 x = *(const f32x4*)(p.x + e);
      o = sched_update4_rt(p, c, acc, x, e);
      *(f32x4*)(p.x_out + e) = o;
    }
    for (int j = j0; j < j1; ++j) {
      const WinEnt en = w.ent[j];
      const long long q = base + (long long)en.w * wrows - (long long)en.start * w.d;
      *(f32x4*)(w.xw + q) = o;
      sched_store_t4<false>(p, q, o);      // (never given x_out_t on an fp32 plan)
    }
  }
}

static hipError_t window_launch(const fdm_sched_args& a, const WinArgs& w, hipStream_t s) {
  hipLaunchKernelGGL(window_sched_kernel, dim3(grid_for(a.n / 4)), dim3(256), 0, s, a, w);
  return hipGetLastError();
}

}  // namespace fdm
