// Kernels of the rig hand-off (include/fdm_hip.h, fdm_rig_*; launched by rig_out.hip): decoded vertex offsets -> blendshape coefficients
// per frame, a ridge-regularised, box-constrained least-squares fit onto a basis.  DESIGN section 2 item 19 is the definition.
//   rig_proj_kernel   grid (tiles of ROW_TILE rows of [B * L_max], chunks of ROW_CHUNK elements of 3V), 4 wavefronts.  Stages the tile's
//                     offsets in LDS through the 16-byte peel of handoff.hpp (a row starts on a 4-byte boundary only), each element at
//                     its logical position; the chunk's tail is zero-filled.  Every wavefront then takes the whole tile into registers
//                     (ROW_TILE x ROW_CHUNK / 64 values per lane) and walks k = wave, wave + 4, ...: 16-byte loads of P[k] (rows padded
//                     with zeros to whole chunks, so aligned and in bounds; K x ROW_CHUNK x 4 bytes per chunk, shared by every tile
//                     of the chunk: workgroup ids run over the tiles first, so the slab is served by the L2), ROW_TILE fused
//                     multiply-add chains per lane, then a halving butterfly over the lanes (ROW_TILE + 2 exchanges) whose shape is the
//                     same for every row slot.  Partial sums go to part [chunk][row][k] through LDS (whole lines).  Plain VALU: the
//                     fp32 MFMA rate on gfx950 is the vector rate, and the kernel is fed by the L2, not bound by either.
//   rig_solve_kernel  one wavefront per output frame, RIG_SW frames per workgroup, coefficient k on lane k mod 64 (two registers at
//                     K > 64).  r[k] = the partial sums of the frame's row in ascending chunk order, starting from the first; the
//                     frame-rate rule (interp_taps, handoff.hpp) applied to r; then the Cholesky solve and the projected Gauss-Seidel sweeps
//                     in the column order of the header, every operation rounded on its own.  G [K][K], L [K][K | 1] (an odd stride:
//                     its column reads are conflict-free), lo and hi sit in LDS: 132.6 KB at K = 128.  A NaN coefficient stays
//                     NaN through the clamp, as numpy's minimum / maximum keep it.
// A frame's values are a function of its own row: no atomics, and neither the batch, L_max, the row's slot in its tile nor the
// workgroup enters an expression.  Input rows at or past frames[b] are never read.  Resource use: profiles/rig_out/resources.txt.
// The kernels of the temporal fit (fdm_rig_set_temporal) follow the two above, under their own heading.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fdm_hip.h"
#include "handoff.hpp"

namespace fdm {

// (rig_proj_kernel's geometry is handoff.hpp's: one partial sum per ROW_CHUNK elements of 3V, ROW_TILE rows per workgroup)
constexpr int RIG_SW = 8;                 // wavefronts (= output frames) per workgroup of rig_solve_kernel
constexpr int RIG_KMAX = 128;

// min(max(x, lo), hi) that keeps a NaN x (fminf / fmaxf would return the bound)
__device__ __forceinline__ float rig_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ float rig_xor(float v, int mask) { return __shfl_xor(v, mask, 64); }
__device__ __forceinline__ float rig_lane(float v, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }

// off: [rows][V3] (rows = B * L_max; lens: [B][2] = {L, L_out}).  P: [K][ldp], ldp = chunks * ROW_CHUNK, zero behind V3.
// part: [chunks][rows][K].  A tile without a live row writes nothing (its partial sums are never read).
__global__ __launch_bounds__(256) void rig_proj_kernel(const float* off, const int* lens, int L_max, int rows, int V3, const float* P, int ldp,
                                                       int K, float* part) {
  __shared__ __attribute__((aligned(16))) float sd[ROW_TILE * ROW_CHUNK];
  __shared__ float so[ROW_TILE * RIG_KMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * ROW_TILE, c0 = blockIdx.y * ROW_CHUNK;
  const int n = min(ROW_CHUNK, V3 - c0);
  bool any = false;
#pragma unroll
  for (int r = 0; r < ROW_TILE; ++r) {
    const int row = row0 + r;
    float* d = sd + r * ROW_CHUNK;
    int b;
    const bool live = row_live(lens, 2, 0, row, L_max, rows, b);
    any |= live;
    if (!live) {
      for (int j = tid; j < ROW_CHUNK; j += 256) d[j] = 0.f;
      continue;
    }
    const float* src = off + (size_t)row * V3 + c0;
    peel_walk<256, 64>(peel_of(src, n), n, tid, PeelLoad{src, d});
    for (int j = n + tid; j < ROW_CHUNK; j += 256) d[j] = 0.f;
  }
  if (!any) return;                                         // (uniform over the workgroup)
  __syncthreads();
  float4 x[ROW_TILE][ROW_Q];
#pragma unroll
  for (int r = 0; r < ROW_TILE; ++r)
#pragma unroll
    for (int q = 0; q < ROW_Q; ++q) x[r][q] = *reinterpret_cast<const float4*>(sd + r * ROW_CHUNK + 4 * (lane + 64 * q));
  for (int k = wave; k < K; k += 4) {
    const float* pk = P + (size_t)k * ldp + c0;
    float4 p[ROW_Q];
#pragma unroll
    for (int q = 0; q < ROW_Q; ++q) p[q] = *reinterpret_cast<const float4*>(pk + 4 * (lane + 64 * q));
    float a[ROW_TILE];
#pragma unroll
    for (int r = 0; r < ROW_TILE; ++r) {
      float s = __fmul_rn(p[0].x, x[r][0].x);
      s = __builtin_fmaf(p[0].y, x[r][0].y, s); s = __builtin_fmaf(p[0].z, x[r][0].z, s); s = __builtin_fmaf(p[0].w, x[r][0].w, s);
#pragma unroll
      for (int q = 1; q < ROW_Q; ++q) {
        s = __builtin_fmaf(p[q].x, x[r][q].x, s); s = __builtin_fmaf(p[q].y, x[r][q].y, s);
        s = __builtin_fmaf(p[q].z, x[r][q].z, s); s = __builtin_fmaf(p[q].w, x[r][q].w, s);
      }
      a[r] = s;
    }
    // halving butterfly: after the masks 32, 16, 8 lane l holds row slot (l >> 3) & 7 summed over the lanes that share l & 7
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
    float b4[4], b2[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float keep = h5 ? a[j + 4] : a[j], give = h5 ? a[j] : a[j + 4]; b4[j] = __fadd_rn(keep, rig_xor(give, 32)); }
#pragma unroll
    for (int j = 0; j < 2; ++j) { const float keep = h4 ? b4[j + 2] : b4[j], give = h4 ? b4[j] : b4[j + 2]; b2[j] = __fadd_rn(keep, rig_xor(give, 16)); }
    float s = __fadd_rn(h3 ? b2[1] : b2[0], rig_xor(h3 ? b2[0] : b2[1], 8));
    s = __fadd_rn(s, rig_xor(s, 4)); s = __fadd_rn(s, rig_xor(s, 2)); s = __fadd_rn(s, rig_xor(s, 1));
    if ((lane & 7) == 0) so[(lane >> 3) * K + k] = s;
  }
  __syncthreads();
  const int live_rows = min(ROW_TILE, rows - row0);
  float* o = part + ((size_t)blockIdx.y * rows + row0) * K;
  for (int i = tid; i < live_rows * K; i += 256) o[i] = so[i];
}

// G [K][K], Lc [K][K] (lower Cholesky factor, row-major), lo / hi [K] (bounded = 0: not read).  coef / proj: [B][Lo_max][K] (proj may
// be null); rows at or past L_out[b] are written as zeros.  Dynamic LDS: (K * K + K * (K | 1) + 2 * K) floats.
__global__ __launch_bounds__(RIG_SW * 64) void rig_solve_kernel(const float* part, int chunks, int rows_in, const int* lens, int L_max, int Lo_max,
                                                                int rows_out, int K, int resample, const float* G, const float* Lc,
                                                                const float* lo, const float* hi, int bounded, int sweeps, float* coef,
                                                                float* proj) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sG = reinterpret_cast<float*>(smem);
  float* sL = sG + K * K;
  float* slo = sL + K * (K | 1);
  float* shi = slo + K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ld = K | 1;
  for (int i = tid; i < K * K; i += RIG_SW * 64) { sG[i] = G[i]; sL[(i / K) * ld + i % K] = Lc[i]; }
  if (bounded) for (int i = tid; i < K; i += RIG_SW * 64) { slo[i] = lo[i]; shi[i] = hi[i]; }
  __syncthreads();
  const int row = blockIdx.x * RIG_SW + wave;
  if (row >= rows_out) return;                              // (uniform over the wavefront; no barrier follows)
  const int b = row / Lo_max, t = row - b * Lo_max;
  const int L = lens[2 * b], Lo = lens[2 * b + 1];
  const int H = K > 64 ? 2 : 1;
  float* oc = coef + (size_t)row * K;
  float* op = proj ? proj + (size_t)row * K : nullptr;
  if (t >= Lo) {
    for (int h = 0; h < H; ++h) { const int k = lane + 64 * h; if (k < K) { oc[k] = 0.f; if (op) op[k] = 0.f; } }
    return;
  }
  int i0 = t, i1 = t;
  float l0 = 1.f, l1 = 0.f;
  if (resample) interp_taps(L, Lo, t, i0, i1, l0, l1);
  float r[2] = {0.f, 0.f}, g[2], c[2] = {0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    if (k >= K) continue;
    const float* p0 = part + ((size_t)b * L_max + i0) * K + k;
    const float* p1 = part + ((size_t)b * L_max + i1) * K + k;
    const size_t cs = (size_t)rows_in * K;
    float s0 = p0[0], s1 = resample ? p1[0] : 0.f;
    for (int q = 1; q < chunks; ++q) {
      s0 = __fadd_rn(s0, p0[q * cs]);
      if (resample) s1 = __fadd_rn(s1, p1[q * cs]);
    }
    r[h] = resample ? __fadd_rn(__fmul_rn(l0, s0), __fmul_rn(l1, s1)) : s0;
    if (op) op[k] = r[h];
  }
  g[0] = r[0]; g[1] = r[1];
  // forward: y_i = g_i / L_ii; g_k -= L_ki y_i for k > i (g becomes y in place)
  for (int i = 0; i < K; ++i) {
    const float gi = i < 64 ? rig_lane(g[0], i) : rig_lane(g[1], i - 64);
    const float y = __fdiv_rn(gi, sL[i * ld + i]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k == i) g[h] = y;
      else if (k > i && k < K) g[h] = __fsub_rn(g[h], __fmul_rn(sL[k * ld + i], y));
    }
  }
  // backward: x_i = y_i / L_ii; y_k -= L_ik x_i for k < i (g becomes x in place)
  for (int i = K - 1; i >= 0; --i) {
    const float yi = i < 64 ? rig_lane(g[0], i) : rig_lane(g[1], i - 64);
    const float x = __fdiv_rn(yi, sL[i * ld + i]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k == i) g[h] = x;
      else if (k < i) g[h] = __fsub_rn(g[h], __fmul_rn(sL[i * ld + k], x));
    }
  }
  if (!bounded) {
    c[0] = g[0]; c[1] = g[1];
  } else {
    float lo_k[2] = {0.f, 0.f}, hi_k[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < K) { lo_k[h] = slo[k]; hi_k[h] = shi[k]; }
      c[h] = rig_clamp(g[h], lo_k[h], hi_k[h]);
      g[h] = r[h];
    }
    // residual g = r - G c, one column of G at a time (G is symmetric: column j is row j)
    for (int j = 0; j < K; ++j) {
      const float cj = j < 64 ? rig_lane(c[0], j) : rig_lane(c[1], j - 64);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        if (k < K) g[h] = __fsub_rn(g[h], __fmul_rn(sG[j * K + k], cj));
      }
    }
    for (int s = 0; s < sweeps; ++s)
      for (int j = 0; j < K; ++j) {
        const float cj = j < 64 ? rig_lane(c[0], j) : rig_lane(c[1], j - 64);
        const float gj = j < 64 ? rig_lane(g[0], j) : rig_lane(g[1], j - 64);
        const float nj = rig_clamp(__fadd_rn(cj, __fdiv_rn(gj, sG[j * K + j])), slo[j], shi[j]);
        const float delta = __fsub_rn(nj, cj);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = lane + 64 * h;
          if (k == j) c[h] = nj;
          if (k < K) g[h] = __fsub_rn(g[h], __fmul_rn(sG[j * K + k], delta));
        }
      }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) { const int k = lane + 64 * h; if (k < K) oc[k] = c[h]; }
}

// ---- the temporal fit (include/fdm_hip.h, fdm_rig_set_temporal): the clip's frames coupled by
// 1/2 (c_f - c_{f-1})^T M (c_f - c_{f-1}).  Q^T G Q = Lam and Q^T M Q = I turn the block-tridiagonal system of a clip into K scalar
// tridiagonal systems along time.  After rig_proj_kernel:
//   rig_modal_in_kernel   rig_solve_kernel's geometry and its chunk sum and frame-rate step, then z_k = sum_j QT[k][j] r_j.  Q sits in LDS
//                         row-major, so lane k reads QT[k][j] = Q[j][k] at j K + k: consecutive banks.  Writes r (the sweeps read it
//                         again), z, proj; the rows at and past L_out[b] of coef and proj as zeros.
//   rig_time_kernel       one lane per (clip, k): grid (B, K / 64 rounded up), one wavefront each.  A lane walks its clip's frames forward
//                         (u over z in place, 1 / w beside it) and back (y over u); at every frame the wavefront's loads and stores are
//                         64 consecutive floats.  The recurrence is sequential by nature: its cost is Lo dependent divisions.
//   rig_modal_out_kernel  x_k = sum_j Q[k][j] y_j with Q^T in LDS (the same bank pattern), the clamp when bounded, coef.
//   rig_sweep_kernel      one colour of one projected Gauss-Seidel sweep: one wavefront per frame of that parity, which reads its two
//                         neighbours (the other parity: nobody writes them in this launch) and rewrites its own row of coef.  G, mu m,
//                         lo, hi in LDS: 65.5 KB at K = 128.  The launch boundary is the only synchronisation between half-sweeps.
// Every expression names the clip's own rows, its own L_out and the frame's index inside the clip; every operation is rounded on its own.
// Resource use: profiles/rig_temporal/resources.txt.

// o_k = sum_j sT[j K + k] v_j: j ascending, the first product starts the sum.  v, o: coefficient k on lane k mod 64, half k / 64.
__device__ __forceinline__ void rig_modal(const float* sT, int K, int lane, const float (&v)[2], float (&o)[2]) {
  o[0] = 0.f; o[1] = 0.f;
  for (int j = 0; j < K; ++j) {
    const float vj = j < 64 ? rig_lane(v[0], j) : rig_lane(v[1], j - 64);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < K) { const float p = __fmul_rn(sT[j * K + k], vj); o[h] = j ? __fadd_rn(o[h], p) : p; }
    }
  }
}

// part, lens, coef, proj: as rig_solve_kernel.  Q [K][K] (column k = mode k).  rbuf, zbuf: [B * Lo_max][K], live rows only.
// Dynamic LDS: K * K floats.
__global__ __launch_bounds__(RIG_SW * 64) void rig_modal_in_kernel(const float* part, int chunks, int rows_in, const int* lens, int L_max, int Lo_max,
                                                                   int rows_out, int K, int resample, const float* Q, float* rbuf, float* zbuf,
                                                                   float* coef, float* proj) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sT = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < K * K; i += RIG_SW * 64) sT[i] = Q[i];
  __syncthreads();
  const int row = blockIdx.x * RIG_SW + wave;
  if (row >= rows_out) return;                              // (uniform over the wavefront; no barrier follows)
  const int b = row / Lo_max, t = row - b * Lo_max;
  const int L = lens[2 * b], Lo = lens[2 * b + 1];
  const int H = K > 64 ? 2 : 1;
  float* op = proj ? proj + (size_t)row * K : nullptr;
  if (t >= Lo) {
    float* oc = coef + (size_t)row * K;
    for (int h = 0; h < H; ++h) { const int k = lane + 64 * h; if (k < K) { oc[k] = 0.f; if (op) op[k] = 0.f; } }
    return;
  }
  int i0 = t, i1 = t;
  float l0 = 1.f, l1 = 0.f;
  if (resample) interp_taps(L, Lo, t, i0, i1, l0, l1);
  float r[2] = {0.f, 0.f}, z[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    if (k >= K) continue;
    const float* p0 = part + ((size_t)b * L_max + i0) * K + k;
    const float* p1 = part + ((size_t)b * L_max + i1) * K + k;
    const size_t cs = (size_t)rows_in * K;
    float s0 = p0[0], s1 = resample ? p1[0] : 0.f;
    for (int q = 1; q < chunks; ++q) {
      s0 = __fadd_rn(s0, p0[q * cs]);
      if (resample) s1 = __fadd_rn(s1, p1[q * cs]);
    }
    r[h] = resample ? __fadd_rn(__fmul_rn(l0, s0), __fmul_rn(l1, s1)) : s0;
    if (op) op[k] = r[h];
    rbuf[(size_t)row * K + k] = r[h];
  }
  rig_modal(sT, K, lane, r, z);
#pragma unroll
  for (int h = 0; h < 2; ++h) { const int k = lane + 64 * h; if (k < K) zbuf[(size_t)row * K + k] = z[h]; }
}

// lam [K].  zu [B * Lo_max][K]: z in, y out.  iw [B * Lo_max][K]: scratch (1 / w_f).  Grid (B, (K + 63) / 64), 64 threads.
__global__ __launch_bounds__(64) void rig_time_kernel(const int* lens, int Lo_max, int K, const float* lam, float* zu, float* iw) {
  const int b = blockIdx.x, k = blockIdx.y * 64 + threadIdx.x;
  const int Lo = lens[2 * b + 1];
  if (k >= K || Lo < 1) return;
  const size_t base = (size_t)b * Lo_max * K + k;
  float* u = zu + base;
  float* w = iw + base;
  const float lk = lam[k];
  const float d_end = __fadd_rn(lk, Lo > 1 ? 1.f : 0.f), d_in = __fadd_rn(lk, 2.f);      // n_f = 1 at the two ends (0 when alone), 2 inside
  float iwp = __fdiv_rn(1.f, d_end), up = u[0];
  w[0] = iwp;
  for (int f = 1; f < Lo; ++f) {
    const float wf = __fsub_rn(f == Lo - 1 ? d_end : d_in, iwp);
    up = __fadd_rn(u[(size_t)f * K], __fmul_rn(up, iwp));
    iwp = __fdiv_rn(1.f, wf);
    u[(size_t)f * K] = up;
    w[(size_t)f * K] = iwp;
  }
  float y = __fmul_rn(up, iwp);
  u[(size_t)(Lo - 1) * K] = y;
  for (int f = Lo - 2; f >= 0; --f) {
    y = __fmul_rn(__fadd_rn(u[(size_t)f * K], y), w[(size_t)f * K]);
    u[(size_t)f * K] = y;
  }
}

// y [B * Lo_max][K] (live rows).  QT [K][K] = Q transposed.  lo / hi [K] (bounded = 0: not read).  Writes the live rows of coef.
// Dynamic LDS: K * K floats.
__global__ __launch_bounds__(RIG_SW * 64) void rig_modal_out_kernel(const float* y, const int* lens, int Lo_max, int rows_out, int K, const float* QT,
                                                                    const float* lo, const float* hi, int bounded, float* coef) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sT = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < K * K; i += RIG_SW * 64) sT[i] = QT[i];
  __syncthreads();
  const int row = blockIdx.x * RIG_SW + wave;
  if (row >= rows_out) return;                              // (uniform over the wavefront; no barrier follows)
  const int b = row / Lo_max, t = row - b * Lo_max;
  if (t >= lens[2 * b + 1]) return;
  float v[2] = {0.f, 0.f}, x[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) { const int k = lane + 64 * h; if (k < K) v[h] = y[(size_t)row * K + k]; }
  rig_modal(sT, K, lane, v, x);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    if (k < K) coef[(size_t)row * K + k] = bounded ? rig_clamp(x[h], lo[k], hi[k]) : x[h];
  }
}

// One colour (0: even frames of a clip, 1: odd) of one sweep, in place in coef.  per = frames of this colour in Lo_max, rows = B * per.
// r [B * Lo_max][K], G [K][K], mvec [K] = mu m, lo / hi [K].  Dynamic LDS: (K * K + 3 * K) floats.
__global__ __launch_bounds__(RIG_SW * 64) void rig_sweep_kernel(const float* r, const int* lens, int Lo_max, int per, int rows, int colour, int K,
                                                                const float* G, const float* mvec, const float* lo, const float* hi, float* coef) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sG = reinterpret_cast<float*>(smem);
  float* smv = sG + K * K;
  float* slo = smv + K;
  float* shi = slo + K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < K * K; i += RIG_SW * 64) sG[i] = G[i];
  for (int i = tid; i < K; i += RIG_SW * 64) { smv[i] = mvec[i]; slo[i] = lo[i]; shi[i] = hi[i]; }
  __syncthreads();
  const int i = blockIdx.x * RIG_SW + wave;
  if (i >= rows) return;                                    // (uniform over the wavefront; no barrier follows)
  const int b = i / per, t = 2 * (i - b * per) + colour;
  const int Lo = lens[2 * b + 1];
  if (t >= Lo) return;
  const int nf = Lo == 1 ? 0 : (t == 0 || t == Lo - 1 ? 1 : 2);
  const float fn = (float)nf;
  const size_t at = ((size_t)b * Lo_max + t) * K;
  float* own = coef + at;
  float c[2] = {0.f, 0.f}, g[2] = {0.f, 0.f}, e[2] = {0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + 64 * h;
    if (k >= K) continue;
    c[h] = own[k];
    g[h] = r[at + k];
    if (nf) {
      const float s = nf == 2 ? __fadd_rn(own[k - K], own[k + K]) : (t > 0 ? own[k - K] : own[k + K]);
      g[h] = __fadd_rn(g[h], __fmul_rn(smv[k], s));
    }
    e[h] = __fmul_rn(fn, smv[k]);
  }
  for (int j = 0; j < K; ++j) {
    const float cj = j < 64 ? rig_lane(c[0], j) : rig_lane(c[1], j - 64);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k < K) g[h] = __fsub_rn(g[h], __fmul_rn(sG[j * K + k], cj));
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) g[h] = __fsub_rn(g[h], __fmul_rn(e[h], c[h]));
  for (int j = 0; j < K; ++j) {
    const float cj = j < 64 ? rig_lane(c[0], j) : rig_lane(c[1], j - 64);
    const float gj = j < 64 ? rig_lane(g[0], j) : rig_lane(g[1], j - 64);
    const float ej = __fmul_rn(fn, smv[j]);
    const float nj = rig_clamp(__fadd_rn(cj, __fdiv_rn(gj, __fadd_rn(sG[j * K + j], ej))), slo[j], shi[j]);
    const float delta = __fsub_rn(nj, cj);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k == j) c[h] = nj;
      if (k < K) g[h] = __fsub_rn(g[h], __fmul_rn(sG[j * K + k], delta));
      if (k == j) g[h] = __fsub_rn(g[h], __fmul_rn(ej, delta));
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) { const int k = lane + 64 * h; if (k < K) own[k] = c[h]; }
}

}  // namespace fdm
