// Time filter hand-off, the recurrences (include/fdm_hip.h, fdm_tfilter_create_recur): a one-pole low-pass
// ("ema") and the One Euro filter (Casiez et al., CHI 2012: a one-pole low-pass whose cutoff rises with the smoothed speed of the vertex)
// of the decoded offsets along time, per clip at its own length.  One kernel, one body: both kinds, the forward and the backward walk,
// with and without a strength, with and without a carried state, fixed and ragged batches.  The definition, stated once:
//   x [B, L_max, N] fp32, N = 3 V; L per clip (0 <= L <= L_max, 0 with a state only).  Constants q (fdm_tfilter_recur_coeffs_host):
//   k = (float)(fps / 2 pi), c0, be, cd, fr = (float)fps, ad = cd / (cd + k), a0 = c0 / (c0 + k).  Every operation below is one fp32
//   operation rounded on its own.
//   ema, per column: y_0 = x_0; y_t = y_{t-1} + a0 (x_t - y_{t-1}).
//   one_euro, per vertex: y_0 = x_0, dh_0 = 0; t >= 1, per column: dx = (x_t - x_{t-1}) fr, dh_t = dh_{t-1} + ad (dx - dh_{t-1}); per
//   vertex: s = sqrt((dh.x dh.x + dh.y dh.y) + dh.z dh.z), fc = c0 + be s, a = fc / (fc + k); per column: y_t = y_{t-1} + a (x_t - y_{t-1}).
//   x_{t-1} is the raw input.
//   causal: f = y.  zero_phase: the causal filter, then the same filter over its result walked from frame L - 1 down to 0, afresh.
//   out = f without a strength; with s_v: out = x where s_v == 0 (a copy), else x + s_v (f - x), x the ORIGINAL input (under zero_phase
//   applied once, after the second walk); the recurrence always runs on the unblended f.  Rows at or past L are written as zeros;
//   input rows at or past L are never read.
//   State (causal only): seen[b] > 0 continues from st[b] = (y_prev, x_prev, dh) [3][N] as if the frames had been contiguous, and the
//   walk's last values are written back (ema: row 0 alone); a clip with L == 0 leaves its state as it is.  time_recur_seen_kernel adds
//   L to seen afterwards, in a launch of its own: every workgroup of the clip reads seen at its start.
//   A clip's bits depend on nothing but its own frames: every element is the fixed chain above.  No atomics.
// Mapping: time is serial, so a thread owns one vertex -- its three columns -- and walks the frames; 64 lanes read one contiguous span
// of 768 bytes of a row, 12 bytes each, which needs the 4-byte alignment a row has and nothing more (no peel).  A workgroup is ONE
// wave of TR_VERTS vertices of one clip: at 4 clips x 5023 vertices that is 316 waves for 1024 SIMDs, so the waves spread over the CUs
// and nothing but the dependent chain and the memory latency is left to hide.  The addresses of later frames do not depend on values:
// a ring of D frames in registers is loaded ahead (frame i + D is requested before frame i's arithmetic), so the chain a frame waits
// on is the arithmetic alone.  The second walk of zero_phase runs in place on y in the same launch: a thread reads an element (D
// frames ahead of the walk) before it writes it, and no other thread touches its columns.
#pragma once
#include <hip/hip_runtime.h>

namespace fdm {

constexpr int TR_EMA = 0, TR_ONE_EURO = 1;        // FDM_TFILTER_EMA / FDM_TFILTER_ONE_EURO
constexpr int TR_CAUSAL = 0, TR_ZERO_PHASE = 1;   // FDM_TFILTER_CAUSAL / FDM_TFILTER_ZERO_PHASE
constexpr int TR_VERTS = 64;                      // vertices per workgroup: one wave, a lane per vertex
constexpr int TR_DEPTH = 16;                      // frames loaded ahead of the walk (fdm_tfilter_set_prefetch: 1, 4, 8 or 16; the bits do not depend on it)
constexpr int TR_NCOEFF = 8;                      // FDM_TFILTER_NCOEFF floats: k, c0, be, cd, fr, ad, a0, 0

struct RecurCoef { float k, c0, be, cd, fr, ad, a0, pad; };
struct F3 { float a[3]; };

__device__ __forceinline__ F3 tr_load(const float* p) { return {{p[0], p[1], p[2]}}; }
__device__ __forceinline__ void tr_store(float* p, const F3& v) { p[0] = v.a[0]; p[1] = v.a[1]; p[2] = v.a[2]; }

// the carried values of one vertex: y_{t-1}, x_{t-1}, dh_{t-1}
struct RecurState { F3 y, xp, dh; };

// One frame: x the input of the walk, S the state before and after.  fresh: this is the first frame ever (y = x, dh = 0) -- chosen by
// selects, not by a branch: the loop body stays one basic block.
template <int KIND> __device__ __forceinline__ void recur_step(const F3& x, RecurState& S, bool fresh, const RecurCoef& q) {
  float a = q.a0;
  if (KIND == TR_ONE_EURO) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float dx = __fmul_rn(__fsub_rn(x.a[c], S.xp.a[c]), q.fr);
      const float dh = __fadd_rn(S.dh.a[c], __fmul_rn(q.ad, __fsub_rn(dx, S.dh.a[c])));
      S.dh.a[c] = fresh ? 0.f : dh;
    }
    const float s2 = __fadd_rn(__fadd_rn(__fmul_rn(S.dh.a[0], S.dh.a[0]), __fmul_rn(S.dh.a[1], S.dh.a[1])), __fmul_rn(S.dh.a[2], S.dh.a[2]));
    const float fc = __fadd_rn(q.c0, __fmul_rn(q.be, sqrtf(s2)));      // sqrtf: the correctly rounded expansion, as in mesh_nrm_kernel (__fsqrt_rn is the bare v_sqrt_f32 here: 1 ulp)
    a = __fdiv_rn(fc, __fadd_rn(fc, q.k));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float y = __fadd_rn(S.y.a[c], __fmul_rn(a, __fsub_rn(x.a[c], S.y.a[c])));
    S.y.a[c] = fresh ? x.a[c] : y;
  }
  S.xp = x;
}

// One walk of L frames (L >= 1) of one vertex.  src, orig, dst: frame 0 of the clip at the vertex's first column, rows N floats apart;
// back: from frame L - 1 down.  BLEND: 0 = write f; 1 = blend f into the walk's own input with strength s; 2 = into orig's frame (the
// second walk of zero_phase, where src is the first walk's result).  src may be dst: frame i + D is read before frame i is written.
// The ring rx (and ro) holds the next D frames of the walk.  While 2 D frames or more remain the body has no branch: the ring's D
// frames move to cx, the D frames after them are requested into the ring, and then the D frames are computed and stored -- the
// requests have D frames of arithmetic to arrive in (left to itself the scheduler sinks them to the end of the body, which is what
// the barrier forbids).  The last frames (fewer than 2 D) go one by one under their two conditions.
template <int KIND, int D, int BLEND>
__device__ __forceinline__ void recur_walk(const float* src, const float* orig, float* dst, int L, size_t N, bool back, bool fresh, float s,
                                           const RecurCoef& q, RecurState& S) {
  F3 rx[D], ro[BLEND == 2 ? D : 1];
  const ptrdiff_t hop = back ? -(ptrdiff_t)N : (ptrdiff_t)N;
  const size_t row0 = back ? (size_t)(L - 1) * N : 0;
  const float* ps = src + row0;                                // the next frame to request
  const float* po = (BLEND == 2 ? orig : src) + row0;
  float* pd = dst + row0;                                      // the next frame to write
  const auto request = [&](int j) {
    rx[j] = tr_load(ps);
    ps += hop;
    if (BLEND == 2) { ro[j] = tr_load(po); po += hop; }
  };
  const auto frame = [&](const F3& x, const F3& o) {           // x: the walk's current frame; o: what the result is blended into
    recur_step<KIND>(x, S, fresh, q);
    fresh = false;
    F3 out = S.y;
    if (BLEND != 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out.a[c] = s == 0.f ? o.a[c] : __fadd_rn(o.a[c], __fmul_rn(s, __fsub_rn(S.y.a[c], o.a[c])));
    }
    tr_store(pd, out);
    pd += hop;
  };
#pragma unroll
  for (int j = 0; j < D; ++j)
    if (j < L) request(j);
  int i0 = 0;
  for (; i0 + 2 * D <= L; i0 += D) {
    F3 cx[D], co[BLEND == 2 ? D : 1];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      cx[j] = rx[j];
      if (BLEND == 2) co[j] = ro[j];
      request(j);
    }
    __builtin_amdgcn_sched_barrier(0);                         // the D requests stay ahead of the D frames' arithmetic, which is free to interleave
#pragma unroll
    for (int j = 0; j < D; ++j) frame(cx[j], BLEND == 2 ? co[j] : cx[j]);
  }
  for (; i0 < L; i0 += D) {                                    // (at most twice; the conditions are uniform over the wave: L is the clip's)
#pragma unroll
    for (int j = 0; j < D; ++j)
      if (i0 + j < L) {
        const F3 x = rx[j], o = BLEND == 2 ? ro[j] : x;
        if (i0 + j + D < L) request(j);
        frame(x, o);
      }
  }
}

// grid (vertex chunks of TR_VERTS, B); lens: L per clip; strength: [V] or null; st [B][3][N] and seen [B], or both null; x and y do not
// overlap (y is read back by the second walk of zero_phase, so it is not __restrict__)
template <int KIND, int D>
__global__ __launch_bounds__(TR_VERTS) void time_recur_kernel(const float* __restrict__ x, const int* __restrict__ lens, int L_max, int V, RecurCoef q,
                                                              const float* __restrict__ strength, int direction, float* st, const int* __restrict__ seen,
                                                              float* y) {
  const int v = blockIdx.x * TR_VERTS + threadIdx.x, b = blockIdx.y;
  if (v >= V) return;
  const size_t N = 3 * (size_t)V;
  const int L = lens[b];
  const float* xb = x + (size_t)b * L_max * N + 3 * (size_t)v;
  float* yb = y + (size_t)b * L_max * N + 3 * (size_t)v;
  for (int t = L; t < L_max; ++t) tr_store(yb + (size_t)t * N, {{0.f, 0.f, 0.f}});
  if (L == 0) return;
  const float s = strength ? strength[v] : 1.f;
  RecurState S = {{{0.f, 0.f, 0.f}}, {{0.f, 0.f, 0.f}}, {{0.f, 0.f, 0.f}}};
  if (direction == TR_ZERO_PHASE) {
    recur_walk<KIND, D, 0>(xb, nullptr, yb, L, N, false, true, s, q, S);
    if (strength) recur_walk<KIND, D, 2>(yb, xb, yb, L, N, true, true, s, q, S);
    else recur_walk<KIND, D, 0>(yb, nullptr, yb, L, N, true, true, s, q, S);
    return;
  }
  float* sb = st ? st + (size_t)b * 3 * N + 3 * (size_t)v : nullptr;
  bool fresh = true;
  if (sb && seen[b] > 0) {
    fresh = false;
    S.y = tr_load(sb);
    if (KIND == TR_ONE_EURO) { S.xp = tr_load(sb + N); S.dh = tr_load(sb + 2 * N); }
  }
  if (strength) recur_walk<KIND, D, 1>(xb, nullptr, yb, L, N, false, fresh, s, q, S);
  else recur_walk<KIND, D, 0>(xb, nullptr, yb, L, N, false, fresh, s, q, S);
  if (sb) {
    tr_store(sb, S.y);
    if (KIND == TR_ONE_EURO) { tr_store(sb + N, S.xp); tr_store(sb + 2 * N, S.dh); }
  }
}

// seen[b] += lens[b] (saturating), after time_recur_kernel on the same stream
__global__ void time_recur_seen_kernel(int* __restrict__ seen, const int* __restrict__ lens, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int s = seen[b], L = lens[b];
  seen[b] = s > 0x7fffffff - L ? 0x7fffffff : s + L;
}

}  // namespace fdm
