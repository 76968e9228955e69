// Time filter hand-off (include/fdm_hip.h, fdm_tfilter_*): a zero-phase FIR filter of the decoded offsets along
// time, per clip at its own length.  One kernel, one body: fixed and ragged batches, with and without a per-vertex strength, both edge
// rules.  The definition, stated once:
//   x [B, L_max, N] fp32, N = 3 V; L per clip (1 <= L <= L_max); half-taps h[0..R], 0 <= R <= TF_RMAX, the full kernel symmetric.
//   e(i) of a clip of L frames -- mirror (TF_MIRROR): L == 1: 0; else p = 2 (L - 1), m = ((i mod p) + p) mod p, e = m < L ? m : p - m
//   (the end sample is not repeated; any R against any L); nearest (TF_NEAREST): e = min(max(i, 0), L - 1).
//   f(t, n): acc = h[0] x[t][n]; for k = 1 .. R: acc = acc + h[k] (x[e(t - k)][n] + x[e(t + k)][n]) -- the pair is summed first, every
//   operation rounded on its own (no contraction): filtering a time-reversed clip gives the time-reversed result bit for bit.
//   y = f without a strength; with s_v of column n's vertex: y = x where s_v == 0 (a copy), else d = f - x, y = x + s_v d (three rounded
//   operations).  Rows at or past L are written as zeros; input rows at or past L are never read.  A clip's bits do not depend on the
//   batch, L_max or a tile size: every element is the fixed chain above.  No atomics.
// Tiling: a workgroup of TF_THREADS owns TF_CHUNK columns and TF_TILE output frames of one clip.  It stages the tile's live rows and
// their 2 R halo rows in LDS -- row j of the image is frame e(t0 - R + j), so the edge rule is applied once, at the load, by the 16-byte
// peel of handoff.hpp (a row starts on a 4-byte boundary only) -- then every thread computes 4 columns of TF_RPT frames from aligned
// 16-byte LDS reads, TF_PASS frames a pass, into a staging image from which the peel stores 16-byte pieces.  Halo rows are read again
// by the neighbouring tile (from L2): 2 R rows on TF_TILE, one third of the rows read at R = 32, 6 % at R = 4.
#pragma once
#include <hip/hip_runtime.h>

#include "handoff.hpp"

namespace fdm {

constexpr int TF_RMAX = 32;                       // half-taps h[0..R], R <= TF_RMAX
constexpr int TF_MIRROR = 0, TF_NEAREST = 1;      // FDM_TFILTER_MIRROR / FDM_TFILTER_NEAREST
constexpr int TF_CHUNK = 96;                      // columns per workgroup: 24 pieces of 16 bytes, a multiple of 3 (chunks end on vertices)
constexpr int TF_TILE = 128;                      // output frames per workgroup
constexpr int TF_THREADS = 192;                   // 24 column pieces x 8 frame slots; 6 groups of 32 lanes walk rows at load and store
constexpr int TF_RPT = 2;                         // frames per thread and pass
constexpr int TF_PASS = TF_THREADS / (TF_CHUNK / 4) * TF_RPT;      // 16 frames per pass
constexpr int TF_TAPS_LDS = 36;                   // TF_RMAX + 1 taps, rounded up to 16 bytes
static_assert(TF_CHUNK % 12 == 0 && TF_THREADS % (TF_CHUNK / 4) == 0 && TF_THREADS % 32 == 0 && TF_TILE % TF_PASS == 0, "time filter tiling");

// dynamic LDS of a launch at radius R: the image, the staging rows, the taps, the chunk's strengths
constexpr size_t tfilter_lds(int R) { return ((size_t)(TF_TILE + 2 * R + TF_PASS + 1) * TF_CHUNK + TF_TAPS_LDS) * sizeof(float); }
static_assert(2 * tfilter_lds(TF_RMAX) <= 160 * 1024, "two workgroups per CU at the largest radius");

__device__ __forceinline__ int tfilter_edge(int i, int L, int edge) {
  if (edge == TF_NEAREST) return min(max(i, 0), L - 1);
  if (L == 1) return 0;
  const int p = 2 * (L - 1), m = ((i % p) + p) % p;
  return m < L ? m : p - m;
}

// grid (column chunks, frame tiles of L_max, B); lens: L per clip; strength: [V] or null; x and y do not overlap
__global__ __launch_bounds__(TF_THREADS) void time_filter_kernel(const float* __restrict__ x, const int* __restrict__ lens, int L_max, int N,
                                                                 const float* __restrict__ taps, int R, int edge,
                                                                 const float* __restrict__ strength, float* __restrict__ y) {
  extern __shared__ float4 tf_lds[];                         // (16-byte aligned: the image and the staging rows are read and written as float4)
  float* img = reinterpret_cast<float*>(tf_lds);             // [TF_TILE + 2 R][TF_CHUNK]
  float* stage = img + (TF_TILE + 2 * R) * TF_CHUNK;         // [TF_PASS][TF_CHUNK]
  float* sh = stage + TF_PASS * TF_CHUNK;                    // [TF_TAPS_LDS]
  float* ss = sh + TF_TAPS_LDS;                              // [TF_CHUNK]
  const int tid = threadIdx.x, b = blockIdx.z, t0 = blockIdx.y * TF_TILE, c0 = blockIdx.x * TF_CHUNK;
  const int nc = min(TF_CHUNK, N - c0), rows_here = min(TF_TILE, L_max - t0);
  const int L = lens[b], nl = min(max(L - t0, 0), rows_here);                  // live frames of this tile
  const float* xb = x + (size_t)b * L_max * N + c0;
  float* yb = y + ((size_t)b * L_max + t0) * N + c0;
  const int grp = tid >> 5, lane = tid & 31;

  if (nl > 0) {                                              // (uniform over the workgroup)
    for (int j = grp; j < nl + 2 * R; j += TF_THREADS / 32) {
      const float* src = xb + (size_t)tfilter_edge(t0 - R + j, L, edge) * N;
      peel_walk<32, 28>(peel_of(src, nc), nc, lane, PeelLoad{src, img + j * TF_CHUNK});
    }
    if (tid <= R) sh[tid] = taps[tid];
    if (tid < TF_CHUNK) ss[tid] = (strength && tid < nc) ? strength[(c0 + tid) / 3] : 1.f;
  }
  __syncthreads();

  const int c4 = tid % (TF_CHUNK / 4), slot = tid / (TF_CHUNK / 4);
  for (int p0 = 0; p0 < rows_here; p0 += TF_PASS) {
#pragma unroll
    for (int i = 0; i < TF_RPT; ++i) {
      const int r = slot + i * (TF_PASS / TF_RPT), t = p0 + r;                 // frame t0 + t of the clip
      int bb;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < rows_here && row_live(lens, 1, 0, b * L_max + t0 + t, L_max, bb)) {
        const float4* ctr = reinterpret_cast<const float4*>(img + (t + R) * TF_CHUNK) + c4;
        const float4 xc = *ctr;
        const float h0 = sh[0];
        float4 acc = make_float4(__fmul_rn(h0, xc.x), __fmul_rn(h0, xc.y), __fmul_rn(h0, xc.z), __fmul_rn(h0, xc.w));
        for (int k = 1; k <= R; ++k) {
          const float hk = sh[k];
          const float4 lo = *(ctr - k * (TF_CHUNK / 4)), hi = *(ctr + k * (TF_CHUNK / 4));
          acc.x = __fadd_rn(acc.x, __fmul_rn(hk, __fadd_rn(lo.x, hi.x)));
          acc.y = __fadd_rn(acc.y, __fmul_rn(hk, __fadd_rn(lo.y, hi.y)));
          acc.z = __fadd_rn(acc.z, __fmul_rn(hk, __fadd_rn(lo.z, hi.z)));
          acc.w = __fadd_rn(acc.w, __fmul_rn(hk, __fadd_rn(lo.w, hi.w)));
        }
        o = acc;
        if (strength) {
          const float4 s = *(reinterpret_cast<const float4*>(ss) + c4);
          o.x = s.x == 0.f ? xc.x : __fadd_rn(xc.x, __fmul_rn(s.x, __fsub_rn(acc.x, xc.x)));
          o.y = s.y == 0.f ? xc.y : __fadd_rn(xc.y, __fmul_rn(s.y, __fsub_rn(acc.y, xc.y)));
          o.z = s.z == 0.f ? xc.z : __fadd_rn(xc.z, __fmul_rn(s.z, __fsub_rn(acc.z, xc.z)));
          o.w = s.w == 0.f ? xc.w : __fadd_rn(xc.w, __fmul_rn(s.w, __fsub_rn(acc.w, xc.w)));
        }
      }
      *(reinterpret_cast<float4*>(stage + r * TF_CHUNK) + c4) = o;
    }
    __syncthreads();
    for (int r = grp; r < min(TF_PASS, rows_here - p0); r += TF_THREADS / 32) {
      float* dst = yb + (size_t)(p0 + r) * N;
      peel_walk<32, 28>(peel_of(dst, nc), nc, lane, PeelStore{dst, stage + r * TF_CHUNK});
    }
    __syncthreads();
  }
}

}  // namespace fdm
