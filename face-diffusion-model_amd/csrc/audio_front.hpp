// Kernels of the audio front end (include/fdm_hip.h, fdm_frontend_*; launched by frontend.hip): raw PCM -> 16 kHz mono fp32,
// processor-normalised and zero-padded, for a group of clips of unequal length, rate, format and channel count per launch.
//   front_resample_kernel   grid (tiles of n_max, clips): one workgroup = FRONT_TILE consecutive outputs of one clip.  It stages the
//                           input span those outputs need in LDS, converting and downmixing on the load (the converted waveform never
//                           goes to memory), at most FRONT_SPAN samples per pass; every thread then walks the taps of its own phase,
//                           (half + j down) mod up, which the phase-major table holds contiguously.  Sum over ascending input index in
//                           fp64 (an fp32 x fp32 product is exact there), rounded once: y[j] is a function of the clip alone -- passes,
//                           tile and batch only decide who computes it.  Outputs from n_out to n_max are written as zeros.
//   front_sum_kernel        grid (chunks, clips): fp64 sum of one chunk of a clip's n_out samples
//   front_var_kernel        grid (chunks, clips): folds the sums in chunk order -> mean; fp64 sum of (y - mean)^2 over its chunk
//   front_norm_kernel       grid (chunks, clips): folds both partial rows in chunk order, normalises its chunk in place
// Chunk count and width are functions of n_out alone (front_chunks_of), reductions inside a workgroup are fixed trees: no atomics,
// the same bits in every batch.  None of these kernels has been timed (profiles/audio_frontend/README.md).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fdm_hip.h"

namespace fdm {

constexpr int FRONT_TILE = 256;           // outputs per workgroup (= threads)
constexpr int FRONT_SPAN = 4096;          // input samples staged in LDS per pass (16 KB)
constexpr int FRONT_GROUP = 16;           // clips per launch (their descriptors travel as a kernel argument)
constexpr int FRONT_CHUNK = 4096;         // samples per statistics chunk up to FRONT_CHUNKS_MAX chunks, wider chunks beyond
constexpr int FRONT_CHUNKS_MAX = 1024;

struct FrontClip {
  const void* data;          // interleaved PCM, device
  const float* taps;         // [up][Q] phase-major taps, device (unused when up == down == 1)
  long long frames, n_out;
  int format, channels, up, down, half, Q;
  int pad0, pad1;
};
struct FrontPack { FrontClip c[FRONT_GROUP]; };

// statistics chunks of a clip of n samples: count (return) and width, from n alone
__host__ __device__ inline int front_chunks_of(long long n, long long* width) {
  long long nch = (n + FRONT_CHUNK - 1) / FRONT_CHUNK;
  nch = nch < 1 ? 1 : (nch > FRONT_CHUNKS_MAX ? FRONT_CHUNKS_MAX : nch);
  *width = ((n + nch - 1) / nch + 255) / 256 * 256;
  return (int)nch;
}

// sample frame i of a clip as mono fp32: convert (exact), then ((c0 + c1) + c2 ...) / channels
__device__ __forceinline__ float front_pcm(const void* d, int format, long long o) {
  if (format == FDM_PCM_S16) return (float)((const short*)d)[o] * (1.f / 32768.f);
  if (format == FDM_PCM_S32) return (float)((const int*)d)[o] * (1.f / 2147483648.f);
  if (format == FDM_PCM_U8) return ((float)((const unsigned char*)d)[o] - 128.f) * (1.f / 128.f);
  return ((const float*)d)[o];
}
__device__ __forceinline__ float front_sample(const FrontClip& c, long long i) {
  const long long o = i * c.channels;
  float s = front_pcm(c.data, c.format, o);
  if (c.channels == 1) return s;
  for (int ch = 1; ch < c.channels; ++ch) s += front_pcm(c.data, c.format, o + ch);
  return s / (float)c.channels;
}

__global__ __launch_bounds__(FRONT_TILE) void front_resample_kernel(float* wav, long long n_max, int b0, FrontPack pk) {
  __shared__ float xs[FRONT_SPAN];
  const FrontClip& c = pk.c[blockIdx.y];
  float* out = wav + (size_t)(b0 + blockIdx.y) * (size_t)n_max;
  const int tid = threadIdx.x;
  const long long j0 = (long long)blockIdx.x * FRONT_TILE, j = j0 + tid;
  if (j0 >= c.n_out) {                      // (uniform over the workgroup) a tile of padding
    if (j < n_max) out[j] = 0.f;
    return;
  }
  const bool live = j < c.n_out;
  if (c.up == c.down) {                     // 16 kHz: no filter
    if (j < n_max) out[j] = live ? front_sample(c, j) : 0.f;
    return;
  }
  const int up = c.up, down = c.down, half = c.half;
  // tap index of input i for output j: half + j down - i up = p + (q0 - i) up with q0 = (half + j down) div up, p = the remainder
  const long long base = (long long)half + j0 * down, qb = base / up;
  const int t = (int)(base - qb * up) + tid * down;          // < up + 255 * down
  const long long q0 = qb + t / up;
  const int p = t % up, qmax = (2 * half - p) / up;
  const long long ilo = q0 - qmax > 0 ? q0 - qmax : 0, ihi = q0 < c.frames - 1 ? q0 : c.frames - 1;
  // inputs the tile's live outputs touch
  const long long jl = (j0 + FRONT_TILE < c.n_out ? j0 + FRONT_TILE : c.n_out) - 1;
  const long long lo_raw = qb - (2 * half) / up, hi_raw = ((long long)half + jl * down) / up;
  const long long tlo = lo_raw > 0 ? lo_raw : 0, thi = hi_raw < c.frames - 1 ? hi_raw : c.frames - 1;
  const float* tp = c.taps + (size_t)p * c.Q;
  double acc = 0.0;
  for (long long s0 = tlo; s0 <= thi; s0 += FRONT_SPAN) {
    const long long s1 = s0 + FRONT_SPAN - 1 < thi ? s0 + FRONT_SPAN - 1 : thi;
    const int cnt = (int)(s1 - s0) + 1;
    for (int k = tid; k < cnt; k += FRONT_TILE) xs[k] = front_sample(c, s0 + k);
    __syncthreads();
    if (live) {
      const long long a = ilo > s0 ? ilo : s0, e = ihi < s1 ? ihi : s1;
      if (a <= e) {
        const int k0 = (int)(a - s0), k1 = (int)(e - s0);
        int q = (int)(q0 - a);
        for (int k = k0; k <= k1; ++k, --q) acc += (double)xs[k] * (double)tp[q];
      }
    }
    __syncthreads();
  }
  if (j < n_max) out[j] = live ? (float)acc : 0.f;
}

// fixed tree over the workgroup's 256 partial sums (every thread returns the total)
__device__ __forceinline__ double front_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
// (thread 0) fold a clip's nch partials in chunk order
__device__ __forceinline__ double front_fold(const double* part, int nch) {
  double s = 0.0;
  for (int i = 0; i < nch; ++i) s += part[(size_t)i * 2];
  return s;
}

// part: [FRONT_GROUP][FRONT_CHUNKS_MAX][2] doubles = {sum, sum of squared deviations} per (clip of the group, chunk)
__global__ __launch_bounds__(256) void front_sum_kernel(const float* wav, long long n_max, int b0, double* part, FrontPack pk) {
  __shared__ double red[256];
  const long long n = pk.c[blockIdx.y].n_out;
  long long width;
  const int nch = front_chunks_of(n, &width), ck = blockIdx.x;
  if (ck >= nch) return;
  const float* x = wav + (size_t)(b0 + blockIdx.y) * (size_t)n_max;
  const long long i1 = (ck + 1) * width < n ? (ck + 1) * width : n;
  double s = 0.0;
  for (long long i = ck * width + threadIdx.x; i < i1; i += 256) s += (double)x[i];
  s = front_block_sum(s, red);
  if (threadIdx.x == 0) part[((size_t)blockIdx.y * FRONT_CHUNKS_MAX + ck) * 2] = s;
}
__global__ __launch_bounds__(256) void front_var_kernel(const float* wav, long long n_max, int b0, double* part, FrontPack pk) {
  __shared__ double red[256];
  __shared__ double mean_s;
  const long long n = pk.c[blockIdx.y].n_out;
  long long width;
  const int nch = front_chunks_of(n, &width), ck = blockIdx.x;
  if (ck >= nch) return;
  double* row = part + (size_t)blockIdx.y * FRONT_CHUNKS_MAX * 2;
  if (threadIdx.x == 0) mean_s = front_fold(row, nch) / (double)n;
  __syncthreads();
  const double mean = mean_s;
  const float* x = wav + (size_t)(b0 + blockIdx.y) * (size_t)n_max;
  const long long i1 = (ck + 1) * width < n ? (ck + 1) * width : n;
  double s = 0.0;
  for (long long i = ck * width + threadIdx.x; i < i1; i += 256) { const double d = (double)x[i] - mean; s += d * d; }
  s = front_block_sum(s, red);
  if (threadIdx.x == 0) row[(size_t)ck * 2 + 1] = s;
}
__global__ __launch_bounds__(256) void front_norm_kernel(float* wav, long long n_max, int b0, const double* part, FrontPack pk) {
  __shared__ double st[2];
  const long long n = pk.c[blockIdx.y].n_out;
  long long width;
  const int nch = front_chunks_of(n, &width), ck = blockIdx.x;
  if (ck >= nch) return;
  const double* row = part + (size_t)blockIdx.y * FRONT_CHUNKS_MAX * 2;
  if (threadIdx.x == 0) {
    st[0] = front_fold(row, nch) / (double)n;
    st[1] = sqrt(front_fold(row + 1, nch) / (double)n + 1e-7);
  }
  __syncthreads();
  const double mean = st[0], sd = st[1];
  float* x = wav + (size_t)(b0 + blockIdx.y) * (size_t)n_max;
  const long long i1 = (ck + 1) * width < n ? (ck + 1) * width : n;
  for (long long i = ck * width + threadIdx.x; i < i1; i += 256) x[i] = (float)(((double)x[i] - mean) / sd);
}

}  // namespace fdm
