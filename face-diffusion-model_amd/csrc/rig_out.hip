// Rig hand-off behind plain C calls (include/fdm_hip.h, fdm_rig_*): vertex offsets as fdm_vq_decode(_ragged) writes them -> blendshape
// coefficients per frame (a ridge-regularised, box-constrained least-squares fit onto a basis), at the consumer's frame rate.
// Kernels: rig_out.hpp.  fdm_rig_create does the fp64 work on the host (the weighted basis, its Gram matrix and Cholesky factor) and
// uploads fp32 copies; a forward call validates (every check before the first launch), grows the scratch when a call is larger
// than any before it, and launches the projection and the solve.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "host.hpp"
#include "rig_out.hpp"

struct fdm_rig : fdm::Handoff {           // lens: {L, L_out} per clip
  int K = 0, V = 0, sweeps = 0, chunks = 0;
  bool bounded = false;
  float *P = nullptr, *G = nullptr, *Lc = nullptr, *lo = nullptr, *hi = nullptr;      // device: [K][chunks * ROW_CHUNK], [K][K] x 2, [K] x 2
  float* part = nullptr;        // partial sums of the call in flight [chunks][B * L_max][K]
  long long part_cap = 0;
};

namespace {
using namespace fdm;

// everything fdm_rig_gram_host and fdm_rig_create share: the basis, the weights and the ridge
int check_basis(const char* who, const float* basis, const float* vweight, int K, int V, double ridge) {
  if (!basis) return fail(FDM_ERR_ARG, "%s: null basis", who);
  if (K < 1 || K > RIG_KMAX || V < 1) return fail(FDM_ERR_ARG, "%s: K = %d (1..%d), V = %d", who, K, RIG_KMAX, V);
  if (V > 0x7fffffff / 3 - ROW_CHUNK) return fail(FDM_ERR_ARG, "%s: V = %d (3 V is a 32-bit int)", who, V);
  if (!(ridge >= 0.0) || std::isinf(ridge)) return fail(FDM_ERR_ARG, "%s: ridge = %g (finite and >= 0)", who, ridge);
  if (vweight)
    for (int v = 0; v < V; ++v)
      if (!(vweight[v] >= 0.f) || std::isinf(vweight[v])) return fail(FDM_ERR_ARG, "%s: weight %d = %g (finite and >= 0)", who, v, (double)vweight[v]);
  return FDM_OK;
}

size_t solve_lds(int K) { return ((size_t)K * K + (size_t)K * (K | 1) + 2 * (size_t)K) * sizeof(float); }

}  // namespace

extern "C" {

int fdm_rig_gram_host(const float* basis, const float* vweight, int K, int V, double ridge, double* gram, float* chol) {
  if (!gram || !chol) return fail(FDM_ERR_ARG, "rig_gram: null argument");
  FCK(check_basis("rig_gram", basis, vweight, K, V, ridge));
  const long long V3 = 3LL * V;
  std::vector<double> ew((size_t)V3);                       // row a of E diag(w), exact in fp64
  for (int a = 0; a < K; ++a) {
    const float* ea = basis + a * V3;
    for (long long i = 0; i < V3; ++i) ew[i] = (double)ea[i] * (vweight ? (double)vweight[i / 3] : 1.0);
    for (int b = 0; b <= a; ++b) {
      const float* eb = basis + b * V3;
      double s = 0.0;
      for (long long i = 0; i < V3; ++i) s += ew[i] * (double)eb[i];
      if (a == b) s += ridge;
      gram[(size_t)a * K + b] = gram[(size_t)b * K + a] = s;
    }
  }
  std::vector<double> l((size_t)K * K, 0.0);                // Cholesky-Banachiewicz, row by row
  for (int i = 0; i < K; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = gram[(size_t)i * K + j];
      for (int q = 0; q < j; ++q) s -= l[(size_t)i * K + q] * l[(size_t)j * K + q];
      if (i == j) {
        // (a pivot that is rounding noise of the fp64 subtractions, K 2^-52 of its diagonal element, counts as 0)
        if (!(s > gram[(size_t)i * K + i] * K * 0x1p-52) || !std::isfinite(s)) return fail(FDM_ERR_ARG, "rig_gram: basis is rank deficient under these weights: raise ridge (pivot %d = %g)", i, s);
        l[(size_t)i * K + i] = std::sqrt(s);
      } else {
        l[(size_t)i * K + j] = s / l[(size_t)j * K + j];
      }
    }
  for (size_t i = 0; i < (size_t)K * K; ++i) {
    chol[i] = (float)l[i];
    if (!std::isfinite(chol[i]) || !std::isfinite((float)gram[i]))
      return fail(FDM_ERR_ARG, "rig_gram: basis is rank deficient under these weights: raise ridge (element %zu does not fit fp32)", i);
  }
  for (int i = 0; i < K; ++i)
    if (!(chol[(size_t)i * K + i] > 0.f)) return fail(FDM_ERR_ARG, "rig_gram: basis is rank deficient under these weights: raise ridge (pivot %d rounds to 0)", i);
  return FDM_OK;
}

int fdm_rig_create(const float* basis, int K, int V, const float* vweight, double ridge, const float* lo, const float* hi, int sweeps,
                   fdm_rig** out) {
  if (!out) return fail(FDM_ERR_ARG, "rig_create: null out");
  FCK(check_basis("rig_create", basis, vweight, K, V, ridge));
  if (!lo != !hi) return fail(FDM_ERR_ARG, "rig_create: bounds need both lo and hi");
  if (lo)
    for (int k = 0; k < K; ++k)
      if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || lo[k] > hi[k])
        return fail(FDM_ERR_ARG, "rig_create: bounds of coefficient %d are [%g, %g] (finite, lo <= hi)", k, (double)lo[k], (double)hi[k]);
  if (sweeps < 0) return fail(FDM_ERR_ARG, "rig_create: sweeps = %d", sweeps);
  std::vector<double> gram((size_t)K * K);
  std::vector<float> chol((size_t)K * K), g32((size_t)K * K);
  FCK(fdm_rig_gram_host(basis, vweight, K, V, ridge, gram.data(), chol.data()));
  for (size_t i = 0; i < gram.size(); ++i) g32[i] = (float)gram[i];
  fdm_rig* R = new (std::nothrow) fdm_rig();
  if (!R) return fail(FDM_ERR_STATE, "rig_create: out of memory");
  const long long V3 = 3LL * V;
  R->K = K; R->V = V; R->sweeps = sweeps; R->bounded = lo != nullptr;
  R->chunks = (int)((V3 + ROW_CHUNK - 1) / ROW_CHUNK);
  return handoff_finish(R, out, [&]() {
    const size_t ldp = (size_t)R->chunks * ROW_CHUNK;
    std::vector<float> P((size_t)K * ldp, 0.f);             // E diag(w) rounded to fp32, rows padded with zeros to whole chunks
    for (int k = 0; k < K; ++k)
      for (long long i = 0; i < V3; ++i)
        P[k * ldp + i] = (float)((double)basis[k * V3 + i] * (vweight ? (double)vweight[i / 3] : 1.0));
    FCK(put(R->mem, &R->P, P.data(), P.size()));
    FCK(put(R->mem, &R->G, g32.data(), g32.size()));
    FCK(put(R->mem, &R->Lc, chol.data(), chol.size()));
    if (lo) { FCK(put(R->mem, &R->lo, lo, (size_t)K)); FCK(put(R->mem, &R->hi, hi, (size_t)K)); }
    HIPCK(hipFuncSetAttribute((const void*)rig_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)solve_lds(RIG_KMAX)));
    return (int)FDM_OK;
  });
}

int fdm_rig_destroy(fdm_rig* R) { return handoff_destroy(R); }

int fdm_rig_forward(fdm_rig* R, const float* offsets, const int* frames, int B, int L_max, double fps_in, double fps_out, float* coef,
                    float* proj, int L_out_max, int* frames_out, void* stream) {
  if (!R || !offsets || !coef) return fail(FDM_ERR_ARG, "rig_forward: null argument");
  FCK(check_fps("rig_forward", fps_in, fps_out));
  if (B < 1 || L_max < 1 || L_out_max < 1) return fail(FDM_ERR_SHAPE, "rig_forward: B = %d, L_max = %d, L_out_max = %d", B, L_max, L_out_max);
  std::vector<int> hl;
  const ClipLens c = clip_lens(frames, B, L_max, fps_in, fps_out, L_out_max, hl);
  if (c.bad == ClipLens::LENGTH) return fail(FDM_ERR_SHAPE, "rig_forward: clip %d has %d frames, the batch is %d long", c.clip, c.L, L_max);
  if (c.bad == ClipLens::OUTPUT)
    return fail(FDM_ERR_SHAPE, "rig_forward: clip %d of %d frames at %g -> %g fps does not fit an output %d long", c.clip, c.L, fps_in, fps_out, L_out_max);
  const long long rows_in = (long long)B * L_max, rows_out = (long long)B * L_out_max;
  if (rows_in > 0x7fffffffLL - ROW_TILE || rows_out > 0x7fffffffLL - RIG_SW || R->chunks > 65535)
    return fail(FDM_ERR_SHAPE, "rig_forward: %lld input and %lld output rows of %d vertices exceed one launch", rows_in, rows_out, R->V);
  FCK(handoff_device(*R, "rig_forward"));
  hipStream_t s = (hipStream_t)stream;
  FCK(grow(R->mem, &R->part, &R->part_cap, (long long)R->chunks * rows_in * R->K));
  FCK(handoff_lens(*R, hl, s));
  const dim3 gp((unsigned)((rows_in + ROW_TILE - 1) / ROW_TILE), (unsigned)R->chunks);
  hipLaunchKernelGGL(rig_proj_kernel, gp, dim3(256), 0, s, offsets, (const int*)R->lens, L_max, (int)rows_in, 3 * R->V, (const float*)R->P,
                     R->chunks * ROW_CHUNK, R->K, R->part);
  const dim3 gs((unsigned)((rows_out + RIG_SW - 1) / RIG_SW));
  hipLaunchKernelGGL(rig_solve_kernel, gs, dim3(RIG_SW * 64), solve_lds(R->K), s, (const float*)R->part, R->chunks, (int)rows_in, (const int*)R->lens,
                     L_max, L_out_max, (int)rows_out, R->K, resamples(fps_in, fps_out) ? 1 : 0, (const float*)R->G, (const float*)R->Lc,
                     (const float*)R->lo, (const float*)R->hi, R->bounded ? 1 : 0, R->sweeps, coef, proj);
  HIPCK(hipGetLastError());
  if (frames_out) for (int b = 0; b < B; ++b) frames_out[b] = hl[2 * b + 1];
  return FDM_OK;
}

}  // extern "C"
