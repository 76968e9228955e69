// Rig hand-off behind plain C calls (include/fdm_hip.h, fdm_rig_*): vertex offsets as fdm_vq_decode(_ragged) writes them -> blendshape
// coefficients per frame (a ridge-regularised, box-constrained least-squares fit onto a basis), at the consumer's frame rate.
// Kernels: rig_out.hpp.  fdm_rig_create does the fp64 work on the host (the weighted basis, its Gram matrix and Cholesky factor) and
// uploads fp32 copies; a forward call validates (every check before the first launch), grows the scratch when a call is larger
// than any before it, and launches the projection and the solve.  fdm_rig_set_temporal couples a clip's frames (DESIGN section 2 item
// 21): its tables come from fdm_rig_temporal_tables_host (fp64, a cyclic Jacobi eigen-decomposition written here), and forward then
// launches the projection, the modal transform, the solve along time, the transform back and two launches per sweep.
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
  // the temporal fit (fdm_rig_set_temporal); temporal = false: the per-frame path, nothing below is read
  std::vector<double> gram;     // G in fp64, kept for the tables
  bool temporal = false;
  float *Q = nullptr, *QT = nullptr, *lam = nullptr, *mvec = nullptr;                  // device: [K][K] x 2, [K] x 2
  float* tbuf = nullptr;        // r, z / u / y and 1 / w of the call in flight, [3][B * L_out_max][K]
  long long tbuf_cap = 0;
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
size_t modal_lds(int K) { return (size_t)K * K * sizeof(float); }
size_t sweep_lds(int K) { return ((size_t)K * K + 3 * (size_t)K) * sizeof(float); }

// Eigen-decomposition of the symmetric a [n][n] by cyclic Jacobi rotations (Rutishauser's update: the rotation angle from
// t = tan, the smaller root).  a is destroyed (its diagonal ends as the eigenvalues), u [n][n] ends with the eigenvectors in its
// columns.  A rotation is skipped once |a_pq| is below 2^-56 of sqrt(|a_pp a_qq|); the loop ends with a sweep that rotates nothing.
// Each column of u has then been through some thousand rotations, and u^T u is off the identity by their accumulated rounding: one
// Newton-Schulz step u <- u (3 I - u^T u) / 2 squares that distance away, and the eigenvalues are taken again as Rayleigh quotients
// of the matrix that came in.
void jacobi_eigen(std::vector<double>& a, std::vector<double>& u, int n) {
  const std::vector<double> a0 = a;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) u[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    int rotated = 0;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[(size_t)p * n + q], app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
        if (!(std::fabs(apq) > 0x1p-56 * std::sqrt(std::fabs(app * aqq)))) continue;
        ++rotated;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {                       // columns p and q of a, then its rows: a <- J^T a J
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = c * akp - s * akq;
          a[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = c * apk - s * aqk;
          a[(size_t)q * n + k] = s * apk + c * aqk;
        }
        a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
        for (int k = 0; k < n; ++k) {
          const double ukp = u[(size_t)k * n + p], ukq = u[(size_t)k * n + q];
          u[(size_t)k * n + p] = c * ukp - s * ukq;
          u[(size_t)k * n + q] = s * ukp + c * ukq;
        }
      }
    if (!rotated) break;
  }
  std::vector<double> h((size_t)n * n), v((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int k = 0; k < n; ++k) s += u[(size_t)k * n + i] * u[(size_t)k * n + j];
      h[(size_t)i * n + j] = (i == j ? 1.5 : 0.0) - 0.5 * s;
    }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int k = 0; k < n; ++k) s += u[(size_t)i * n + k] * h[(size_t)k * n + j];
      v[(size_t)i * n + j] = s;
    }
  u = v;
  for (int i = 0; i < n; ++i)                                // h = a0 u
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int k = 0; k < n; ++k) s += a0[(size_t)i * n + k] * u[(size_t)k * n + j];
      h[(size_t)i * n + j] = s;
    }
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += u[(size_t)k * n + j] * h[(size_t)k * n + j];
    a[(size_t)j * n + j] = s;
  }
}

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

int fdm_rig_temporal_tables_host(const double* gram, int K, double smooth, const float* sweights, double* lam, double* Q) {
  if (!gram || !lam || !Q) return fail(FDM_ERR_ARG, "rig_temporal_tables: null argument");
  if (K < 1 || K > RIG_KMAX) return fail(FDM_ERR_ARG, "rig_temporal_tables: K = %d (1..%d)", K, RIG_KMAX);
  if (!(smooth > 0.0) || std::isinf(smooth)) return fail(FDM_ERR_ARG, "rig_temporal_tables: smooth = %g (finite and > 0; 0 is the per-frame fit and has no tables)", smooth);
  std::vector<double> d((size_t)K);
  for (int k = 0; k < K; ++k) {
    const double m = sweights ? (double)sweights[k] : 1.0;
    if (!(m > 0.0) || std::isinf(m)) return fail(FDM_ERR_ARG, "rig_temporal_tables: smoothing weight %d = %g (finite and > 0)", k, m);
    d[k] = 1.0 / std::sqrt(smooth * m);
    if (!std::isfinite(d[k]) || !(d[k] > 0.0)) return fail(FDM_ERR_ARG, "rig_temporal_tables: smooth * weight %d = %g is out of range", k, smooth * m);
  }
  std::vector<double> a((size_t)K * K), u((size_t)K * K);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) {
      a[(size_t)i * K + j] = d[i] * gram[(size_t)i * K + j] * d[j];
      if (!std::isfinite(a[(size_t)i * K + j])) return fail(FDM_ERR_ARG, "rig_temporal_tables: element %d, %d of D G D is not finite", i, j);
    }
  jacobi_eigen(a, u, K);
  std::vector<int> order((size_t)K);
  for (int k = 0; k < K; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * K + x] < a[(size_t)y * K + y]; });
  for (int k = 0; k < K; ++k) {
    const int src = order[k];
    lam[k] = a[(size_t)src * K + src];
    if (!(lam[k] > 0.0) || !std::isfinite(lam[k])) return fail(FDM_ERR_ARG, "rig_temporal_tables: eigenvalue %d = %g (the Gram matrix must be positive definite: raise ridge)", k, lam[k]);
    int big = 0;                                            // sign: the largest-magnitude entry positive, lowest index on a tie
    for (int j = 1; j < K; ++j)
      if (std::fabs(u[(size_t)j * K + src]) > std::fabs(u[(size_t)big * K + src])) big = j;
    const double sign = u[(size_t)big * K + src] < 0.0 ? -1.0 : 1.0;
    for (int j = 0; j < K; ++j) Q[(size_t)j * K + k] = d[j] * (sign * u[(size_t)j * K + src]);
  }
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
  R->gram = gram;
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

int fdm_rig_set_temporal(fdm_rig* R, double smooth, const float* sweights) {
  if (!R) return fail(FDM_ERR_ARG, "rig_set_temporal: null object");
  if (!(smooth >= 0.0) || std::isinf(smooth)) return fail(FDM_ERR_ARG, "rig_set_temporal: smooth = %g (finite and >= 0)", smooth);
  const int K = R->K;
  if (sweights)
    for (int k = 0; k < K; ++k)
      if (!(sweights[k] > 0.f) || std::isinf(sweights[k])) return fail(FDM_ERR_ARG, "rig_set_temporal: smoothing weight %d = %g (finite and > 0)", k, (double)sweights[k]);
  if (smooth == 0.0) { R->temporal = false; return FDM_OK; }
  std::vector<double> lam((size_t)K), Q((size_t)K * K);
  FCK(fdm_rig_temporal_tables_host(R->gram.data(), K, smooth, sweights, lam.data(), Q.data()));
  std::vector<float> q32((size_t)K * K), qt32((size_t)K * K), lam32((size_t)K), mv32((size_t)K);
  for (int k = 0; k < K; ++k) {
    lam32[k] = (float)lam[k];
    mv32[k] = (float)(smooth * (sweights ? (double)sweights[k] : 1.0));
    if (!(lam32[k] > 0.f) || !std::isfinite(lam32[k]) || !(mv32[k] > 0.f) || !std::isfinite(mv32[k]))
      return fail(FDM_ERR_ARG, "rig_set_temporal: eigenvalue %d = %g or smooth * weight = %g does not fit fp32", k, lam[k], (double)mv32[k]);
    for (int j = 0; j < K; ++j) {
      q32[(size_t)j * K + k] = qt32[(size_t)k * K + j] = (float)Q[(size_t)j * K + k];
      if (!std::isfinite(q32[(size_t)j * K + k])) return fail(FDM_ERR_ARG, "rig_set_temporal: element %d, %d of Q does not fit fp32", j, k);
    }
  }
  if (R->on_device && fdm_device_ok()) {
    HIPCK(hipDeviceSynchronize());                          // a call in flight may still read the tables of before
    if (!R->Q) {
      FCK(R->mem.alloc_t(&R->Q, q32.size())); FCK(R->mem.alloc_t(&R->QT, q32.size()));
      FCK(R->mem.alloc_t(&R->lam, (size_t)K)); FCK(R->mem.alloc_t(&R->mvec, (size_t)K));
      HIPCK(hipFuncSetAttribute((const void*)rig_modal_in_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)modal_lds(RIG_KMAX)));
      HIPCK(hipFuncSetAttribute((const void*)rig_modal_out_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)modal_lds(RIG_KMAX)));
      HIPCK(hipFuncSetAttribute((const void*)rig_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sweep_lds(RIG_KMAX)));
    }
    HIPCK(hipMemcpy(R->Q, q32.data(), q32.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(R->QT, qt32.data(), qt32.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(R->lam, lam32.data(), (size_t)K * sizeof(float), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(R->mvec, mv32.data(), (size_t)K * sizeof(float), hipMemcpyHostToDevice));
    HIPCK(hipDeviceSynchronize());
  }
  R->temporal = true;
  return FDM_OK;
}

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
  if (R->temporal) {
    const int K = R->K;
    FCK(grow(R->mem, &R->tbuf, &R->tbuf_cap, 3 * rows_out * K));
    float *rbuf = R->tbuf, *zu = rbuf + rows_out * K, *iw = zu + rows_out * K;
    hipLaunchKernelGGL(rig_modal_in_kernel, gs, dim3(RIG_SW * 64), modal_lds(K), s, (const float*)R->part, R->chunks, (int)rows_in,
                       (const int*)R->lens, L_max, L_out_max, (int)rows_out, K, resamples(fps_in, fps_out) ? 1 : 0, (const float*)R->Q, rbuf, zu,
                       coef, proj);
    hipLaunchKernelGGL(rig_time_kernel, dim3((unsigned)B, (unsigned)((K + 63) / 64)), dim3(64), 0, s, (const int*)R->lens, L_out_max, K,
                       (const float*)R->lam, zu, iw);
    hipLaunchKernelGGL(rig_modal_out_kernel, gs, dim3(RIG_SW * 64), modal_lds(K), s, (const float*)zu, (const int*)R->lens, L_out_max,
                       (int)rows_out, K, (const float*)R->QT, (const float*)R->lo, (const float*)R->hi, R->bounded ? 1 : 0, coef);
    if (R->bounded)
      for (int sw = 0; sw < 2 * R->sweeps; ++sw) {          // colour 0 (even frames of a clip), then colour 1, per sweep
        const int colour = sw & 1, per = (L_out_max + 1 - colour) / 2;
        if (!per) continue;
        const long long rows = (long long)B * per;
        hipLaunchKernelGGL(rig_sweep_kernel, dim3((unsigned)((rows + RIG_SW - 1) / RIG_SW)), dim3(RIG_SW * 64), sweep_lds(K), s, (const float*)rbuf,
                           (const int*)R->lens, L_out_max, per, (int)rows, colour, K, (const float*)R->G, (const float*)R->mvec,
                           (const float*)R->lo, (const float*)R->hi, coef);
      }
    HIPCK(hipGetLastError());
    if (frames_out) for (int b = 0; b < B; ++b) frames_out[b] = hl[2 * b + 1];
    return FDM_OK;
  }
  hipLaunchKernelGGL(rig_solve_kernel, gs, dim3(RIG_SW * 64), solve_lds(R->K), s, (const float*)R->part, R->chunks, (int)rows_in, (const int*)R->lens,
                     L_max, L_out_max, (int)rows_out, R->K, resamples(fps_in, fps_out) ? 1 : 0, (const float*)R->G, (const float*)R->Lc,
                     (const float*)R->lo, (const float*)R->hi, R->bounded ? 1 : 0, R->sweeps, coef, proj);
  HIPCK(hipGetLastError());
  if (frames_out) for (int b = 0; b < B; ++b) frames_out[b] = hl[2 * b + 1];
  return FDM_OK;
}

}  // extern "C"
