// Time filter hand-off behind plain C calls (include/fdm_hip.h, fdm_tfilter_*): the decoded offsets smoothed along time, per clip at its
// own length, before any other hand-off reads them.  Kernel: tfilter.hpp (the definition is stated there and in the header).  The taps
// are built on the host in fp64 (fdm_tfilter_taps_host) and handed over as fp32; fdm_tfilter_create validates and uploads them with the
// optional per-vertex strength; a forward call validates (every check before the launch) and launches once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "host.hpp"
#include "tfilter.hpp"

struct fdm_tfilter : fdm::Handoff {       // lens: L per clip
  int V = 0, R = 0, edge = 0;
  float* taps = nullptr;                  // device: [R + 1], [V] or null
  float* strength = nullptr;
  hipStream_t stream = nullptr;
};

namespace {
using namespace fdm;

// Savitzky-Golay smoothing taps: the centre row of the least-squares fit of a polynomial of `order` over the window -R .. R.  The fit
// is made in the discrete orthogonal (Gram) polynomials of the window, built by Gram-Schmidt in fp64 over the monomials: the centre row
// is h_k = sum_j p_j(0) p_j(k) / <p_j, p_j>.  Odd polynomials vanish at 0, so orders 2 and 3 share a row, as do 4 and 5.
void savgol_taps(int R, int order, double* taps) {
  const int n = 2 * R + 1;
  std::vector<std::vector<double>> p;
  for (int k = 0; k <= R; ++k) taps[k] = 0.0;
  for (int j = 0; j <= order; ++j) {
    std::vector<double> q((size_t)n);
    for (int i = 0; i < n; ++i) q[i] = std::pow((double)(i - R) / (double)(R > 0 ? R : 1), j);
    for (int pass = 0; pass < 2; ++pass)         // (twice: the second pass removes what rounding left of the first)
      for (const auto& u : p) {
        double num = 0.0, den = 0.0;
        for (int i = 0; i < n; ++i) { num += q[i] * u[i]; den += u[i] * u[i]; }
        for (int i = 0; i < n; ++i) q[i] -= num / den * u[i];
      }
    double nn = 0.0;
    for (int i = 0; i < n; ++i) nn += q[i] * q[i];
    for (int k = 0; k <= R; ++k) taps[k] += q[R] * q[R + k] / nn;
    p.push_back(q);
  }
}

}  // namespace

extern "C" {

int fdm_tfilter_taps_host(int kind, int radius, double param, double* taps) {
  if (!taps) return fail(FDM_ERR_ARG, "tfilter_taps: null taps");
  if (radius < 0 || radius > TF_RMAX) return fail(FDM_ERR_ARG, "tfilter_taps: radius %d outside [0, %d]", radius, TF_RMAX);
  if (kind == FDM_TFILTER_GAUSSIAN) {
    if (!(param > 0.0) || std::isinf(param)) return fail(FDM_ERR_ARG, "tfilter_taps: sigma %g (finite and > 0)", param);
    double sum = 0.0;
    for (int k = radius; k >= 0; --k) {          // (the small ones first)
      taps[k] = std::exp(-(double)k * (double)k / (2.0 * param * param));
      sum += k ? 2.0 * taps[k] : taps[k];
    }
    for (int k = 0; k <= radius; ++k) taps[k] /= sum;
    return FDM_OK;
  }
  if (kind == FDM_TFILTER_SAVGOL) {
    const int order = (param >= 2.0 && param <= 5.0) ? (int)param : 0;      // (a NaN or a huge value is never converted)
    if (order < 2 || param != (double)order) return fail(FDM_ERR_ARG, "tfilter_taps: polynomial order %g (2, 3, 4 or 5)", param);
    if (order >= 2 * radius + 1) return fail(FDM_ERR_ARG, "tfilter_taps: order %d needs a window longer than %d frames", order, 2 * radius + 1);
    savgol_taps(radius, order, taps);
    return FDM_OK;
  }
  return fail(FDM_ERR_ARG, "tfilter_taps: unknown kind %d", kind);
}

int fdm_tfilter_create(int V, int radius, const float* taps, const float* strength, int edge, void* stream, fdm_tfilter** out) {
  if (!out) return fail(FDM_ERR_ARG, "tfilter_create: null out");
  if (!taps) return fail(FDM_ERR_ARG, "tfilter_create: null taps");
  if (V < 1 || V > 0x7fffffff / 3) return fail(FDM_ERR_ARG, "tfilter_create: V = %d (3 V is a positive 32-bit int)", V);
  if (radius < 0 || radius > TF_RMAX) return fail(FDM_ERR_ARG, "tfilter_create: radius %d outside [0, %d]", radius, TF_RMAX);
  for (int k = 0; k <= radius; ++k)
    if (!std::isfinite(taps[k])) return fail(FDM_ERR_ARG, "tfilter_create: tap %d is not finite", k);
  if (strength)
    for (int v = 0; v < V; ++v)
      if (!(strength[v] >= 0.f && strength[v] <= 1.f)) return fail(FDM_ERR_ARG, "tfilter_create: strength %g of vertex %d (in [0, 1])", (double)strength[v], v);
  if (edge != FDM_TFILTER_MIRROR && edge != FDM_TFILTER_NEAREST) return fail(FDM_ERR_ARG, "tfilter_create: unknown edge rule %d", edge);
  fdm_tfilter* T = new (std::nothrow) fdm_tfilter();
  if (!T) return fail(FDM_ERR_STATE, "tfilter_create: out of memory");
  T->V = V; T->R = radius; T->edge = edge; T->stream = (hipStream_t)stream;
  return handoff_finish(T, out, [&]() {
    FCK(put(T->mem, &T->taps, taps, (size_t)radius + 1));
    if (strength) FCK(put(T->mem, &T->strength, strength, (size_t)V));
    HIPCK(hipFuncSetAttribute((const void*)time_filter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tfilter_lds(TF_RMAX)));
    return (int)FDM_OK;
  });
}

int fdm_tfilter_destroy(fdm_tfilter* T) { return handoff_destroy(T); }

int fdm_tfilter_forward(fdm_tfilter* T, const float* x, const int* lens, int B, int L_max, float* y) {
  if (!T || !x || !y) return fail(FDM_ERR_ARG, "tfilter_forward: null argument");
  if (B < 1 || L_max < 1) return fail(FDM_ERR_SHAPE, "tfilter_forward: B = %d, L_max = %d", B, L_max);
  std::vector<int> hl((size_t)B);
  for (int b = 0; b < B; ++b) {
    hl[b] = lens ? lens[b] : L_max;
    if (hl[b] < 1 || hl[b] > L_max) return fail(FDM_ERR_SHAPE, "tfilter_forward: clip %d has %d frames, the batch is %d long (1 .. L_max)", b, hl[b], L_max);
  }
  const long long rows = (long long)B * L_max, N = 3LL * T->V;
  const long long tiles = ((long long)L_max + TF_TILE - 1) / TF_TILE, chunks = (N + TF_CHUNK - 1) / TF_CHUNK;
  if (rows > 0x7fffffffLL || B > 65535 || tiles > 65535) return fail(FDM_ERR_SHAPE, "tfilter_forward: %d clips of %d frames exceed one launch", B, L_max);
  const uintptr_t x0 = (uintptr_t)x, y0 = (uintptr_t)y, bytes = (uintptr_t)(rows * N) * sizeof(float);
  if (x0 < y0 + bytes && y0 < x0 + bytes) return fail(FDM_ERR_ARG, "tfilter_forward: y overlaps x (the filter does not run in place)");
  FCK(handoff_device(*T, "tfilter_forward"));
  FCK(handoff_lens(*T, hl, T->stream));
  hipLaunchKernelGGL(time_filter_kernel, dim3((unsigned)chunks, (unsigned)tiles, (unsigned)B), dim3(TF_THREADS), tfilter_lds(T->R), T->stream, x,
                     (const int*)T->lens, L_max, (int)N, (const float*)T->taps, T->R, T->edge, (const float*)T->strength, y);
  HIPCK(hipGetLastError());
  return FDM_OK;
}

}  // extern "C"
