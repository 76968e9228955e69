// Time filter hand-off behind plain C calls (include/fdm_hip.h, fdm_tfilter_*): the decoded offsets smoothed along time, per clip at its
// own length, before any other hand-off reads them.  Kernel: tfilter.hpp (the definition is stated there and in the header).  The taps
// are built on the host in fp64 (fdm_tfilter_taps_host) and handed over as fp32; fdm_tfilter_create validates and uploads them with the
// optional per-vertex strength; a forward call validates (every check before the launch) and launches once.  The recurrences (trecur.hpp:
// ema and One Euro, causal with a carried state or zero-phase) are the same object made by fdm_tfilter_create_recur: their constants
// come from fdm_tfilter_recur_coeffs_host, and fdm_tfilter_forward serves both families.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "host.hpp"
#include "tfilter.hpp"
#include "trecur.hpp"

struct fdm_tfilter : fdm::Handoff {       // lens: L per clip
  int V = 0, R = 0, edge = 0;
  bool recur = false;                     // made by fdm_tfilter_create_recur: kind, direction, q and depth are read, R, edge and taps are not
  int kind = 0, direction = 0, depth = fdm::TR_DEPTH;
  fdm::RecurCoef q = {};
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

int strength_ok(const char* who, const float* strength, int V) {
  if (strength)
    for (int v = 0; v < V; ++v)
      if (!(strength[v] >= 0.f && strength[v] <= 1.f)) return fail(FDM_ERR_ARG, "%s: strength %g of vertex %d (in [0, 1])", who, (double)strength[v], v);
  return FDM_OK;
}

template <int KIND, int D> void recur_launch(const fdm_tfilter* T, const float* x, int B, int L_max, float* st, const int* seen, float* y) {
  hipLaunchKernelGGL((time_recur_kernel<KIND, D>), dim3((unsigned)((T->V + TR_VERTS - 1) / TR_VERTS), (unsigned)B), dim3(TR_VERTS), 0, T->stream, x,
                     (const int*)T->lens, L_max, T->V, T->q, (const float*)T->strength, T->direction, st, seen, y);
}
template <int KIND> void recur_launch(const fdm_tfilter* T, const float* x, int B, int L_max, float* st, const int* seen, float* y) {
  switch (T->depth) {
    case 1: return recur_launch<KIND, 1>(T, x, B, L_max, st, seen, y);
    case 4: return recur_launch<KIND, 4>(T, x, B, L_max, st, seen, y);
    case 8: return recur_launch<KIND, 8>(T, x, B, L_max, st, seen, y);
    default: return recur_launch<KIND, TR_DEPTH>(T, x, B, L_max, st, seen, y);
  }
}

// what fdm_tfilter_forward and fdm_tfilter_forward_state share: every check, the lengths, the launch (st and seen: both or neither)
int tfilter_run(const char* who, fdm_tfilter* T, const float* x, const int* lens, int B, int L_max, float* st, int* seen, float* y) {
  if (!T || !x || !y) return fail(FDM_ERR_ARG, "%s: null argument", who);
  const int L_min = st ? 0 : 1;
  if (B < 1 || L_max < 1) return fail(FDM_ERR_SHAPE, "%s: B = %d, L_max = %d", who, B, L_max);
  std::vector<int> hl((size_t)B);
  for (int b = 0; b < B; ++b) {
    hl[b] = lens ? lens[b] : L_max;
    if (hl[b] < L_min || hl[b] > L_max)
      return fail(FDM_ERR_SHAPE, "%s: clip %d has %d frames, the batch is %d long (%d .. L_max)", who, b, hl[b], L_max, L_min);
  }
  const long long rows = (long long)B * L_max, N = 3LL * T->V;
  const long long tiles = ((long long)L_max + TF_TILE - 1) / TF_TILE, chunks = (N + TF_CHUNK - 1) / TF_CHUNK;
  if (rows > 0x7fffffffLL || B > 65535 || (!T->recur && tiles > 65535)) return fail(FDM_ERR_SHAPE, "%s: %d clips of %d frames exceed one launch", who, B, L_max);
  const uintptr_t x0 = (uintptr_t)x, y0 = (uintptr_t)y, bytes = (uintptr_t)(rows * N) * sizeof(float);
  if (x0 < y0 + bytes && y0 < x0 + bytes) return fail(FDM_ERR_ARG, "%s: y overlaps x (the filter does not run in place)", who);
  FCK(handoff_device(*T, who));
  FCK(handoff_lens(*T, hl, T->stream));
  if (!T->recur)
    hipLaunchKernelGGL(time_filter_kernel, dim3((unsigned)chunks, (unsigned)tiles, (unsigned)B), dim3(TF_THREADS), tfilter_lds(T->R), T->stream, x,
                       (const int*)T->lens, L_max, (int)N, (const float*)T->taps, T->R, T->edge, (const float*)T->strength, y);
  else if (T->kind == TR_EMA)
    recur_launch<TR_EMA>(T, x, B, L_max, st, seen, y);
  else
    recur_launch<TR_ONE_EURO>(T, x, B, L_max, st, seen, y);
  HIPCK(hipGetLastError());
  if (st) {
    hipLaunchKernelGGL(time_recur_seen_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, T->stream, seen, (const int*)T->lens, B);
    HIPCK(hipGetLastError());
  }
  return FDM_OK;
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
  FCK(strength_ok("tfilter_create", strength, V));
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
  return tfilter_run("tfilter_forward", T, x, lens, B, L_max, nullptr, nullptr, y);
}

int fdm_tfilter_recur_coeffs_host(int kind, double fps, double cutoff, double beta, double d_cutoff, float* coeffs) {
  if (!coeffs) return fail(FDM_ERR_ARG, "tfilter_recur_coeffs: null coeffs");
  if (kind != FDM_TFILTER_EMA && kind != FDM_TFILTER_ONE_EURO) return fail(FDM_ERR_ARG, "tfilter_recur_coeffs: unknown kind %d", kind);
  if (!(fps > 0.0) || std::isinf(fps)) return fail(FDM_ERR_ARG, "tfilter_recur_coeffs: fps %g (finite and > 0)", fps);
  if (!(cutoff > 0.0) || std::isinf(cutoff)) return fail(FDM_ERR_ARG, "tfilter_recur_coeffs: cutoff %g Hz (finite and > 0)", cutoff);
  RecurCoef q = {};
  q.k = (float)(fps / (2.0 * 3.14159265358979323846));
  q.c0 = (float)cutoff;
  q.fr = (float)fps;
  if (kind == FDM_TFILTER_ONE_EURO) {
    if (!(beta >= 0.0) || std::isinf(beta)) return fail(FDM_ERR_ARG, "tfilter_recur_coeffs: beta %g (finite and >= 0)", beta);
    if (!(d_cutoff > 0.0) || std::isinf(d_cutoff)) return fail(FDM_ERR_ARG, "tfilter_recur_coeffs: d_cutoff %g Hz (finite and > 0)", d_cutoff);
    q.be = (float)beta;
    q.cd = (float)d_cutoff;
    q.ad = q.cd / (q.cd + q.k);
  }
  q.a0 = q.c0 / (q.c0 + q.k);
  const float c[TR_NCOEFF] = {q.k, q.c0, q.be, q.cd, q.fr, q.ad, q.a0, 0.f};
  for (int i = 0; i < TR_NCOEFF; ++i)      // (a double past fp32's range, or below it, is refused here, not handed on)
    if (!std::isfinite(c[i])) return fail(FDM_ERR_ARG, "tfilter_recur_coeffs: coefficient %d is not finite in fp32", i);
  if (!(q.k > 0.f) || !(q.c0 > 0.f) || !(q.fr > 0.f) || (kind == FDM_TFILTER_ONE_EURO && !(q.cd > 0.f && q.ad > 0.f)))
    return fail(FDM_ERR_ARG, "tfilter_recur_coeffs: a cutoff or the frame rate rounds to zero in fp32");
  for (int i = 0; i < TR_NCOEFF; ++i) coeffs[i] = c[i];
  return FDM_OK;
}

int fdm_tfilter_create_recur(int V, int kind, const float* coeffs, const float* strength, int direction, void* stream, fdm_tfilter** out) {
  if (!out) return fail(FDM_ERR_ARG, "tfilter_create_recur: null out");
  if (!coeffs) return fail(FDM_ERR_ARG, "tfilter_create_recur: null coeffs");
  if (V < 1 || V > 0x7fffffff / 3) return fail(FDM_ERR_ARG, "tfilter_create_recur: V = %d (3 V is a positive 32-bit int)", V);
  if (kind != FDM_TFILTER_EMA && kind != FDM_TFILTER_ONE_EURO) return fail(FDM_ERR_ARG, "tfilter_create_recur: unknown kind %d", kind);
  if (direction != FDM_TFILTER_CAUSAL && direction != FDM_TFILTER_ZERO_PHASE) return fail(FDM_ERR_ARG, "tfilter_create_recur: unknown direction %d", direction);
  for (int i = 0; i < TR_NCOEFF; ++i)
    if (!std::isfinite(coeffs[i])) return fail(FDM_ERR_ARG, "tfilter_create_recur: coefficient %d is not finite", i);
  const RecurCoef q = {coeffs[0], coeffs[1], coeffs[2], coeffs[3], coeffs[4], coeffs[5], coeffs[6], 0.f};
  if (!(q.k > 0.f) || !(q.c0 > 0.f) || !(q.fr > 0.f) || !(q.a0 > 0.f))
    return fail(FDM_ERR_ARG, "tfilter_create_recur: k = %g, cutoff = %g, fps = %g, a0 = %g (each > 0)", (double)q.k, (double)q.c0, (double)q.fr, (double)q.a0);
  if (q.be < 0.f) return fail(FDM_ERR_ARG, "tfilter_create_recur: beta = %g (>= 0)", (double)q.be);
  if (kind == FDM_TFILTER_ONE_EURO && !(q.cd > 0.f && q.ad > 0.f))
    return fail(FDM_ERR_ARG, "tfilter_create_recur: d_cutoff = %g, ad = %g (each > 0)", (double)q.cd, (double)q.ad);
  FCK(strength_ok("tfilter_create_recur", strength, V));
  fdm_tfilter* T = new (std::nothrow) fdm_tfilter();
  if (!T) return fail(FDM_ERR_STATE, "tfilter_create_recur: out of memory");
  T->V = V; T->recur = true; T->kind = kind; T->direction = direction; T->q = q; T->stream = (hipStream_t)stream;
  return handoff_finish(T, out, [&]() {
    if (strength) FCK(put(T->mem, &T->strength, strength, (size_t)V));
    return (int)FDM_OK;
  });
}

int fdm_tfilter_set_prefetch(fdm_tfilter* T, int depth) {
  if (!T || !T->recur) return fail(FDM_ERR_ARG, "tfilter_set_prefetch: not a recurrence object");
  if (depth != 1 && depth != 4 && depth != 8 && depth != 16) return fail(FDM_ERR_ARG, "tfilter_set_prefetch: depth %d (1, 4, 8 or 16)", depth);
  T->depth = depth;
  return FDM_OK;
}

int fdm_tfilter_forward_state(fdm_tfilter* T, const float* x, const int* lens, int B, int L_max, float* st, int* seen, float* y) {
  if (!T || !st || !seen) return fail(FDM_ERR_ARG, "tfilter_forward_state: null argument");
  if (!T->recur) return fail(FDM_ERR_ARG, "tfilter_forward_state: an FIR filter carries no state (fdm_tfilter_create_recur makes the filters that do)");
  if (T->direction != FDM_TFILTER_CAUSAL) return fail(FDM_ERR_ARG, "tfilter_forward_state: a zero-phase filter walks the whole clip back: only a causal one carries a state");
  return tfilter_run("tfilter_forward_state", T, x, lens, B, L_max, st, seen, y);
}

}  // extern "C"
