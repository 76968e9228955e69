// Parametric-head fit behind plain C calls (include/fdm_hip.h, fdm_flame_fit_*): target vertices -> expression coefficients, joint
// rotations and a translation of a head made by fdm_flame_create, by `iters` damped Gauss-Newton steps.  Kernels: flame_fit.hpp; the
// forward map is flame_out.hpp's own (the object's tables and scratch are used, so a fit object and its head share one stream).  Every
// check is made before the first launch; the launch count is a function of iters alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "flame_fit.hpp"
#include "flame_obj.hpp"

struct fdm_flame_fit : fdm::Handoff {
  fdm_flame* F = nullptr;
  fdm::FitDesc fd;
  int iters = 20;
  float lambda = 1e-6f, ridge_expr = 0.f, ridge_pose = 0.f, pivot_tol = fdm::FIT_PIVOT_TOL;
  float* vw = nullptr;                    // device: the vertex weights, or null
  float msum = 0.f;                       // their sum (V without weights), fp64 on the host, rounded once
  float *dX = nullptr, *dE = nullptr, *part = nullptr, *Hs = nullptr, *tr = nullptr, *verts = nullptr, *th_e = nullptr, *th_p = nullptr;
  int* status = nullptr;
  long long dX_cap = 0, dE_cap = 0, part_cap = 0, Hs_cap = 0, tr_cap = 0, verts_cap = 0, th_e_cap = 0, th_p_cap = 0, status_cap = 0;
};

namespace {
using namespace fdm;

struct Call {                             // one validated call
  int B, L_max, NS, shape_rows;
  long long rows, tiles;
  std::vector<int> hl;
};

int check_call(const char* who, fdm_flame_fit* T, const float* target, const float* shape, int NS, int shape_rows, const int* frames, int B, int L_max,
               Call& c) {
  if (!T || !target) return fail(FDM_ERR_ARG, "%s: null argument", who);
  fdm_flame* F = T->F;
  if (NS < 0 || NS > F->expr_at) return fail(FDM_ERR_ARG, "%s: NS = %d (0..expr_at = %d)", who, NS, F->expr_at);
  if (NS > 0 && !shape) return fail(FDM_ERR_ARG, "%s: null shape with %d coefficients", who, NS);
  if (B < 1 || L_max < 1) return fail(FDM_ERR_SHAPE, "%s: B = %d, L_max = %d", who, B, L_max);
  if (shape_rows != 1 && shape_rows != B) return fail(FDM_ERR_ARG, "%s: shape_rows = %d (1 or B = %d)", who, shape_rows, B);
  const ClipLens cl = clip_lens(frames, B, L_max, 0.0, 0.0, 0, c.hl);
  if (cl.bad == ClipLens::LENGTH) return fail(FDM_ERR_SHAPE, "%s: clip %d has %d frames, the batch is %d long", who, cl.clip, cl.L, L_max);
  c.rows = (long long)B * L_max;
  if (c.rows > 0x7fffffffLL - 64 || F->chunks > 65535)
    return fail(FDM_ERR_SHAPE, "%s: %lld rows of %d vertices exceed one launch", who, c.rows, F->V);
  c.B = B; c.L_max = L_max; c.NS = NS; c.shape_rows = shape_rows;
  c.tiles = (c.rows + ROW_TILE - 1) / ROW_TILE;
  return handoff_device(*T, who);
}

// the scratch of a call of this size, in the head object and in the fit
int reserve(fdm_flame_fit* T, const Call& c, bool want_verts) {
  fdm_flame* F = T->F;
  const int J = F->J, PF = 9 * (J - 1), NT = T->fd.n_expr + PF, P = T->fd.P, ld = F->chunks * ROW_CHUNK;
  FCK(grow(F->mem, &F->xf, &F->xf_cap, c.tiles * ROW_TILE * J * 12));
  FCK(grow(F->mem, &F->pf, &F->pf_cap, c.rows * PF));
  FCK(grow(F->mem, &F->cf, &F->cf_cap, c.tiles * NT * ROW_TILE));
  FCK(grow(F->mem, &F->vid, &F->vid_cap, (long long)c.shape_rows * ld));
  FCK(grow(T->mem, &T->dX, &T->dX_cap, c.rows * 3 * T->fd.n_free * J * 12));
  FCK(grow(T->mem, &T->dE, &T->dE_cap, c.rows * T->fd.n_expr * J * 3));
  FCK(grow(T->mem, &T->part, &T->part_cap, c.rows * F->chunks * fit_np(P)));
  FCK(grow(T->mem, &T->Hs, &T->Hs_cap, c.rows * fit_np(P)));
  FCK(grow(T->mem, &T->tr, &T->tr_cap, c.rows * 3));
  FCK(grow(T->mem, &T->status, &T->status_cap, c.rows));
  if (want_verts) FCK(grow(T->mem, &T->verts, &T->verts_cap, c.rows * 3 * F->V));
  return FDM_OK;
}

// one Gauss-Newton step at (expr, pose, tr): pose stage, derivative stage, normal equations, reduce, solve (theta += delta)
void step(fdm_flame_fit* T, const Call& c, const float* target, const float* shape, const float* pose0, float* expr, float* pose, float* tr, float* delta,
          int* status, hipStream_t s) {
  fdm_flame* F = T->F;
  const FitDesc& fd = T->fd;
  const int J = F->J, PF = 9 * (J - 1), P = fd.P, ld = F->chunks * ROW_CHUNK, rows = (int)c.rows;
  flame_launch_pose(F, shape, c.shape_rows, c.NS, expr, fd.n_expr, pose, c.L_max, c.rows, s);
  hipLaunchKernelGGL(flame_fit_deriv_kernel, dim3((unsigned)((c.rows + 63) / 64)), dim3(64), 0, s, shape, c.shape_rows, c.NS, (const float*)expr,
                     (const float*)pose, (const int*)F->lens, c.L_max, rows, J, F->expr_at, (const float*)F->JT, (const float*)F->JD, (const int*)F->par,
                     (const float*)F->xf, fd, T->dX, T->dE);
  FlameFitArgs a;
  a.vid = F->vid; a.shape_rows = c.shape_rows; a.D = F->D; a.ld = ld;
  a.row_expr = F->expr_at; a.row_pose = F->NB; a.PF = PF;
  a.cf = F->cf; a.xf = F->xf; a.dX = T->dX; a.dE = T->dE; a.wts = F->wts; a.J = J; a.vw = T->vw; a.tr = tr; a.target = target;
  a.lens = F->lens; a.L_max = c.L_max; a.rows = rows; a.V3 = 3 * F->V; a.chunks = F->chunks; a.fd = fd; a.part = T->part;
  hipLaunchKernelGGL(flame_fit_normal_kernel, dim3((unsigned)c.tiles, (unsigned)F->chunks), dim3(256), flame_fit_lds(fd.n_expr, fd.n_free, P, J), s, a);
  const int NP = fit_np(P);
  hipLaunchKernelGGL(flame_fit_reduce_kernel, dim3((unsigned)rows, (unsigned)((NP + 255) / 256)), dim3(256), 0, s, (const float*)T->part,
                     (const int*)F->lens, c.L_max, rows, F->chunks, NP, T->Hs);
  hipLaunchKernelGGL(flame_fit_solve_kernel, dim3((unsigned)rows), dim3(256), (size_t)(P * (P + 1) + 2 * P) * sizeof(float), s, (const float*)T->Hs,
                     (const int*)F->lens, c.L_max, fd, 3 * J, T->lambda, T->pivot_tol, T->ridge_expr, T->ridge_pose, pose0, expr, pose, tr, delta, status);
}

}  // namespace

extern "C" {

int fdm_flame_fit_create(fdm_flame* F, const int* free_joints, int n_free, int n_expr, int transl, const float* vertex_weights, fdm_flame_fit** out) {
  if (!out) return fail(FDM_ERR_ARG, "flame_fit_create: null out");
  if (!F) return fail(FDM_ERR_ARG, "flame_fit_create: null head");
  if (n_free < 0 || n_free > F->J) return fail(FDM_ERR_ARG, "flame_fit_create: n_free = %d (0..J = %d)", n_free, F->J);
  if (n_free > 0 && !free_joints) return fail(FDM_ERR_ARG, "flame_fit_create: null free_joints with n_free = %d", n_free);
  if (n_expr < 0 || n_expr > F->NB - F->expr_at)
    return fail(FDM_ERR_ARG, "flame_fit_create: n_expr = %d (0..NE = NB - expr_at = %d)", n_expr, F->NB - F->expr_at);
  if (transl != 0 && transl != 1) return fail(FDM_ERR_ARG, "flame_fit_create: transl = %d (0 or 1)", transl);
  for (int i = 0; i < n_free; ++i) {
    if (free_joints[i] < 0 || free_joints[i] >= F->J)
      return fail(FDM_ERR_ARG, "flame_fit_create: free_joints[%d] = %d (joint index out of range 0..%d)", i, free_joints[i], F->J - 1);
    for (int k = 0; k < i; ++k)
      if (free_joints[k] == free_joints[i]) return fail(FDM_ERR_ARG, "flame_fit_create: joint %d is given twice (free_joints[%d] and [%d])", free_joints[i], k, i);
  }
  const int P = n_expr + 3 * n_free + 3 * transl;
  if (P < 1 || P > FIT_PMAX) return fail(FDM_ERR_ARG, "flame_fit_create: P = %d free parameters (1..%d)", P, FIT_PMAX);
  double msum = (double)F->V;
  if (vertex_weights) {
    msum = 0.0;
    for (int v = 0; v < F->V; ++v) {
      const float w = vertex_weights[v];
      if (!std::isfinite(w) || w < 0.f) return fail(FDM_ERR_ARG, "flame_fit_create: vertex_weights[%d] = %g (finite and not negative)", v, (double)w);
      msum += (double)w;
    }
    if (!(msum > 0.0)) return fail(FDM_ERR_ARG, "flame_fit_create: vertex_weights are all zero");
  }
  fdm_flame_fit* T = new (std::nothrow) fdm_flame_fit();
  if (!T) return fail(FDM_ERR_STATE, "flame_fit_create: out of memory");
  T->F = F;
  memset(&T->fd, 0, sizeof(T->fd));
  T->fd.n_expr = n_expr; T->fd.n_free = n_free; T->fd.transl = transl; T->fd.P = P;
  for (int i = 0; i < n_free; ++i) T->fd.free_j[i] = free_joints[i];
  T->msum = (float)msum;
  if (!F->on_device) { *out = T; return FDM_OK; }          // validates; forward ends in FDM_ERR_STATE
  return handoff_finish(T, out, [&]() {
    if (vertex_weights) FCK(put(T->mem, &T->vw, vertex_weights, (size_t)F->V));
    HIPCK(hipFuncSetAttribute((const void*)flame_fit_normal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)flame_fit_lds(FIT_PMAX, FLAME_JMAX, FIT_PMAX, FLAME_JMAX)));
    HIPCK(hipFuncSetAttribute((const void*)flame_fit_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((FIT_PMAX * (FIT_PMAX + 1) + 2 * FIT_PMAX) * sizeof(float))));
    return (int)FDM_OK;
  });
}

int fdm_flame_fit_destroy(fdm_flame_fit* T) { return handoff_destroy(T); }

int fdm_flame_fit_set(fdm_flame_fit* T, const char* key, double value) {
  if (!T || !key) return fail(FDM_ERR_ARG, "flame_fit_set: null argument");
  const std::string k(key);
  if (k == "iters") {
    if (!(value >= 1.0) || value > 10000.0 || value != std::floor(value)) return fail(FDM_ERR_ARG, "flame_fit_set: iters = %g (a whole number, 1..10000)", value);
    T->iters = (int)value;
    return FDM_OK;
  }
  if (k == "pivot_tol") {
    if (!(value >= 0.0) || value > 1.0) return fail(FDM_ERR_ARG, "flame_fit_set: pivot_tol = %g (0..1)", value);
    T->pivot_tol = (float)value;
    return FDM_OK;
  }
  if (k != "lambda" && k != "ridge_expr" && k != "ridge_pose") return fail(FDM_ERR_ARG, "flame_fit_set: unknown key %s (iters, lambda, ridge_expr, ridge_pose, pivot_tol)", key);
  if (!(value >= 0.0) || std::isinf(value)) return fail(FDM_ERR_ARG, "flame_fit_set: %s = %g (finite and not negative)", key, value);
  (k == "lambda" ? T->lambda : k == "ridge_expr" ? T->ridge_expr : T->ridge_pose) = (float)value;
  return FDM_OK;
}

int fdm_flame_fit_forward(fdm_flame_fit* T, const float* target, const float* shape, int NS, int shape_rows, const float* pose0, const int* frames, int B,
                          int L_max, float* expr, float* pose, float* transl, float* rms, float* verts, int* status, void* stream) {
  Call c;
  if (T && (!pose || (T->fd.n_expr > 0 && !expr))) return fail(FDM_ERR_ARG, "flame_fit_forward: null expr or pose");
  FCK(check_call("flame_fit_forward", T, target, shape, NS, shape_rows, frames, B, L_max, c));
  fdm_flame* F = T->F;
  const bool final_pass = rms || verts;
  FCK(reserve(T, c, final_pass && !verts));
  FCK(handoff_lens(*F, c.hl, (hipStream_t)stream));
  hipStream_t s = (hipStream_t)stream;
  float* tr = transl ? transl : T->tr;
  int* st = status ? status : T->status;
  hipLaunchKernelGGL(flame_fit_init_kernel, dim3((unsigned)c.rows), dim3(256), 0, s, pose0, (const int*)F->lens, L_max, (int)c.rows, T->fd.n_expr, 3 * F->J,
                     expr, pose, tr, st);
  flame_launch_shape(F, shape, NS, shape_rows, s);
  for (int it = 0; it < T->iters; ++it) step(T, c, target, shape, pose0, expr, pose, tr, nullptr, st, s);
  HIPCK(hipGetLastError());
  if (final_pass) {
    float* vo = verts ? verts : T->verts;
    FCK(fdm_flame_forward(F, shape, NS, shape_rows, T->fd.n_expr ? expr : nullptr, T->fd.n_expr, pose, T->fd.transl ? tr : nullptr, nullptr, frames, B, L_max,
                          vo, nullptr, nullptr, nullptr, stream));
    if (rms)
      hipLaunchKernelGGL(flame_fit_rms_kernel, dim3((unsigned)c.rows), dim3(256), 0, s, (const float*)vo, target, (const float*)T->vw, (const int*)F->lens,
                         L_max, 3 * F->V, F->chunks, T->msum, rms);
    HIPCK(hipGetLastError());
  }
  return FDM_OK;
}

int fdm_flame_fit_step(fdm_flame_fit* T, const float* target, const float* shape, int NS, int shape_rows, const float* pose0, const float* expr,
                       const float* pose, const float* transl, const int* frames, int B, int L_max, float* H, float* delta, float* dX, float* dE,
                       float* xforms, int* status, void* stream) {
  Call c;
  if (T && (!pose || !status || (T->fd.n_expr > 0 && !expr) || (T->fd.transl && !transl))) return fail(FDM_ERR_ARG, "flame_fit_step: null expr, pose, transl or status");
  FCK(check_call("flame_fit_step", T, target, shape, NS, shape_rows, frames, B, L_max, c));
  fdm_flame* F = T->F;
  FCK(reserve(T, c, false));
  const int J = F->J, P = T->fd.P;
  FCK(grow(T->mem, &T->th_e, &T->th_e_cap, c.rows * T->fd.n_expr));
  FCK(grow(T->mem, &T->th_p, &T->th_p_cap, c.rows * 3 * J));
  FCK(handoff_lens(*F, c.hl, (hipStream_t)stream));
  hipStream_t s = (hipStream_t)stream;
  // the step works on copies: the caller's parameters are left as they are
  if (T->fd.n_expr) HIPCK(hipMemcpyAsync(T->th_e, expr, (size_t)c.rows * T->fd.n_expr * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCK(hipMemcpyAsync(T->th_p, pose, (size_t)c.rows * 3 * J * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (T->fd.transl) HIPCK(hipMemcpyAsync(T->tr, transl, (size_t)c.rows * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCK(hipMemsetAsync(status, 0, (size_t)c.rows * sizeof(int), s));
  HIPCK(hipMemsetAsync(T->Hs, 0, (size_t)c.rows * fit_np(P) * sizeof(float), s));      // dead rows read as zeros
  if (delta) HIPCK(hipMemsetAsync(delta, 0, (size_t)c.rows * P * sizeof(float), s));
  if (dX && T->fd.n_free) HIPCK(hipMemsetAsync(T->dX, 0, (size_t)c.rows * 3 * T->fd.n_free * J * 12 * sizeof(float), s));
  if (dE && T->fd.n_expr) HIPCK(hipMemsetAsync(T->dE, 0, (size_t)c.rows * T->fd.n_expr * J * 3 * sizeof(float), s));
  flame_launch_shape(F, shape, NS, shape_rows, s);
  step(T, c, target, shape, pose0, T->th_e, T->th_p, T->tr, delta, status, s);
  HIPCK(hipGetLastError());
  if (H) HIPCK(hipMemcpyAsync(H, T->Hs, (size_t)c.rows * fit_np(P) * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (dX && T->fd.n_free) HIPCK(hipMemcpyAsync(dX, T->dX, (size_t)c.rows * 3 * T->fd.n_free * J * 12 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (dE && T->fd.n_expr) HIPCK(hipMemcpyAsync(dE, T->dE, (size_t)c.rows * T->fd.n_expr * J * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (xforms) HIPCK(hipMemcpyAsync(xforms, F->xf, (size_t)c.rows * J * 12 * sizeof(float), hipMemcpyDeviceToDevice, s));
  return FDM_OK;
}

}  // extern "C"
