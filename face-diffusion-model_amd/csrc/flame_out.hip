// Parametric-head hand-off behind plain C calls (include/fdm_hip.h, fdm_flame_*): shape / expression coefficients and axis-angle joint
// rotations -> posed vertices of a head of the SMPL / FLAME family (linear blend skinning), with the decoder's offsets as an optional
// displacement.  Kernels: flame_out.hpp.  fdm_flame_create does the fp64 work on the host (the coefficient-major directions, the
// folded joint regressor) and uploads fp32 copies; a forward call validates (every check before the first launch), grows the scratch
// when a call is larger than any before it, and launches the pose kernel, the identity blend and the blend-and-skin kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "flame_obj.hpp"
#include "flame_out.hpp"

namespace {
using namespace fdm;

int finite_field(const char* who, const char* field, const float* p, long long n) {
  for (long long i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return fail(FDM_ERR_ARG, "%s: %s element %lld = %g (not finite)", who, field, i, (double)p[i]);
  return FDM_OK;
}

int check_model(const char* who, const fdm_flame_model* m) {
  if (!m) return fail(FDM_ERR_ARG, "%s: null model", who);
  if (m->V < 1 || m->V > 0x7fffffff / 3 - ROW_CHUNK) return fail(FDM_ERR_ARG, "%s: V = %d (3 V is a positive 32-bit int)", who, m->V);
  if (m->J < 1 || m->J > FLAME_JMAX) return fail(FDM_ERR_ARG, "%s: J = %d (1..%d)", who, m->J, FLAME_JMAX);
  if (m->NB < 0 || m->NB > FLAME_NBMAX) return fail(FDM_ERR_ARG, "%s: NB = %d (0..%d)", who, m->NB, FLAME_NBMAX);
  if (m->expr_at < 0 || m->expr_at > m->NB) return fail(FDM_ERR_ARG, "%s: expr_at = %d (0..NB = %d)", who, m->expr_at, m->NB);
  if (!m->v_template) return fail(FDM_ERR_ARG, "%s: null v_template", who);
  if (m->NB > 0 && !m->shapedirs) return fail(FDM_ERR_ARG, "%s: null shapedirs", who);
  if (m->J > 1 && !m->posedirs) return fail(FDM_ERR_ARG, "%s: null posedirs", who);
  if (!m->j_regressor) return fail(FDM_ERR_ARG, "%s: null j_regressor", who);
  if (!m->parents) return fail(FDM_ERR_ARG, "%s: null parents", who);
  if (!m->lbs_weights) return fail(FDM_ERR_ARG, "%s: null lbs_weights", who);
  for (int j = 1; j < m->J; ++j)
    if (m->parents[j] < 0 || m->parents[j] >= j) return fail(FDM_ERR_ARG, "%s: parents[%d] = %d (0..%d)", who, j, m->parents[j], j - 1);
  const long long V3 = 3LL * m->V;
  FCK(finite_field(who, "v_template", m->v_template, V3));
  if (m->NB > 0) FCK(finite_field(who, "shapedirs", m->shapedirs, V3 * m->NB));
  if (m->J > 1) FCK(finite_field(who, "posedirs", m->posedirs, 9LL * (m->J - 1) * V3));
  FCK(finite_field(who, "j_regressor", m->j_regressor, (long long)m->J * m->V));
  FCK(finite_field(who, "lbs_weights", m->lbs_weights, (long long)m->V * m->J));
  return FDM_OK;
}

// the tables of the header, D with row stride ld >= 3 V (elements behind 3 V are left as they are)
void tables(const fdm_flame_model* m, float* D, long long ld, float* JT, float* JD) {
  const int V = m->V, J = m->J, NB = m->NB, P = 9 * (J - 1);
  const long long V3 = 3LL * V;
  for (long long i = 0; i < V3; ++i)
    for (int k = 0; k < NB; ++k) D[k * ld + i] = m->shapedirs[i * NB + k];
  for (int p = 0; p < P; ++p)
    for (long long i = 0; i < V3; ++i) D[(NB + p) * ld + i] = m->posedirs[p * V3 + i];
  std::vector<double> acc((size_t)3 * (NB + 1));
  for (int j = 0; j < J; ++j) {
    std::fill(acc.begin(), acc.end(), 0.0);
    const float* rj = m->j_regressor + (size_t)j * V;
    for (int v = 0; v < V; ++v) {
      const double r = (double)rj[v];
      if (r == 0.0) continue;                               // (exact: a zero weight adds +0)
      for (int a = 0; a < 3; ++a) {
        acc[(size_t)a * (NB + 1) + NB] += r * (double)m->v_template[3 * (size_t)v + a];
        const float* sd = NB ? m->shapedirs + (3 * (size_t)v + a) * NB : nullptr;
        double* dst = acc.data() + (size_t)a * (NB + 1);
        for (int k = 0; k < NB; ++k) dst[k] += r * (double)sd[k];
      }
    }
    for (int a = 0; a < 3; ++a) {
      JT[3 * j + a] = (float)acc[(size_t)a * (NB + 1) + NB];
      for (int k = 0; k < NB; ++k) JD[(size_t)k * 3 * J + 3 * j + a] = (float)acc[(size_t)a * (NB + 1) + k];
    }
  }
}

}  // namespace

namespace fdm {
void flame_launch_pose(fdm_flame* F, const float* shape, int shape_rows, int NS, const float* expr, int NE, const float* pose, int L_max, long long rows,
                       hipStream_t s) {
  const long long tiles = (rows + ROW_TILE - 1) / ROW_TILE;
  hipLaunchKernelGGL(flame_pose_kernel, dim3((unsigned)((tiles * ROW_TILE + 63) / 64)), dim3(64), 0, s, shape, shape_rows, NS, expr, NE, pose,
                     (const int*)F->lens, L_max, (int)rows, F->J, F->expr_at, (const float*)F->JT, (const float*)F->JD, (const int*)F->par, F->xf, F->pf,
                     F->cf);
}
void flame_launch_shape(fdm_flame* F, const float* shape, int NS, int shape_rows, hipStream_t s) {
  const int ld = F->chunks * ROW_CHUNK;
  hipLaunchKernelGGL(flame_shape_kernel, dim3((unsigned)((ld / 4 + 255) / 256), (unsigned)shape_rows), dim3(256), 0, s, (const float*)F->T,
                     (const float*)F->D, ld, shape, NS, F->vid);
}
}  // namespace fdm

extern "C" {

int fdm_flame_tables_host(const fdm_flame_model* m, float* D, float* JT, float* JD) {
  FCK(check_model("flame_tables", m));
  if (!JT || ((m->NB > 0 || m->J > 1) && !D) || (m->NB > 0 && !JD)) return fail(FDM_ERR_ARG, "flame_tables: null output");
  tables(m, D, 3LL * m->V, JT, JD);
  return FDM_OK;
}

int fdm_flame_create(const fdm_flame_model* m, const int* lmk_verts, const float* lmk_bary, int NL, fdm_flame** out) {
  if (!out) return fail(FDM_ERR_ARG, "flame_create: null out");
  FCK(check_model("flame_create", m));
  if (NL < 0 || NL > FLAME_NLMAX) return fail(FDM_ERR_ARG, "flame_create: NL = %d (0..%d)", NL, FLAME_NLMAX);
  if (NL > 0 && (!lmk_verts || !lmk_bary)) return fail(FDM_ERR_ARG, "flame_create: null lmk_verts or lmk_bary with NL = %d", NL);
  for (int i = 0; i < 3 * NL; ++i)
    if (lmk_verts[i] < 0 || lmk_verts[i] >= m->V) return fail(FDM_ERR_ARG, "flame_create: lmk_verts element %d = %d (0..%d)", i, lmk_verts[i], m->V - 1);
  if (NL > 0) FCK(finite_field("flame_create", "lmk_bary", lmk_bary, 3LL * NL));
  fdm_flame* F = new (std::nothrow) fdm_flame();
  if (!F) return fail(FDM_ERR_STATE, "flame_create: out of memory");
  const int V = m->V, J = m->J, NB = m->NB, P = 9 * (J - 1);
  const long long V3 = 3LL * V;
  F->V = V; F->J = J; F->NB = NB; F->expr_at = m->expr_at; F->NL = NL;
  F->chunks = (int)((V3 + ROW_CHUNK - 1) / ROW_CHUNK);
  F->parents.assign(m->parents, m->parents + J);
  F->parents[0] = 0;
  return handoff_finish(F, out, [&]() {
    const size_t ld = (size_t)F->chunks * ROW_CHUNK;
    std::vector<float> D((size_t)(NB + P) * ld, 0.f), T(ld, 0.f), JT((size_t)3 * J), JD((size_t)NB * 3 * J);
    tables(m, D.data(), (long long)ld, JT.data(), JD.data());
    for (long long i = 0; i < V3; ++i) T[i] = m->v_template[i];
    FCK(put(F->mem, &F->D, D.data(), D.size()));
    FCK(put(F->mem, &F->T, T.data(), T.size()));
    FCK(put(F->mem, &F->JT, JT.data(), JT.size()));
    FCK(put(F->mem, &F->JD, JD.data(), JD.size()));
    FCK(put(F->mem, &F->wts, m->lbs_weights, (size_t)V * J));
    FCK(put(F->mem, &F->par, F->parents.data(), (size_t)J));
    if (NL) { FCK(put(F->mem, &F->lv, lmk_verts, (size_t)3 * NL)); FCK(put(F->mem, &F->lb, lmk_bary, (size_t)3 * NL)); }
    HIPCK(hipFuncSetAttribute((const void*)flame_skin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)flame_skin_lds(FLAME_NBMAX + 9 * (FLAME_JMAX - 1), FLAME_JMAX)));
    return (int)FDM_OK;
  });
}

int fdm_flame_destroy(fdm_flame* F) { return handoff_destroy(F); }

int fdm_flame_forward(fdm_flame* F, const float* shape, int NS, int shape_rows, const float* expr, int NE, const float* pose, const float* transl,
                      const float* extra, const int* frames, int B, int L_max, float* verts, float* lmk, float* xforms, float* posefeat,
                      void* stream) {
  if (!F || !pose || !verts) return fail(FDM_ERR_ARG, "flame_forward: null argument");
  if (NS < 0 || NS > F->expr_at) return fail(FDM_ERR_ARG, "flame_forward: NS = %d (0..expr_at = %d)", NS, F->expr_at);
  if (NE < 0 || NE > F->NB - F->expr_at) return fail(FDM_ERR_ARG, "flame_forward: NE = %d (0..NB - expr_at = %d)", NE, F->NB - F->expr_at);
  if ((NS > 0 && !shape) || (NE > 0 && !expr)) return fail(FDM_ERR_ARG, "flame_forward: null %s with %d coefficients", NS > 0 && !shape ? "shape" : "expr", NS > 0 && !shape ? NS : NE);
  if (lmk && !F->NL) return fail(FDM_ERR_ARG, "flame_forward: landmarks asked of an object made without an embedding");
  if (B < 1 || L_max < 1) return fail(FDM_ERR_SHAPE, "flame_forward: B = %d, L_max = %d", B, L_max);
  if (shape_rows != 1 && shape_rows != B) return fail(FDM_ERR_ARG, "flame_forward: shape_rows = %d (1 or B = %d)", shape_rows, B);
  std::vector<int> hl;
  const ClipLens c = clip_lens(frames, B, L_max, 0.0, 0.0, 0, hl);
  if (c.bad == ClipLens::LENGTH) return fail(FDM_ERR_SHAPE, "flame_forward: clip %d has %d frames, the batch is %d long", c.clip, c.L, L_max);
  const long long rows = (long long)B * L_max;
  if (rows > 0x7fffffffLL - 64 || F->chunks > 65535)
    return fail(FDM_ERR_SHAPE, "flame_forward: %lld rows of %d vertices exceed one launch", rows, F->V);
  FCK(handoff_device(*F, "flame_forward"));
  hipStream_t s = (hipStream_t)stream;
  const int J = F->J, P = 9 * (J - 1), NT = NE + P, V3 = 3 * F->V, ld = F->chunks * ROW_CHUNK;
  const long long tiles = (rows + ROW_TILE - 1) / ROW_TILE;
  FCK(grow(F->mem, &F->xf, &F->xf_cap, tiles * ROW_TILE * J * 12));
  FCK(grow(F->mem, &F->pf, &F->pf_cap, rows * P));
  FCK(grow(F->mem, &F->cf, &F->cf_cap, tiles * NT * ROW_TILE));
  FCK(grow(F->mem, &F->vid, &F->vid_cap, (long long)shape_rows * ld));
  FCK(handoff_lens(*F, hl, s));
  flame_launch_pose(F, shape, shape_rows, NS, expr, NE, pose, L_max, rows, s);
  flame_launch_shape(F, shape, NS, shape_rows, s);
  FlameSkinArgs a;
  a.vid = F->vid; a.shape_rows = shape_rows; a.D = F->D; a.ld = ld;
  a.row_expr = F->expr_at; a.NE = NE; a.row_pose = F->NB; a.P = P;
  a.cf = F->cf; a.xf = F->xf; a.wts = F->wts; a.J = J; a.transl = transl; a.extra = extra;
  a.lens = F->lens; a.L_max = L_max; a.rows = (int)rows; a.V3 = V3; a.out = verts;
  hipLaunchKernelGGL(flame_skin_kernel, dim3((unsigned)tiles, (unsigned)F->chunks), dim3(64), flame_skin_lds(NT, J), s, a);
  if (lmk)
    hipLaunchKernelGGL(flame_lmk_kernel, dim3((unsigned)((rows * F->NL + 255) / 256)), dim3(256), 0, s, (const float*)verts, (const int*)F->lens, L_max,
                       (int)rows, V3, (const int*)F->lv, (const float*)F->lb, F->NL, lmk);
  HIPCK(hipGetLastError());
  if (xforms) HIPCK(hipMemcpyAsync(xforms, F->xf, (size_t)rows * J * 12 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (posefeat && P) HIPCK(hipMemcpyAsync(posefeat, F->pf, (size_t)rows * P * sizeof(float), hipMemcpyDeviceToDevice, s));
  return FDM_OK;
}

}  // extern "C"
