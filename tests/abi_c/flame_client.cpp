// Parameters to posed vertices without Python or torch: fdm_flame_create -> fdm_flame_forward on one seeded synthetic head (an odd vertex
// count over two chunks, a three-joint chain, shape and expression coefficients, translation, extra displacements, landmarks, two clips
// of unequal length), compared with the rule of include/fdm_hip.h evaluated in this program in fp64 from the model's own arrays.
// Tolerance per element, a priori: (n + 2) 2^-24 S for the blend and the skinning (n accumulated terms, S the expression with every
// term replaced by its absolute value) plus what an error e in every transform and pose-feature entry can move the vertex by, with
// e = 64 (depth + 1) 2^-24 max(1, |joint|): a few dozen fp32 operations per chain level on entries of that size.
// Built and run by tests/test_flame_out_gpu.py:
//   hipcc flame_client.cpp -I include -L <dir> -lfdm_hip ; flame_client
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "fdm_hip.h"

#define CK(x) do { if ((x) != 0) { printf("FAIL %s: %s\n", #x, fdm_last_error()); return 1; } } while (0)
#define HK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static unsigned g_s = 97531u;
static float rnd() { g_s = g_s * 1664525u + 1013904223u; return (float)((g_s >> 8) & 0xffff) / 65536.f - 0.5f; }

template <typename T> static int up(T** d, const std::vector<T>& h) {
  HK(hipMalloc(d, h.size() * sizeof(T) + 16));
  HK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

int main() {
  if (!fdm_device_ok()) { printf("no gfx950 device\n"); return 2; }
  const int V = 301, J = 3, NB = 6, expr_at = 4, NS = 3, NE = 2, P = 9 * (J - 1), V3 = 3 * V, B = 2, L = 5, NL = 2;
  const int parents[J] = {0, 0, 1}, frames[B] = {5, 3};
  std::vector<float> vt(V3), sd((size_t)V3 * NB), pd((size_t)P * V3), jr((size_t)J * V, 0.f), w((size_t)V * J);
  for (auto& x : vt) x = 0.2f * rnd();
  for (auto& x : sd) x = 0.02f * rnd();
  for (auto& x : pd) x = 0.02f * rnd();
  for (int j = 0; j < J; ++j) for (int i = 0; i < 4; ++i) jr[(size_t)j * V + (37 * j + 11 * i) % V] = 0.25f;
  for (int v = 0; v < V; ++v) { float s = 0.f; for (int j = 0; j < J; ++j) s += (w[(size_t)v * J + j] = 0.55f + rnd()); for (int j = 0; j < J; ++j) w[(size_t)v * J + j] /= s; }
  const int lv[3 * NL] = {0, 150, 300, 7, 8, 9};
  const float lb[3 * NL] = {0.2f, 0.3f, 0.5f, 0.6f, 0.3f, 0.1f};
  const int rows = B * L;
  std::vector<float> shape(NS), expr((size_t)rows * NE), pose((size_t)rows * 3 * J), transl((size_t)rows * 3), extra((size_t)rows * V3);
  for (auto& x : shape) x = 2.f * rnd();
  for (auto& x : expr) x = 2.f * rnd();
  for (auto& x : pose) x = 1.2f * rnd();
  for (int i = 0; i < 3 * J; ++i) { pose[i] = 0.f; pose[3 * J + i] = (i % 3 == 1) ? 1.5707964f : 0.f; pose[2 * 3 * J + i] = (i % 3 == 0) ? 2.f : -1.75f; }   // zero, a quarter turn, > pi
  for (auto& x : transl) x = rnd();
  for (auto& x : extra) x = 0.02f * rnd();

  const fdm_flame_model m = {V, J, NB, expr_at, vt.data(), sd.data(), pd.data(), jr.data(), parents, w.data()};
  std::vector<float> D((size_t)(NB + P) * V3), JT(3 * J), JD((size_t)NB * 3 * J);
  CK(fdm_flame_tables_host(&m, D.data(), JT.data(), JD.data()));
  for (int k = 0; k < NB; ++k) for (int i = 0; i < V3; ++i) if (D[(size_t)k * V3 + i] != sd[(size_t)i * NB + k]) { printf("FAIL: D is not shapedirs transposed\n"); return 1; }
  fdm_flame* f = nullptr;
  CK(fdm_flame_create(&m, lv, lb, NL, &f));

  hipStream_t st;
  HK(hipStreamCreate(&st));
  float *d_shape, *d_expr, *d_pose, *d_tr, *d_x, *d_out, *d_lmk, *d_xf, *d_pf;
  if (up(&d_shape, shape) || up(&d_expr, expr) || up(&d_pose, pose) || up(&d_tr, transl) || up(&d_x, extra)) return 1;
  const size_t n_out = (size_t)rows * V3, n_lmk = (size_t)rows * NL * 3, n_xf = (size_t)rows * J * 12, n_pf = (size_t)rows * P;
  HK(hipMalloc(&d_out, n_out * 4)); HK(hipMalloc(&d_lmk, n_lmk * 4)); HK(hipMalloc(&d_xf, n_xf * 4)); HK(hipMalloc(&d_pf, n_pf * 4));
  HK(hipMemset(d_out, 0xff, n_out * 4)); HK(hipMemset(d_lmk, 0xff, n_lmk * 4));          // NaN everywhere: the call writes its outputs whole
  // refusals come back as codes, before any launch
  if (fdm_flame_forward(f, d_shape, expr_at + 1, 1, d_expr, NE, d_pose, d_tr, d_x, frames, B, L, d_out, d_lmk, d_xf, d_pf, st) != FDM_ERR_ARG) { printf("FAIL: NS > expr_at accepted\n"); return 1; }
  if (fdm_flame_forward(f, d_shape, NS, 1, d_expr, NE, d_pose, d_tr, d_x, frames, B, L - 1, d_out, d_lmk, d_xf, d_pf, st) != FDM_ERR_SHAPE) { printf("FAIL: a clip longer than the batch accepted\n"); return 1; }
  CK(fdm_flame_forward(f, d_shape, NS, 1, d_expr, NE, d_pose, d_tr, d_x, frames, B, L, d_out, d_lmk, d_xf, d_pf, st));
  HK(hipStreamSynchronize(st));
  std::vector<float> out(n_out), lmk(n_lmk);
  HK(hipMemcpy(out.data(), d_out, n_out * 4, hipMemcpyDeviceToHost));
  HK(hipMemcpy(lmk.data(), d_lmk, n_lmk * 4, hipMemcpyDeviceToHost));

  const double u = std::ldexp(1.0, -24);
  const int n_terms = (1 + NS + NE + P + 1) + J + 4 + 1;
  double worst = 0.0, worst_abs = 0.0;
  std::vector<double> Dp(V3, 0.0);
  for (int p = 0; p < P; ++p) for (int i = 0; i < V3; ++i) Dp[i] += std::fabs((double)pd[(size_t)p * V3 + i]);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < L; ++t) {
      const int row = b * L + t;
      const float* o = out.data() + (size_t)row * V3;
      if (t >= frames[b]) {
        for (int i = 0; i < V3; ++i) if (o[i] != 0.f) { printf("FAIL: row %d past its clip is not zero\n", row); return 1; }
        for (int i = 0; i < NL * 3; ++i) if (lmk[(size_t)row * NL * 3 + i] != 0.f) { printf("FAIL: landmark row %d past its clip is not zero\n", row); return 1; }
        continue;
      }
      // v_shaped and the joints regressed from it
      std::vector<double> vs(V3), va(V3);
      for (int i = 0; i < V3; ++i) {
        double s = vt[i], a = std::fabs((double)vt[i]);
        for (int k = 0; k < NS; ++k) { const double c = (double)shape[k] * sd[(size_t)i * NB + k]; s += c; a += std::fabs(c); }
        for (int k = 0; k < NE; ++k) { const double c = (double)expr[(size_t)row * NE + k] * sd[(size_t)i * NB + expr_at + k]; s += c; a += std::fabs(c); }
        vs[i] = s; va[i] = a;
      }
      double Jf[J][3], jmax = 1.0;
      for (int j = 0; j < J; ++j) for (int a = 0; a < 3; ++a) {
        double s = 0.0;
        for (int v = 0; v < V; ++v) s += (double)jr[(size_t)j * V + v] * vs[3 * v + a];
        Jf[j][a] = s; jmax = std::fmax(jmax, std::fabs(s));
      }
      double R[J][9], G[J][12], A[J][12], pf[P > 0 ? P : 1];
      int depth = 0, dj[J] = {0, 0, 0};
      for (int j = 0; j < J; ++j) {
        const double rx = pose[(size_t)row * 3 * J + 3 * j], ry = pose[(size_t)row * 3 * J + 3 * j + 1], rz = pose[(size_t)row * 3 * J + 3 * j + 2];
        const double ex = rx + 1e-8, ey = ry + 1e-8, ez = rz + 1e-8, ang = std::sqrt(ex * ex + ey * ey + ez * ez);
        const double x = rx / ang, y = ry / ang, z = rz / ang, s = std::sin(ang), c1 = 1.0 - std::cos(ang);
        const double K[9] = {0, -z, y, z, 0, -x, -y, x, 0};
        const double KK[9] = {-(y * y + z * z), x * y, x * z, x * y, -(x * x + z * z), y * z, x * z, y * z, -(x * x + y * y)};
        for (int e = 0; e < 9; ++e) R[j][e] = (e % 4 == 0 ? 1.0 : 0.0) + s * K[e] + c1 * KK[e];
        if (j >= 1) for (int e = 0; e < 9; ++e) pf[9 * (j - 1) + e] = R[j][e] - (e % 4 == 0 ? 1.0 : 0.0);
        if (j == 0) {
          for (int a = 0; a < 3; ++a) { for (int c = 0; c < 3; ++c) G[0][4 * a + c] = R[0][3 * a + c]; G[0][4 * a + 3] = Jf[0][a]; }
        } else {
          const int p = parents[j];
          dj[j] = dj[p] + 1; depth = dj[j] > depth ? dj[j] : depth;
          for (int a = 0; a < 3; ++a) {
            for (int c = 0; c < 3; ++c) G[j][4 * a + c] = G[p][4 * a] * R[j][c] + G[p][4 * a + 1] * R[j][3 + c] + G[p][4 * a + 2] * R[j][6 + c];
            G[j][4 * a + 3] = G[p][4 * a] * (Jf[j][0] - Jf[p][0]) + G[p][4 * a + 1] * (Jf[j][1] - Jf[p][1]) + G[p][4 * a + 2] * (Jf[j][2] - Jf[p][2]) + G[p][4 * a + 3];
          }
        }
        for (int a = 0; a < 3; ++a) {
          for (int c = 0; c < 3; ++c) A[j][4 * a + c] = G[j][4 * a + c];
          A[j][4 * a + 3] = G[j][4 * a + 3] - (G[j][4 * a] * Jf[j][0] + G[j][4 * a + 1] * Jf[j][1] + G[j][4 * a + 2] * Jf[j][2]);
        }
      }
      const double e_pose = 64.0 * (depth + 1) * u * jmax;
      std::vector<double> want(V3);
      for (int v = 0; v < V; ++v) {
        double p3[3], a3[3];
        for (int a = 0; a < 3; ++a) {
          const int i = 3 * v + a;
          double s = vs[i], q = va[i];
          for (int p = 0; p < P; ++p) { const double c = pf[p] * pd[(size_t)p * V3 + i]; s += c; q += std::fabs(c); }
          const double x = extra[(size_t)row * V3 + i];
          p3[a] = s + x; a3[a] = q + std::fabs(x);
        }
        double T[12], Ta[12], W = 0.0;
        for (int e = 0; e < 12; ++e) { T[e] = 0.0; Ta[e] = 0.0; }
        for (int j = 0; j < J; ++j) { const double wj = w[(size_t)v * J + j]; W += std::fabs(wj); for (int e = 0; e < 12; ++e) { T[e] += wj * A[j][e]; Ta[e] += std::fabs(wj * A[j][e]); } }
        for (int c = 0; c < 3; ++c) {
          const double tr = transl[(size_t)row * 3 + c];
          const double val = T[4 * c] * p3[0] + T[4 * c + 1] * p3[1] + T[4 * c + 2] * p3[2] + T[4 * c + 3] + tr;
          const double S = Ta[4 * c] * a3[0] + Ta[4 * c + 1] * a3[1] + Ta[4 * c + 2] * a3[2] + Ta[4 * c + 3] + std::fabs(tr);
          const double prop = e_pose * W * (a3[0] + a3[1] + a3[2] + 1.0) + e_pose * (Ta[4 * c] * Dp[3 * v] + Ta[4 * c + 1] * Dp[3 * v + 1] + Ta[4 * c + 2] * Dp[3 * v + 2]);
          const double tol = (n_terms + 2) * u * S + prop, err = std::fabs((double)o[3 * v + c] - val);
          want[3 * v + c] = val;
          if (!(err <= tol)) { printf("FAIL: row %d vertex %d.%d: %.9g, fp64 %.9g, |err| %.3g > %.3g\n", row, v, c, (double)o[3 * v + c], val, err, tol); return 1; }
          worst = std::fmax(worst, err / tol); worst_abs = std::fmax(worst_abs, err);
        }
      }
      for (int l = 0; l < NL; ++l) for (int c = 0; c < 3; ++c) {      // landmarks from the device's own vertices: three terms
        double s = 0.0, q = 0.0;
        for (int k = 0; k < 3; ++k) { const double term = (double)lb[3 * l + k] * o[3 * lv[3 * l + k] + c]; s += term; q += std::fabs(term); }
        if (!(std::fabs((double)lmk[((size_t)row * NL + l) * 3 + c] - s) <= 5 * u * q)) { printf("FAIL: row %d landmark %d.%d\n", row, l, c); return 1; }
      }
    }
  CK(fdm_flame_destroy(f));
  HK(hipFree(d_shape)); HK(hipFree(d_expr)); HK(hipFree(d_pose)); HK(hipFree(d_tr)); HK(hipFree(d_x)); HK(hipFree(d_out)); HK(hipFree(d_lmk)); HK(hipFree(d_xf)); HK(hipFree(d_pf));
  printf("flame_client ok (%d vertices, %d joints, %d + %d frames: max |device - fp64| = %.2e, worst err / tolerance = %.3f, libfdm_hip version %d)\n", V, J, frames[0],
         frames[1], worst_abs, worst, fdm_version());
  return 0;
}
