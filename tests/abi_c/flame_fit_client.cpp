// Vertices to parameters without Python or torch: fdm_flame_create -> fdm_flame_forward (the targets, from known parameters) ->
// fdm_flame_fit_create / _set / _forward on one seeded synthetic head (an odd vertex count over two chunks, a three-joint chain, two
// clips of unequal length; expression coefficients and the last joint free).  The program checks the refusals that come back as codes,
// that every live row ends with status 0 and an rms below 1e-4 of the head's size (a loose sanity figure: the bounds live in
// tests/flame_fit_cases.py), that dead rows are zeros, and that a second call gives the same bits.  With a path as its argument it
// writes the model, the targets and its outputs there, and tests/test_flame_fit_gpu.py repeats the call through Python on the same
// inputs and compares bit for bit.
// Built and run by tests/test_flame_fit_gpu.py:
//   hipcc flame_fit_client.cpp -I include -L <dir> -lfdm_hip ; flame_fit_client [dump.bin]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fdm_hip.h"

#define CK(x) do { if ((x) != 0) { printf("FAIL %s: %s\n", #x, fdm_last_error()); return 1; } } while (0)
#define HK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static unsigned g_s = 24680u;
static float rnd() { g_s = g_s * 1664525u + 1013904223u; return (float)((g_s >> 8) & 0xffff) / 65536.f - 0.5f; }

template <typename T> static int up(T** d, const std::vector<T>& h) {
  HK(hipMalloc(d, h.size() * sizeof(T) + 16));
  HK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
template <typename T> static void put(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
  if (!fdm_device_ok()) { printf("no gfx950 device\n"); return 2; }
  const int V = 301, J = 3, NB = 6, expr_at = 2, NE = 4, P = 9 * (J - 1), V3 = 3 * V, B = 2, L = 5, iters = 12;
  const int parents[J] = {0, 0, 1}, frames[B] = {5, 3}, free_j[1] = {2};
  std::vector<float> vt(V3), sd((size_t)V3 * NB), pd((size_t)P * V3), jr((size_t)J * V, 0.f), w((size_t)V * J);
  for (auto& x : vt) x = 0.2f * rnd();
  for (auto& x : sd) x = 0.02f * rnd();
  for (auto& x : pd) x = 0.02f * rnd();
  for (int j = 0; j < J; ++j) for (int i = 0; i < 4; ++i) jr[(size_t)j * V + (37 * j + 11 * i) % V] = 0.25f;
  for (int v = 0; v < V; ++v) { float s = 0.f; for (int j = 0; j < J; ++j) s += (w[(size_t)v * J + j] = 0.55f + rnd()); for (int j = 0; j < J; ++j) w[(size_t)v * J + j] /= s; }
  const int rows = B * L;
  std::vector<float> expr((size_t)rows * NE), pose((size_t)rows * 3 * J, 0.f);
  for (auto& x : expr) x = 3.f * rnd();
  for (int r = 0; r < rows; ++r) for (int c = 0; c < 3; ++c) pose[(size_t)r * 3 * J + 3 * free_j[0] + c] = 0.4f * rnd();

  const fdm_flame_model m = {V, J, NB, expr_at, vt.data(), sd.data(), pd.data(), jr.data(), parents, w.data()};
  fdm_flame* head = nullptr;
  CK(fdm_flame_create(&m, nullptr, nullptr, 0, &head));
  hipStream_t st;
  HK(hipStreamCreate(&st));
  float *d_expr, *d_pose, *d_y, *d_e, *d_p, *d_rms;
  int* d_st;
  if (up(&d_expr, expr) || up(&d_pose, pose)) return 1;
  const size_t n_y = (size_t)rows * V3, n_e = (size_t)rows * NE, n_p = (size_t)rows * 3 * J;
  HK(hipMalloc(&d_y, n_y * 4)); HK(hipMalloc(&d_e, n_e * 4)); HK(hipMalloc(&d_p, n_p * 4)); HK(hipMalloc(&d_rms, rows * 4)); HK(hipMalloc(&d_st, rows * 4));
  CK(fdm_flame_forward(head, nullptr, 0, 1, d_expr, NE, d_pose, nullptr, nullptr, frames, B, L, d_y, nullptr, nullptr, nullptr, st));
  HK(hipStreamSynchronize(st));
  std::vector<float> y(n_y);
  HK(hipMemcpy(y.data(), d_y, n_y * 4, hipMemcpyDeviceToHost));

  fdm_flame_fit* fit = nullptr;
  const int twice[2] = {2, 2};
  if (fdm_flame_fit_create(head, twice, 2, NE, 0, nullptr, &fit) != FDM_ERR_ARG) { printf("FAIL: a joint given twice accepted\n"); return 1; }
  if (fdm_flame_fit_create(head, free_j, 1, NE + 1, 0, nullptr, &fit) != FDM_ERR_ARG) { printf("FAIL: n_expr > NE accepted\n"); return 1; }
  CK(fdm_flame_fit_create(head, free_j, 1, NE, 0, nullptr, &fit));
  if (fdm_flame_fit_set(fit, "iters", 0) != FDM_ERR_ARG || fdm_flame_fit_set(fit, "lambda", -1) != FDM_ERR_ARG) { printf("FAIL: a bad setting accepted\n"); return 1; }
  CK(fdm_flame_fit_set(fit, "iters", iters));
  if (fdm_flame_fit_forward(fit, d_y, nullptr, 0, 1, nullptr, frames, B, L - 1, d_e, d_p, nullptr, d_rms, nullptr, d_st, st) != FDM_ERR_SHAPE) { printf("FAIL: a clip longer than the batch accepted\n"); return 1; }
  std::vector<float> e1(n_e), p1(n_p), rms(rows), e2(n_e), p2(n_p);
  std::vector<int> status(rows);
  for (int pass = 0; pass < 2; ++pass) {
    HK(hipMemsetAsync(d_e, 0xff, n_e * 4, st)); HK(hipMemsetAsync(d_p, 0xff, n_p * 4, st));          // NaN everywhere: the call writes its outputs whole
    CK(fdm_flame_fit_forward(fit, d_y, nullptr, 0, 1, nullptr, frames, B, L, d_e, d_p, nullptr, d_rms, nullptr, d_st, st));
    HK(hipStreamSynchronize(st));
    HK(hipMemcpy((pass ? e2 : e1).data(), d_e, n_e * 4, hipMemcpyDeviceToHost));
    HK(hipMemcpy((pass ? p2 : p1).data(), d_p, n_p * 4, hipMemcpyDeviceToHost));
  }
  HK(hipMemcpy(rms.data(), d_rms, rows * 4, hipMemcpyDeviceToHost));
  HK(hipMemcpy(status.data(), d_st, rows * 4, hipMemcpyDeviceToHost));
  if (memcmp(e1.data(), e2.data(), n_e * 4) || memcmp(p1.data(), p2.data(), n_p * 4)) { printf("FAIL: two calls differ\n"); return 1; }
  double worst_rms = 0.0, worst_par = 0.0;
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < L; ++t) {
      const int r = b * L + t;
      const bool live = t < frames[b];
      if (!live) {
        for (int k = 0; k < NE; ++k) if (e1[(size_t)r * NE + k] != 0.f) { printf("FAIL: dead row %d has expression %g\n", r, e1[(size_t)r * NE + k]); return 1; }
        for (int k = 0; k < 3 * J; ++k) if (p1[(size_t)r * 3 * J + k] != 0.f) { printf("FAIL: dead row %d has pose %g\n", r, p1[(size_t)r * 3 * J + k]); return 1; }
        if (rms[r] != 0.f || status[r] != 0) { printf("FAIL: dead row %d has rms %g, status %d\n", r, rms[r], status[r]); return 1; }
        continue;
      }
      if (status[r] != 0) { printf("FAIL: row %d failed at column %d\n", r, status[r] - 1); return 1; }
      worst_rms = std::fmax(worst_rms, (double)rms[r]);
      for (int k = 0; k < NE; ++k) worst_par = std::fmax(worst_par, std::fabs((double)e1[(size_t)r * NE + k] - expr[(size_t)r * NE + k]));
      for (int k = 0; k < 3 * J; ++k) worst_par = std::fmax(worst_par, std::fabs((double)p1[(size_t)r * 3 * J + k] - pose[(size_t)r * 3 * J + k]));
    }
  if (!(worst_rms < 1e-4 * 0.2)) { printf("FAIL: rms %g after %d iterations\n", worst_rms, iters); return 1; }
  if (argc > 1) {
    FILE* f = fopen(argv[1], "wb");
    if (!f) { printf("FAIL: cannot write %s\n", argv[1]); return 1; }
    const int hdr[10] = {V, J, NB, expr_at, NE, 1, 0, B, L, iters};
    fwrite(hdr, 4, 10, f); fwrite(free_j, 4, 1, f); fwrite(frames, 4, B, f); fwrite(parents, 4, J, f);
    put(f, vt); put(f, sd); put(f, pd); put(f, jr); put(f, w); put(f, y); put(f, e1); put(f, p1); put(f, rms); put(f, status);
    fclose(f);
  }
  CK(fdm_flame_fit_destroy(fit));
  CK(fdm_flame_destroy(head));
  printf("flame_fit_client ok (%d vertices, %d joints, %d + %d frames, %d iterations: rms max %.3g, max |parameter - truth| %.3g, libfdm_hip version %d)\n",
         V, J, frames[0], frames[1], iters, worst_rms, worst_par, fdm_version());
  return 0;
}
