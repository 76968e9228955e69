// Host side of the rig hand-off under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the fp64 Gram matrix
// and its Cholesky factor, fdm_rig_create's checks with the rank-deficient path, fdm_rig_forward's argument checks and destroy
// (csrc/rig_out.hip; the frame rule is host.hpp's), with the two symbols that unit takes from fdm_hip.hip supplied here (no device is
// ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/rig_host_check.cpp rig_out.hip -o ../../tools/_build/rig_host_check
//   ../../tools/_build/rig_host_check          -> "rig_host_check ok", exit status 0
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../include/fdm_hip.h"

namespace fdm {
static std::string g_err;
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace fdm
extern "C" int fdm_device_ok(void) { return 0; }

#define EXPECT(cond) do { if (!(cond)) { printf("FAIL line %d: %s (last error: %s)\n", __LINE__, #cond, fdm::g_err.c_str()); return 1; } } while (0)

int main() {
  // a seeded basis (an LCG: no library state), per-vertex weights, exactly sized buffers
  const int K = 37, V = 211, V3 = 3 * V;
  std::vector<float> E((size_t)K * V3), w(V);
  unsigned s = 12345u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)((s >> 8) & 0xffff) / 65536.f - 0.5f; };
  for (auto& e : E) e = next();
  for (auto& x : w) x = 1.f + next();
  const double ridge = 0.25;
  std::vector<double> G((size_t)K * K, -1.0);
  std::vector<float> Lc((size_t)K * K, -1.f);
  EXPECT(fdm_rig_gram_host(E.data(), w.data(), K, V, ridge, G.data(), Lc.data()) == FDM_OK);
  double worst_g = 0.0, worst_l = 0.0;
  for (int a = 0; a < K; ++a)
    for (int b = 0; b < K; ++b) {
      long double t = a == b ? ridge : 0.0;
      for (int i = 0; i < V3; ++i) t += (long double)E[(size_t)a * V3 + i] * w[i / 3] * E[(size_t)b * V3 + i];
      worst_g = std::fmax(worst_g, std::fabs((double)t - G[(size_t)a * K + b]));
      EXPECT(G[(size_t)a * K + b] == G[(size_t)b * K + a]);
      long double ll = 0.0;                                  // L L^T gives G back to fp32 rounding of L
      for (int q = 0; q < K; ++q) ll += (long double)Lc[(size_t)a * K + q] * Lc[(size_t)b * K + q];
      worst_l = std::fmax(worst_l, std::fabs((double)ll - G[(size_t)a * K + b]));
      if (b > a) EXPECT(Lc[(size_t)a * K + b] == 0.f);
    }
  EXPECT(worst_g <= 1e-10 && worst_l <= 1e-4);
  EXPECT(fdm_rig_gram_host(E.data(), nullptr, K, V, 0.0, G.data(), Lc.data()) == FDM_OK);
  EXPECT(fdm_rig_gram_host(nullptr, w.data(), K, V, ridge, G.data(), Lc.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_gram_host(E.data(), w.data(), K, V, ridge, nullptr, Lc.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_gram_host(E.data(), w.data(), K, V, ridge, G.data(), nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_gram_host(E.data(), w.data(), 0, V, ridge, G.data(), Lc.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_gram_host(E.data(), w.data(), 129, V, ridge, G.data(), Lc.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_gram_host(E.data(), w.data(), K, 0, ridge, G.data(), Lc.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_gram_host(E.data(), w.data(), K, V, -1.0, G.data(), Lc.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_gram_host(E.data(), w.data(), K, V, NAN, G.data(), Lc.data()) == FDM_ERR_ARG);

  // create: every refusal, the rank-deficient path (two equal rows, no ridge; all-zero weights), then the object without a device
  std::vector<float> lo(K, 0.f), hi(K, 1.f);
  fdm_rig* r = nullptr;
  EXPECT(fdm_rig_create(E.data(), K, V, w.data(), ridge, lo.data(), hi.data(), 16, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_create(nullptr, K, V, w.data(), ridge, lo.data(), hi.data(), 16, &r) == FDM_ERR_ARG);
  EXPECT(fdm_rig_create(E.data(), 0, V, w.data(), ridge, lo.data(), hi.data(), 16, &r) == FDM_ERR_ARG);
  EXPECT(fdm_rig_create(E.data(), K, V, w.data(), INFINITY, lo.data(), hi.data(), 16, &r) == FDM_ERR_ARG);
  EXPECT(fdm_rig_create(E.data(), K, V, w.data(), ridge, lo.data(), nullptr, 16, &r) == FDM_ERR_ARG);
  EXPECT(fdm_rig_create(E.data(), K, V, w.data(), ridge, nullptr, hi.data(), 16, &r) == FDM_ERR_ARG);
  EXPECT(fdm_rig_create(E.data(), K, V, w.data(), ridge, lo.data(), hi.data(), -1, &r) == FDM_ERR_ARG);
  { std::vector<float> bad = w; bad[V - 1] = -0.5f; EXPECT(fdm_rig_create(E.data(), K, V, bad.data(), ridge, lo.data(), hi.data(), 16, &r) == FDM_ERR_ARG); }
  { std::vector<float> bad = w; bad[0] = NAN; EXPECT(fdm_rig_create(E.data(), K, V, bad.data(), ridge, lo.data(), hi.data(), 16, &r) == FDM_ERR_ARG); }
  { std::vector<float> bad = lo; bad[K - 1] = 2.f; EXPECT(fdm_rig_create(E.data(), K, V, w.data(), ridge, bad.data(), hi.data(), 16, &r) == FDM_ERR_ARG); }
  { std::vector<float> bad = hi; bad[3] = INFINITY; EXPECT(fdm_rig_create(E.data(), K, V, w.data(), ridge, lo.data(), bad.data(), 16, &r) == FDM_ERR_ARG); }
  std::vector<float> twin = E;
  for (int i = 0; i < V3; ++i) twin[(size_t)(K - 1) * V3 + i] = twin[(size_t)5 * V3 + i];
  EXPECT(fdm_rig_create(twin.data(), K, V, w.data(), 0.0, lo.data(), hi.data(), 16, &r) == FDM_ERR_ARG);
  EXPECT(fdm::g_err.find("basis is rank deficient under these weights: raise ridge") != std::string::npos);
  const std::string deficient = fdm::g_err;
  std::vector<float> none(V, 0.f);
  EXPECT(fdm_rig_create(E.data(), K, V, none.data(), 0.0, lo.data(), hi.data(), 16, &r) == FDM_ERR_ARG && r == nullptr);
  EXPECT(fdm_rig_create(twin.data(), K, V, w.data(), 1e-3, nullptr, nullptr, 0, &r) == FDM_OK && r != nullptr);
  EXPECT(fdm_rig_destroy(r) == FDM_OK);
  r = nullptr;
  EXPECT(fdm_rig_create(E.data(), K, V, w.data(), ridge, lo.data(), hi.data(), 16, &r) == FDM_OK && r != nullptr);
  const int B = 3, L_max = 7;
  const int frames[B] = {7, 1, 4};
  int got[B] = {0, 0, 0};
  const float* x = (const float*)0x1000;           // never dereferenced: no call gets as far as a launch
  float* y = (float*)0x2000;
  EXPECT(fdm_rig_forward(nullptr, x, frames, B, L_max, 30, 60, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_forward(r, nullptr, frames, B, L_max, 30, 60, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_forward(r, x, frames, B, L_max, 30, 60, nullptr, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_forward(r, x, frames, B, L_max, -30, 60, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_forward(r, x, frames, B, L_max, 30, NAN, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_forward(r, x, frames, 0, L_max, 30, 60, y, y, 14, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_rig_forward(r, x, frames, B, 6, 30, 60, y, y, 14, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_rig_forward(r, x, frames, B, L_max, 30, 60, y, y, 13, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_rig_forward(r, x, frames, B, L_max, 0, 0, y, y, 6, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(got[0] == 0 && got[1] == 0 && got[2] == 0);
  EXPECT(fdm_rig_forward(r, x, frames, B, L_max, 30, 60, y, y, 14, got, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_rig_forward(r, x, nullptr, B, L_max, 30, 25, y, nullptr, 5, nullptr, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_rig_destroy(r) == FDM_OK && fdm_rig_destroy(nullptr) == FDM_OK);
  printf("rig_host_check ok (K = %d over %d vertices: max |G - long double| = %.2e, max |L L^T - G| = %.2e; refused: \"%s\")\n", K, V, worst_g,
         worst_l, deficient.c_str());
  return 0;
}
