// Host side of the time filter hand-off under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the fp64 taps
// (fdm_tfilter_taps_host) into exactly sized buffers and every refusal of fdm_tfilter_create and fdm_tfilter_forward (csrc/tfilter.hip),
// with the two symbols that unit takes from fdm_hip.hip supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/tfilter_host_check.cpp tfilter.hip -o ../../tools/_build/tfilter_host_check
//   ../../tools/_build/tfilter_host_check          -> "tfilter_host_check ok", exit status 0
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

static double full_sum(const std::vector<double>& h) {
  double s = h[0];
  for (size_t k = 1; k < h.size(); ++k) s += 2.0 * h[k];
  return s;
}

int main() {
  // taps into buffers of exactly R + 1 doubles: every radius, both kinds, every order the window admits
  int made = 0;
  for (int R = 0; R <= 32; ++R) {
    std::vector<double> h((size_t)R + 1, -7.0);
    EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, R, 0.4 + 0.3 * R, h.data()) == FDM_OK);
    EXPECT(std::fabs(full_sum(h) - 1.0) < 1e-14);
    for (int k = 1; k <= R; ++k) EXPECT(h[k] > 0.0 && h[k] <= h[k - 1]);
    ++made;
    for (int order = 2; order <= 5; ++order) {
      std::vector<double> g((size_t)R + 1, -7.0);
      const int rc = fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, R, (double)order, g.data());
      if (order >= 2 * R + 1) { EXPECT(rc == FDM_ERR_ARG && g[0] == -7.0); continue; }
      EXPECT(rc == FDM_OK && std::fabs(full_sum(g) - 1.0) < 1e-12);      // the fit reproduces a constant
      ++made;
    }
  }
  {
    std::vector<double> g(5), c(5);          // order 2 at R = 4 is the classic (59, 54, 39, 14, -21) / 231
    const double want[5] = {59.0, 54.0, 39.0, 14.0, -21.0};
    EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 4, 2.0, g.data()) == FDM_OK && fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 4, 3.0, c.data()) == FDM_OK);
    for (int k = 0; k < 5; ++k) EXPECT(std::fabs(g[k] - want[k] / 231.0) < 1e-14 && std::fabs(c[k] - g[k]) < 1e-14);
  }
  std::vector<double> h(33);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, 4, 1.0, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, -1, 1.0, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, 33, 1.0, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, 4, 0.0, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, 4, -2.0, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, 4, (double)NAN, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, 4, (double)INFINITY, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 8, 0.0, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 8, 1.0, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 8, 1e300, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 8, 6.0, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 8, 2.5, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 8, (double)NAN, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_SAVGOL, 1, 3.0, h.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_taps_host(2, 8, 2.0, h.data()) == FDM_ERR_ARG);

  // the object without a device: create validates (exactly sized taps and strength), forward refuses in order and ends in FDM_ERR_STATE
  const int V = 7, R = 3;
  std::vector<float> taps((size_t)R + 1), s((size_t)V);
  std::vector<double> hd((size_t)R + 1);
  EXPECT(fdm_tfilter_taps_host(FDM_TFILTER_GAUSSIAN, R, 1.2, hd.data()) == FDM_OK);
  for (int k = 0; k <= R; ++k) taps[k] = (float)hd[k];
  for (int v = 0; v < V; ++v) s[v] = (float)v / (float)(V - 1);
  fdm_tfilter* T = nullptr;
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_create(V, R, nullptr, s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create(0, R, taps.data(), nullptr, FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create(-2, R, taps.data(), nullptr, FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create(V, -1, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create(V, 33, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  taps[R] = NAN;
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  taps[R] = -INFINITY;
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  taps[R] = (float)hd[R];
  s[V - 1] = 1.0001f;
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  s[V - 1] = -0.5f;
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  s[V - 1] = NAN;
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  s[V - 1] = 1.f;
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), 2, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), -1, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  fdm_tfilter* T0 = nullptr;
  EXPECT(fdm_tfilter_create(V, 0, taps.data(), nullptr, FDM_TFILTER_NEAREST, nullptr, &T0) == FDM_OK && T0 != nullptr);
  EXPECT(fdm_tfilter_create(V, R, taps.data(), s.data(), FDM_TFILTER_MIRROR, nullptr, &T) == FDM_OK && T != nullptr);

  const int B = 3, L_max = 7;
  const int lens[B] = {7, 1, 4}, zero[B] = {7, 0, 4}, neg[B] = {-1, 1, 4}, big[B] = {7, 1, 8};
  const float* x = (const float*)0x100000;          // never dereferenced: no call gets as far as a launch
  float* y = (float*)0x200000;
  const long long n = (long long)B * L_max * 3 * V;      // floats of the batch
  EXPECT(fdm_tfilter_forward(nullptr, x, lens, B, L_max, y) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward(T, nullptr, lens, B, L_max, y) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward(T, x, lens, 0, L_max, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward(T, x, lens, -1, L_max, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward(T, x, nullptr, B, 0, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward(T, x, zero, B, L_max, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward(T, x, neg, B, L_max, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward(T, x, big, B, L_max, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, 6, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, (float*)x) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, (float*)x + 1) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, (float*)x + (n - 1)) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, (float*)x - (n - 1)) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, (float*)x + n) == FDM_ERR_STATE);       // adjacent: no overlap, as far as the device check
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, (float*)x - n) == FDM_ERR_STATE);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, y) == FDM_ERR_STATE);
  EXPECT(fdm_tfilter_forward(T0, x, nullptr, B, L_max, y) == FDM_ERR_STATE);
  EXPECT(fdm_tfilter_destroy(T) == FDM_OK && fdm_tfilter_destroy(T0) == FDM_OK && fdm_tfilter_destroy(nullptr) == FDM_OK);
  printf("tfilter_host_check ok (%d tap rows, %d vertices, radius %d)\n", made, V, R);
  return 0;
}
