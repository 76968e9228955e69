// Host side of the time filter's recurrences under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the
// constants (fdm_tfilter_recur_coeffs_host) into exactly sized buffers and every refusal of fdm_tfilter_create_recur and
// fdm_tfilter_forward_state (csrc/tfilter.hip) that is reached before any device call, with the two symbols that unit takes from
// fdm_hip.hip supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/trecur_host_check.cpp tfilter.hip -o ../../tools/_build/trecur_host_check
//   ../../tools/_build/trecur_host_check          -> "trecur_host_check ok", exit status 0
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
  // the constants into buffers of exactly FDM_TFILTER_NCOEFF floats, against the definition evaluated here
  int made = 0;
  const double rates[] = {0.5, 24.0, 25.0, 29.97, 30.0, 60.0, 1000.0}, cuts[] = {0.05, 1.0, 1.7, 12.5, 400.0};
  for (double fps : rates)
    for (double c : cuts) {
      std::vector<float> q(FDM_TFILTER_NCOEFF, -7.f);
      const float k = (float)(fps / (2.0 * 3.14159265358979323846)), c0 = (float)c;
      EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_EMA, fps, c, 123.0, -5.0, q.data()) == FDM_OK);      // (beta and d_cutoff are not read)
      EXPECT(q[0] == k && q[1] == c0 && q[2] == 0.f && q[3] == 0.f && q[4] == (float)fps && q[5] == 0.f && q[6] == c0 / (c0 + k) && q[7] == 0.f);
      std::vector<float> e(FDM_TFILTER_NCOEFF, -7.f);
      const float cd = 0.7f;
      EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, fps, c, 0.25, (double)cd, e.data()) == FDM_OK);
      EXPECT(e[0] == k && e[1] == c0 && e[2] == 0.25f && e[3] == cd && e[4] == (float)fps && e[5] == cd / (cd + k) && e[6] == q[6] && e[7] == 0.f);
      made += 2;
    }
  std::vector<float> q(FDM_TFILTER_NCOEFF, -7.f);
  const double bad_pos[] = {0.0, -1.0, (double)NAN, (double)INFINITY, 1e300, 1e-300};
  for (double b : bad_pos) {
    EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_EMA, b, 1.0, 0.0, 1.0, q.data()) == FDM_ERR_ARG);
    EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_EMA, 30.0, b, 0.0, 1.0, q.data()) == FDM_ERR_ARG);
    EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, b, 1.0, 0.1, 1.0, q.data()) == FDM_ERR_ARG);
    EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, 30.0, b, 0.1, 1.0, q.data()) == FDM_ERR_ARG);
    EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, 30.0, 1.0, 0.1, b, q.data()) == FDM_ERR_ARG);
  }
  EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, 30.0, 1.0, -0.1, 1.0, q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, 30.0, 1.0, (double)NAN, 1.0, q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, 30.0, 1.0, (double)INFINITY, 1.0, q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, 30.0, 1.0, 1e300, 1.0, q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_EMA, 30.0, 1.0, 0.0, 1.0, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_recur_coeffs_host(2, 30.0, 1.0, 0.0, 1.0, q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_recur_coeffs_host(-1, 30.0, 1.0, 0.0, 1.0, q.data()) == FDM_ERR_ARG);
  for (float v : q) EXPECT(v == -7.f);          // a refusal writes nothing

  // the object without a device: create validates (exactly sized coefficients and strength)
  const int V = 7;
  std::vector<float> good(FDM_TFILTER_NCOEFF), ema(FDM_TFILTER_NCOEFF), s((size_t)V);
  EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_ONE_EURO, 30.0, 1.0, 0.5, 1.0, good.data()) == FDM_OK);
  EXPECT(fdm_tfilter_recur_coeffs_host(FDM_TFILTER_EMA, 30.0, 1.0, 0.0, 0.0, ema.data()) == FDM_OK);
  for (int v = 0; v < V; ++v) s[v] = (float)v / (float)(V - 1);
  fdm_tfilter* T = nullptr;
  EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_ONE_EURO, good.data(), s.data(), FDM_TFILTER_CAUSAL, nullptr, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_ONE_EURO, nullptr, s.data(), FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create_recur(0, FDM_TFILTER_ONE_EURO, good.data(), nullptr, FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create_recur(-2, FDM_TFILTER_ONE_EURO, good.data(), nullptr, FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create_recur(V, 2, good.data(), s.data(), FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create_recur(V, -1, good.data(), s.data(), FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_ONE_EURO, good.data(), s.data(), 2, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_ONE_EURO, good.data(), s.data(), -1, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  const struct { int i; float v; } bad[] = {{0, 0.f}, {0, -1.f}, {0, NAN}, {1, 0.f}, {1, -1.f}, {1, INFINITY}, {2, -0.5f}, {2, NAN}, {3, 0.f}, {3, -INFINITY},
                                            {4, 0.f}, {4, -30.f}, {4, NAN}, {5, 0.f}, {5, NAN}, {6, 0.f}, {6, INFINITY}, {7, NAN}};
  for (const auto& b : bad) {
    std::vector<float> c = good;
    c[(size_t)b.i] = b.v;
    EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_ONE_EURO, c.data(), s.data(), FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  }
  EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_ONE_EURO, ema.data(), nullptr, FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_ERR_ARG && T == nullptr);      // cd = ad = 0
  const float bad_s[] = {1.0001f, -0.5f, NAN};
  for (float b : bad_s) {
    s[V - 1] = b;
    EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_EMA, ema.data(), s.data(), FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_ERR_ARG && T == nullptr);
  }
  s[V - 1] = 1.f;
  fdm_tfilter *E = nullptr, *Z = nullptr, *F = nullptr;
  EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_ONE_EURO, good.data(), s.data(), FDM_TFILTER_CAUSAL, nullptr, &T) == FDM_OK && T != nullptr);
  EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_EMA, ema.data(), nullptr, FDM_TFILTER_CAUSAL, nullptr, &E) == FDM_OK && E != nullptr);
  EXPECT(fdm_tfilter_create_recur(V, FDM_TFILTER_ONE_EURO, good.data(), nullptr, FDM_TFILTER_ZERO_PHASE, nullptr, &Z) == FDM_OK && Z != nullptr);
  const float taps[2] = {0.5f, 0.25f};
  EXPECT(fdm_tfilter_create(V, 1, taps, nullptr, FDM_TFILTER_MIRROR, nullptr, &F) == FDM_OK && F != nullptr);
  EXPECT(fdm_tfilter_set_prefetch(T, 1) == FDM_OK && fdm_tfilter_set_prefetch(T, 16) == FDM_OK && fdm_tfilter_set_prefetch(T, 8) == FDM_OK);
  EXPECT(fdm_tfilter_set_prefetch(T, 0) == FDM_ERR_ARG && fdm_tfilter_set_prefetch(T, 3) == FDM_ERR_ARG && fdm_tfilter_set_prefetch(F, 8) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_set_prefetch(nullptr, 8) == FDM_ERR_ARG);

  // forward: every refusal in order, ending in FDM_ERR_STATE (no device)
  const int B = 3, L_max = 7;
  const int lens[B] = {7, 1, 4}, zero[B] = {7, 0, 4}, neg[B] = {-1, 1, 4}, big[B] = {7, 1, 8};
  const float* x = (const float*)0x100000;          // never dereferenced: no call gets as far as a launch
  float *y = (float*)0x200000, *st = (float*)0x300000;
  int* seen = (int*)0x400000;
  const long long n = (long long)B * L_max * 3 * V;
  EXPECT(fdm_tfilter_forward_state(nullptr, x, lens, B, L_max, st, seen, y) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward_state(T, nullptr, lens, B, L_max, st, seen, y) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward_state(T, x, lens, B, L_max, nullptr, seen, y) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward_state(T, x, lens, B, L_max, st, nullptr, y) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward_state(T, x, lens, B, L_max, st, seen, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward_state(F, x, lens, B, L_max, st, seen, y) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward_state(Z, x, lens, B, L_max, st, seen, y) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward_state(T, x, lens, 0, L_max, st, seen, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward_state(T, x, nullptr, B, 0, st, seen, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward_state(T, x, neg, B, L_max, st, seen, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward_state(T, x, big, B, L_max, st, seen, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward_state(T, x, lens, B, 6, st, seen, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward_state(T, x, lens, B, L_max, st, seen, (float*)x + (n - 1)) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward_state(T, x, lens, B, L_max, st, seen, (float*)x + n) == FDM_ERR_STATE);       // adjacent: as far as the device check
  EXPECT(fdm_tfilter_forward_state(T, x, zero, B, L_max, st, seen, y) == FDM_ERR_STATE);                   // L = 0 is a length with a state
  EXPECT(fdm_tfilter_forward_state(E, x, nullptr, B, L_max, st, seen, y) == FDM_ERR_STATE);
  // the stateless call serves the recurrences too: L = 0 is refused there, zero-phase is not
  EXPECT(fdm_tfilter_forward(T, x, zero, B, L_max, y) == FDM_ERR_SHAPE);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, (float*)x) == FDM_ERR_ARG);
  EXPECT(fdm_tfilter_forward(T, x, lens, B, L_max, y) == FDM_ERR_STATE && fdm_tfilter_forward(Z, x, nullptr, B, L_max, y) == FDM_ERR_STATE);
  EXPECT(fdm_tfilter_forward(F, x, lens, B, L_max, y) == FDM_ERR_STATE);
  EXPECT(fdm_tfilter_destroy(T) == FDM_OK && fdm_tfilter_destroy(E) == FDM_OK && fdm_tfilter_destroy(Z) == FDM_OK && fdm_tfilter_destroy(F) == FDM_OK);
  printf("trecur_host_check ok (%d coefficient rows, %d vertices)\n", made, V);
  return 0;
}
