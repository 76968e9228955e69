// Host side of the temporal rig fit under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the Jacobi tables
// of fdm_rig_temporal_tables_host (Q^T G Q = Lam, Q^T M Q = I, order and sign rule) at K = 1, 37 and 128 with exactly sized buffers,
// every refusal, and fdm_rig_set_temporal on an object without a device (csrc/rig_out.hip), with the two symbols that unit takes
// from fdm_hip.hip supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/rig_temporal_host_check.cpp rig_out.hip -o ../../tools/_build/rig_temporal_host_check
//   ../../tools/_build/rig_temporal_host_check          -> "rig_temporal_host_check ok", exit status 0
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

static unsigned g_seed = 2468u;
static float next() { g_seed = g_seed * 1664525u + 1013904223u; return (float)((g_seed >> 8) & 0xffff) / 65536.f - 0.5f; }

// the tables of one seeded rig: the two identities to 1e-12 of max |G|, ascending eigenvalues, the sign rule
static int check_tables(int K, int V, bool weighted, double* worst) {
  const int V3 = 3 * V;
  std::vector<float> E((size_t)K * V3), m((size_t)K);
  for (auto& e : E) e = next();
  for (auto& x : m) x = 1.f + next();
  std::vector<double> G((size_t)K * K), lam((size_t)K, -1.0), Q((size_t)K * K, -1.0);
  std::vector<float> Lc((size_t)K * K);
  EXPECT(fdm_rig_gram_host(E.data(), nullptr, K, V, 0.25, G.data(), Lc.data()) == FDM_OK);
  double tr = 0.0, gmax = 0.0;
  for (int k = 0; k < K; ++k) tr += G[(size_t)k * K + k];
  for (double g : G) gmax = std::fmax(gmax, std::fabs(g));
  const double mu = tr / K;
  EXPECT(fdm_rig_temporal_tables_host(G.data(), K, mu, weighted ? m.data() : nullptr, lam.data(), Q.data()) == FDM_OK);
  for (int a = 0; a < K; ++a) {
    EXPECT(lam[a] > 0.0 && (a == 0 || lam[a] >= lam[a - 1]));
    int big = 0;                                            // Q = D U: undo D before looking for the largest entry of the eigenvector
    for (int j = 1; j < K; ++j) {
      const double dj = std::sqrt(mu * (weighted ? m[j] : 1.f)), db = std::sqrt(mu * (weighted ? m[big] : 1.f));
      if (std::fabs(Q[(size_t)j * K + a] * dj) > std::fabs(Q[(size_t)big * K + a] * db)) big = j;
    }
    EXPECT(Q[(size_t)big * K + a] > 0.0);
    for (int b = 0; b < K; ++b) {
      long double qgq = 0.0, qmq = 0.0;
      for (int i = 0; i < K; ++i) {
        long double gq = 0.0;
        for (int j = 0; j < K; ++j) gq += (long double)G[(size_t)i * K + j] * Q[(size_t)j * K + b];
        qgq += (long double)Q[(size_t)i * K + a] * gq;
        qmq += (long double)Q[(size_t)i * K + a] * mu * (weighted ? m[i] : 1.f) * Q[(size_t)i * K + b];
      }
      *worst = std::fmax(*worst, std::fabs((double)qgq - (a == b ? lam[a] : 0.0)) / gmax);
      *worst = std::fmax(*worst, std::fabs((double)qmq - (a == b ? 1.0 : 0.0)) / gmax);
    }
  }
  EXPECT(*worst <= 1e-12);
  return 0;
}

int main() {
  double worst = 0.0;
  if (check_tables(1, 2, false, &worst) || check_tables(37, 211, true, &worst) || check_tables(128, 50, false, &worst)) return 1;

  // refusals of the tables
  const int K = 5, V = 9;
  std::vector<float> E((size_t)K * 3 * V), m(K, 1.f), Lc((size_t)K * K);
  for (auto& e : E) e = next();
  std::vector<double> G((size_t)K * K), lam(K), Q((size_t)K * K);
  EXPECT(fdm_rig_gram_host(E.data(), nullptr, K, V, 0.5, G.data(), Lc.data()) == FDM_OK);
  EXPECT(fdm_rig_temporal_tables_host(nullptr, K, 1.0, m.data(), lam.data(), Q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_temporal_tables_host(G.data(), K, 1.0, m.data(), nullptr, Q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_temporal_tables_host(G.data(), K, 1.0, m.data(), lam.data(), nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_temporal_tables_host(G.data(), 0, 1.0, m.data(), lam.data(), Q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_temporal_tables_host(G.data(), 129, 1.0, m.data(), lam.data(), Q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_temporal_tables_host(G.data(), K, 0.0, m.data(), lam.data(), Q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_temporal_tables_host(G.data(), K, -1.0, m.data(), lam.data(), Q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_temporal_tables_host(G.data(), K, NAN, m.data(), lam.data(), Q.data()) == FDM_ERR_ARG);
  EXPECT(fdm_rig_temporal_tables_host(G.data(), K, INFINITY, m.data(), lam.data(), Q.data()) == FDM_ERR_ARG);
  { std::vector<float> bad = m; bad[K - 1] = 0.f; EXPECT(fdm_rig_temporal_tables_host(G.data(), K, 1.0, bad.data(), lam.data(), Q.data()) == FDM_ERR_ARG); }
  { std::vector<float> bad = m; bad[0] = NAN; EXPECT(fdm_rig_temporal_tables_host(G.data(), K, 1.0, bad.data(), lam.data(), Q.data()) == FDM_ERR_ARG); }
  { std::vector<float> bad = m; bad[2] = INFINITY; EXPECT(fdm_rig_temporal_tables_host(G.data(), K, 1.0, bad.data(), lam.data(), Q.data()) == FDM_ERR_ARG); }
  { std::vector<double> neg = G; for (auto& g : neg) g = -g; EXPECT(fdm_rig_temporal_tables_host(neg.data(), K, 1.0, m.data(), lam.data(), Q.data()) == FDM_ERR_ARG); }
  const std::string refused = fdm::g_err;

  // set_temporal on an object without a device: validates, switches the path, forward still ends in FDM_ERR_STATE
  fdm_rig* r = nullptr;
  std::vector<float> lo(K, 0.f), hi(K, 1.f);
  EXPECT(fdm_rig_create(E.data(), K, V, nullptr, 0.5, lo.data(), hi.data(), 16, &r) == FDM_OK && r != nullptr);
  EXPECT(fdm_rig_set_temporal(nullptr, 1.0, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_set_temporal(r, -1.0, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_set_temporal(r, NAN, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_rig_set_temporal(r, INFINITY, m.data()) == FDM_ERR_ARG);
  { std::vector<float> bad = m; bad[1] = -2.f; EXPECT(fdm_rig_set_temporal(r, 1.0, bad.data()) == FDM_ERR_ARG && fdm_rig_set_temporal(r, 0.0, bad.data()) == FDM_ERR_ARG); }
  EXPECT(fdm_rig_set_temporal(r, 1e-60, nullptr) == FDM_ERR_ARG);          // eigenvalues past fp32
  EXPECT(fdm_rig_set_temporal(r, 1e60, nullptr) == FDM_ERR_ARG);           // mu past fp32
  EXPECT(fdm_rig_set_temporal(r, 3.0, m.data()) == FDM_OK && fdm_rig_set_temporal(r, 3.0, nullptr) == FDM_OK);
  const float* x = (const float*)0x1000;           // never dereferenced: no call gets as far as a launch
  float* y = (float*)0x2000;
  const int frames[2] = {7, 0};
  EXPECT(fdm_rig_forward(r, x, frames, 2, 7, 30, 60, y, y, 14, nullptr, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_rig_forward(r, x, frames, 2, 7, 30, 60, y, y, 13, nullptr, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_rig_set_temporal(r, 0.0, nullptr) == FDM_OK);
  EXPECT(fdm_rig_forward(r, x, frames, 2, 7, 30, 60, y, y, 14, nullptr, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_rig_destroy(r) == FDM_OK);
  printf("rig_temporal_host_check ok (K = 1, 37, 128: max |Q^T G Q - Lam|, |Q^T M Q - I| over max |G| = %.2e; refused: \"%s\")\n", worst, refused.c_str());
  return 0;
}
