// Host side of the parametric-head hand-off under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the
// fp64 tables of fdm_flame_tables_host against long double, fdm_flame_create's checks, fdm_flame_forward's argument checks and destroy
// (csrc/flame_out.hip), with the two symbols that unit takes from fdm_hip.hip supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/flame_host_check.cpp flame_out.hip -o ../../tools/_build/flame_host_check
//   ../../tools/_build/flame_host_check          -> "flame_host_check ok", exit status 0
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
#define REFUSED(call, word) EXPECT((call) == FDM_ERR_ARG && fdm::g_err.find(word) != std::string::npos)

int main() {
  // a seeded model (an LCG: no library state), exactly sized buffers
  const int V = 211, J = 5, NB = 9, expr_at = 6, P = 9 * (J - 1), V3 = 3 * V;
  unsigned s = 2468u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)((s >> 8) & 0xffff) / 65536.f - 0.5f; };
  std::vector<float> vt((size_t)V3), sd((size_t)V3 * NB), pd((size_t)P * V3), jr((size_t)J * V), w((size_t)V * J);
  for (auto& x : vt) x = next();
  for (auto& x : sd) x = 0.01f * next();
  for (auto& x : pd) x = 0.01f * next();
  for (auto& x : jr) x = (next() > 0.4f) ? 0.1f + next() * 0.1f : 0.f;
  for (auto& x : w) x = 0.6f + next();
  const int parents[J] = {-1, 0, 1, 1, 1};
  fdm_flame_model m = {V, J, NB, expr_at, vt.data(), sd.data(), pd.data(), jr.data(), parents, w.data()};
  std::vector<float> D((size_t)(NB + P) * V3, -1.f), JT((size_t)J * 3, -1.f), JD((size_t)NB * 3 * J, -1.f);
  EXPECT(fdm_flame_tables_host(&m, D.data(), JT.data(), JD.data()) == FDM_OK);
  double worst = 0.0;
  for (int j = 0; j < J; ++j)
    for (int a = 0; a < 3; ++a) {
      long double t = 0.0;
      for (int v = 0; v < V; ++v) t += (long double)jr[(size_t)j * V + v] * vt[3 * (size_t)v + a];
      worst = std::fmax(worst, std::fabs((double)t - (double)JT[3 * j + a]) / (std::fabs((double)t) + 1e-30));
      for (int k = 0; k < NB; ++k) {
        long double u = 0.0;
        for (int v = 0; v < V; ++v) u += (long double)jr[(size_t)j * V + v] * sd[(3 * (size_t)v + a) * NB + k];
        EXPECT(std::fabs((double)u - (double)JD[(size_t)k * 3 * J + 3 * j + a]) <= std::fabs((double)u) * 0x1p-23 + 1e-30);
      }
    }
  EXPECT(worst <= 0x1p-23);
  for (int k = 0; k < NB; ++k)
    for (int i = 0; i < V3; ++i) EXPECT(D[(size_t)k * V3 + i] == sd[(size_t)i * NB + k]);
  for (int p = 0; p < P; ++p)
    for (int i = 0; i < V3; ++i) EXPECT(D[(size_t)(NB + p) * V3 + i] == pd[(size_t)p * V3 + i]);
  EXPECT(fdm_flame_tables_host(nullptr, D.data(), JT.data(), JD.data()) == FDM_ERR_ARG);
  EXPECT(fdm_flame_tables_host(&m, nullptr, JT.data(), JD.data()) == FDM_ERR_ARG);
  EXPECT(fdm_flame_tables_host(&m, D.data(), nullptr, JD.data()) == FDM_ERR_ARG);
  EXPECT(fdm_flame_tables_host(&m, D.data(), JT.data(), nullptr) == FDM_ERR_ARG);

  // create: every refusal names its field; then the object without a device
  const int lv[6] = {0, 1, 2, V - 1, 5, 7};
  const float lb[6] = {0.2f, 0.3f, 0.5f, 1.f, 0.f, 0.f};
  fdm_flame* f = nullptr;
  EXPECT(fdm_flame_create(&m, lv, lb, 2, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_flame_create(nullptr, lv, lb, 2, &f) == FDM_ERR_ARG);
  { fdm_flame_model b = m; b.v_template = nullptr; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "v_template"); }
  { fdm_flame_model b = m; b.shapedirs = nullptr; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "shapedirs"); }
  { fdm_flame_model b = m; b.posedirs = nullptr; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "posedirs"); }
  { fdm_flame_model b = m; b.j_regressor = nullptr; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "j_regressor"); }
  { fdm_flame_model b = m; b.parents = nullptr; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "parents"); }
  { fdm_flame_model b = m; b.lbs_weights = nullptr; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "lbs_weights"); }
  { fdm_flame_model b = m; b.J = 0; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "J = 0"); }
  { fdm_flame_model b = m; b.J = 9; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "J = 9"); }
  { fdm_flame_model b = m; b.NB = 513; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "NB = 513"); }
  { fdm_flame_model b = m; b.NB = -1; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "NB = -1"); }
  { fdm_flame_model b = m; b.expr_at = NB + 1; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "expr_at"); }
  { fdm_flame_model b = m; b.V = 0; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "V = 0"); }
  { const int bad[J] = {0, 0, 2, 1, 1}; fdm_flame_model b = m; b.parents = bad; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "parents[2] = 2"); }
  { const int bad[J] = {0, 0, 1, 1, -1}; fdm_flame_model b = m; b.parents = bad; REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "parents[4] = -1"); }
  { std::vector<float> bad = sd; bad.back() = NAN; fdm_flame_model b = m; b.shapedirs = bad.data(); REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "shapedirs element"); }
  { std::vector<float> bad = pd; bad.back() = INFINITY; fdm_flame_model b = m; b.posedirs = bad.data(); REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "posedirs element"); }
  { std::vector<float> bad = w; bad[0] = NAN; fdm_flame_model b = m; b.lbs_weights = bad.data(); REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "lbs_weights element 0"); }
  { std::vector<float> bad = jr; bad.back() = NAN; fdm_flame_model b = m; b.j_regressor = bad.data(); REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "j_regressor element"); }
  { std::vector<float> bad = vt; bad[7] = -INFINITY; fdm_flame_model b = m; b.v_template = bad.data(); REFUSED(fdm_flame_create(&b, lv, lb, 2, &f), "v_template element 7"); }
  REFUSED(fdm_flame_create(&m, lv, lb, 257, &f), "NL");
  REFUSED(fdm_flame_create(&m, nullptr, lb, 2, &f), "lmk");
  { const int bad[6] = {0, 1, 2, V, 5, 7}; REFUSED(fdm_flame_create(&m, bad, lb, 2, &f), "lmk_verts element 3"); }
  { const float bad[6] = {0.2f, 0.3f, 0.5f, NAN, 0.f, 0.f}; REFUSED(fdm_flame_create(&m, lv, bad, 2, &f), "lmk_bary"); }
  EXPECT(f == nullptr);
  { fdm_flame_model b = m; b.J = 1; b.NB = 0; b.expr_at = 0; b.shapedirs = nullptr; b.posedirs = nullptr;   // the smallest model
    EXPECT(fdm_flame_create(&b, nullptr, nullptr, 0, &f) == FDM_OK && f != nullptr && fdm_flame_destroy(f) == FDM_OK); f = nullptr; }
  fdm_flame* bare = nullptr;
  EXPECT(fdm_flame_create(&m, nullptr, nullptr, 0, &bare) == FDM_OK && bare != nullptr);
  EXPECT(fdm_flame_create(&m, lv, lb, 2, &f) == FDM_OK && f != nullptr);
  const int B = 3, L = 7;
  const int frames[B] = {7, 0, 4}, neg[B] = {7, -1, 4};
  const float* x = (const float*)0x1000;           // never dereferenced: no call gets as far as a launch
  float* y = (float*)0x2000;
  EXPECT(fdm_flame_forward(nullptr, x, 2, 1, x, 3, x, x, x, frames, B, L, y, y, y, y, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_flame_forward(f, x, 2, 1, x, 3, nullptr, x, x, frames, B, L, y, y, y, y, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_flame_forward(f, x, 2, 1, x, 3, x, x, x, frames, B, L, nullptr, y, y, y, nullptr) == FDM_ERR_ARG);
  REFUSED(fdm_flame_forward(f, nullptr, 2, 1, x, 3, x, x, x, frames, B, L, y, y, y, y, nullptr), "shape");
  REFUSED(fdm_flame_forward(f, x, 2, 1, nullptr, 3, x, x, x, frames, B, L, y, y, y, y, nullptr), "expr");
  REFUSED(fdm_flame_forward(f, x, expr_at + 1, 1, x, 3, x, x, x, frames, B, L, y, y, y, y, nullptr), "NS = 7");
  REFUSED(fdm_flame_forward(f, x, 2, 1, x, NB - expr_at + 1, x, x, x, frames, B, L, y, y, y, y, nullptr), "NE = 4");
  REFUSED(fdm_flame_forward(f, x, 2, 2, x, 3, x, x, x, frames, B, L, y, y, y, y, nullptr), "shape_rows");
  REFUSED(fdm_flame_forward(bare, x, 2, 1, x, 3, x, x, x, frames, B, L, y, y, y, y, nullptr), "embedding");
  EXPECT(fdm_flame_forward(f, x, 2, 1, x, 3, x, x, x, frames, 0, L, y, y, y, y, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_flame_forward(f, x, 2, 1, x, 3, x, x, x, frames, B, 6, y, y, y, y, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_flame_forward(f, x, 2, 1, x, 3, x, x, x, neg, B, L, y, y, y, y, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_flame_forward(f, x, 2, 1, x, 3, x, x, x, frames, B, L, y, y, y, y, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_flame_forward(f, nullptr, 0, B, nullptr, 0, x, nullptr, nullptr, nullptr, B, L, y, nullptr, nullptr, nullptr, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_flame_destroy(f) == FDM_OK && fdm_flame_destroy(bare) == FDM_OK && fdm_flame_destroy(nullptr) == FDM_OK);
  printf("flame_host_check ok (%d vertices, %d joints, %d coefficients: max relative |JT - long double| = %.2e)\n", V, J, NB, worst);
  return 0;
}
