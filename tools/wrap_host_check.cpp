// Host side of the wrap hand-off under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the fp64 binding
// coordinates (fdm_wrap_coords_host) and the argument checks of fdm_wrap_create (with face_idx given) and fdm_wrap_forward
// (csrc/wrap_out.hip), with the two symbols that unit takes from fdm_hip.hip supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/wrap_host_check.cpp wrap_out.hip -o ../../tools/_build/wrap_host_check
//   ../../tools/_build/wrap_host_check          -> "wrap_host_check ok", exit status 0
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
  // a rows x cols height field, two triangles per cell, plus a face without area; one target vertex over every face; exactly sized buffers
  const int rows = 23, cols = 29, V = rows * cols;
  std::vector<float> S((size_t)3 * V);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) {
      float* p = &S[3 * (size_t)(r * cols + c)];
      p[0] = 0.05f * c; p[1] = 0.05f * r; p[2] = 0.015f * std::sin(0.9f * c + 0.4f * r);
    }
  std::vector<int> faces;
  for (int r = 0; r + 1 < rows; ++r)
    for (int c = 0; c + 1 < cols; ++c) {
      const int a = r * cols + c;
      const int t[6] = {a, a + 1, a + cols, a + 1, a + cols + 1, a + cols};
      faces.insert(faces.end(), t, t + 6);
    }
  const int deg[3] = {5, 5, 9};
  faces.insert(faces.end(), deg, deg + 3);
  const int F = (int)faces.size() / 3, Vt = F - 1;
  std::vector<float> T((size_t)3 * Vt), uvh((size_t)3 * Vt, -7.f), dist((size_t)Vt, -7.f), w((size_t)Vt);
  std::vector<int> fi((size_t)Vt);
  const double cu = 0.25, cv = 0.5, ch = 0.03;
  for (int j = 0; j < Vt; ++j) {          // q = a + cu e1 + cv e2 + ch nh of face j, in double, rounded to float
    const float *a = &S[3 * (size_t)faces[3 * j]], *b = &S[3 * (size_t)faces[3 * j + 1]], *c = &S[3 * (size_t)faces[3 * j + 2]];
    const double e1[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]}, e2[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    for (int k = 0; k < 3; ++k) T[3 * (size_t)j + k] = (float)(a[k] + cu * e1[k] + cv * e2[k] + ch * n[k] / len);
    fi[j] = j;
    w[j] = (float)j / (float)(Vt - 1);
  }
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_OK);
  for (int j = 0; j < Vt; ++j) {          // the coordinates come back to the rounding of T; an interior point lies |h| away
    EXPECT(std::fabs(uvh[3 * (size_t)j] - cu) < 1e-4 && std::fabs(uvh[3 * (size_t)j + 1] - cv) < 1e-4 && std::fabs(uvh[3 * (size_t)j + 2] - ch) < 1e-6);
    EXPECT(std::fabs(dist[j] - ch) < 1e-6);
  }
  EXPECT(fdm_wrap_coords_host(nullptr, faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_coords_host(S.data(), nullptr, F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, nullptr, Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, nullptr, uvh.data(), dist.data()) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), nullptr, dist.data()) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), 0, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V - 1, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), 0, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  fi[3] = F - 1;                          // the face without area
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  fi[3] = F;
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  fi[3] = -1;
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  fi[3] = 3;
  const float keep = T[4];
  T[4] = NAN;
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  T[4] = keep;
  S[7] = INFINITY;
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_ERR_ARG);
  S[7] = 0.05f * 0;                       // vertex 2, y: row 0

  // the object without a device: create validates and binds, forward refuses in order and ends in FDM_ERR_STATE
  fdm_wrap* W = nullptr;
  EXPECT(fdm_wrap_create(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), w.data(), nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_create(nullptr, faces.data(), F, V, T.data(), Vt, fi.data(), w.data(), &W) == FDM_ERR_ARG && W == nullptr);
  EXPECT(fdm_wrap_create(S.data(), faces.data(), F, V, T.data(), Vt, nullptr, w.data(), &W) == FDM_ERR_STATE && W == nullptr);
  w[2] = 1.5f;
  EXPECT(fdm_wrap_create(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), w.data(), &W) == FDM_ERR_ARG && W == nullptr);
  w[2] = NAN;
  EXPECT(fdm_wrap_create(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), w.data(), &W) == FDM_ERR_ARG && W == nullptr);
  w[2] = 0.f;
  fi[0] = F;
  EXPECT(fdm_wrap_create(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), w.data(), &W) == FDM_ERR_ARG && W == nullptr);
  fi[0] = F - 1;
  EXPECT(fdm_wrap_create(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), w.data(), &W) == FDM_ERR_ARG && W == nullptr);
  fi[0] = 0;
  EXPECT(fdm_wrap_create(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), w.data(), &W) == FDM_OK && W != nullptr);
  std::vector<int> fi2((size_t)Vt, -1);
  std::vector<float> uvh2((size_t)3 * Vt), dist2((size_t)Vt);
  EXPECT(fdm_wrap_binding(nullptr, fi2.data(), uvh2.data(), dist2.data()) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_binding(W, fi2.data(), nullptr, nullptr) == FDM_OK && fi2 == fi);
  EXPECT(fdm_wrap_coords_host(S.data(), faces.data(), F, V, T.data(), Vt, fi.data(), uvh.data(), dist.data()) == FDM_OK);
  EXPECT(fdm_wrap_binding(W, nullptr, uvh2.data(), dist2.data()) == FDM_OK && uvh2 == uvh && dist2 == dist);
  const int B = 3, L_max = 7;
  const int frames[B] = {7, 0, 4}, neg[B] = {7, -1, 4}, big[B] = {7, 8, 4};
  const float* x = (const float*)0x1000;           // never dereferenced: no call gets as far as a launch
  float* y = (float*)0x2000;
  EXPECT(fdm_wrap_forward(nullptr, x, frames, B, L_max, x, 1, 0, y, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_forward(W, nullptr, frames, B, L_max, x, 1, 0, y, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_forward(W, x, frames, B, L_max, x, 1, 0, nullptr, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_forward(W, x, frames, B, L_max, x, 1, 2, y, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_forward(W, x, frames, B, L_max, x, 2, 0, y, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_forward(W, x, frames, B, L_max, nullptr, 1, 0, y, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_wrap_forward(W, x, frames, 0, L_max, nullptr, 0, 0, y, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_wrap_forward(W, x, frames, B, 0, x, 1, 0, y, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_wrap_forward(W, x, frames, B, 6, x, 1, 0, y, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_wrap_forward(W, x, neg, B, L_max, x, 1, 0, y, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_wrap_forward(W, x, big, B, L_max, x, 1, 0, y, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_wrap_forward(W, x, frames, B, L_max, x, 1, 0, y, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_wrap_forward(W, x, nullptr, B, L_max, nullptr, 0, FDM_WRAP_OFFSETS, y, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_wrap_forward(W, x, frames, B, L_max, x, B, FDM_WRAP_OFFSETS, y, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_wrap_destroy(W) == FDM_OK && fdm_wrap_destroy(nullptr) == FDM_OK);
  printf("wrap_host_check ok (%d target vertices over %d faces of %d vertices)\n", Vt, F, V);
  return 0;
}
