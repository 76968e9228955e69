// Host side of the mesh hand-off under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the incident-face
// lists, the frame rule and fdm_mesh_create / _forward's argument checks (csrc/mesh_out.hip), with the two symbols that unit takes
// from fdm_hip.hip supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/mesh_host_check.cpp mesh_out.hip -o ../../tools/_build/mesh_host_check
//   ../../tools/_build/mesh_host_check          -> "mesh_host_check ok", exit status 0
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
  // a rows x cols grid, two triangles per cell, plus an isolated vertex and a face without area; exactly sized buffers
  const int rows = 37, cols = 41, V = rows * cols + 1;
  std::vector<int> faces;
  for (int r = 0; r + 1 < rows; ++r)
    for (int c = 0; c + 1 < cols; ++c) {
      const int a = r * cols + c;
      const int t[6] = {a, a + 1, a + cols, a + 1, a + cols + 1, a + cols};
      faces.insert(faces.end(), t, t + 6);
    }
  const int deg[3] = {5, 5, 9};
  faces.insert(faces.end(), deg, deg + 3);
  const int F = (int)faces.size() / 3;
  std::vector<int> off(V + 1, -1), items((size_t)3 * F, -1);
  EXPECT(fdm_mesh_adjacency_host(faces.data(), F, V, off.data(), items.data()) == FDM_OK);
  EXPECT(off[0] == 0 && off[V] == 3 * F && off[V - 1] == off[V]);          // the last vertex is isolated
  for (int v = 0; v < V; ++v) {
    int count = 0;
    for (int i = 0; i < 3 * F; ++i) count += faces[i] == v;
    EXPECT(off[v + 1] - off[v] == count);
    for (int j = off[v]; j < off[v + 1]; ++j) {
      const int f = items[j];
      EXPECT(f >= 0 && f < F && (faces[3 * f] == v || faces[3 * f + 1] == v || faces[3 * f + 2] == v));
      EXPECT(j == off[v] || items[j - 1] <= f);
    }
  }
  int twice = 0;
  for (int j = off[5]; j < off[6]; ++j) twice += items[j] == F - 1;
  EXPECT(twice == 2);                                                       // one entry per corner
  EXPECT(fdm_mesh_adjacency_host(nullptr, F, V, off.data(), items.data()) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_adjacency_host(faces.data(), F, V, nullptr, items.data()) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_adjacency_host(faces.data(), F, V, off.data(), nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_adjacency_host(faces.data(), -1, V, off.data(), items.data()) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_adjacency_host(faces.data(), F, 0, off.data(), items.data()) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_adjacency_host(faces.data(), F, rows * cols - 1, off.data(), items.data()) == FDM_ERR_ARG);
  std::vector<int> one(2, 7);
  EXPECT(fdm_mesh_adjacency_host(faces.data(), 0, 1, one.data(), items.data()) == FDM_OK && one[0] == 0 && one[1] == 0);

  // the frame rule against its expression
  const double rates[5][2] = {{30, 60}, {30, 25}, {25, 30}, {30, 24}, {30, 30}};
  for (const auto& r : rates)
    for (int L = 0; L <= 1000; ++L) {
      int n = -1;
      EXPECT(fdm_mesh_frames(L, r[0], r[1], &n) == FDM_OK);
      int want = L;
      if (L > 0 && r[0] != r[1]) { want = (int)((double)L / r[0] * r[1]); want = want < 1 ? 1 : want; }
      EXPECT(n == want);
    }
  int n = 0;
  EXPECT(fdm_mesh_frames(5, 30, 60, nullptr) == FDM_ERR_ARG && fdm_mesh_frames(-1, 30, 60, &n) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_frames(5, -1, 60, &n) == FDM_ERR_ARG && fdm_mesh_frames(5, 30, NAN, &n) == FDM_ERR_ARG && fdm_mesh_frames(5, INFINITY, 1, &n) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_frames(0x7fffffff, 1, 4, &n) == FDM_ERR_SHAPE);
  EXPECT(fdm_mesh_frames(0x7fffffff, 4, 1, &n) == FDM_OK && n == 0x7fffffff / 4);

  // the object without a device: create validates, forward refuses in order and ends in FDM_ERR_STATE
  fdm_mesh* m = nullptr;
  EXPECT(fdm_mesh_create(faces.data(), F, V, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_create(nullptr, F, V, &m) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_create(faces.data(), F, 10, &m) == FDM_ERR_ARG && m == nullptr);
  EXPECT(fdm_mesh_create(faces.data(), F, V, &m) == FDM_OK && m != nullptr);
  const int B = 3, L_max = 7;
  const int frames[B] = {7, 1, 4};
  int got[B] = {0, 0, 0};
  const float* x = (const float*)0x1000;           // never dereferenced: no call gets as far as a launch
  float* y = (float*)0x2000;
  const int N = FDM_MESH_NORMALS;
  EXPECT(fdm_mesh_forward(nullptr, x, frames, B, L_max, x, 1, 30, 60, N, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, nullptr, frames, B, L_max, x, 1, 30, 60, N, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, 30, 60, N, nullptr, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 2, 30, 60, N, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, nullptr, 1, 30, 60, N, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, 30, 60, N | 8, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, 30, 60, N | FDM_MESH_INTERLEAVED, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, 30, 60, FDM_MESH_INTERLEAVED, y, nullptr, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, 30, 60, N, y, nullptr, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, -30, 60, N, y, y, 14, got, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_mesh_forward(m, x, frames, 0, L_max, x, 0, 30, 60, N, y, y, 14, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_mesh_forward(m, x, frames, B, 6, x, 1, 30, 60, N, y, y, 14, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, 30, 60, N, y, y, 13, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, 0, 0, N, y, y, 6, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(got[0] == 0 && got[1] == 0 && got[2] == 0);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, 1, 30, 60, N, y, y, 14, got, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_mesh_forward(m, x, nullptr, B, L_max, nullptr, 0, 30, 25, N | FDM_MESH_INTERLEAVED | FDM_MESH_F16, y, nullptr, 5, nullptr, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_mesh_forward(m, x, frames, B, L_max, x, B, 0, 0, FDM_MESH_F16, y, nullptr, 7, got, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_mesh_destroy(m) == FDM_OK && fdm_mesh_destroy(nullptr) == FDM_OK);
  printf("mesh_host_check ok (%d faces over %d vertices)\n", F, V);
  return 0;
}
