// Host side of the render hand-off under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the argument checks
// of fdm_render_create, fdm_render_set_view, fdm_render_set and fdm_render_forward (csrc/render_out.hip, with the mesh unit it calls),
// each refusal a code and a message, with the two symbols those units take from fdm_hip.hip supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/render_host_check.cpp render_out.hip mesh_out.hip -o ../../tools/_build/render_host_check
//   ../../tools/_build/render_host_check          -> "render_host_check ok", exit status 0
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
// the call is refused with FDM_ERR_ARG, says why, and hands out no object
#define REFUSED(call) do { fdm::g_err.clear(); r = nullptr; EXPECT((call) == FDM_ERR_ARG); EXPECT(!fdm::g_err.empty() && r == nullptr); } while (0)

int main() {
  // a rows x cols grid, exactly sized buffers
  const int rows = 7, cols = 9, V = rows * cols;
  std::vector<int> faces;
  for (int r = 0; r + 1 < rows; ++r)
    for (int c = 0; c + 1 < cols; ++c) {
      const int a = r * cols + c;
      const int t[6] = {a, a + 1, a + cols, a + 1, a + cols + 1, a + cols};
      faces.insert(faces.end(), t, t + 6);
    }
  const int F = (int)faces.size() / 3, W = 37, H = 29;
  std::vector<float> cam = {48.f, 48.f, 18.5f, 14.5f, 0.01f, 3.f}, R = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t = {0, 0, -1};
  std::vector<float> lights(4 * 9);
  for (int l = 0; l < 9; ++l) { lights[4 * l] = 0.f; lights[4 * l + 1] = 0.6f; lights[4 * l + 2] = 0.8f; lights[4 * l + 3] = 0.25f; }
  std::vector<float> base = {0.3f, 0.3f, 0.3f}, bg = {1.f, 1.f, 1.f};
  fdm_render* r = nullptr;
  const float* C = cam.data();
  // create: null arguments
  EXPECT(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), nullptr) == FDM_ERR_ARG);
  REFUSED(fdm_render_create(nullptr, F, V, W, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, nullptr, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, nullptr, t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), nullptr, lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), nullptr, 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, nullptr, bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), nullptr, &r));
  // sizes, bad W / H
  REFUSED(fdm_render_create(faces.data(), 0, V, W, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, 0, W, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, 0, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, W, 4097, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, -3, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  // face indices out of range
  REFUSED(fdm_render_create(faces.data(), F, V - 1, W, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  faces[3 * (F - 1) + 2] = -1;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 5, 0.2f, base.data(), bg.data(), &r));
  faces[3 * (F - 1) + 2] = V - 1 - 1;
  // more than 8 lights, a non-unit direction, a negative or non-finite light
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 9, 0.2f, base.data(), bg.data(), &r));
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), -1, 0.2f, base.data(), bg.data(), &r));
  lights[4 * 7 + 2] = 0.9f;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  lights[4 * 7 + 2] = 0.8f; lights[4 * 7 + 3] = -1.f;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  lights[4 * 7 + 3] = NAN;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  lights[4 * 7 + 3] = 0.25f;
  // near >= far, near <= 0, focal length, non-finite numbers, colours
  cam[4] = 3.f;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  cam[4] = 0.f;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  cam[4] = 0.01f; cam[0] = 0.f;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  cam[0] = 48.f; R[4] = INFINITY;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  R[4] = 1.f;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, -0.5f, base.data(), bg.data(), &r));
  base[1] = -0.1f;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  base[1] = 0.3f; bg[2] = 1.5f;
  REFUSED(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r));
  bg[2] = 1.f;

  // the object without a device: create validates, set_view and set refuse in turn, forward refuses in order and ends in FDM_ERR_STATE
  EXPECT(fdm_render_create(faces.data(), F, V, W, H, C, R.data(), t.data(), lights.data(), 8, 0.2f, base.data(), bg.data(), &r) == FDM_OK && r != nullptr);
  fdm_render* obj = r;
#define VIEW_REFUSED(call) do { fdm::g_err.clear(); EXPECT((call) == FDM_ERR_ARG); EXPECT(!fdm::g_err.empty()); } while (0)
  VIEW_REFUSED(fdm_render_set_view(nullptr, C, R.data(), t.data(), lights.data(), 8, 0.2f));
  VIEW_REFUSED(fdm_render_set_view(obj, nullptr, R.data(), t.data(), lights.data(), 8, 0.2f));
  VIEW_REFUSED(fdm_render_set_view(obj, C, nullptr, t.data(), lights.data(), 8, 0.2f));
  VIEW_REFUSED(fdm_render_set_view(obj, C, R.data(), nullptr, lights.data(), 8, 0.2f));
  VIEW_REFUSED(fdm_render_set_view(obj, C, R.data(), t.data(), nullptr, 1, 0.2f));
  VIEW_REFUSED(fdm_render_set_view(obj, C, R.data(), t.data(), lights.data(), 9, 0.2f));
  lights[1] = 0.7f;
  VIEW_REFUSED(fdm_render_set_view(obj, C, R.data(), t.data(), lights.data(), 1, 0.2f));
  lights[1] = 0.6f; cam[5] = 0.005f;
  VIEW_REFUSED(fdm_render_set_view(obj, C, R.data(), t.data(), lights.data(), 8, 0.2f));
  cam[5] = 3.f; t[1] = NAN;
  VIEW_REFUSED(fdm_render_set_view(obj, C, R.data(), t.data(), lights.data(), 8, 0.2f));
  t[1] = 0.f;
  EXPECT(fdm_render_set_view(obj, C, R.data(), t.data(), nullptr, 0, 0.f) == FDM_OK);
  EXPECT(fdm_render_set_view(obj, C, R.data(), t.data(), lights.data(), 8, 0.2f) == FDM_OK);
  VIEW_REFUSED(fdm_render_set(nullptr, "chunk_frames", 1));
  VIEW_REFUSED(fdm_render_set(obj, nullptr, 1));
  VIEW_REFUSED(fdm_render_set(obj, "chunk", 1));
  VIEW_REFUSED(fdm_render_set(obj, "chunk_frames", -1));
  VIEW_REFUSED(fdm_render_set(obj, "chunk_frames", 4097));
  EXPECT(fdm_render_set(obj, "chunk_frames", 2) == FDM_OK && fdm_render_set(obj, "chunk_frames", 0) == FDM_OK);
  const int B = 3, L_max = 7;
  const int frames[B] = {7, 0, 4}, neg[B] = {7, -1, 4}, big[B] = {7, 8, 4};
  int got[B] = {-5, -5, -5};
  const float* x = (const float*)0x1000;           // never dereferenced: no call gets as far as a launch
  unsigned char* y = (unsigned char*)0x2000;
  VIEW_REFUSED(fdm_render_forward(nullptr, x, frames, B, L_max, x, 1, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr));
  VIEW_REFUSED(fdm_render_forward(obj, nullptr, frames, B, L_max, x, 1, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr));
  VIEW_REFUSED(fdm_render_forward(obj, x, frames, B, L_max, x, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, L_max, got, nullptr));
  VIEW_REFUSED(fdm_render_forward(obj, x, frames, B, L_max, x, 2, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr));
  VIEW_REFUSED(fdm_render_forward(obj, x, frames, B, L_max, nullptr, 1, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr));
  VIEW_REFUSED(fdm_render_forward(obj, x, frames, B, L_max, x, 1, -30.0, 60.0, nullptr, y, nullptr, nullptr, L_max, got, nullptr));
  VIEW_REFUSED(fdm_render_forward(obj, x, frames, B, L_max, x, 1, 30.0, (double)INFINITY, nullptr, y, nullptr, nullptr, L_max, got, nullptr));
  EXPECT(fdm_render_forward(obj, x, frames, 0, L_max, nullptr, 0, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_render_forward(obj, x, frames, B, 0, x, 1, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_render_forward(obj, x, frames, B, L_max, x, 1, 0, 0, nullptr, y, nullptr, nullptr, 0, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_render_forward(obj, x, frames, B, 6, x, 1, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_render_forward(obj, x, neg, B, L_max, x, 1, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_render_forward(obj, x, big, B, L_max, x, 1, 0, 0, nullptr, y, nullptr, nullptr, L_max, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_render_forward(obj, x, frames, B, L_max, x, 1, 30.0, 60.0, nullptr, y, nullptr, nullptr, 13, got, nullptr) == FDM_ERR_SHAPE);
  EXPECT(fdm_render_forward(obj, x, frames, B, L_max, x, 1, 30.0, 60.0, nullptr, y, nullptr, nullptr, 14, got, nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_render_forward(obj, x, nullptr, B, L_max, nullptr, 0, 0, 0, x, y, (float*)y, (int*)y, L_max, nullptr, nullptr) == FDM_ERR_STATE);
  EXPECT(got[0] == -5 && got[1] == -5 && got[2] == -5);      // a refused call writes no lengths
  EXPECT(fdm_render_destroy(obj) == FDM_OK && fdm_render_destroy(nullptr) == FDM_OK);
  printf("render_host_check ok (%d faces of %d vertices, %d x %d)\n", F, V, W, H);
  return 0;
}
