// Host side of the render hand-off's planes under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the
// table of fdm_render_yuv_coeffs_host into an exactly sized buffer, the refusals of fdm_render_set "yuv_matrix" / "yuv_range" /
// "yuv_layout", and the argument checks of fdm_render_forward_planes on an object without a device, each a code and a message
// (csrc/render_out.hip, with the mesh unit it calls); the two symbols those units take from fdm_hip.hip are supplied here (no device
// is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/render_planes_host_check.cpp render_out.hip mesh_out.hip -o ../../tools/_build/render_planes_host_check
//   ../../tools/_build/render_planes_host_check          -> "render_planes_host_check ok", exit status 0
#include <cstdarg>
#include <cstdio>
#include <cstring>
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
// the call is refused with `code` and a message that holds `word`
#define REFUSED_AS(call, code, word) do { fdm::g_err.clear(); EXPECT((call) == (code)); EXPECT(fdm::g_err.find(word) != std::string::npos); } while (0)
#define REFUSED(call, word) REFUSED_AS(call, FDM_ERR_ARG, word)

static int make(int W, int H, fdm_render** out) {
  static const int faces[6] = {0, 1, 2, 0, 2, 3};
  static const float cam[6] = {48.f, 48.f, 16.f, 16.f, 0.01f, 3.f}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, -1};
  static const float light[4] = {0.f, 0.6f, 0.8f, 0.25f}, base[3] = {0.3f, 0.3f, 0.3f}, bg[3] = {1.f, 1.f, 1.f};
  return fdm_render_create(faces, 2, 4, W, H, cam, R, t, light, 1, 0.2f, base, bg, out);
}

int main() {
  // the four tables, each into a buffer of exactly ten ints (a write past it is the sanitizer's to find)
  static const int want[4][10] = {{16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, 16},
                                  {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329, 0},
                                  {11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639, 16},
                                  {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005, 0}};
  for (int m = 0; m < 2; ++m)
    for (int full = 0; full < 2; ++full) {
      std::vector<int> k(10, -7);
      EXPECT(fdm_render_yuv_coeffs_host(m ? 709 : 601, full, k.data()) == FDM_OK);
      EXPECT(std::memcmp(k.data(), want[2 * m + full], sizeof(want[0])) == 0);
    }
  std::vector<int> k(10, -7);
  for (int m : {0, 2020, 600, -709, 1}) {
    REFUSED(fdm_render_yuv_coeffs_host(m, 0, k.data()), "601 or 709");
    for (int v : k) EXPECT(v == -7);              // a refused call writes nothing
  }
  REFUSED(fdm_render_yuv_coeffs_host(709, 1, nullptr), "null");

  // the three keys on an object without a device
  fdm_render* r = nullptr;
  EXPECT(make(32, 32, &r) == FDM_OK && r != nullptr);
  for (long long v : {0LL, 2020LL, 600LL, 1LL, -709LL, 709LL + (1LL << 32)}) REFUSED(fdm_render_set(r, "yuv_matrix", v), "601 or 709");
  for (long long v : {-1LL, 2LL, 16LL, 1LL << 32}) REFUSED(fdm_render_set(r, "yuv_range", v), "0 limited, 1 full");
  for (long long v : {-1LL, 2LL, 420LL, 1LL << 32}) REFUSED(fdm_render_set(r, "yuv_layout", v), "0 I420, 1 NV12");
  REFUSED(fdm_render_set(r, "yuv", 1), "unknown key");
  for (const char* key : {"chunk_frames", "samples", "yuv_matrix", "yuv_range", "yuv_layout"}) EXPECT(fdm::g_err.find(key) != std::string::npos);
  for (long long v : {601LL, 709LL}) EXPECT(fdm_render_set(r, "yuv_matrix", v) == FDM_OK);
  for (long long v : {1LL, 0LL}) EXPECT(fdm_render_set(r, "yuv_range", v) == FDM_OK && fdm_render_set(r, "yuv_layout", v) == FDM_OK);

  // the planes call: every check before the missing device is reported (no pointer is dereferenced)
  const float* x = (const float*)0x1000;
  unsigned char* y = (unsigned char*)0x2000;
  const int frames[2] = {3, 0}, bad[2] = {3, 4};
  fdm_render_planes none = {nullptr, nullptr, nullptr, nullptr, nullptr}, yuv = none, alpha = none, all = none, odd_at = none;
  yuv.yuv = y;
  alpha.alpha = y;
  all.rgb = y; all.depth = (float*)0x3000; all.face = (int*)0x4000; all.alpha = (unsigned char*)0x5000; all.yuv = (unsigned char*)0x6000;
  odd_at.yuv = y + 1;
  REFUSED(fdm_render_forward_planes(nullptr, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, &yuv, 3, nullptr, nullptr), "null");
  REFUSED(fdm_render_forward_planes(r, nullptr, frames, 2, 3, nullptr, 0, 0, 0, nullptr, &yuv, 3, nullptr, nullptr), "null");
  REFUSED(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, nullptr, 3, nullptr, nullptr), "null");
  REFUSED(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, &none, 3, nullptr, nullptr), "every output is null");
  REFUSED(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, &odd_at, 3, nullptr, nullptr), "aligned");
  REFUSED(fdm_render_forward_planes(r, x, frames, 2, 3, x, 3, 0, 0, nullptr, &yuv, 3, nullptr, nullptr), "tmpl_rows");
  REFUSED(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 1, 0, 0, nullptr, &yuv, 3, nullptr, nullptr), "null template");
  REFUSED(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, -1.0, 30.0, nullptr, &yuv, 3, nullptr, nullptr), "frame rates");
  REFUSED_AS(fdm_render_forward_planes(r, x, frames, 0, 3, nullptr, 0, 0, 0, nullptr, &yuv, 3, nullptr, nullptr), FDM_ERR_SHAPE, "B = 0");
  REFUSED_AS(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, &yuv, 0, nullptr, nullptr), FDM_ERR_SHAPE, "L_out_max = 0");
  REFUSED_AS(fdm_render_forward_planes(r, x, bad, 2, 3, nullptr, 0, 0, 0, nullptr, &yuv, 3, nullptr, nullptr), FDM_ERR_SHAPE, "clip 1 has 4 frames");
  REFUSED_AS(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 30.0, 60.0, nullptr, &yuv, 5, nullptr, nullptr), FDM_ERR_SHAPE, "gives 6 frames");
  int got[2] = {-7, -7};
  for (const fdm_render_planes* p : {&yuv, &alpha, &all})
    for (long long S : {1LL, 4LL, 16LL}) {
      EXPECT(fdm_render_set(r, "samples", S) == FDM_OK);
      REFUSED_AS(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, p, 3, got, nullptr), FDM_ERR_STATE, "no gfx950 device");
    }
  EXPECT(got[0] == -7 && got[1] == -7);
  EXPECT(fdm_render_destroy(r) == FDM_OK);

  // yuv needs an even width and height; alpha does not
  for (int odd = 0; odd < 2; ++odd) {
    EXPECT(make(odd ? 32 : 31, odd ? 17 : 32, &r) == FDM_OK);
    REFUSED(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, &yuv, 3, nullptr, nullptr), "even width and height");
    REFUSED(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, &all, 3, nullptr, nullptr), "even width and height");
    REFUSED_AS(fdm_render_forward_planes(r, x, frames, 2, 3, nullptr, 0, 0, 0, nullptr, &alpha, 3, nullptr, nullptr), FDM_ERR_STATE, "no gfx950 device");
    EXPECT(fdm_render_destroy(r) == FDM_OK);
  }
  printf("render_planes_host_check ok\n");
  return 0;
}
