// Host side of multi-sample rendering under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the table of
// fdm_render_sample_pattern_host into exactly sized buffers, the refusals of fdm_render_set "samples" (a count other than 1, 4 or 16;
// more than 2^26 keys per frame) and of an unknown key, each a code and a message (csrc/render_out.hip, with the mesh unit it calls);
// the two symbols those units take from fdm_hip.hip are supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/render_aa_host_check.cpp render_out.hip mesh_out.hip -o ../../tools/_build/render_aa_host_check
//   ../../tools/_build/render_aa_host_check          -> "render_aa_host_check ok", exit status 0
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
// the call is refused with FDM_ERR_ARG and a message that holds `word`
#define REFUSED(call, word) do { fdm::g_err.clear(); EXPECT((call) == FDM_ERR_ARG); EXPECT(fdm::g_err.find(word) != std::string::npos); } while (0)

static int make(int W, int H, fdm_render** out) {
  static const int faces[6] = {0, 1, 2, 0, 2, 3};
  static const float cam[6] = {48.f, 48.f, 16.f, 16.f, 0.01f, 3.f}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, -1};
  static const float light[4] = {0.f, 0.6f, 0.8f, 0.25f}, base[3] = {0.3f, 0.3f, 0.3f}, bg[3] = {1.f, 1.f, 1.f};
  return fdm_render_create(faces, 2, 4, W, H, cam, R, t, light, 1, 0.2f, base, bg, out);
}

int main() {
  // the three tables, each into a buffer of exactly 2 S ints (a write past it is the sanitizer's to find)
  const int want4[8] = {96, 32, 224, 96, 32, 160, 160, 224};
  for (int S : {1, 4, 16}) {
    std::vector<int> xy(2 * (size_t)S, -7);
    EXPECT(fdm_render_sample_pattern_host(S, xy.data()) == FDM_OK);
    for (int s = 0; s < S; ++s) {
      const int x = S == 1 ? 128 : S == 4 ? want4[2 * s] : 32 + 64 * (s % 4), y = S == 1 ? 128 : S == 4 ? want4[2 * s + 1] : 32 + 64 * (s / 4);
      EXPECT(xy[2 * s] == x && xy[2 * s + 1] == y);
    }
  }
  int two[2] = {-7, -7};
  for (int S : {0, 2, 8, 32, -4, 3, 17}) {
    REFUSED(fdm_render_sample_pattern_host(S, two), "1, 4 or 16");
    EXPECT(two[0] == -7 && two[1] == -7);         // a refused call writes nothing
  }
  REFUSED(fdm_render_sample_pattern_host(4, nullptr), "null");

  // "samples" on an object without a device
  fdm_render* r = nullptr;
  EXPECT(make(37, 29, &r) == FDM_OK && r != nullptr);
  for (long long n : {2LL, -1LL, 17LL, 0LL, 8LL, 1LL << 32}) REFUSED(fdm_render_set(r, "samples", n), "1, 4 or 16");
  REFUSED(fdm_render_set(r, "sample", 4), "unknown key");
  EXPECT(fdm::g_err.find("chunk_frames") != std::string::npos && fdm::g_err.find("samples") != std::string::npos);
  REFUSED(fdm_render_set(nullptr, "samples", 4), "null");
  REFUSED(fdm_render_set(r, nullptr, 4), "null");
  for (long long n : {4LL, 16LL, 1LL}) EXPECT(fdm_render_set(r, "samples", n) == FDM_OK);
  EXPECT(fdm_render_set(r, "chunk_frames", 2) == FDM_OK);
  // a call at 16 samples still ends at the missing device, after every check
  EXPECT(fdm_render_set(r, "samples", 16) == FDM_OK);
  const int frames[1] = {3};
  EXPECT(fdm_render_forward(r, (const float*)0x1000, frames, 1, 3, nullptr, 0, 0, 0, nullptr, (unsigned char*)0x2000, nullptr, nullptr, 3, nullptr,
                            nullptr) == FDM_ERR_STATE);
  EXPECT(fdm_render_destroy(r) == FDM_OK);

  // W H S <= 2^26 keys per frame: 4096^2 at 4 samples and 2048^2 at 16 are the largest
  EXPECT(make(4096, 4096, &r) == FDM_OK);
  EXPECT(fdm_render_set(r, "samples", 4) == FDM_OK);
  REFUSED(fdm_render_set(r, "samples", 16), "2^26");
  EXPECT(fdm_render_set(r, "samples", 1) == FDM_OK && fdm_render_destroy(r) == FDM_OK);
  EXPECT(make(2048, 2048, &r) == FDM_OK);
  EXPECT(fdm_render_set(r, "samples", 16) == FDM_OK && fdm_render_destroy(r) == FDM_OK);
  EXPECT(make(2049, 2048, &r) == FDM_OK);
  REFUSED(fdm_render_set(r, "samples", 16), "2^26");
  EXPECT(fdm_render_set(r, "samples", 4) == FDM_OK && fdm_render_destroy(r) == FDM_OK);
  EXPECT(make(4096, 4095, &r) == FDM_OK);
  EXPECT(fdm_render_set(r, "samples", 4) == FDM_OK);
  REFUSED(fdm_render_set(r, "samples", 16), "2^26");
  EXPECT(fdm_render_destroy(r) == FDM_OK);
  printf("render_aa_host_check ok\n");
  return 0;
}
