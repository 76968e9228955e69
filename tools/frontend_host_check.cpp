// Host side of the audio front end under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python):
// the tap / ratio / length tables (csrc/host_tables.hip) and fdm_frontend_create / _samples / _forward's argument checks and table
// layout (csrc/frontend.hip), with the two symbols those units take from fdm_hip.hip supplied here (no device is ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/frontend_host_check.cpp host_tables.hip frontend.hip -o ../../tools/_build/frontend_host_check
//   ../../tools/_build/frontend_host_check          -> "frontend_host_check ok", exit status 0
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
  // ratios, lengths (64-bit), taps: every supported corner, and the largest table (m = 2048: 40961 taps)
  const int rates[] = {48000, 44100, 32000, 24000, 22050, 11025, 8000, 96000, 16000, 125, 16000 * 2048};
  for (int rate : rates) {
    int up = 0, down = 0;
    EXPECT(fdm_resample_ratio_host(rate, &up, &down) == FDM_OK);
    EXPECT((long long)up * rate == (long long)down * 16000);
    std::vector<double> h(20 * (size_t)std::max(up, down) + 1);
    EXPECT(fdm_resample_taps_host(up, down, h.data()) == (int)h.size());
    double sum = 0;
    for (double v : h) sum += v;
    EXPECT(std::fabs(sum - up) < 1e-9 && h.front() == h.back());
    const long long frames[] = {1, 2, down, (1LL << 31) / down, (1LL << 31) / down + 1, (1LL << 40) + 12345};
    for (long long f : frames) EXPECT(fdm_resample_len_host(rate, f) == (f * up + down - 1) / down);
  }
  int u, d;
  EXPECT(fdm_resample_ratio_host(0, &u, &d) == FDM_ERR_ARG && fdm_resample_ratio_host(16001, &u, &d) == FDM_ERR_SHAPE);
  EXPECT(fdm_resample_len_host(48000, 0) == FDM_ERR_SHAPE && fdm_resample_taps_host(1, 3, nullptr) == FDM_ERR_ARG);

  // the object: table layout on the host, then every refusal of forward (none reaches a launch; no device here)
  fdm_frontend* fe = nullptr;
  const int want[] = {48000, 44100, 11025, 16000, 48000, 16000 * 2048};
  EXPECT(fdm_frontend_create(want, 6, nullptr) == FDM_ERR_ARG && fdm_frontend_create(nullptr, 1, &fe) == FDM_ERR_ARG);
  const int bad[] = {48000, 16001};
  EXPECT(fdm_frontend_create(bad, 2, &fe) == FDM_ERR_SHAPE);
  EXPECT(fdm_frontend_create(want, 6, &fe) == FDM_OK && fe);
  short pcm[64] = {0};
  float wav[64];
  int ns[3] = {0, 0, 0};
  fdm_pcm ok = {pcm, FDM_PCM_S16, 2, 48000, 30};
  long long n = 0;
  EXPECT(fdm_frontend_samples(&ok, 5, &n) == FDM_OK && n == 15);
  EXPECT(fdm_frontend_samples(nullptr, 0, &n) == FDM_ERR_ARG && fdm_frontend_samples(&ok, -1, &n) == FDM_ERR_ARG);
  auto fwd = [&](fdm_pcm c, int B, int pad, long long n_max) { fdm_pcm cs[2] = {ok, c}; return fdm_frontend_forward(fe, cs, B, pad, 1, wav, n_max, ns, nullptr); };
  fdm_pcm c = ok;
  EXPECT(fdm_frontend_forward(nullptr, &ok, 1, 0, 1, wav, 64, ns, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_frontend_forward(fe, nullptr, 1, 0, 1, wav, 64, ns, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_frontend_forward(fe, &ok, 1, 0, 1, nullptr, 64, ns, nullptr) == FDM_ERR_ARG);
  EXPECT(fdm_frontend_forward(fe, &ok, 1, 0, 1, wav, 64, nullptr, nullptr) == FDM_ERR_ARG);
  c = ok; c.data = nullptr; EXPECT(fwd(c, 2, 0, 64) == FDM_ERR_ARG);
  c = ok; c.format = 4; EXPECT(fwd(c, 2, 0, 64) == FDM_ERR_ARG);
  c = ok; c.channels = 9; EXPECT(fwd(c, 2, 0, 64) == FDM_ERR_ARG);
  c = ok; c.rate = 22050; EXPECT(fwd(c, 2, 0, 64) == FDM_ERR_ARG);
  c = ok; c.data = (const char*)pcm + 1; EXPECT(fwd(c, 2, 0, 64) == FDM_ERR_ARG);
  EXPECT(fwd(ok, 2, -1, 64) == FDM_ERR_ARG);
  EXPECT(fwd(ok, 0, 0, 64) == FDM_ERR_SHAPE);
  c = ok; c.frames = 0; EXPECT(fwd(c, 2, 0, 64) == FDM_ERR_SHAPE);
  EXPECT(fwd(ok, 2, 0, 9) == FDM_ERR_SHAPE && fwd(ok, 2, 55, 64) == FDM_ERR_SHAPE && fwd(ok, 2, 0, 1LL << 32) == FDM_ERR_SHAPE);
  EXPECT(ns[0] == 0 && ns[1] == 0);
  c = ok; c.rate = 16000; c.format = FDM_PCM_U8; c.channels = 1;
  EXPECT(fwd(c, 2, 3, 64) == FDM_ERR_STATE);          // every check passed: there is no device, and no fallback
  EXPECT(fdm_frontend_destroy(fe) == FDM_OK && fdm_frontend_destroy(nullptr) == FDM_OK);
  printf("frontend_host_check ok\n");
  return 0;
}
