// Raw audio to encoder features without Python or torch: int16 stereo 48 kHz PCM -> fdm_frontend_forward -> fdm_hubert_forward_ragged
// (a 2-layer HuBERT whose weights arrive by state-dict name from a flat record file).  Checks status codes, lengths, n_frames, the
// padding and that the waveform is normalised.  Built and run by tests/test_audio_frontend_gpu.py:
//   hipcc frontend_smoke.cpp -I include -L <dir> -lfdm_hip ; frontend_smoke weights.bin
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "fdm_hip.h"

#define CK(x) do { if ((x) != 0) { printf("FAIL %s: %s\n", #x, fdm_last_error()); return 1; } } while (0)
#define HK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: frontend_smoke weights.bin\n"); return 2; }
  if (!fdm_device_ok()) { printf("no gfx950 device\n"); return 2; }
  hipStream_t st;
  HK(hipStreamCreate(&st));

  // two clips of unequal length: 0.5 s and 0.3 s of 48 kHz stereo int16 (a tone plus an offset, other phase on the right channel)
  const int B = 2, rate = 48000, pad = 16000;
  const long long frames[B] = {24000, 14401};
  short* d_pcm[B];
  fdm_pcm clips[B];
  for (int b = 0; b < B; ++b) {
    std::vector<short> h(frames[b] * 2);
    for (long long i = 0; i < frames[b]; ++i) {
      h[2 * i] = (short)(9000.0 * std::sin(0.02 * i * (b + 1)) + 700.0);
      h[2 * i + 1] = (short)(6000.0 * std::cos(0.013 * i) - 300.0);
    }
    HK(hipMalloc(&d_pcm[b], h.size() * sizeof(short)));
    HK(hipMemcpy(d_pcm[b], h.data(), h.size() * sizeof(short), hipMemcpyHostToDevice));
    clips[b] = fdm_pcm{d_pcm[b], FDM_PCM_S16, 2, rate, frames[b]};
  }
  const int rates[1] = {rate};
  fdm_frontend* fe = nullptr;
  CK(fdm_frontend_create(rates, 1, &fe));
  long long n[B], n_max = 0;
  for (int b = 0; b < B; ++b) {
    CK(fdm_frontend_samples(&clips[b], pad, &n[b]));
    const long long want = (frames[b] + 2) / 3 + pad;          // ceil(frames / 3) + pad
    if (n[b] != want) { printf("FAIL: clip %d: %lld samples, expected %lld\n", b, n[b], want); return 1; }
    n_max = n[b] > n_max ? n[b] : n_max;
  }
  float* wav = nullptr;
  HK(hipMalloc(&wav, (size_t)B * n_max * sizeof(float)));
  HK(hipMemset(wav, 0xff, (size_t)B * n_max * sizeof(float)));          // NaN everywhere: the call writes the whole batch
  int n_samples[B] = {0, 0};

  // refusals come back as codes, before any launch
  fdm_pcm bad = clips[0];
  bad.rate = 44100;
  if (fdm_frontend_forward(fe, &bad, 1, pad, 1, wav, n_max, n_samples, st) != FDM_ERR_ARG) { printf("FAIL: a rate without a table was accepted\n"); return 1; }
  bad = clips[0];
  bad.channels = 9;
  if (fdm_frontend_forward(fe, &bad, 1, pad, 1, wav, n_max, n_samples, st) != FDM_ERR_ARG) { printf("FAIL: 9 channels accepted\n"); return 1; }
  if (fdm_frontend_forward(fe, clips, B, pad, 1, wav, n_max - 1, n_samples, st) != FDM_ERR_SHAPE) { printf("FAIL: a batch too narrow was accepted\n"); return 1; }
  if (fdm_frontend_forward(fe, clips, 0, pad, 1, wav, n_max, n_samples, st) != FDM_ERR_SHAPE) { printf("FAIL: B = 0 accepted\n"); return 1; }
  if (n_samples[0] != 0 || n_samples[1] != 0) { printf("FAIL: a refused call wrote lengths\n"); return 1; }

  CK(fdm_frontend_forward(fe, clips, B, pad, 1, wav, n_max, n_samples, st));
  HK(hipStreamSynchronize(st));
  std::vector<float> h((size_t)B * n_max);
  HK(hipMemcpy(h.data(), wav, h.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    if (n_samples[b] != n[b]) { printf("FAIL: clip %d: n_samples = %d, expected %lld\n", b, n_samples[b], n[b]); return 1; }
    const long long n_out = n[b] - pad;
    double s = 0, q = 0;
    for (long long i = 0; i < n_out; ++i) { const double v = h[(size_t)b * n_max + i]; s += v; q += v * v; }
    const double mean = s / n_out, var = q / n_out - mean * mean;
    if (!(std::fabs(mean) < 1e-5) || !(std::fabs(var - 1.0) < 1e-4)) { printf("FAIL: clip %d: mean %.3e, variance %.6f after normalisation\n", b, mean, var); return 1; }
    for (long long i = n_out; i < n_max; ++i)
      if (h[(size_t)b * n_max + i] != 0.f) { printf("FAIL: clip %d: sample %lld of the padding is %g\n", b, i, h[(size_t)b * n_max + i]); return 1; }
    printf("clip %d: %lld frames at %d Hz -> %d samples (mean %.2e, variance %.6f)\n", b, frames[b], rate, n_samples[b], mean, var);
  }

  // the encoder takes the batch as it is
  fdm_audio_encoder* enc = nullptr;
  CK(fdm_hubert_create(0, 2, FDM_F32, &enc));
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  int n_weights = 0;
  for (;;) {
    unsigned nl = 0;
    if (fread(&nl, 4, 1, f) != 1) break;
    std::string name(nl, '\0');
    unsigned long long cnt = 0;
    if (fread(&name[0], 1, nl, f) != nl || fread(&cnt, 8, 1, f) != 1) { printf("truncated record\n"); return 2; }
    std::vector<float> v(cnt);
    if (fread(v.data(), 4, cnt, f) != cnt) { printf("truncated record %s\n", name.c_str()); return 2; }
    CK(fdm_hubert_set_weights(enc, name.c_str(), v.data(), (long long)cnt, st));
    HK(hipStreamSynchronize(st));          // (v is host memory that goes away)
    ++n_weights;
  }
  fclose(f);
  int N[B], N_max = 0;
  for (int b = 0; b < B; ++b) { N[b] = fdm_hubert_frames(n_samples[b]); N_max = N[b] > N_max ? N[b] : N_max; }
  float* out = nullptr;
  HK(hipMalloc(&out, (size_t)B * N_max * 1024 * sizeof(float)));
  int n_frames[B] = {0, 0};
  CK(fdm_hubert_forward_ragged(enc, wav, n_samples, B, (int)n_max, out, n_frames, st));
  HK(hipStreamSynchronize(st));
  std::vector<float> ho((size_t)B * N_max * 1024);
  HK(hipMemcpy(ho.data(), out, ho.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    if (n_frames[b] != N[b] || N[b] < 2) { printf("FAIL: clip %d: n_frames = %d, fdm_hubert_frames = %d\n", b, n_frames[b], N[b]); return 1; }
    for (size_t i = 0; i < (size_t)N[b] * 1024; ++i)
      if (!std::isfinite(ho[(size_t)b * N_max * 1024 + i])) { printf("FAIL: clip %d: feature %zu is not finite\n", b, i); return 1; }
    printf("clip %d: %d encoder frames\n", b, n_frames[b]);
  }
  CK(fdm_hubert_destroy(enc));
  CK(fdm_frontend_destroy(fe));
  for (int b = 0; b < B; ++b) HK(hipFree(d_pcm[b]));
  HK(hipFree(wav)); HK(hipFree(out));
  printf("frontend_smoke ok (%d weights, libfdm_hip version %d)\n", n_weights, fdm_version());
  return 0;
}
