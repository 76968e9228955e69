// Audio front end behind plain C calls (include/fdm_hip.h, fdm_frontend_*): raw PCM -> the [B, n_max] waveform batch and host
// lengths that fdm_hubert_forward_ragged takes.  Tables come from host_tables.hip, kernels from audio_front.hpp.  Everything is
// allocated in fdm_frontend_create; a forward call only validates (every check before the first launch) and launches.
#include <hip/hip_runtime.h>

#include <vector>

#include "audio_front.hpp"
#include "host.hpp"

struct fdm_frontend {
  struct Rate { int rate = 0, up = 1, down = 1, half = 0, Q = 0; std::vector<float> tab; float* dev = nullptr; };
  std::vector<Rate> rates;
  fdm::Arena mem;
  double* part = nullptr;      // statistics partials of one launch group [FRONT_GROUP][FRONT_CHUNKS_MAX][2]
  bool on_device = false;
  const Rate* find(int rate) const {
    for (const Rate& r : rates) if (r.rate == rate) return &r;
    return nullptr;
  }
};

namespace {
using namespace fdm;

const int PCM_BYTES[4] = {2, 4, 1, 4};      // FDM_PCM_S16, _S32, _U8, _F32

// n_out of a clip (negative: the error of the ratio or of frames)
long long clip_len(const fdm_pcm& c) { return fdm_resample_len_host(c.rate, c.frames); }

}  // namespace

extern "C" {

int fdm_frontend_create(const int* rates, int n_rates, fdm_frontend** out) {
  if (!out) return fail(FDM_ERR_ARG, "frontend_create: null out");
  if (n_rates < 0 || (n_rates > 0 && !rates)) return fail(FDM_ERR_ARG, "frontend_create: %d rates (or a null list)", n_rates);
  for (int i = 0; i < n_rates; ++i) {
    int up, down;
    FCK(fdm_resample_ratio_host(rates[i], &up, &down));
  }
  fdm_frontend* F = new (std::nothrow) fdm_frontend();
  if (!F) return fail(FDM_ERR_STATE, "frontend_create: out of memory");
  std::vector<double> h;
  for (int i = 0; i < n_rates; ++i) {
    if (F->find(rates[i])) continue;
    fdm_frontend::Rate r;
    r.rate = rates[i];
    (void)fdm_resample_ratio_host(r.rate, &r.up, &r.down);
    if (r.up != r.down) {          // phase-major table: tab[p][q] = h[p + q up], zero beyond the last tap
      r.half = 10 * std::max(r.up, r.down);
      const int n = 2 * r.half + 1;
      r.Q = (n + r.up - 1) / r.up;
      h.resize(n);
      (void)fdm_resample_taps_host(r.up, r.down, h.data());
      r.tab.assign((size_t)r.up * r.Q, 0.f);
      for (int k = 0; k < n; ++k) r.tab[(size_t)(k % r.up) * r.Q + k / r.up] = (float)h[k];
    }
    F->rates.push_back(std::move(r));
  }
  if (fdm_device_ok()) {
    auto upload = [&]() {
      for (auto& r : F->rates) {
        if (r.tab.empty()) continue;
        FCK(F->mem.alloc_t(&r.dev, r.tab.size()));
        HIPCK(hipMemcpy(r.dev, r.tab.data(), r.tab.size() * sizeof(float), hipMemcpyHostToDevice));
      }
      FCK(F->mem.alloc_t(&F->part, (size_t)FRONT_GROUP * FRONT_CHUNKS_MAX * 2, true));
      return (int)FDM_OK;
    };
    const int r = upload();
    if (r != FDM_OK) { F->mem.release(); delete F; return r; }
    F->on_device = true;
  }
  *out = F;
  return FDM_OK;
}

int fdm_frontend_destroy(fdm_frontend* F) {
  if (!F) return FDM_OK;
  if (F->on_device) (void)hipDeviceSynchronize();
  F->mem.release();
  delete F;
  return FDM_OK;
}

int fdm_frontend_samples(const fdm_pcm* clip, int pad, long long* n) {
  if (!clip || !n) return fail(FDM_ERR_ARG, "frontend_samples: null argument");
  if (pad < 0) return fail(FDM_ERR_ARG, "frontend_samples: pad = %d", pad);
  const long long n_out = clip_len(*clip);
  if (n_out < 0) return (int)n_out;
  *n = n_out + pad;
  return FDM_OK;
}

int fdm_frontend_forward(fdm_frontend* F, const fdm_pcm* clips, int B, int pad, int normalize, float* wav, long long n_max, int* n_samples,
                         void* stream) {
  if (!F || !clips || !wav || !n_samples) return fail(FDM_ERR_ARG, "frontend_forward: null argument");
  if (pad < 0) return fail(FDM_ERR_ARG, "frontend_forward: pad = %d", pad);
  if (B < 1) return fail(FDM_ERR_SHAPE, "frontend_forward: B = %d", B);
  for (int b = 0; b < B; ++b) {
    const fdm_pcm& c = clips[b];
    if (!c.data) return fail(FDM_ERR_ARG, "frontend_forward: clip %d: null data", b);
    if (c.format < FDM_PCM_S16 || c.format > FDM_PCM_F32) return fail(FDM_ERR_ARG, "frontend_forward: clip %d: unknown format %d", b, c.format);
    if (c.channels < 1 || c.channels > 8) return fail(FDM_ERR_ARG, "frontend_forward: clip %d: %d channels (1..8)", b, c.channels);
    if (c.rate != 16000 && !F->find(c.rate)) return fail(FDM_ERR_ARG, "frontend_forward: clip %d: the object was not created for %d Hz", b, c.rate);
    if ((uintptr_t)c.data % PCM_BYTES[c.format]) return fail(FDM_ERR_ARG, "frontend_forward: clip %d: data is not aligned to its %d-byte samples", b, PCM_BYTES[c.format]);
  }
  std::vector<long long> n_out(B);
  for (int b = 0; b < B; ++b) {
    n_out[b] = clip_len(clips[b]);
    if (n_out[b] < 0) return (int)n_out[b];
    if (n_out[b] + pad > n_max || n_out[b] + pad > 0x7fffffffLL)
      return fail(FDM_ERR_SHAPE, "frontend_forward: clip %d gives %lld samples, the batch is %lld wide (and a length is a 32-bit int)", b, n_out[b] + pad, n_max);
  }
  if (n_max > 0x7fffffffLL) return fail(FDM_ERR_SHAPE, "frontend_forward: n_max = %lld (fdm_hubert_forward_ragged takes a 32-bit width)", n_max);
  const long long tiles = (n_max + FRONT_TILE - 1) / FRONT_TILE;
  if (!F->on_device || !fdm_device_ok()) return fail(FDM_ERR_STATE, "frontend_forward: no gfx950 device visible (there is no CPU fallback)");
  hipStream_t s = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += FRONT_GROUP) {
    const int g = std::min(FRONT_GROUP, B - b0);
    FrontPack pk;
    memset(&pk, 0, sizeof(pk));
    int nch_max = 1;
    for (int i = 0; i < g; ++i) {
      const fdm_pcm& c = clips[b0 + i];
      const fdm_frontend::Rate* r = F->find(c.rate);
      FrontClip& d = pk.c[i];
      d.data = c.data; d.frames = c.frames; d.n_out = n_out[b0 + i]; d.format = c.format; d.channels = c.channels;
      d.up = d.down = 1;
      if (r && r->up != r->down) { d.taps = r->dev; d.up = r->up; d.down = r->down; d.half = r->half; d.Q = r->Q; }
      long long width;
      nch_max = std::max(nch_max, front_chunks_of(d.n_out, &width));
    }
    hipLaunchKernelGGL(front_resample_kernel, dim3((unsigned)tiles, g), dim3(FRONT_TILE), 0, s, wav, n_max, b0, pk);
    if (normalize) {
      hipLaunchKernelGGL(front_sum_kernel, dim3(nch_max, g), dim3(256), 0, s, (const float*)wav, n_max, b0, F->part, pk);
      hipLaunchKernelGGL(front_var_kernel, dim3(nch_max, g), dim3(256), 0, s, (const float*)wav, n_max, b0, F->part, pk);
      hipLaunchKernelGGL(front_norm_kernel, dim3(nch_max, g), dim3(256), 0, s, wav, n_max, b0, (const double*)F->part, pk);
    }
    HIPCK(hipGetLastError());
  }
  for (int b = 0; b < B; ++b) n_samples[b] = (int)(n_out[b] + pad);
  return FDM_OK;
}

}  // extern "C"
