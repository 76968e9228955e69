// Host-side helpers shared by the C layers of libfdm_hip.so (fdm_hip.hip, plan.hip, tune.hip, host_tables.hip, encoders.hip):
// error macros, the operand-kind table, device-memory arenas, the operand / GEMM-argument constructors, and what the hand-off units
// (mesh_out.hip, rig_out.hip, flame_out.hip) share: the frame rule, the clip lengths of a call and the object lifecycle.  No device code;
// the kernel units (gemm_*.hip, attn_*.hip) do not include it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kernels.hpp"

#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fdm::fail(FDM_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)
#define FCK(x) do { int r_ = (x); if (r_ != FDM_OK) return r_; } while (0)

namespace fdm {

// blocks of 256 threads for a grid-stride loop over n elements
inline int grid_for(long long n) { long long b = (n + 255) / 256; return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }

// ---- operand kinds (FDM_F32 | FDM_BF16 | FDM_F16X3 | FDM_F16): the one place that knows their geometry
struct Kind {
  int bytes;       // per element of one plane
  int planes;      // 2 = split kind (hi plane, lo plane lo_off elements behind it)
  int bk;          // k-tile of the GEMM kernels (K must be a multiple)
  int epc;         // elements per 16 bytes (row strides and offsets must be multiples)
  size_t full() const { return (size_t)bytes * planes; }      // bytes per matrix element over all planes
};
inline bool kind_ok(int dtype) { return dtype >= FDM_F32 && dtype <= FDM_F16; }
inline const Kind& kind(int dtype) {      // (callers check kind_ok first; an unknown code reads as FDM_F32)
  static const Kind table[4] = {{4, 1, 32, 4}, {2, 1, 64, 8}, {2, 2, 64, 8}, {2, 1, 64, 8}};
  return table[kind_ok(dtype) ? dtype : FDM_F32];
}

struct Wt { float* p = nullptr; long long n = 0; };       // fp32 weight / buffer by reference state-dict name
struct Mat { void* p = nullptr; long long lo = 0; };      // operand-kind matrix: pointer + hi->lo plane distance (elements; 0 = one plane)

// device allocations with one lifetime
struct Arena {
  std::vector<void*> allocs;
  int alloc(void** out, size_t bytes, bool zero = false) {
    void* p = nullptr;
    HIPCK(hipMalloc(&p, bytes ? bytes : 16));
    if (zero) HIPCK(hipMemset(p, 0, bytes ? bytes : 16));
    allocs.push_back(p);
    *out = p;
    return FDM_OK;
  }
  template <typename T> int alloc_t(T** out, size_t n, bool zero = false) { return alloc((void**)out, n * sizeof(T), zero); }
  void free_one(void* p) {      // (the caller has drained whatever may still read p)
    auto it = std::find(allocs.begin(), allocs.end(), p);
    if (it == allocs.end()) return;
    allocs.erase(it);
    (void)hipFree(p);
  }
  void release() { for (void* p : allocs) (void)hipFree(p); allocs.clear(); }
};

// a scratch array of an object that grows when a call is larger than any before it (that call waits for the device first: the old
// array may still be read)
template <typename T> int grow(Arena& mem, T** p, long long* cap, long long n) {
  if (n <= *cap) return FDM_OK;
  if (*p) { HIPCK(hipDeviceSynchronize()); mem.free_one(*p); *p = nullptr; *cap = 0; }
  FCK(mem.alloc_t(p, (size_t)n));
  *cap = n;
  return FDM_OK;
}

// the frame rates of the hand-offs (fdm_mesh_*, fdm_rig_*): finite and >= 0; resampling happens when both are given and differ
inline int check_fps(const char* who, double fps_in, double fps_out) {
  if (!(fps_in >= 0.0) || !(fps_out >= 0.0) || std::isinf(fps_in) || std::isinf(fps_out))
    return fail(FDM_ERR_ARG, "%s: frame rates %g -> %g (finite and >= 0; 0 = no resampling)", who, fps_in, fps_out);
  return FDM_OK;
}
inline bool resamples(double fps_in, double fps_out) { return fps_in > 0.0 && fps_out > 0.0 && fps_in != fps_out; }

// L_out of a clip of L frames (the rule of the audio encoder's interpolated length); < 0: does not fit an int
inline long long frames_out_of(int L, double fps_in, double fps_out) {
  if (L == 0 || !resamples(fps_in, fps_out)) return L;
  const double x = (double)L / fps_in * fps_out;
  if (!(x < 2147483648.0)) return -1;
  const long long n = (long long)x;
  return n < 1 ? 1 : n;
}

// The clip lengths of a hand-off call as the kernels read them: hl = {L, L_out} per clip, or L alone (L_out_max = 0: no frame rates).
// frames: L per clip, null = L_max.  `bad` says what failed at clip `clip` (the caller words the refusal).
struct ClipLens { enum { OK, LENGTH, OUTPUT } bad = OK; int clip = 0, L = 0; long long Lo = 0; };
inline ClipLens clip_lens(const int* frames, int B, int L_max, double fps_in, double fps_out, int L_out_max, std::vector<int>& hl) {
  const int per = L_out_max > 0 ? 2 : 1;
  hl.resize((size_t)per * B);
  ClipLens c;
  for (c.clip = 0; c.clip < B; ++c.clip) {
    c.L = frames ? frames[c.clip] : L_max;
    if (c.L < 0 || c.L > L_max) { c.bad = ClipLens::LENGTH; return c; }
    hl[(size_t)per * c.clip] = c.L;
    if (per == 1) continue;
    c.Lo = frames_out_of(c.L, fps_in, fps_out);
    if (c.Lo < 0 || c.Lo > L_out_max) { c.bad = ClipLens::OUTPUT; return c; }
    hl[2 * (size_t)c.clip + 1] = (int)c.Lo;
  }
  return c;
}

// ---- what the hand-off objects (fdm_mesh, fdm_rig, fdm_flame) share.  Made without a visible device, one refuses forward().
struct Handoff {
  Arena mem;
  int* lens = nullptr;          // device: hl of clip_lens for the call in flight
  long long lens_cap = 0;
  bool on_device = false;
};
template <typename T, typename S> int put(Arena& mem, T** dst, const S* src, size_t n) {      // src in a new device array
  FCK(mem.alloc_t(dst, n));
  if (n) HIPCK(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
  return FDM_OK;
}
// the tail of *_create: with a device, run `upload` (on failure the object is released and deleted); hand the object out
template <typename T, typename F> int handoff_finish(T* obj, T** out, F upload) {
  if (fdm_device_ok()) {
    const int r = upload();
    if (r != FDM_OK) { obj->mem.release(); delete obj; return r; }
    obj->on_device = true;
  }
  *out = obj;
  return FDM_OK;
}
template <typename T> int handoff_destroy(T* obj) {
  if (!obj) return FDM_OK;
  if (obj->on_device) (void)hipDeviceSynchronize();
  obj->mem.release();
  delete obj;
  return FDM_OK;
}
inline int handoff_device(const Handoff& h, const char* who) {
  if (!h.on_device || !fdm_device_ok()) return fail(FDM_ERR_STATE, "%s: no gfx950 device visible (there is no CPU fallback)", who);
  return FDM_OK;
}
inline int handoff_lens(Handoff& h, const std::vector<int>& hl, hipStream_t s) {
  FCK(grow(h.mem, &h.lens, &h.lens_cap, (long long)hl.size()));
  HIPCK(hipMemcpyAsync(h.lens, hl.data(), hl.size() * sizeof(int), hipMemcpyHostToDevice, s));
  return FDM_OK;
}

inline int need_weight(const std::map<std::string, Wt>& w, const char* who, const std::string& name, long long n, const float** out) {
  auto it = w.find(name);
  if (it == w.end()) return fail(FDM_ERR_STATE, "%smissing weight %s", who, name.c_str());
  if (it->second.n != n) return fail(FDM_ERR_SHAPE, "%sweight %s has %lld elements, expected %lld", who, name.c_str(), it->second.n, n);
  *out = it->second.p;
  return FDM_OK;
}

// GEMM args with the defaults the op layer's callers use (dense row-major operands, one batch)
inline fdm_gemm_args dense_gemm(int dtype, const void* A, const void* W, int M, int N, int K) {
  fdm_gemm_args a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.lda = K; a.W = W; a.ldw = K; a.M = M; a.N = N; a.K = K; a.batch = 1; a.dtype = dtype;
  a.ldr = N; a.ldo_f32 = N; a.ldo_t = N; a.ln_eps = 1e-5f;
  return a;
}

// operand-kind copy of n fp32 elements, allocated from `mem` (FDM_F32: the fp32 array itself; split kinds: fdm_op_cast writes the
// lo plane n elements after the hi plane)
inline int to_operand(Arena& mem, int dtype, const float* src, long long n, Mat* out, void* stream) {
  out->lo = kind(dtype).planes == 2 ? n : 0;
  if (dtype == FDM_F32) { out->p = (void*)src; return FDM_OK; }
  FCK(mem.alloc(&out->p, (size_t)n * kind(dtype).full()));
  return fdm_op_cast(src, out->p, n, dtype, stream);
}

// host tables that the plan layer also uses directly (host_tables.hip; include/fdm_hip.h states the rules)
int window_layout(int L, int W, int O, std::vector<int>& starts);
void window_weights(int L, int W, int O, const std::vector<int>& starts, std::vector<float>& out);

}  // namespace fdm
