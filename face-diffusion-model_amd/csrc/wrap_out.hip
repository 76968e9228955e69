// Wrap hand-off behind plain C calls (include/fdm_hip.h, fdm_wrap_*): a mesh of another topology follows the animated face through a
// surface binding.  Kernels: wrap_out.hpp.  fdm_wrap_create binds (the nearest-face search on the device unless the caller brings
// face_idx; the coordinates on the host in fp64), resolves every target vertex's face to its three source vertices and uploads the
// records; a forward call validates (every check before the first launch) and launches once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "host.hpp"
#include "wrap_out.hpp"

struct fdm_wrap : fdm::Handoff {          // lens: L per clip
  int V = 0, Vt = 0;
  bool weighted = false;
  std::vector<int> face_idx;              // host copies of the binding: [Vt], [Vt][3], [Vt]
  std::vector<float> uvh, dist;
  int4* abc = nullptr;                    // device: [Vt] {a, b, c, 0}, [Vt] {u, v, h, w}, [Vt][3]
  float4* uvhw = nullptr;
  float* rest_t = nullptr;
};

namespace {
using namespace fdm;

struct D3 { double x, y, z; };
inline D3 sub(const D3& a, const D3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline double dot(const D3& a, const D3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline D3 cross(const D3& a, const D3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline D3 at(const float* p, long long i) { return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]}; }

// dist2 of the region walk of the header, in double
double closest_dist2(const D3& q, const D3& a, const D3& b, const D3& c) {
  const D3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b), ap = sub(q, a), bp = sub(q, b), cp = sub(q, c);
  const double d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, d43 = d4 - d3, d56 = d5 - d6;
  double n1 = 0.0, m1 = 1.0, n2 = 0.0, m2 = 1.0;
  D3 o = a, u = ab;
  if (d1 <= 0.0 && d2 <= 0.0) {
  } else if (d3 >= 0.0 && d4 <= d3) {
    o = b;
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    n1 = d1; m1 = d1 - d3;
  } else if (d6 >= 0.0 && d5 <= d6) {
    o = c;
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    n2 = d2; m2 = d2 - d6;
  } else if (va <= 0.0 && d43 >= 0.0 && d56 >= 0.0) {
    o = b; u = bc; n1 = d43; m1 = d43 + d56;
  } else {
    const double s = (va + vb) + vc;
    n1 = vb; m1 = s; n2 = vc; m2 = s;
  }
  const double t1 = n1 / m1, t2 = n2 / m2;
  const D3 p = {(o.x + t1 * u.x) + t2 * ac.x, (o.y + t1 * u.y) + t2 * ac.y, (o.z + t1 * u.z) + t2 * ac.z};
  const D3 r = sub(q, p);
  return dot(r, r);
}

// sizes, a triangle list over V vertices, finite coordinates
int check_meshes(const char* who, const float* src_rest, const int* faces, int F, int V, const float* dst_rest, int Vt) {
  if (!src_rest || !faces || !dst_rest) return fail(FDM_ERR_ARG, "%s: null argument", who);
  if (F < 1 || V < 1 || Vt < 1) return fail(FDM_ERR_ARG, "%s: F = %d, V = %d, Vt = %d", who, F, V, Vt);
  if (F > 0x7fffffff / 3 || V > 0x7fffffff / 3 || Vt > 0x7fffffff / 3)
    return fail(FDM_ERR_ARG, "%s: F = %d, V = %d, Vt = %d (3 F, 3 V and 3 Vt are 32-bit ints)", who, F, V, Vt);
  for (long long i = 0; i < 3LL * F; ++i)
    if (faces[i] < 0 || faces[i] >= V) return fail(FDM_ERR_ARG, "%s: face %lld names vertex %d of %d", who, i / 3, faces[i], V);
  for (long long i = 0; i < 3LL * V; ++i)
    if (!std::isfinite(src_rest[i])) return fail(FDM_ERR_ARG, "%s: source vertex %lld has a non-finite coordinate", who, i / 3);
  for (long long i = 0; i < 3LL * Vt; ++i)
    if (!std::isfinite(dst_rest[i])) return fail(FDM_ERR_ARG, "%s: target vertex %lld has a non-finite coordinate", who, i / 3);
  return FDM_OK;
}

// the search of fdm_wrap_create: face_idx [Vt] on the host.  Temporaries live in an arena of their own, released on every path.
int nearest_on_device(const float* src_rest, const int* faces, int F, int V, const float* dst_rest, int Vt, std::vector<int>& face_idx) {
  const long long nvb = ((long long)Vt + WRAP_VB - 1) / WRAP_VB, tiles = ((long long)F + WRAP_FT - 1) / WRAP_FT;
  // faces are split where Vt alone does not fill the chip (about 1024 workgroups), a split scanning at least WRAP_SPLIT_TILES tiles
  long long nsplit = std::min(std::max(1LL, tiles / WRAP_SPLIT_TILES), std::max(1LL, 1024 / nvb));
  const long long tiles_per = (tiles + nsplit - 1) / nsplit;
  nsplit = (tiles + tiles_per - 1) / tiles_per;
  Arena tmp;
  float *rest = nullptr, *dst = nullptr, *part_d = nullptr;
  int *fc = nullptr, *part_f = nullptr, *idx = nullptr;
  face_idx.assign((size_t)Vt, -1);
  auto run = [&]() {
    FCK(put(tmp, &rest, src_rest, (size_t)V * 3));
    FCK(put(tmp, &fc, faces, (size_t)F * 3));
    FCK(put(tmp, &dst, dst_rest, (size_t)Vt * 3));
    FCK(tmp.alloc_t(&part_d, (size_t)nsplit * Vt));
    FCK(tmp.alloc_t(&part_f, (size_t)nsplit * Vt));
    FCK(tmp.alloc_t(&idx, (size_t)Vt));
    hipLaunchKernelGGL(wrap_nearest_kernel, dim3((unsigned)nvb, (unsigned)nsplit), dim3(WRAP_VB), 0, (hipStream_t)0, (const float*)rest,
                       (const int*)fc, F, (const float*)dst, Vt, (int)tiles_per, part_d, part_f);
    hipLaunchKernelGGL(wrap_combine_kernel, dim3((unsigned)nvb), dim3(256), 0, (hipStream_t)0, (const float*)part_d, (const int*)part_f,
                       (int)nsplit, Vt, idx);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(face_idx.data(), idx, (size_t)Vt * sizeof(int), hipMemcpyDeviceToHost));      // (waits for both launches)
    return (int)FDM_OK;
  };
  const int r = run();
  tmp.release();
  return r;
}

}  // namespace

extern "C" {

int fdm_wrap_coords_host(const float* src_rest, const int* faces, int F, int V, const float* dst_rest, int Vt, const int* face_idx, float* uvh,
                         float* dist) {
  if (!face_idx || !uvh || !dist) return fail(FDM_ERR_ARG, "wrap_coords: null argument");
  FCK(check_meshes("wrap_coords", src_rest, faces, F, V, dst_rest, Vt));
  for (int j = 0; j < Vt; ++j) {
    const int f = face_idx[j];
    if (f < 0 || f >= F) return fail(FDM_ERR_ARG, "wrap_coords: target vertex %d is bound to face %d of %d", j, f, F);
    const D3 a = at(src_rest, faces[3LL * f]), b = at(src_rest, faces[3LL * f + 1]), c = at(src_rest, faces[3LL * f + 2]), q = at(dst_rest, j);
    const D3 e1 = sub(b, a), e2 = sub(c, a), r = sub(q, a), n = cross(e1, e2);
    const double nn = dot(n, n), g11 = dot(e1, e1), g12 = dot(e1, e2), g22 = dot(e2, e2), r1 = dot(e1, r), r2 = dot(e2, r);
    const double det = g11 * g22 - g12 * g12;
    if (!(nn > 0.0) || !(det > 0.0)) return fail(FDM_ERR_ARG, "wrap_coords: target vertex %d is bound to face %d, which has no area", j, f);
    const double len = std::sqrt(nn);
    const D3 nh = {n.x / len, n.y / len, n.z / len};
    uvh[3LL * j] = (float)((g22 * r1 - g12 * r2) / det);
    uvh[3LL * j + 1] = (float)((g11 * r2 - g12 * r1) / det);
    uvh[3LL * j + 2] = (float)dot(r, nh);
    dist[j] = (float)std::sqrt(closest_dist2(q, a, b, c));
  }
  return FDM_OK;
}

int fdm_wrap_create(const float* src_rest, const int* faces, int F, int V, const float* dst_rest, int Vt, const int* face_idx,
                    const float* weights, fdm_wrap** out) {
  if (!out) return fail(FDM_ERR_ARG, "wrap_create: null out");
  FCK(check_meshes("wrap_create", src_rest, faces, F, V, dst_rest, Vt));
  if (weights)
    for (int j = 0; j < Vt; ++j)
      if (!(weights[j] >= 0.f && weights[j] <= 1.f)) return fail(FDM_ERR_ARG, "wrap_create: weight %g of target vertex %d (finite, in [0, 1])", (double)weights[j], j);
  if (face_idx)
    for (int j = 0; j < Vt; ++j)
      if (face_idx[j] < 0 || face_idx[j] >= F) return fail(FDM_ERR_ARG, "wrap_create: target vertex %d is bound to face %d of %d", j, face_idx[j], F);
  if (!face_idx && !fdm_device_ok()) return fail(FDM_ERR_STATE, "wrap_create: no gfx950 device visible for the nearest-face search (there is no CPU fallback; pass face_idx)");
  fdm_wrap* W = new (std::nothrow) fdm_wrap();
  if (!W) return fail(FDM_ERR_STATE, "wrap_create: out of memory");
  W->V = V; W->Vt = Vt; W->weighted = weights != nullptr;
  W->uvh.resize((size_t)Vt * 3); W->dist.resize((size_t)Vt);
  int r = FDM_OK;
  if (face_idx) {
    W->face_idx.assign(face_idx, face_idx + Vt);
  } else {
    r = nearest_on_device(src_rest, faces, F, V, dst_rest, Vt, W->face_idx);
    for (int j = 0; r == FDM_OK && j < Vt; ++j)
      if (W->face_idx[j] < 0 || W->face_idx[j] >= F)
        r = fail(FDM_ERR_ARG, "wrap_create: target vertex %d has no candidate face (no face with area at a finite distance)", j);
  }
  if (r == FDM_OK) r = fdm_wrap_coords_host(src_rest, faces, F, V, dst_rest, Vt, W->face_idx.data(), W->uvh.data(), W->dist.data());
  if (r != FDM_OK) { delete W; return r; }
  // each vertex's face resolved to its three source vertices: the frame loop does not chase two levels
  std::vector<int4> abc((size_t)Vt);
  std::vector<float4> uvhw((size_t)Vt);
  for (int j = 0; j < Vt; ++j) {
    const int* f = faces + 3LL * W->face_idx[j];
    abc[j] = make_int4(f[0], f[1], f[2], 0);
    uvhw[j] = make_float4(W->uvh[3LL * j], W->uvh[3LL * j + 1], W->uvh[3LL * j + 2], weights ? weights[j] : 1.f);
  }
  return handoff_finish(W, out, [&]() {
    FCK(put(W->mem, &W->abc, abc.data(), (size_t)Vt));
    FCK(put(W->mem, &W->uvhw, uvhw.data(), (size_t)Vt));
    FCK(put(W->mem, &W->rest_t, dst_rest, (size_t)Vt * 3));
    return (int)FDM_OK;
  });
}

int fdm_wrap_destroy(fdm_wrap* W) { return handoff_destroy(W); }

int fdm_wrap_binding(const fdm_wrap* W, int* face_idx, float* uvh, float* dist) {
  if (!W) return fail(FDM_ERR_ARG, "wrap_binding: null argument");
  if (face_idx) std::copy(W->face_idx.begin(), W->face_idx.end(), face_idx);
  if (uvh) std::copy(W->uvh.begin(), W->uvh.end(), uvh);
  if (dist) std::copy(W->dist.begin(), W->dist.end(), dist);
  return FDM_OK;
}

int fdm_wrap_forward(fdm_wrap* W, const float* offsets, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows, int flags,
                     float* out, void* stream) {
  if (!W || !offsets || !out) return fail(FDM_ERR_ARG, "wrap_forward: null argument");
  if (flags & ~FDM_WRAP_OFFSETS) return fail(FDM_ERR_ARG, "wrap_forward: unknown flag bits 0x%x", flags & ~FDM_WRAP_OFFSETS);
  if (tmpl_rows != 0 && tmpl_rows != 1 && tmpl_rows != B) return fail(FDM_ERR_ARG, "wrap_forward: tmpl_rows = %d (0, 1 or B = %d)", tmpl_rows, B);
  if (tmpl_rows && !tmpl) return fail(FDM_ERR_ARG, "wrap_forward: tmpl_rows = %d with a null template", tmpl_rows);
  if (B < 1 || L_max < 1) return fail(FDM_ERR_SHAPE, "wrap_forward: B = %d, L_max = %d", B, L_max);
  std::vector<int> hl;
  const ClipLens c = clip_lens(frames, B, L_max, 0.0, 0.0, 0, hl);
  if (c.bad != ClipLens::OK) return fail(FDM_ERR_SHAPE, "wrap_forward: clip %d has %d frames, the batch is %d long", c.clip, c.L, L_max);
  const long long rows = (long long)B * L_max, nvb = ((long long)W->Vt + WRAP_VB - 1) / WRAP_VB;
  if (rows > 0x7fffffffLL || nvb > 65535) return fail(FDM_ERR_SHAPE, "wrap_forward: %lld output rows of %d vertices exceed one launch", rows, W->Vt);
  FCK(handoff_device(*W, "wrap_forward"));
  hipStream_t s = (hipStream_t)stream;
  FCK(handoff_lens(*W, hl, s));
  const int V3 = 3 * W->V, tstride = tmpl_rows == B && B > 1 ? V3 : 0;
  const int mode = (W->weighted ? 1 : 0) | (flags & FDM_WRAP_OFFSETS ? 2 : 0);
  hipLaunchKernelGGL(wrap_follow_kernel, dim3((unsigned)rows, (unsigned)nvb), dim3(WRAP_VB), 0, s, offsets, tmpl_rows ? tmpl : (const float*)nullptr,
                     tstride, (const int*)W->lens, L_max, V3, (const int4*)W->abc, (const float4*)W->uvhw, (const float*)W->rest_t, W->Vt, mode, out);
  HIPCK(hipGetLastError());
  return FDM_OK;
}

}  // extern "C"
