// Kernels of the wrap hand-off (include/fdm_hip.h, fdm_wrap_*; launched by wrap_out.hip): a mesh of another topology follows the
// animated face through a surface binding.  DESIGN section 2 item 22 is the definition; the header spells out every operation.
//   wrap_nearest_kernel  grid (blocks of WRAP_VB target vertices, face splits): one target vertex per lane.  The rest triangles of the
//                        split are staged through LDS WRAP_FT at a time -- thread i of the workgroup forms face i's a, b, c, ab, ac, bc
//                        and whether it has area, once -- and every lane scans the tile in ascending face order, so a wave reads one
//                        LDS address at a time (broadcasts).  The region walk is selects over all candidates: no divergence, two
//                        divisions per test.  Writes the split's minimum (dist2, face) per vertex.
//   wrap_combine_kernel  one thread per target vertex: the partial minima in ascending split order under the same `<`, so the lowest
//                        dist2 and then the lowest face index win, whatever the split.
//   wrap_follow_kernel   grid (rows of [B, L_max], blocks of WRAP_VB target vertices), one thread per target vertex: reads its binding
//                        record (two 16-byte loads, coalesced), gathers the three source vertices of the frame from global memory (the
//                        frame's positions are 12 V bytes: the gathers hit the L2, as in mesh_nrm_kernel), forms y, and stages the
//                        block's 3 WRAP_VB floats in LDS so that the row is stored with the 16-byte peel of handoff.hpp.  Rows at or
//                        past frames[b] are written as zeros by the same launch and their input is not read.
// Nothing is accumulated across threads and there are no atomics: a value depends on the clip's own row and the vertex's own record.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fdm_hip.h"
#include "handoff.hpp"

namespace fdm {

constexpr int WRAP_VB = 256;              // target vertices per workgroup (= threads), both kernels
constexpr int WRAP_FT = 256;              // faces per LDS tile of wrap_nearest_kernel (= threads: one face formed per thread)
constexpr int WRAP_SPLIT_TILES = 4;       // fewest tiles a split of the face list scans (each split reads q again and writes a partial)
constexpr int WRAP_FREC = 20;             // floats per staged face: a, b, c, ab, ac, bc, has-area, pad (80 bytes: five 16-byte reads)

__device__ __forceinline__ float wrap_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}
// two rounded products and one rounded subtraction: x y - z w
__device__ __forceinline__ float wrap_pms(float x, float y, float z, float w) { return __fsub_rn(__fmul_rn(x, y), __fmul_rn(z, w)); }

// rest [V][3], faces [F][3], dst [Vt][3].  Split s of `nsplit` scans the tiles [s * tiles_per, (s + 1) * tiles_per) of the face list.
// part_d / part_f: [nsplit][Vt], the split's minimum and its face (-1: no candidate).
__global__ __launch_bounds__(WRAP_VB) void wrap_nearest_kernel(const float* rest, const int* faces, int F, const float* dst, int Vt,
                                                               int tiles_per, float* part_d, int* part_f) {
  __shared__ __attribute__((aligned(16))) float sm[WRAP_FT * WRAP_FREC];
  const int tid = threadIdx.x, j = blockIdx.x * WRAP_VB + tid, split = blockIdx.y;
  const bool mine = j < Vt;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (mine) { qx = dst[3 * (size_t)j]; qy = dst[3 * (size_t)j + 1]; qz = dst[3 * (size_t)j + 2]; }
  float best = __builtin_inff();
  int best_f = -1;
  const int f_begin = min((long long)split * tiles_per * WRAP_FT, (long long)F);
  const int f_end = (int)min(((long long)split + 1) * tiles_per * WRAP_FT, (long long)F);
  for (int f0 = f_begin; f0 < f_end; f0 += WRAP_FT) {
    const int nf = min(WRAP_FT, f_end - f0);
    __syncthreads();                                        // the tile before this one has been read
    if (tid < nf) {
      const int* fv = faces + 3 * (size_t)(f0 + tid);
      const float *pa = rest + 3 * (size_t)fv[0], *pb = rest + 3 * (size_t)fv[1], *pc = rest + 3 * (size_t)fv[2];
      const float ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], cx = pc[0], cy = pc[1], cz = pc[2];
      const float abx = __fsub_rn(bx, ax), aby = __fsub_rn(by, ay), abz = __fsub_rn(bz, az);
      const float acx = __fsub_rn(cx, ax), acy = __fsub_rn(cy, ay), acz = __fsub_rn(cz, az);
      const float nx = wrap_pms(aby, acz, abz, acy), ny = wrap_pms(abz, acx, abx, acz), nz = wrap_pms(abx, acy, aby, acx);
      const float d = wrap_dot(nx, ny, nz, nx, ny, nz);
      float4* r = reinterpret_cast<float4*>(sm + tid * WRAP_FREC);
      r[0] = make_float4(ax, ay, az, bx);
      r[1] = make_float4(by, bz, cx, cy);
      r[2] = make_float4(cz, abx, aby, abz);
      r[3] = make_float4(acx, acy, acz, __fsub_rn(cx, bx));
      r[4] = make_float4(__fsub_rn(cy, by), __fsub_rn(cz, bz), d > 0.f ? 1.f : 0.f, 0.f);
    }
    __syncthreads();
    for (int i = 0; i < nf; ++i) {
      const float4* r = reinterpret_cast<const float4*>(sm + i * WRAP_FREC);
      const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
      const float ax = r0.x, ay = r0.y, az = r0.z, bx = r0.w, by = r1.x, bz = r1.y, cx = r1.z, cy = r1.w, cz = r2.x;
      const float abx = r2.y, aby = r2.z, abz = r2.w, acx = r3.x, acy = r3.y, acz = r3.z, bcx = r3.w, bcy = r4.x, bcz = r4.y;
      if (r4.z == 0.f) continue;                            // (uniform: the face has no area)
      const float apx = __fsub_rn(qx, ax), apy = __fsub_rn(qy, ay), apz = __fsub_rn(qz, az);
      const float bpx = __fsub_rn(qx, bx), bpy = __fsub_rn(qy, by), bpz = __fsub_rn(qz, bz);
      const float cpx = __fsub_rn(qx, cx), cpy = __fsub_rn(qy, cy), cpz = __fsub_rn(qz, cz);
      const float d1 = wrap_dot(abx, aby, abz, apx, apy, apz), d2 = wrap_dot(acx, acy, acz, apx, apy, apz);
      const float d3 = wrap_dot(abx, aby, abz, bpx, bpy, bpz), d4 = wrap_dot(acx, acy, acz, bpx, bpy, bpz);
      const float d5 = wrap_dot(abx, aby, abz, cpx, cpy, cpz), d6 = wrap_dot(acx, acy, acz, cpx, cpy, cpz);
      const float vc = wrap_pms(d1, d4, d3, d2), vb = wrap_pms(d5, d2, d1, d6), va = wrap_pms(d3, d6, d5, d4);
      const float d43 = __fsub_rn(d4, d3), d56 = __fsub_rn(d5, d6);
      const bool rA = d1 <= 0.f && d2 <= 0.f;
      const bool rB = !rA && d3 >= 0.f && d4 <= d3;
      const bool rAB = !rA && !rB && vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
      const bool v01 = rA || rB || rAB;
      const bool rC = !v01 && d6 >= 0.f && d5 <= d6;
      const bool rAC = !v01 && !rC && vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
      const bool v04 = v01 || rC || rAC;
      const bool rBC = !v04 && va <= 0.f && d43 >= 0.f && d56 >= 0.f;
      const bool rIn = !v04 && !rBC;
      const float s = __fadd_rn(__fadd_rn(va, vb), vc);
      const float n1 = rAB ? d1 : (rBC ? d43 : (rIn ? vb : 0.f));
      const float m1 = rAB ? __fsub_rn(d1, d3) : (rBC ? __fadd_rn(d43, d56) : (rIn ? s : 1.f));
      const float n2 = rAC ? d2 : (rIn ? vc : 0.f);
      const float m2 = rAC ? __fsub_rn(d2, d6) : (rIn ? s : 1.f);
      const float t1 = __fdiv_rn(n1, m1), t2 = __fdiv_rn(n2, m2);
      const bool fromB = rB || rBC;
      const float ox = fromB ? bx : (rC ? cx : ax), oy = fromB ? by : (rC ? cy : ay), oz = fromB ? bz : (rC ? cz : az);
      const float ux = rBC ? bcx : abx, uy = rBC ? bcy : aby, uz = rBC ? bcz : abz;
      const float px = __fadd_rn(__fadd_rn(ox, __fmul_rn(t1, ux)), __fmul_rn(t2, acx));
      const float py = __fadd_rn(__fadd_rn(oy, __fmul_rn(t1, uy)), __fmul_rn(t2, acy));
      const float pz = __fadd_rn(__fadd_rn(oz, __fmul_rn(t1, uz)), __fmul_rn(t2, acz));
      const float rx = __fsub_rn(qx, px), ry = __fsub_rn(qy, py), rz = __fsub_rn(qz, pz);
      const float dist2 = wrap_dot(rx, ry, rz, rx, ry, rz);
      if (dist2 < best) { best = dist2; best_f = f0 + i; }
    }
  }
  if (mine) {
    part_d[(size_t)split * Vt + j] = best;
    part_f[(size_t)split * Vt + j] = best_f;
  }
}

// face_idx [Vt]: -1 where no split had a candidate
__global__ __launch_bounds__(256) void wrap_combine_kernel(const float* part_d, const int* part_f, int nsplit, int Vt, int* face_idx) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= Vt) return;
  float best = __builtin_inff();
  int best_f = -1;
  for (int s = 0; s < nsplit; ++s) {
    const float d = part_d[(size_t)s * Vt + j];
    if (d < best) { best = d; best_f = part_f[(size_t)s * Vt + j]; }
  }
  face_idx[j] = best_f;
}

// abc: [Vt] {a, b, c, 0} source vertex indices; uvhw: [Vt] {u, v, h, w}; rest_t [Vt][3].  lens: [B] frames.  tmpl_stride: 0 or 3 V.
// mode: 0 = y; 1 = T + w (y - T); 2 = y - T (offsets, no weights); 3 = w (y - T)
__global__ __launch_bounds__(WRAP_VB) void wrap_follow_kernel(const float* off, const float* tmpl, int tmpl_stride, const int* lens, int L_max,
                                                              int V3, const int4* abc, const float4* uvhw, const float* rest_t, int Vt, int mode,
                                                              float* out) {
  __shared__ float sm[WRAP_VB * 3];
  const int row = blockIdx.x, tid = threadIdx.x, v0 = blockIdx.y * WRAP_VB, j = v0 + tid;
  int b;
  const bool live = row_live(lens, 1, 0, row, L_max, b);
  float yx = 0.f, yy = 0.f, yz = 0.f;
  if (live && j < Vt) {
    const int4 idx = abc[j];
    const float4 k = uvhw[j];
    const float* x = off + (size_t)row * V3;
    const float *xa = x + 3 * (size_t)idx.x, *xb = x + 3 * (size_t)idx.y, *xc = x + 3 * (size_t)idx.z;
    float ax = xa[0], ay = xa[1], az = xa[2], bx = xb[0], by = xb[1], bz = xb[2], cx = xc[0], cy = xc[1], cz = xc[2];
    if (tmpl) {
      const float* tp = tmpl + (size_t)b * tmpl_stride;
      const float *ta = tp + 3 * (size_t)idx.x, *tb = tp + 3 * (size_t)idx.y, *tc = tp + 3 * (size_t)idx.z;
      ax = __fadd_rn(ax, ta[0]); ay = __fadd_rn(ay, ta[1]); az = __fadd_rn(az, ta[2]);
      bx = __fadd_rn(bx, tb[0]); by = __fadd_rn(by, tb[1]); bz = __fadd_rn(bz, tb[2]);
      cx = __fadd_rn(cx, tc[0]); cy = __fadd_rn(cy, tc[1]); cz = __fadd_rn(cz, tc[2]);
    }
    const float e1x = __fsub_rn(bx, ax), e1y = __fsub_rn(by, ay), e1z = __fsub_rn(bz, az);
    const float e2x = __fsub_rn(cx, ax), e2y = __fsub_rn(cy, ay), e2z = __fsub_rn(cz, az);
    float nx = wrap_pms(e1y, e2z, e1z, e2y), ny = wrap_pms(e1z, e2x, e1x, e2z), nz = wrap_pms(e1x, e2y, e1y, e2x);
    const float d = wrap_dot(nx, ny, nz, nx, ny, nz);
    if (d > 0.f) {
      const float r = sqrtf(d);           // the correctly rounded expansion, as in mesh_nrm_kernel
      nx = __fdiv_rn(nx, r); ny = __fdiv_rn(ny, r); nz = __fdiv_rn(nz, r);
    } else {
      nx = ny = nz = 0.f;
    }
    yx = __fadd_rn(__fadd_rn(__fadd_rn(ax, __fmul_rn(k.x, e1x)), __fmul_rn(k.y, e2x)), __fmul_rn(k.z, nx));
    yy = __fadd_rn(__fadd_rn(__fadd_rn(ay, __fmul_rn(k.x, e1y)), __fmul_rn(k.y, e2y)), __fmul_rn(k.z, ny));
    yz = __fadd_rn(__fadd_rn(__fadd_rn(az, __fmul_rn(k.x, e1z)), __fmul_rn(k.y, e2z)), __fmul_rn(k.z, nz));
    if (mode) {
      const float tx = rest_t[3 * (size_t)j], ty = rest_t[3 * (size_t)j + 1], tz = rest_t[3 * (size_t)j + 2];
      yx = __fsub_rn(yx, tx); yy = __fsub_rn(yy, ty); yz = __fsub_rn(yz, tz);
      if (mode & 1) { yx = __fmul_rn(k.w, yx); yy = __fmul_rn(k.w, yy); yz = __fmul_rn(k.w, yz); }
      if (mode == 1) { yx = __fadd_rn(tx, yx); yy = __fadd_rn(ty, yy); yz = __fadd_rn(tz, yz); }
    }
  }
  sm[3 * tid] = yx; sm[3 * tid + 1] = yy; sm[3 * tid + 2] = yz;
  __syncthreads();
  const int n = 3 * min(WRAP_VB, Vt - v0);
  float* dst = out + (size_t)row * 3 * Vt + 3 * (size_t)v0;
  peel_walk<WRAP_VB, 64>(peel_of(dst, n), n, tid, PeelStore{dst, sm});
}

}  // namespace fdm
