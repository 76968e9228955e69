// Kernels of the mesh hand-off (include/fdm_hip.h, fdm_mesh_*; launched by mesh_out.hip): decoded vertex offsets -> positions at the
// consumer's frame rate and area-weighted vertex normals, planar or interleaved, fp32 or fp16.  DESIGN section 2 item 18 is the definition.
//   mesh_pos_kernel   grid (rows of [B, L_out_max], blocks of MESH_POS_TILE elements of 3V): p = offset + template (one fp32 add), then,
//                     when the rates differ, the time resampling of interp_taps (handoff.hpp) at the clip's own length.  A thread owns
//                     elements 256 apart, so a wavefront's loads and stores are whole lines.  Writes the planar position output
//                     (rounded at the store for fp16; rows at or past L_out[b] as zeros) and / or the fp32 copy the normals are
//                     computed from (`P`: the fp32 planar output itself when there is one, scratch otherwise).
//   mesh_nrm_kernel   one workgroup = MESH_VB consecutive vertices of one output frame, one thread per vertex: walks the vertex's CSR
//                     list of incident faces in ascending face index, recomputes each face normal from P (the frame's positions are 12 V
//                     bytes: the gathers hit the L2) and adds it to a running sum that starts from the first term; normalises; stages
//                     the block's results in LDS so that the stores are contiguous lines whatever the layout (3 or 6 values per vertex).
//                     Workgroup ids are dealt so that the blocks of one frame share id mod 8 (the dispatcher deals consecutive ids to
//                     the 8 XCDs in turn): a frame's gathers then meet in one L2.  That placement is a hint, not a dependency.
// Every value is a function of the clip's own rows: nothing is accumulated across threads, there are no atomics, and neither the
// batch, L_max, L_out_max nor a tile size enters an expression.  Input rows at or past frames[b] are never read.  Call times:
// profiles/mesh_out/README.md (with normals 9-13 % of the byte floor: the gathers bound it; kernel times have not been taken).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fdm_hip.h"
#include "handoff.hpp"

namespace fdm {

constexpr int MESH_POS_TILE = 1024;       // elements of a row per workgroup of mesh_pos_kernel (4 per thread, 256 apart)
constexpr int MESH_VB = 256;              // vertices per workgroup of mesh_nrm_kernel (= threads)

// lens: [B][2] ints = {L, L_out} of each clip.  pos / P: either may be null.  tmpl_stride: 0 (one row for all) or V3.
template <typename PT>
__global__ __launch_bounds__(256) void mesh_pos_kernel(const float* off, const float* tmpl, int tmpl_stride, const int* lens, int L_max,
                                                       int Lo_max, int V3, int resample, PT* pos, float* P) {
  const int row = blockIdx.x;
  int b;
  const bool live = row_live(lens, 2, 1, row, Lo_max, b);
  const int t = row - b * Lo_max;
  int i0 = t, i1 = t;
  float l0 = 1.f, l1 = 0.f;
  if (live && resample) interp_taps(lens[2 * b], lens[2 * b + 1], t, i0, i1, l0, l1);
  const float* x0 = off + ((size_t)b * L_max + i0) * V3;
  const float* x1 = off + ((size_t)b * L_max + i1) * V3;
  const float* tp = tmpl ? tmpl + (size_t)b * tmpl_stride : nullptr;
  const size_t o = (size_t)row * V3;
#pragma unroll
  for (int k = 0; k < MESH_POS_TILE / 256; ++k) {
    const int e = blockIdx.y * MESH_POS_TILE + k * 256 + threadIdx.x;
    if (e >= V3) break;
    float y = 0.f;
    if (live) {
      if (!resample) {
        y = tp ? __fadd_rn(x0[e], tp[e]) : x0[e];
      } else {
        const float p0 = tp ? __fadd_rn(x0[e], tp[e]) : x0[e], p1 = tp ? __fadd_rn(x1[e], tp[e]) : x1[e];
        y = __fadd_rn(__fmul_rn(l0, p0), __fmul_rn(l1, p1));
      }
    }
    if (pos) pos[o + e] = (PT)y;
    if (P && live) P[o + e] = y;
  }
}

// P: fp32 positions [rows][3V] (rows at or past L_out[b] are not read).  out: planar normals [rows][V][3] (inter = 0) or interleaved
// position + normal [rows][V][6] (inter = 1); rows at or past L_out[b] are written as zeros.  nblk = blocks of MESH_VB vertices.
template <typename OT>
__global__ __launch_bounds__(MESH_VB) void mesh_nrm_kernel(const float* P, const int* lens, int Lo_max, int V, const int* faces, const int* adj_off,
                                                           const int* adj, int rows, int nblk, OT* out, int inter) {
  __shared__ float sm[MESH_VB * 6];
  const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
  const int row = (k / nblk) * 8 + xcd, blk = k % nblk;
  if (row >= rows) return;                                  // (uniform over the workgroup)
  int b;
  const bool live = row_live(lens, 2, 1, row, Lo_max, b);
  const int tid = threadIdx.x, v0 = blk * MESH_VB, v = v0 + tid;
  const float* p = P + (size_t)row * V * 3;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  if (live && v < V) {
    const int j0 = adj_off[v], j1 = adj_off[v + 1];
    for (int j = j0; j < j1; ++j) {
      const int* f = faces + (size_t)adj[j] * 3;
      const float *pa = p + (size_t)f[0] * 3, *pb = p + (size_t)f[1] * 3, *pc = p + (size_t)f[2] * 3;
      const float ax = pa[0], ay = pa[1], az = pa[2];
      const float e1x = __fsub_rn(pb[0], ax), e1y = __fsub_rn(pb[1], ay), e1z = __fsub_rn(pb[2], az);
      const float e2x = __fsub_rn(pc[0], ax), e2y = __fsub_rn(pc[1], ay), e2z = __fsub_rn(pc[2], az);
      const float nx = __fsub_rn(__fmul_rn(e1y, e2z), __fmul_rn(e1z, e2y));
      const float ny = __fsub_rn(__fmul_rn(e1z, e2x), __fmul_rn(e1x, e2z));
      const float nz = __fsub_rn(__fmul_rn(e1x, e2y), __fmul_rn(e1y, e2x));
      if (j == j0) { sx = nx; sy = ny; sz = nz; }
      else { sx = __fadd_rn(sx, nx); sy = __fadd_rn(sy, ny); sz = __fadd_rn(sz, nz); }
    }
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(sx, sx), __fmul_rn(sy, sy)), __fmul_rn(sz, sz));
    if (d > 0.f) {
      const float r = sqrtf(d);           // the correctly rounded expansion (__fsqrt_rn is the bare v_sqrt_f32 here: 1 ulp)
      sx = __fdiv_rn(sx, r); sy = __fdiv_rn(sy, r); sz = __fdiv_rn(sz, r);
    } else {
      sx = sy = sz = 0.f;
    }
  }
  const int per = inter ? 6 : 3;
  float* s = sm + tid * per;
  if (inter) {
    const bool rd = live && v < V;
    s[0] = rd ? p[(size_t)v * 3] : 0.f; s[1] = rd ? p[(size_t)v * 3 + 1] : 0.f; s[2] = rd ? p[(size_t)v * 3 + 2] : 0.f;
    s += 3;
  }
  s[0] = sx; s[1] = sy; s[2] = sz;
  __syncthreads();
  const int n = (V - v0 < MESH_VB ? V - v0 : MESH_VB) * per;
  OT* o = out + ((size_t)row * V + v0) * per;
  for (int i = tid; i < n; i += MESH_VB) o[i] = (OT)sm[i];
}

}  // namespace fdm
