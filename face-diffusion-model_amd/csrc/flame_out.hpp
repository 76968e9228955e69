// Kernels of the parametric-head hand-off (include/fdm_hip.h, fdm_flame_*; launched by flame_out.hip): shape / expression coefficients
// and axis-angle joint rotations -> posed vertices, linear blend skinning of the SMPL / FLAME family.  DESIGN section 2 item 20 is the
// definition.
//   flame_pose_kernel   one lane per row of [B * L_max] (64 per workgroup), fp32, every operation rounded on its own: the joints from the
//                       folded regressor (JT + JD coef), a Rodrigues rotation per joint, the kinematic chain made relative to the rest
//                       joints, the pose feature.  The chain reads its parent by a run-time index, so the joints and the chain live in LDS
//                       columns (element-major: lane l reads bank l), never in indexed registers: no scratch.  It also writes the row's
//                       blend coefficients (expression, then pose feature) transposed per tile of ROW_TILE rows, [tile][term][ROW_TILE],
//                       which is what flame_skin_kernel reads.
//   flame_shape_kernel  v_id = v_template + sum_k shape_k D_k per shape row, 16 bytes per lane, fused multiply-adds, k ascending.
//   flame_skin_kernel   grid (tiles of ROW_TILE rows, chunks of ROW_CHUNK elements of 3V), ONE wavefront per workgroup.  The tile's
//                       coefficients, transforms and the chunk's skinning weights are staged in LDS (wave-uniform reads are broadcasts).
//                       Each lane holds ROW_TILE x 12 accumulators (16-byte pieces lane + 64 q of the chunk) and walks the terms in
//                       ascending order: one 16-byte load of D per piece (rows padded with zeros to whole chunks, so aligned and in
//                       bounds; the slab of a chunk is shared by every tile of the chunk: workgroup ids run over the tiles first, so it
//                       is served by the L2), ROW_TILE x 12 fused multiply-adds.  Then per row: the blended chunk goes to a 3 KB LDS row;
//                       `extra` is added there through the 16-byte peel of handoff.hpp (a row starts on a 4-byte boundary only); the lanes
//                       change to one vertex each (lane + 64 i: stride-3 reads, conflict-free), blend the transforms in ascending joint
//                       order, apply them and write the vertex back; the row leaves through the same peel as 16-byte stores.  Plain
//                       VALU: the fp32 MFMA rate on gfx950 is the vector rate, and the order of the sum is part of the rule.
//   flame_lmk_kernel    landmarks from the posed vertices, one lane per (row, landmark).
// A frame's values are a function of its own row and the model: no atomics, and neither the batch, L_max, the row's slot in its tile
// nor the workgroup enters an expression.  Input rows at or past frames[b] are never read.  Resource use: profiles/flame_out/resources.txt.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fdm_hip.h"
#include "flame_math.hpp"
#include "handoff.hpp"

namespace fdm {

// (flame_skin_kernel's geometry is handoff.hpp's: ROW_CHUNK elements of 3V = 256 whole vertices and ROW_TILE rows per workgroup)
constexpr int FLAME_NBMAX = 512;
constexpr int FLAME_NLMAX = 256;

// shape [shape_rows][NS], expr [rows][NE], pose [rows][3 J]; lens [B]; JT [3 J], JD [NB][3 J], parents [J].
// xf [tiles * ROW_TILE][J][12] (row-major 3 x 4 per joint), pf [rows][9 (J - 1)], cf [tiles][NE + 9 (J - 1)][ROW_TILE].  Dead rows: zeros.
__global__ __launch_bounds__(64) void flame_pose_kernel(const float* shape, int shape_rows, int NS, const float* expr, int NE, const float* pose,
                                                       const int* lens, int L_max, int rows, int J, int expr_at, const float* JT, const float* JD,
                                                       const int* parents, float* xf, float* pf, float* cf) {
  __shared__ float sJ[3 * FLAME_JMAX][64];                  // the row's joints
  __shared__ float sG[12 * FLAME_JMAX][64];                 // the row's chain (world transforms)
  const int tid = threadIdx.x;
  const int row = blockIdx.x * 64 + tid;                    // < tiles * ROW_TILE rounded up to 64: guarded below
  const int rows_pad = (rows + ROW_TILE - 1) / ROW_TILE * ROW_TILE;
  if (row >= rows_pad) return;
  const int J3 = 3 * J, P = 9 * (J - 1), NT = NE + P;
  float* ox = xf + (size_t)row * J * 12;
  float* oc = cf + ((size_t)(row / ROW_TILE) * NT) * ROW_TILE + (row % ROW_TILE);
  int b;
  if (!row_live(lens, 1, 0, row, L_max, rows, b)) {
    for (int i = 0; i < J * 12; ++i) ox[i] = 0.f;
    for (int i = 0; i < NT; ++i) oc[(size_t)i * ROW_TILE] = 0.f;
    if (row < rows) for (int i = 0; i < P; ++i) pf[(size_t)row * P + i] = 0.f;
    return;
  }
  float jf[3 * FLAME_JMAX];
  flame_joints(jf, JT, JD, J3, shape + (size_t)(shape_rows == 1 ? 0 : b) * NS, NS, expr + (size_t)row * NE, NE, expr_at, oc);
#pragma unroll
  for (int i = 0; i < 3 * FLAME_JMAX; ++i) if (i < J3) sJ[i][tid] = jf[i];
  const float* pr = pose + (size_t)row * J3;
  for (int j = 0; j < J; ++j) {
    float R[9];
    flame_rodrigues(pr[3 * j], pr[3 * j + 1], pr[3 * j + 2], R);
    if (j >= 1) {
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        const float f = __fsub_rn(R[e], e % 4 == 0 ? 1.f : 0.f);
        pf[(size_t)row * P + 9 * (j - 1) + e] = f;
        oc[(size_t)(NE + 9 * (j - 1) + e) * ROW_TILE] = f;
      }
    }
    const float jx = sJ[3 * j][tid], jy = sJ[3 * j + 1][tid], jz = sJ[3 * j + 2][tid];
    float G[12];                                            // row-major 3 x 4: the joint's world transform
    if (j == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) { G[4 * a] = R[3 * a]; G[4 * a + 1] = R[3 * a + 1]; G[4 * a + 2] = R[3 * a + 2]; }
      G[3] = jx; G[7] = jy; G[11] = jz;
    } else {
      const int p = parents[j];
      float Gp[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) Gp[e] = sG[12 * p + e][tid];
      const float dx = __fsub_rn(jx, sJ[3 * p][tid]), dy = __fsub_rn(jy, sJ[3 * p + 1][tid]), dz = __fsub_rn(jz, sJ[3 * p + 2][tid]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) G[4 * a + c] = flame_dot3(Gp[4 * a], Gp[4 * a + 1], Gp[4 * a + 2], R[c], R[3 + c], R[6 + c]);
        G[4 * a + 3] = __fadd_rn(flame_dot3(Gp[4 * a], Gp[4 * a + 1], Gp[4 * a + 2], dx, dy, dz), Gp[4 * a + 3]);
      }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) sG[12 * j + e][tid] = G[e];
    // relative to the rest pose: t -= R_chain Jf_j
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      ox[12 * j + 4 * a] = G[4 * a]; ox[12 * j + 4 * a + 1] = G[4 * a + 1]; ox[12 * j + 4 * a + 2] = G[4 * a + 2];
      ox[12 * j + 4 * a + 3] = __fsub_rn(G[4 * a + 3], flame_dot3(G[4 * a], G[4 * a + 1], G[4 * a + 2], jx, jy, jz));
    }
  }
}

// vid [shape_rows][ld] = T [ld] + sum_k shape [row][k] D [k][ld]; ld is a multiple of 4, T and D are zero behind 3V
__global__ __launch_bounds__(256) void flame_shape_kernel(const float* T, const float* D, int ld, const float* shape, int NS, float* vid) {
  const int i4 = blockIdx.x * 256 + threadIdx.x;
  if (4 * i4 >= ld) return;
  const float* sh = shape + (size_t)blockIdx.y * NS;
  float4 v = *reinterpret_cast<const float4*>(T + 4 * i4);
  for (int k = 0; k < NS; ++k) {
    const float c = sh[k];
    const float4 d = *reinterpret_cast<const float4*>(D + (size_t)k * ld + 4 * i4);
    v.x = __builtin_fmaf(c, d.x, v.x); v.y = __builtin_fmaf(c, d.y, v.y); v.z = __builtin_fmaf(c, d.z, v.z); v.w = __builtin_fmaf(c, d.w, v.w);
  }
  *reinterpret_cast<float4*>(vid + (size_t)blockIdx.y * ld + 4 * i4) = v;
}

struct FlameSkinArgs {
  const float* vid; int shape_rows;       // [shape_rows][ld]
  const float* D; int ld;                 // [NB + 9 (J - 1)][ld]
  int row_expr, NE, row_pose, P;          // the terms: D rows row_expr + k (k < NE), then row_pose + p (p < P)
  const float* cf;                        // [tiles][NE + P][ROW_TILE]
  const float* xf;                        // [tiles * ROW_TILE][J][12]
  const float* wts; int J;                // [V][J]
  const float* transl;                    // [rows][3] or null
  const float* extra;                     // [rows][V3] or null
  const int* lens; int L_max, rows, V3;
  float* out;                             // [rows][V3]
};

// dynamic LDS (floats): cf (NE + P) * ROW_TILE | xf ROW_TILE * J * 12 | weights J * 256 | one row ROW_CHUNK
__host__ __device__ inline size_t flame_skin_lds(int NT, int J) { return ((size_t)NT * ROW_TILE + (size_t)ROW_TILE * J * 12 + (size_t)J * 256 + ROW_CHUNK) * sizeof(float); }

__global__ __launch_bounds__(64) void flame_skin_kernel(const FlameSkinArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NT = a.NE + a.P, J = a.J;
  float* s_cf = reinterpret_cast<float*>(smem);             // [NT][ROW_TILE]
  float* s_xf = s_cf + NT * ROW_TILE;                       // [ROW_TILE][J][12]
  float* s_w = s_xf + ROW_TILE * J * 12;                    // [J][256]
  float* s_v = s_w + J * 256;                               // [ROW_CHUNK]
  const int lane = threadIdx.x;
  const int row0 = blockIdx.x * ROW_TILE, c0 = blockIdx.y * ROW_CHUNK;
  const int n = min(ROW_CHUNK, a.V3 - c0);                // live elements of the chunk: a multiple of 3
  int clip[ROW_TILE];
  bool live[ROW_TILE], any = false;
#pragma unroll
  for (int r = 0; r < ROW_TILE; ++r) {
    const int row = row0 + r;
    live[r] = row_live(a.lens, 1, 0, row, a.L_max, a.rows, clip[r]);
    any |= live[r];
  }
  {
    const float4* g = reinterpret_cast<const float4*>(a.cf + (size_t)blockIdx.x * NT * ROW_TILE);
    for (int i = lane; i < NT * ROW_TILE / 4; i += 64) reinterpret_cast<float4*>(s_cf)[i] = g[i];
    const float4* x = reinterpret_cast<const float4*>(a.xf + (size_t)row0 * J * 12);
    for (int i = lane; i < ROW_TILE * J * 3; i += 64) reinterpret_cast<float4*>(s_xf)[i] = x[i];
    const int nv = n / 3, v0 = c0 / 3;
    for (int i = lane; i < nv * J; i += 64) s_w[(i % J) * 256 + i / J] = a.wts[(size_t)v0 * J + i];
  }
  __syncthreads();
  float4 acc[ROW_TILE][ROW_Q];
  if (any) {                                                // (uniform over the workgroup)
#pragma unroll
    for (int r = 0; r < ROW_TILE; ++r) {
      const float* v = a.vid + (size_t)(a.shape_rows == 1 ? 0 : clip[r]) * a.ld + c0;
#pragma unroll
      for (int q = 0; q < ROW_Q; ++q) acc[r][q] = *reinterpret_cast<const float4*>(v + 4 * (lane + 64 * q));
    }
    for (int t = 0; t < NT; ++t) {
      const float* dk = a.D + (size_t)(t < a.NE ? a.row_expr + t : a.row_pose + (t - a.NE)) * a.ld + c0;
      float4 d[ROW_Q];
#pragma unroll
      for (int q = 0; q < ROW_Q; ++q) d[q] = *reinterpret_cast<const float4*>(dk + 4 * (lane + 64 * q));
      const float4 ca = *reinterpret_cast<const float4*>(s_cf + t * ROW_TILE), cb = *reinterpret_cast<const float4*>(s_cf + t * ROW_TILE + 4);
      const float c[ROW_TILE] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
      for (int r = 0; r < ROW_TILE; ++r)
#pragma unroll
        for (int q = 0; q < ROW_Q; ++q) {
          acc[r][q].x = __builtin_fmaf(c[r], d[q].x, acc[r][q].x); acc[r][q].y = __builtin_fmaf(c[r], d[q].y, acc[r][q].y);
          acc[r][q].z = __builtin_fmaf(c[r], d[q].z, acc[r][q].z); acc[r][q].w = __builtin_fmaf(c[r], d[q].w, acc[r][q].w);
        }
    }
  }
#pragma unroll
  for (int r = 0; r < ROW_TILE; ++r) {
    const int row = row0 + r;
    if (row >= a.rows) break;                               // (uniform)
    float* dst = a.out + (size_t)row * a.V3 + c0;
    const Peel pd = peel_of(dst, n);                        // the row's own 16-byte boundary
    if (live[r]) {
#pragma unroll
      for (int q = 0; q < ROW_Q; ++q) *reinterpret_cast<float4*>(s_v + 4 * (lane + 64 * q)) = acc[r][q];
      __syncthreads();
      if (a.extra) {                                        // `extra` rows are 4-byte aligned like the output's: a peel of their own
        const float* src = a.extra + (size_t)row * a.V3 + c0;
        peel_walk<64, 32>(peel_of(src, n), n, lane, PeelAdd{src, s_v});
        __syncthreads();
      }
      const float* X = s_xf + r * J * 12;
      float tx = 0.f, ty = 0.f, tz = 0.f;
      if (a.transl) { tx = a.transl[(size_t)row * 3]; ty = a.transl[(size_t)row * 3 + 1]; tz = a.transl[(size_t)row * 3 + 2]; }
      for (int i = 0; i < 4; ++i) {
        const int vl = lane + 64 * i;
        if (3 * vl >= n) break;
        const float vx = s_v[3 * vl], vy = s_v[3 * vl + 1], vz = s_v[3 * vl + 2];
        float T[12];
        const float w0 = s_w[vl];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = __fmul_rn(w0, X[e]);
        for (int j = 1; j < J; ++j) {
          const float w = s_w[j * 256 + vl];
#pragma unroll
          for (int e = 0; e < 12; ++e) T[e] = __builtin_fmaf(w, X[12 * j + e], T[e]);
        }
        float o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
          o[c] = __fadd_rn(__builtin_fmaf(T[4 * c + 2], vz, __builtin_fmaf(T[4 * c + 1], vy, __fmul_rn(T[4 * c], vx))), T[4 * c + 3]);
        if (a.transl) { o[0] = __fadd_rn(o[0], tx); o[1] = __fadd_rn(o[1], ty); o[2] = __fadd_rn(o[2], tz); }
        s_v[3 * vl] = o[0]; s_v[3 * vl + 1] = o[1]; s_v[3 * vl + 2] = o[2];
      }
    } else {
      for (int i = lane; i < ROW_CHUNK; i += 64) s_v[i] = 0.f;
    }
    __syncthreads();
    peel_walk<64, 32>(pd, n, lane, PeelStore{dst, s_v});
    __syncthreads();
  }
}

// lmk [rows][NL][3] = sum_c bary_c out[vertex_c]: fma(b2, o2, fma(b1, o1, b0 * o0)); dead rows: zeros
__global__ __launch_bounds__(256) void flame_lmk_kernel(const float* out, const int* lens, int L_max, int rows, int V3, const int* lv, const float* lb,
                                                        int NL, float* lmk) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)rows * NL) return;
  const int row = (int)(i / NL), l = (int)(i - (long long)row * NL);
  float* o = lmk + (size_t)i * 3;
  int b;
  if (!row_live(lens, 1, 0, row, L_max, b)) { o[0] = o[1] = o[2] = 0.f; return; }
  const float* p = out + (size_t)row * V3;
  const float* p0 = p + 3 * (size_t)lv[3 * l];
  const float* p1 = p + 3 * (size_t)lv[3 * l + 1];
  const float* p2 = p + 3 * (size_t)lv[3 * l + 2];
  const float b0 = lb[3 * l], b1 = lb[3 * l + 1], b2 = lb[3 * l + 2];
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = __builtin_fmaf(b2, p2[c], __builtin_fmaf(b1, p1[c], __fmul_rn(b0, p0[c])));
}

}  // namespace fdm
