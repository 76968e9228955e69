// Kernels of the parametric-head fit (include/fdm_hip.h, fdm_flame_fit_*; launched by flame_fit.hip): target vertices -> expression
// coefficients, the axis-angle of a chosen set of joints and a translation, by a fixed number of damped Gauss-Newton steps.  DESIGN
// section 2 item 26 is the definition; the forward map is item 20's, through flame_out.hpp's own kernels (flame_pose_kernel writes the
// transforms and blend coefficients of the current parameters at every step, so the residual is the forward's bit for bit).
//   flame_fit_init_kernel    theta = (0, pose0, 0) for live rows, zeros for dead rows; status = 0.
//   flame_fit_deriv_kernel   one lane per row, the chain in LDS columns as flame_pose_kernel (same joints and rotations: flame_joints,
//                            flame_rodrigues).  Per free joint component the derivative of every joint's relative transform (dX), per
//                            expression column the derivative of the transforms' translation parts (dE).  Every operation rounded.
//   flame_fit_normal_kernel  grid (tiles of ROW_TILE rows, chunks of 256 vertices), 256 threads.  The blended vertex of all ROW_TILE rows
//                            is accumulated once per chunk (one load of the D slab per term, ROW_TILE x 3 fused multiply-adds per thread:
//                            flame_skin_kernel's sum, same bits); then per row and per sub-block of 32 vertices the 96 x (P + 1) block
//                            [J | r] is formed in LDS and every thread accumulates up to three 4 x 4 tiles of the upper triangle of
//                            [J r]^T M [J r] over the elements in ascending order.  One packed partial per (row, chunk).
//   flame_fit_reduce_kernel  sums the chunks' partials in ascending chunk order (rounded adds).  No atomics anywhere.
//   flame_fit_solve_kernel   one workgroup per row: the damped matrix in LDS, right-looking Cholesky, forward and back substitution,
//                            theta += delta.  A pivot that is not > pivot_tol x its damped diagonal sets status[row] and leaves theta.
//   flame_fit_rms_kernel     one workgroup per row: sqrt(sum m |verts - target|^2 / sum m), a fixed tree per chunk, chunks ascending.
// A frame's values are a function of its own row and the model.  Rows at or past frames[b] are never read.  Resource use:
// profiles/flame_fit/resources.txt.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fdm_hip.h"
#include "flame_math.hpp"

namespace fdm {

constexpr int FIT_PMAX = 128;             // free parameters
constexpr int FIT_SUB = 32;               // vertices per sub-block of the normal-equations kernel
constexpr int FIT_LDJ = 3 * FIT_SUB + 1;  // LDS stride of a column of the sub-block (odd: lanes on different columns hit different banks)
constexpr float FIT_PIVOT_TOL = 0x1p-18f;   // the default of the setting "pivot_tol"

struct FitDesc {                          // the free set of one fit object
  int n_expr, n_free, transl, P;          // P = n_expr + 3 n_free + 3 transl
  int free_j[FLAME_JMAX];
};

// theta0: expr [rows][n_expr] = 0; pose [rows][3 J] = pose0 (or 0), dead rows 0; tr [rows][3] = 0; status [rows] = 0
__global__ __launch_bounds__(256) void flame_fit_init_kernel(const float* pose0, const int* lens, int L_max, int rows, int n_expr, int J3, float* expr,
                                                            float* pose, float* tr, int* status) {
  const int row = blockIdx.x;
  int b;
  const bool live = row_live(lens, 1, 0, row, L_max, b);
  for (int i = threadIdx.x; i < n_expr; i += 256) expr[(size_t)row * n_expr + i] = 0.f;
  for (int i = threadIdx.x; i < J3; i += 256) pose[(size_t)row * J3 + i] = live && pose0 ? pose0[(size_t)row * J3 + i] : 0.f;
  if (threadIdx.x < 3) tr[(size_t)row * 3 + threadIdx.x] = 0.f;
  if (threadIdx.x == 0) status[row] = 0;
}

// d R / d r_c (c = 0..2) of R = I + a K + b K K with K = hat(r), t2 = |r|^2, a = sin / angle, b = (1 - cos) / t2:
//   dR_c[i][j] = ((a hat(e_c)[i][j] + b S_c[i][j]) + (a1 r_c) K[i][j]) + (b1 r_c) KK[i][j],  S_c = e_c r^T + r e_c^T - 2 r_c I,
//   KK = r r^T - t2 I, a1 = (cos - a) / t2, b1 = (a - 2 b) / t2.  Small-angle branch t2 < 1e-2: the series in t2 below.
__device__ __forceinline__ void flame_drodrigues(float rx, float ry, float rz, float (&dR)[3][9]) {
  const float r[3] = {rx, ry, rz};
  const float t2 = __fadd_rn(__fadd_rn(__fmul_rn(rx, rx), __fmul_rn(ry, ry)), __fmul_rn(rz, rz));
  float a, b, a1, b1;
  if (t2 < 1e-2f) {
    a = __fadd_rn(1.f, __fmul_rn(t2, __fadd_rn(-1.f / 6.f, __fmul_rn(t2, 1.f / 120.f))));
    b = __fadd_rn(0.5f, __fmul_rn(t2, __fadd_rn(-1.f / 24.f, __fmul_rn(t2, 1.f / 720.f))));
    a1 = __fadd_rn(-1.f / 3.f, __fmul_rn(t2, __fadd_rn(1.f / 30.f, __fmul_rn(t2, -1.f / 840.f))));
    b1 = __fadd_rn(-1.f / 12.f, __fmul_rn(t2, __fadd_rn(1.f / 180.f, __fmul_rn(t2, -1.f / 6720.f))));
  } else {
    const float th = __fsqrt_rn(t2);
    const float s = sinf(th), c = cosf(th);
    a = __fdiv_rn(s, th);
    b = __fdiv_rn(__fsub_rn(1.f, c), t2);
    a1 = __fdiv_rn(__fsub_rn(c, a), t2);
    b1 = __fdiv_rn(__fsub_rn(a, __fmul_rn(2.f, b)), t2);
  }
  const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float ar = __fmul_rn(a1, r[c]), br = __fmul_rn(b1, r[c]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        // hat(e_c)[i][j]: +1 at (c+2, c+1), -1 at (c+1, c+2) (indices mod 3)
        const float h = (i == (c + 2) % 3 && j == (c + 1) % 3) ? 1.f : ((i == (c + 1) % 3 && j == (c + 2) % 3) ? -1.f : 0.f);
        float S = 0.f;
        if (i == c) S = __fadd_rn(S, r[j]);
        if (j == c) S = __fadd_rn(S, r[i]);
        if (i == j) S = __fsub_rn(S, __fmul_rn(2.f, r[c]));
        const float kk = __fsub_rn(__fmul_rn(r[i], r[j]), i == j ? t2 : 0.f);
        dR[c][3 * i + j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, h), __fmul_rn(b, S)), __fmul_rn(ar, K[3 * i + j])), __fmul_rn(br, kk));
      }
  }
}

// xf [tiles * ROW_TILE][J][12] of flame_pose_kernel at the same parameters.  dX [rows][3 n_free][J][12]: d A_j / d pose[free_j[f]][c] at
// q = 3 f + c; dE [rows][n_expr][J][3]: d A_j.t / d expr_k.  Dead rows are not written (and not read later).
//   pose column (f, c), joints ascending: dG_0 = [dR_c if f is joint 0 else 0 | 0]; for j >= 1 with p = parents[j], d = Jf_j - Jf_p:
//     dG_j.R = dG_p.R R_j, plus G_p.R dR_c when j is the free joint (then dG_p is zero and the first term is left out);
//     dG_j.t = dG_p.R d + dG_p.t;  dA_j = [dG_j.R | dG_j.t - dG_j.R Jf_j].  3-term sums as flame_dot3.
//   expression column k with e = JD[expr_at + k]: h_0 = e_0; h_j = G_p.R (e_j - e_p) + h_p; dE_j = h_j - G_j.R e_j.
__global__ __launch_bounds__(64) void flame_fit_deriv_kernel(const float* shape, int shape_rows, int NS, const float* expr, const float* pose,
                                                            const int* lens, int L_max, int rows, int J, int expr_at, const float* JT,
                                                            const float* JD, const int* parents, const float* xf, const FitDesc fd, float* dX,
                                                            float* dE) {
  __shared__ float sJ[3 * FLAME_JMAX][64];                  // the row's joints
  __shared__ float sR[9 * FLAME_JMAX][64];                  // the joints' own rotations
  __shared__ float sD[12 * FLAME_JMAX][64];                 // the chain of the column in flight
  const int tid = threadIdx.x;
  const int row = blockIdx.x * 64 + tid;
  int b;
  if (!row_live(lens, 1, 0, row, L_max, rows, b)) return;
  const int J3 = 3 * J;
  float jf[3 * FLAME_JMAX];
  flame_joints(jf, JT, JD, J3, shape + (size_t)(shape_rows == 1 ? 0 : b) * NS, NS, expr + (size_t)row * fd.n_expr, fd.n_expr, expr_at, nullptr);
#pragma unroll
  for (int i = 0; i < 3 * FLAME_JMAX; ++i) if (i < J3) sJ[i][tid] = jf[i];
  const float* pr = pose + (size_t)row * J3;
  for (int j = 0; j < J; ++j) {
    float R[9];
    flame_rodrigues(pr[3 * j], pr[3 * j + 1], pr[3 * j + 2], R);
#pragma unroll
    for (int e = 0; e < 9; ++e) sR[9 * j + e][tid] = R[e];
  }
  const float* X = xf + (size_t)row * J * 12;               // G_j.R = A_j.R
  for (int f = 0; f < fd.n_free; ++f) {
    const int jfree = fd.free_j[f];
    float dR[3][9];
    flame_drodrigues(pr[3 * jfree], pr[3 * jfree + 1], pr[3 * jfree + 2], dR);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = dX + (((size_t)row * 3 * fd.n_free + 3 * f + c) * J) * 12;
      for (int j = 0; j < J; ++j) {
        float G[12];
        if (j == 0) {
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            G[4 * a] = jfree == 0 ? dR[c][3 * a] : 0.f; G[4 * a + 1] = jfree == 0 ? dR[c][3 * a + 1] : 0.f;
            G[4 * a + 2] = jfree == 0 ? dR[c][3 * a + 2] : 0.f; G[4 * a + 3] = 0.f;
          }
        } else {
          const int p = parents[j];
          float Gp[12];
#pragma unroll
          for (int e = 0; e < 12; ++e) Gp[e] = sD[12 * p + e][tid];
          const float dx = __fsub_rn(sJ[3 * j][tid], sJ[3 * p][tid]), dy = __fsub_rn(sJ[3 * j + 1][tid], sJ[3 * p + 1][tid]),
                      dz = __fsub_rn(sJ[3 * j + 2][tid], sJ[3 * p + 2][tid]);
          if (j == jfree) {
            const float* Xp = X + 12 * p;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
              for (int e = 0; e < 3; ++e) G[4 * a + e] = flame_dot3(Xp[4 * a], Xp[4 * a + 1], Xp[4 * a + 2], dR[c][e], dR[c][3 + e], dR[c][6 + e]);
          } else {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
              for (int e = 0; e < 3; ++e)
                G[4 * a + e] = flame_dot3(Gp[4 * a], Gp[4 * a + 1], Gp[4 * a + 2], sR[9 * j + e][tid], sR[9 * j + 3 + e][tid], sR[9 * j + 6 + e][tid]);
          }
#pragma unroll
          for (int a = 0; a < 3; ++a) G[4 * a + 3] = __fadd_rn(flame_dot3(Gp[4 * a], Gp[4 * a + 1], Gp[4 * a + 2], dx, dy, dz), Gp[4 * a + 3]);
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) sD[12 * j + e][tid] = G[e];
        const float jx = sJ[3 * j][tid], jy = sJ[3 * j + 1][tid], jz = sJ[3 * j + 2][tid];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          o[12 * j + 4 * a] = G[4 * a]; o[12 * j + 4 * a + 1] = G[4 * a + 1]; o[12 * j + 4 * a + 2] = G[4 * a + 2];
          o[12 * j + 4 * a + 3] = __fsub_rn(G[4 * a + 3], flame_dot3(G[4 * a], G[4 * a + 1], G[4 * a + 2], jx, jy, jz));
        }
      }
    }
  }
  for (int k = 0; k < fd.n_expr; ++k) {
    const float* e = JD + (size_t)(expr_at + k) * J3;
    float* o = dE + (((size_t)row * fd.n_expr + k) * J) * 3;
    for (int j = 0; j < J; ++j) {
      float h[3];
      const float ex = e[3 * j], ey = e[3 * j + 1], ez = e[3 * j + 2];
      if (j == 0) {
        h[0] = ex; h[1] = ey; h[2] = ez;
      } else {
        const int p = parents[j];
        const float* Xp = X + 12 * p;
        const float dx = __fsub_rn(ex, e[3 * p]), dy = __fsub_rn(ey, e[3 * p + 1]), dz = __fsub_rn(ez, e[3 * p + 2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) h[a] = __fadd_rn(flame_dot3(Xp[4 * a], Xp[4 * a + 1], Xp[4 * a + 2], dx, dy, dz), sD[3 * p + a][tid]);
      }
      const float* Xj = X + 12 * j;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sD[3 * j + a][tid] = h[a];
        o[3 * j + a] = __fsub_rn(h[a], flame_dot3(Xj[4 * a], Xj[4 * a + 1], Xj[4 * a + 2], ex, ey, ez));
      }
    }
  }
}

struct FlameFitArgs {
  const float* vid; int shape_rows;       // [shape_rows][ld]
  const float* D; int ld;                 // [NB + 9 (J - 1)][ld]
  int row_expr, row_pose, PF;             // the blend's terms: D rows row_expr + k (k < n_expr), then row_pose + p (p < PF = 9 (J - 1))
  const float* cf;                        // [tiles][n_expr + PF][ROW_TILE]
  const float* xf;                        // [tiles * ROW_TILE][J][12]
  const float* dX;                        // [rows][3 n_free][J][12]
  const float* dE;                        // [rows][n_expr][J][3]
  const float* wts; int J;                // [V][J]
  const float* vw;                        // [V] vertex weights or null
  const float* tr;                        // [rows][3] the translation (read when fd.transl)
  const float* target;                    // [rows][V3]
  const int* lens; int L_max, rows, V3, chunks;
  FitDesc fd;
  float* part;                            // [rows][chunks][NP], NP = (P + 1)(P + 2) / 2: the upper triangle of [J r]^T M [J r], row-major packed
};

__host__ __device__ inline int fit_np(int P) { return (P + 1) * (P + 2) / 2; }
__host__ __device__ inline int fit_idx(int P, int a, int b) { return a * (2 * (P + 1) - a + 1) / 2 + (b - a); }      // a <= b <= P
// dynamic LDS (floats): cf NT * ROW_TILE | xf ROW_TILE * J * 12 | weights J * 256 | v ROW_TILE * ROW_CHUNK | dX 3 n_free * J * 12 |
// dE n_expr * J * 3 | block 4 ceil((P + 1) / 4) * FIT_LDJ | m 3 FIT_SUB
__host__ __device__ inline size_t flame_fit_lds(int n_expr, int n_free, int P, int J) {
  const int NT = n_expr + 9 * (J - 1), nb = (P + 1 + 3) / 4;
  return ((size_t)NT * ROW_TILE + (size_t)ROW_TILE * J * 12 + (size_t)J * 256 + (size_t)ROW_TILE * ROW_CHUNK + (size_t)3 * n_free * J * 12 +
          (size_t)n_expr * J * 3 + (size_t)4 * nb * FIT_LDJ + 3 * FIT_SUB) * sizeof(float);
}

__global__ __launch_bounds__(256) void flame_fit_normal_kernel(const FlameFitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const FitDesc& fd = a.fd;
  const int J = a.J, NE = fd.n_expr, NT = NE + a.PF, P = fd.P, NQ = 3 * fd.n_free, nb = (P + 1 + 3) / 4, ntile = nb * (nb + 1) / 2;
  float* s_cf = reinterpret_cast<float*>(smem);             // [NT][ROW_TILE]
  float* s_xf = s_cf + NT * ROW_TILE;                       // [ROW_TILE][J][12]
  float* s_w = s_xf + ROW_TILE * J * 12;                    // [J][256]
  float* s_v = s_w + J * 256;                               // [ROW_TILE][ROW_CHUNK]
  float* s_dx = s_v + ROW_TILE * ROW_CHUNK;                 // [NQ][J][12]
  float* s_de = s_dx + NQ * J * 12;                         // [NE][J][3]
  float* s_j = s_de + NE * J * 3;                           // [4 nb][FIT_LDJ]
  float* s_m = s_j + 4 * nb * FIT_LDJ;                      // [3 FIT_SUB]
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * ROW_TILE, chunk = blockIdx.y, c0 = chunk * ROW_CHUNK;
  const int n = min(ROW_CHUNK, a.V3 - c0);                  // live elements of the chunk: a multiple of 3
  int clip[ROW_TILE];
  bool any = false;
#pragma unroll
  for (int r = 0; r < ROW_TILE; ++r) any |= row_live(a.lens, 1, 0, row0 + r, a.L_max, a.rows, clip[r]);
  if (!any) return;                                         // (uniform)
  {
    const float* g = a.cf + (size_t)blockIdx.x * NT * ROW_TILE;
    for (int i = tid; i < NT * ROW_TILE; i += 256) s_cf[i] = g[i];
    const float* x = a.xf + (size_t)row0 * J * 12;
    for (int i = tid; i < ROW_TILE * J * 12; i += 256) s_xf[i] = x[i];
    const int nv = n / 3, v0 = c0 / 3;
    for (int i = tid; i < nv * J; i += 256) s_w[(i % J) * 256 + i / J] = a.wts[(size_t)v0 * J + i];
  }
  __syncthreads();
  {  // the blend of flame_skin_kernel: v = v_id, then fma(c_t, D_t, v) over the terms in ascending order (D and v_id are padded to whole chunks)
    float acc[ROW_TILE][3];
#pragma unroll
    for (int r = 0; r < ROW_TILE; ++r) {
      const float* v = a.vid + (size_t)(a.shape_rows == 1 ? 0 : clip[r]) * a.ld + c0;
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[r][q] = v[tid + 256 * q];
    }
    for (int t = 0; t < NT; ++t) {
      const float* dk = a.D + (size_t)(t < NE ? a.row_expr + t : a.row_pose + (t - NE)) * a.ld + c0;
      const float d[3] = {dk[tid], dk[tid + 256], dk[tid + 512]};
#pragma unroll
      for (int r = 0; r < ROW_TILE; ++r) {
        const float c = s_cf[t * ROW_TILE + r];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[r][q] = __builtin_fmaf(c, d[q], acc[r][q]);
      }
    }
#pragma unroll
    for (int r = 0; r < ROW_TILE; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) s_v[r * ROW_CHUNK + tid + 256 * q] = acc[r][q];
  }
  // the thread's tiles of the upper triangle: tile = w + 4 (lane + 64 s), s < 3 (waves interleaved so that few tiles still use all four)
  int ta[3], tb[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int t = (tid >> 6) + 4 * ((tid & 63) + 64 * s);
    ta[s] = tb[s] = -1;
    if (t < ntile) {
      int x = 0, rem = t;
      while (rem >= nb - x) { rem -= nb - x; ++x; }
      ta[s] = x; tb[s] = x + rem;
    }
  }
  const int vl = tid & (FIT_SUB - 1), cg = tid / FIT_SUB;   // vertex of the sub-block, column group (8 of them)
  for (int r = 0; r < ROW_TILE; ++r) {
    const int row = row0 + r;
    int clip_r;
    if (!row_live(a.lens, 1, 0, row, a.L_max, a.rows, clip_r)) continue;      // (uniform)
    __syncthreads();
    for (int i = tid; i < NQ * J * 12; i += 256) s_dx[i] = a.dX[(size_t)row * NQ * J * 12 + i];
    for (int i = tid; i < NE * J * 3; i += 256) s_de[i] = a.dE[(size_t)row * NE * J * 3 + i];
    float acc[3][16];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[s][e] = 0.f;
    const float* X = s_xf + r * J * 12;
    float t3[3] = {0.f, 0.f, 0.f};
    if (fd.transl) { t3[0] = a.tr[(size_t)row * 3]; t3[1] = a.tr[(size_t)row * 3 + 1]; t3[2] = a.tr[(size_t)row * 3 + 2]; }
    for (int sb = 0; sb * 3 * FIT_SUB < n; ++sb) {
      __syncthreads();                                      // the tables are in; the block of the sub-block before is read
      const int vc = sb * FIT_SUB + vl;                     // vertex of the chunk
      const bool on = 3 * vc < n;
      float T[12], v[3] = {0.f, 0.f, 0.f}, w[FLAME_JMAX];
#pragma unroll
      for (int j = 0; j < FLAME_JMAX; ++j) w[j] = (on && j < J) ? s_w[j * 256 + vc] : 0.f;
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = __fmul_rn(w[0], X[e]);
#pragma unroll
      for (int j = 1; j < FLAME_JMAX; ++j)
        if (j < J) {
#pragma unroll
          for (int e = 0; e < 12; ++e) T[e] = __builtin_fmaf(w[j], X[12 * j + e], T[e]);
        }
      if (on) { v[0] = s_v[r * ROW_CHUNK + 3 * vc]; v[1] = s_v[r * ROW_CHUNK + 3 * vc + 1]; v[2] = s_v[r * ROW_CHUNK + 3 * vc + 2]; }
      if (cg == 0) {
        const float m = on ? (a.vw ? a.vw[c0 / 3 + vc] : 1.f) : 0.f;
        s_m[3 * vl] = m; s_m[3 * vl + 1] = m; s_m[3 * vl + 2] = m;
      }
      for (int q = cg; q < 4 * nb; q += 8) {
        float o[3] = {0.f, 0.f, 0.f};
        if (on && q <= P) {
          if (q < NE) {                                     // T.R d_q + sum_j w_j dE_qj
            const float* dq = a.D + (size_t)(a.row_expr + q) * a.ld + c0 + 3 * vc;
            const float d0 = dq[0], d1 = dq[1], d2 = dq[2];
            const float* E = s_de + q * J * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              float e = __fmul_rn(w[0], E[c]);
#pragma unroll
              for (int j = 1; j < FLAME_JMAX; ++j) if (j < J) e = __builtin_fmaf(w[j], E[3 * j + c], e);
              o[c] = __fadd_rn(__builtin_fmaf(T[4 * c + 2], d2, __builtin_fmaf(T[4 * c + 1], d1, __fmul_rn(T[4 * c], d0))), e);
            }
          } else if (q < NE + NQ) {                         // (sum_j w_j dA_qj) applied to the blended vertex
            const float* Xq = s_dx + (q - NE) * J * 12;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              float tq[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) tq[e] = __fmul_rn(w[0], Xq[4 * c + e]);
#pragma unroll
              for (int j = 1; j < FLAME_JMAX; ++j)
                if (j < J) {
#pragma unroll
                  for (int e = 0; e < 4; ++e) tq[e] = __builtin_fmaf(w[j], Xq[12 * j + 4 * c + e], tq[e]);
                }
              o[c] = __fadd_rn(__builtin_fmaf(tq[2], v[2], __builtin_fmaf(tq[1], v[1], __fmul_rn(tq[0], v[0]))), tq[3]);
            }
          } else if (q < P) {                               // translation: the identity
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = c == q - NE - NQ ? 1.f : 0.f;
          } else {                                          // the residual: forward (+ translation) - target
            const float* y = a.target + (size_t)row * a.V3 + c0 + 3 * vc;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              float f = __fadd_rn(__builtin_fmaf(T[4 * c + 2], v[2], __builtin_fmaf(T[4 * c + 1], v[1], __fmul_rn(T[4 * c], v[0]))), T[4 * c + 3]);
              if (fd.transl) f = __fadd_rn(f, t3[c]);
              o[c] = __fsub_rn(f, y[c]);
            }
          }
        }
        s_j[q * FIT_LDJ + 3 * vl] = o[0]; s_j[q * FIT_LDJ + 3 * vl + 1] = o[1]; s_j[q * FIT_LDJ + 3 * vl + 2] = o[2];
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if (ta[s] < 0) continue;
        const float* ja = s_j + 4 * ta[s] * FIT_LDJ;
        const float* jb = s_j + 4 * tb[s] * FIT_LDJ;
        for (int i = 0; i < 3 * FIT_SUB; ++i) {
          const float m = s_m[i];
          float am[4], bb[4];
#pragma unroll
          for (int x = 0; x < 4; ++x) { am[x] = __fmul_rn(m, ja[x * FIT_LDJ + i]); bb[x] = jb[x * FIT_LDJ + i]; }
#pragma unroll
          for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[s][4 * x + y] = __builtin_fmaf(am[x], bb[y], acc[s][4 * x + y]);
        }
      }
    }
    float* o = a.part + ((size_t)row * a.chunks + chunk) * fit_np(P);
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (ta[s] < 0) continue;
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          const int ia = 4 * ta[s] + x, ib = 4 * tb[s] + y;
          if (ia <= ib && ib <= P) o[fit_idx(P, ia, ib)] = acc[s][4 * x + y];
        }
    }
  }
}

// Hs [rows][NP] = part[row][0] + part[row][1] + .. (rounded adds, ascending); dead rows are left alone
__global__ __launch_bounds__(256) void flame_fit_reduce_kernel(const float* part, const int* lens, int L_max, int rows, int chunks, int NP, float* Hs) {
  const int row = blockIdx.x;
  const int i = blockIdx.y * 256 + threadIdx.x;
  int b;
  if (i >= NP || !row_live(lens, 1, 0, row, L_max, b)) return;
  const float* p = part + (size_t)row * chunks * NP + i;
  float s = p[0];
  for (int c = 1; c < chunks; ++c) s = __fadd_rn(s, p[(size_t)c * NP]);
  Hs[(size_t)row * NP + i] = s;
}

// One damped Gauss-Newton step of a row.  With H, g of Hs (g_a = Hs[a][P]), rho_q = ridge_expr for expression columns, ridge_pose for pose
// columns, 0 for the translation, theta0 = (0, pose0, 0):
//   A = H + diag(rho + lambda) (one rounded add of the rounded sum rho_q + lambda), b_q = -(g_q + rho_q (theta_q - theta0_q)).
//   Cholesky, right-looking, columns ascending: pivot p = A_jj; the row FAILS when not p > pivot_tol x (the damped diagonal before
//   elimination; pivot_tol = 0 is the plain test p > 0); l_jj = sqrt(p), l_ij = A_ij / l_jj, then A_ik = fma(-l_ij, l_kj, A_ik) for j < k <= i.
//   forward: y_j = b_j / l_jj, b_i = fma(-l_ij, y_j, b_i) for i > j, j ascending; back: x_j = y_j / l_jj, y_i = fma(-l_ji, x_j, y_i) for i < j,
//   j descending; theta_q += x_q (rounded add).  delta (or null) receives x.  A failed row: status = failing column + 1, theta left.
__global__ __launch_bounds__(256) void flame_fit_solve_kernel(const float* Hs, const int* lens, int L_max, const FitDesc fd, int J3, float lambda, float pivot_tol,
                                                             float ridge_expr, float ridge_pose, const float* pose0, float* expr, float* pose,
                                                             float* tr, float* delta, int* status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int P = fd.P, ldA = P + 1, NQ = 3 * fd.n_free;
  float* A = reinterpret_cast<float*>(smem);                // [P][P + 1], the lower triangle is used
  float* bv = A + P * ldA;                                  // [P]
  float* dg = bv + P;                                       // [P] the damped diagonal
  __shared__ int bad;
  const int row = blockIdx.x, tid = threadIdx.x;
  int b;
  if (!row_live(lens, 1, 0, row, L_max, b)) return;
  const float* H = Hs + (size_t)row * fit_np(P);
  if (tid == 0) bad = 0;
  for (int i = tid; i < P * P; i += 256) {
    const int r = i / P, c = i - r * P;
    if (c <= r) A[r * ldA + c] = H[fit_idx(P, c, r)];
  }
  __syncthreads();
  for (int q = tid; q < P; q += 256) {
    float rho = 0.f, th, th0 = 0.f;
    if (q < fd.n_expr) { rho = ridge_expr; th = expr[(size_t)row * fd.n_expr + q]; }
    else if (q < fd.n_expr + NQ) {
      const int qq = q - fd.n_expr, at = 3 * fd.free_j[qq / 3] + qq % 3;
      rho = ridge_pose; th = pose[(size_t)row * J3 + at];
      if (pose0) th0 = pose0[(size_t)row * J3 + at];
    } else th = tr[(size_t)row * 3 + (q - fd.n_expr - NQ)];
    const float d = __fadd_rn(A[q * ldA + q], __fadd_rn(rho, lambda));
    A[q * ldA + q] = d; dg[q] = d;
    bv[q] = -__fadd_rn(H[fit_idx(P, q, P)], __fmul_rn(rho, __fsub_rn(th, th0)));
  }
  __syncthreads();
  for (int j = 0; j < P; ++j) {
    const float p = A[j * ldA + j];
    if (!(p > __fmul_rn(pivot_tol, dg[j]))) { if (tid == 0) { bad = j + 1; status[row] = j + 1; } break; }      // (uniform: p is one LDS word)
    const float l = __fsqrt_rn(p);
    __syncthreads();
    for (int i = j + 1 + tid; i < P; i += 256) A[i * ldA + j] = __fdiv_rn(A[i * ldA + j], l);
    if (tid == 0) A[j * ldA + j] = l;
    __syncthreads();
    const int m = P - 1 - j;                                // the trailing rows j + 1 .. P - 1
    for (int e = tid; e < m * m; e += 256) {
      const int i = j + 1 + e / m, k = j + 1 + e % m;
      if (k <= i) A[i * ldA + k] = __builtin_fmaf(-A[i * ldA + j], A[k * ldA + j], A[i * ldA + k]);
    }
    __syncthreads();
  }
  __syncthreads();
  if (bad) {
    if (delta) for (int q = tid; q < P; q += 256) delta[(size_t)row * P + q] = 0.f;
    return;
  }
  for (int j = 0; j < P; ++j) {
    const float y = __fdiv_rn(bv[j], A[j * ldA + j]);
    __syncthreads();
    if (tid == 0) bv[j] = y;
    for (int i = j + 1 + tid; i < P; i += 256) bv[i] = __builtin_fmaf(-A[i * ldA + j], y, bv[i]);
    __syncthreads();
  }
  for (int j = P - 1; j >= 0; --j) {
    const float x = __fdiv_rn(bv[j], A[j * ldA + j]);
    __syncthreads();
    if (tid == 0) bv[j] = x;
    for (int i = tid; i < j; i += 256) bv[i] = __builtin_fmaf(-A[j * ldA + i], x, bv[i]);
    __syncthreads();
  }
  for (int q = tid; q < P; q += 256) {
    const float x = bv[q];
    if (delta) delta[(size_t)row * P + q] = x;
    float* t;
    if (q < fd.n_expr) t = expr + (size_t)row * fd.n_expr + q;
    else if (q < fd.n_expr + NQ) { const int qq = q - fd.n_expr; t = pose + (size_t)row * J3 + 3 * fd.free_j[qq / 3] + qq % 3; }
    else t = tr + (size_t)row * 3 + (q - fd.n_expr - NQ);
    *t = __fadd_rn(*t, x);
  }
}

// rms [row] = sqrt(S / msum), S = sum over chunks (ascending, rounded adds) of the chunk's tree sum of e_v = m_v ((dx dx + dy dy) + dz dz),
// d = verts - target (rounded), over 256 slots (slots past the chunk's vertices hold 0): s[t] += s[t + h] for h = 128, 64, .., 1.
// Dead rows: 0.
__global__ __launch_bounds__(256) void flame_fit_rms_kernel(const float* verts, const float* target, const float* vw, const int* lens, int L_max, int V3,
                                                           int chunks, float msum, float* rms) {
  __shared__ float s[256];
  const int row = blockIdx.x, tid = threadIdx.x;
  int b;
  if (!row_live(lens, 1, 0, row, L_max, b)) { if (tid == 0) rms[row] = 0.f; return; }
  float S = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const int e0 = c * ROW_CHUNK + 3 * tid;
    float e = 0.f;
    if (e0 < V3) {
      const float* x = verts + (size_t)row * V3 + e0;
      const float* y = target + (size_t)row * V3 + e0;
      const float dx = __fsub_rn(x[0], y[0]), dy = __fsub_rn(x[1], y[1]), dz = __fsub_rn(x[2], y[2]);
      e = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      if (vw) e = __fmul_rn(vw[e0 / 3], e);
    }
    __syncthreads();
    s[tid] = e;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
      if (tid < h) s[tid] = __fadd_rn(s[tid], s[tid + h]);
      __syncthreads();
    }
    if (tid == 0) S = __fadd_rn(S, s[0]);
  }
  if (tid == 0) rms[row] = __fsqrt_rn(__fdiv_rn(S, msum));
}

}  // namespace fdm
