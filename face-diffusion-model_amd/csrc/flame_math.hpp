// Device helpers of the parametric head shared by its forward kernels (flame_out.hpp) and its fit kernels (flame_fit.hpp): the joints
// from the folded regressor and the Rodrigues rotation, so that both directions compute them with the same operations.
// __device__ __forceinline__ only.
#pragma once
#include <hip/hip_runtime.h>

#include "handoff.hpp"

namespace fdm {

constexpr int FLAME_JMAX = 8;

// ((a0 b0 + a1 b1) + a2 b2), every operation rounded
__device__ __forceinline__ float flame_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
}

// joints: JT + sum_k shape_k JD_k + sum_k expr_k JD_(expr_at + k), k ascending, product and sum rounded.  oc (or null): the row's
// column of the blend coefficients, which receives the expression coefficients (stride ROW_TILE)
__device__ __forceinline__ void flame_joints(float (&jf)[3 * FLAME_JMAX], const float* JT, const float* JD, int J3, const float* sh, int NS,
                                             const float* ex, int NE, int expr_at, float* oc) {
#pragma unroll
  for (int i = 0; i < 3 * FLAME_JMAX; ++i) jf[i] = i < J3 ? JT[i] : 0.f;
  for (int k = 0; k < NS; ++k) {
    const float c = sh[k];
    const float* d = JD + (size_t)k * J3;
#pragma unroll
    for (int i = 0; i < 3 * FLAME_JMAX; ++i) if (i < J3) jf[i] = __fadd_rn(jf[i], __fmul_rn(c, d[i]));
  }
  for (int k = 0; k < NE; ++k) {
    const float c = ex[k];
    if (oc) oc[(size_t)k * ROW_TILE] = c;
    const float* d = JD + (size_t)(expr_at + k) * J3;
#pragma unroll
    for (int i = 0; i < 3 * FLAME_JMAX; ++i) if (i < J3) jf[i] = __fadd_rn(jf[i], __fmul_rn(c, d[i]));
  }
}

// Rodrigues: angle = |r + 1e-8|, axis = r / angle, R = I + sin K + (1 - cos) K K (row-major)
__device__ __forceinline__ void flame_rodrigues(float rx, float ry, float rz, float (&R)[9]) {
  const float ex_ = __fadd_rn(rx, 1e-8f), ey_ = __fadd_rn(ry, 1e-8f), ez_ = __fadd_rn(rz, 1e-8f);
  const float angle = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(ex_, ex_), __fmul_rn(ey_, ey_)), __fmul_rn(ez_, ez_)));
  const float x = __fdiv_rn(rx, angle), y = __fdiv_rn(ry, angle), z = __fdiv_rn(rz, angle);
  const float s = sinf(angle), omc = __fsub_rn(1.f, cosf(angle));
  const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), zz = __fmul_rn(z, z);
  const float xy = __fmul_rn(x, y), xz = __fmul_rn(x, z), yz = __fmul_rn(y, z);
  const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
  const float KK[9] = {-__fadd_rn(yy, zz), xy, xz, xy, -__fadd_rn(xx, zz), yz, xz, yz, -__fadd_rn(xx, yy)};
#pragma unroll
  for (int e = 0; e < 9; ++e) R[e] = __fadd_rn(__fadd_rn(e % 4 == 0 ? 1.f : 0.f, __fmul_rn(s, K[e])), __fmul_rn(omc, KK[e]));
}

}  // namespace fdm
