// Device helpers shared by the hand-off kernels (mesh_out.hpp, rig_out.hpp, flame_out.hpp) and linear_interp_kernel (elementwise.hpp):
// the rules that DESIGN section 2 items 18-20 state once.  __device__ __forceinline__ only.
#pragma once
#include <hip/hip_runtime.h>

namespace fdm {

// ---- the row geometry of rig_proj_kernel and flame_skin_kernel: a row of 3V floats is cut into chunks, the rows into tiles
constexpr int ROW_CHUNK = 768;            // elements of a row per workgroup = 64 lanes x 3 pieces x 4 (a multiple of 3: chunks end on vertices)
constexpr int ROW_TILE = 8;               // rows of [B * L_max] per workgroup
constexpr int ROW_Q = ROW_CHUNK / 256;    // 16-byte pieces per lane and row (piece q of lane l = elements 4 (l + 64 q) ..)

// ---- the frame-rate rule, F.interpolate(mode='linear', align_corners=True) over time.  Output frame t of Lo of a clip of L frames is
// l0 x[i0] + l1 x[i1] (two products, one sum), in fp32, every operation rounded on its own.  This function is the definition:
// linear_interp_kernel (Tin = L, Tout = Lo), mesh_pos_kernel and rig_solve_kernel call it and state nothing of their own.
__device__ __forceinline__ void interp_taps(int L, int Lo, int t, int& i0, int& i1, float& l0, float& l1) {
  const float scale = Lo > 1 ? (float)(L - 1) / (float)(Lo - 1) : 0.f;
  const float src = __fmul_rn(scale, (float)t);
  i0 = min((int)src, L - 1);
  i1 = i0 + (i0 < L - 1 ? 1 : 0);
  l1 = __fsub_rn(src, (float)i0);
  l0 = __fsub_rn(1.f, l1);
}

// ---- whether a row of [B][span] is one of its clip's own frames; its clip goes to b.  lens holds `stride` ints per clip ({L, L_out}
// of mesh and rig: 2; L alone of flame: 1), `col` is the one that bounds this row's index.
__device__ __forceinline__ bool row_live(const int* lens, int stride, int col, int row, int span, int& b) {
  b = row / span;
  return row - b * span < lens[stride * b + col];
}
// the same for a row that may lie at or past `rows` (the padding of a tile): clip 0, not live, lens not read
__device__ __forceinline__ bool row_live(const int* lens, int stride, int col, int row, int span, int rows, int& b) {
  bool live = false;
  b = 0;
  if (row < rows) live = row_live(lens, stride, col, row, span, b);
  return live;
}

// ---- the 16-byte peel.  A row of 3V floats starts on a 4-byte boundary only (12 V bytes per row), so n elements at p are walked as
// `head` <= 3 single elements up to p's own 16-byte boundary, `nb` 16-byte pieces, and <= 3 single elements from `done` on.
struct Peel { int head, nb, done; };__device__ __forceinline__ Peel peel_of(const void* p, int n) {
  const unsigned long long addr = (unsigned long long)p;
  const int head = min(n, (int)((4 - ((addr >> 2) & 3)) & 3));
  const int nb = (n - head) >> 2;
  return {head, nb, head + 4 * nb};
}
// THREADS threads walk the peel: thread tid takes the pieces tid, tid + THREADS, ..; the first `head` threads the head; the threads
// from TAIL0 on the tail.  op.piece(i) handles elements i .. i + 3 (16-byte aligned in global memory), op.one(i) element i.
template <int THREADS, int TAIL0, typename Op>
__device__ __forceinline__ void peel_walk(const Peel& p, int n, int tid, const Op& op) {
  for (int m = tid; m < p.nb; m += THREADS) op.piece(p.head + 4 * m);
  if (tid < p.head) op.one(tid);
  if (tid >= TAIL0 && tid - TAIL0 < n - p.done) op.one(p.done + tid - TAIL0);
}
struct PeelLoad {                         // s = g (g: the row in global memory; s: its copy in LDS, 4-byte aligned only)
  const float* g; float* s;
  __device__ __forceinline__ void piece(int i) const {
    const float4 v = *reinterpret_cast<const float4*>(g + i);
    float* q = s + i;
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
  }
  __device__ __forceinline__ void one(int i) const { s[i] = g[i]; }
};
struct PeelAdd {                          // s = s + g, rounded
  const float* g; float* s;
  __device__ __forceinline__ void piece(int i) const {
    const float4 e = *reinterpret_cast<const float4*>(g + i);
    float* q = s + i;
    q[0] = __fadd_rn(q[0], e.x); q[1] = __fadd_rn(q[1], e.y); q[2] = __fadd_rn(q[2], e.z); q[3] = __fadd_rn(q[3], e.w);
  }
  __device__ __forceinline__ void one(int i) const { s[i] = __fadd_rn(s[i], g[i]); }
};
struct PeelStore {                        // g = s
  float* g; const float* s;
  __device__ __forceinline__ void piece(int i) const {
    *reinterpret_cast<float4*>(g + i) = make_float4(s[i], s[i + 1], s[i + 2], s[i + 3]);
  }
  __device__ __forceinline__ void one(int i) const { g[i] = s[i]; }
};

}  // namespace fdm
