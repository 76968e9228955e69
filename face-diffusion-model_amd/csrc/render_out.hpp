// Kernels of the render hand-off (include/fdm_hip.h, fdm_render_*; launched by render_out.hip): the animated mesh -> shaded image frames.
// DESIGN section 2 item 23 is the definition; the header spells out every operation.  A call works through its live output frames a
// chunk at a time; per chunk:
//   render_pos_kernel      grid (chunk rows, blocks of RENDER_POS_TILE elements of 3V): p = offset + template, then the time resampling of
//                          interp_taps (handoff.hpp) at the clip's own length -- mesh_pos_kernel's expressions on a table of (clip, frame)
//                          rows instead of the whole [B, L_out_max] rectangle.  The vertex normals of the chunk are mesh_nrm_kernel's
//                          (render_out.hip calls the mesh hand-off on these positions) unless the caller brings them.
//   render_vertex_kernel   one lane per (chunk row, vertex): camera transform, projection, snapping to 8 sub-pixel bits, the `bad` test and
//                          the camera-space normal; two 16-byte records per vertex.
//   render_raster_kernel<S>   S = 1, 4 or 16 samples per pixel (fdm_render_set "samples").  One lane per (chunk row, face): setup (drop,
//                          int64 area, orientation) and the clamped box of pixels that have a sample inside the triangle's box.  The
//                          visibility buffer is [n][H][W][S], the samples of a pixel adjacent.  A box is handed to the whole wavefront:
//                          the lanes that hold one are taken in turn by ballot, the triangle travels by shuffles, and the 64 lanes take
//                          the box's (pixel, sample) items 64 apart in that order, so at S > 1 one atomicMax wave-instruction covers 512
//                          contiguous bytes of a pixel row.  At S = 1 alone a box of at most RENDER_LANE_BOX pixels is walked by its own
//                          lane instead; at S > 1 there is no per-lane walk (profiles/render_out/README.md says why).  Every covered
//                          sample's key goes into the buffer with a 64-bit atomicMax (a vector global atomic): a maximum, so the buffer
//                          does not depend on the order the triangles arrive in.
//   render_resolve_kernel<S, YUV>   the per-pixel work is one device function, render_pixel<S>: reads the pixel's 8 S contiguous bytes
//                          of keys (16 at a time at S > 1) and writes 0 back (the buffer is clear for the next chunk), shades every
//                          sample that has a fragment (a triangle's setup and normals are kept while consecutive samples name the same
//                          face), sums the channels in sample order, scales by 1 / S -> three 8-bit channels, the largest key, the count
//                          of covered samples.  The kernel writes whichever of rgb / depth / face / alpha (coverage count -> 8 bits) the
//                          call asks for, one lane per (chunk row, pixel); with YUV also the frame's Y'CbCr 4:2:0 planes (I420 or NV12)
//                          from the 8-bit rgb, one lane per 2 x 2 block of pixels.  The keys are cleared as they are read, so every
//                          plane comes out of this one pass and no rgb image is written that the caller did not ask for.
//                          fdm_render_forward is the call with alpha and yuv null.
//   render_resolve_kernel<S, YUV, MAT>   MAT = false is the kernel above, instruction for instruction (an object with no material).  MAT =
//                          true (fdm_render_set_material, DESIGN item 25): the colour that stands where `base` stands comes from the
//                          object's material behind one wavefront-uniform switch (the kind is a kernel argument) -- interpolated vertex
//                          colours, a colour table looked up at the interpolated scalar, or a texture read nearest or bilinear at the
//                          interpolated uv of the winning face's corners -- and `unlit` puts k = 1 in place of the Lambert sum.  The
//                          held face keeps its three corners' attributes next to its setup and normals.
//   render_scalar_kernel   kind 2 alone, one lane per (chunk row, vertex): the scalar field resampled by render_pos_kernel's
//                          expressions on the same live-row table, then u = fmin(fmax((s - lo) / span, 0), 1).
//   vertex_dist_kernel     fdm_op_vertex_dist: the distance of two vertex sets per (row, vertex), for error fields.
// No cooperative launch, grid barrier or spin-wait.  Resource figures: profiles/render_out/resources.txt.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fdm_hip.h"
#include "handoff.hpp"

namespace fdm {

constexpr int RENDER_POS_TILE = 1024;     // elements of a row per workgroup of render_pos_kernel (4 per thread, 256 apart)
constexpr int RENDER_TB = 256;            // threads per workgroup of the vertex, raster and resolve kernels
constexpr int RENDER_LANE_BOX = 16;       // a clamped box of more pixels than this is walked by the whole wavefront
constexpr int RENDER_MAX_LIGHTS = 8;
constexpr int RENDER_SNAP_MAX = 1 << 20;  // |X|, |Y| of a vertex that is not bad

struct RenderView {                       // kernel argument (by value): fdm_render_set_view changes it without touching the device
  float fx, fy, cx, cy, znear, zfar;
  float R[9], t[3];
  int n_lights;
  float dir[RENDER_MAX_LIGHTS][3], intensity[RENDER_MAX_LIGHTS];
  float ambient, base[3], background[3];
};

__device__ __forceinline__ float render_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}
__device__ __forceinline__ bool render_finite(float x) { return fabsf(x) < __builtin_inff(); }      // false for NaN

// Sample s of a pixel, in units of 1 / 256 pixel from the pixel's corner.  S = 1: the centre.  S = 4: the rotated grid
// (96, 32), (224, 96), (32, 160), (160, 224).  S = 16: the 4 x 4 grid, s = 4 j + i at (32 + 64 i, 32 + 64 j).  Every offset of
// S > 1 lies in 32 .. 224 (the raster box relies on it).
template <int S> __host__ __device__ __forceinline__ void render_sample_offset(int s, int& ox, int& oy) {
  if (S == 1) { ox = 128; oy = 128; }
  else if (S == 4) { ox = 32 + 64 * ((0x2031 >> (4 * s)) & 3); oy = 32 + 64 * s; }
  else { ox = 32 + 64 * (s & 3); oy = 32 + 64 * (s >> 2); }
}

// rowtab: [n] {clip, output frame} of the chunk's rows.  lens: [B][2] = {L, L_out}.  P: [n][V3].  tmpl_stride: 0 or V3.
__global__ __launch_bounds__(256) void render_pos_kernel(const float* off, const float* tmpl, int tmpl_stride, const int* lens, const int2* rowtab,
                                                         int L_max, int V3, int resample, float* P) {
  const int2 bt = rowtab[blockIdx.x];
  const int b = bt.x, t = bt.y;
  int i0 = t, i1 = t;
  float l0 = 1.f, l1 = 0.f;
  if (resample) interp_taps(lens[2 * b], lens[2 * b + 1], t, i0, i1, l0, l1);
  const float* x0 = off + ((size_t)b * L_max + i0) * V3;
  const float* x1 = off + ((size_t)b * L_max + i1) * V3;
  const float* tp = tmpl ? tmpl + (size_t)b * tmpl_stride : nullptr;
  float* o = P + (size_t)blockIdx.x * V3;
#pragma unroll
  for (int k = 0; k < RENDER_POS_TILE / 256; ++k) {
    const int e = blockIdx.y * RENDER_POS_TILE + k * 256 + threadIdx.x;
    if (e >= V3) break;
    float y;
    if (!resample) {
      y = tp ? __fadd_rn(x0[e], tp[e]) : x0[e];
    } else {
      const float p0 = tp ? __fadd_rn(x0[e], tp[e]) : x0[e], p1 = tp ? __fadd_rn(x1[e], tp[e]) : x1[e];
      y = __fadd_rn(__fmul_rn(l0, p0), __fmul_rn(l1, p1));
    }
    o[e] = y;
  }
}

// P: [n][V][3] positions of the chunk.  N: the chunk's normals [n][V][3] (rowtab == null), or the caller's [B][Lo_max][V][3] read at the
// row's (clip, frame).  xyw: [n][V] {X, Y, bits(w), bad}; nc: [n][V] {nc.x, nc.y, nc.z, 0}.
__global__ __launch_bounds__(RENDER_TB) void render_vertex_kernel(const float* P, const float* N, const int2* rowtab, int Lo_max, int V,
                                                                  const RenderView vw, int4* xyw, float4* nc) {
  const int row = blockIdx.y, v = blockIdx.x * RENDER_TB + threadIdx.x;
  if (v >= V) return;
  const float* p = P + ((size_t)row * V + v) * 3;
  size_t nrow = row;
  if (rowtab) { const int2 bt = rowtab[row]; nrow = (size_t)bt.x * Lo_max + bt.y; }
  const float* n = N + (nrow * V + v) * 3;
  const float px = p[0], py = p[1], pz = p[2], nx = n[0], ny = n[1], nz = n[2];
  const float* R = vw.R;
  const float pcx = __fadd_rn(render_dot(R[0], R[1], R[2], px, py, pz), vw.t[0]);
  const float pcy = __fadd_rn(render_dot(R[3], R[4], R[5], px, py, pz), vw.t[1]);
  const float pcz = __fadd_rn(render_dot(R[6], R[7], R[8], px, py, pz), vw.t[2]);
  const float d = -pcz;
  const float w = __fdiv_rn(1.f, d);
  const float sx = __fadd_rn(__fmul_rn(vw.fx, __fmul_rn(pcx, w)), vw.cx);
  const float sy = __fsub_rn(vw.cy, __fmul_rn(vw.fy, __fmul_rn(pcy, w)));
  const float rx = rintf(__fmul_rn(256.f, sx)), ry = rintf(__fmul_rn(256.f, sy));
  bool bad = !(render_finite(px) && render_finite(py) && render_finite(pz) && render_finite(d) && render_finite(sx) && render_finite(sy));
  bad = bad || !(d > vw.znear) || !(d < vw.zfar) || !(fabsf(rx) <= (float)RENDER_SNAP_MAX) || !(fabsf(ry) <= (float)RENDER_SNAP_MAX);
  const size_t o = (size_t)row * V + v;
  xyw[o] = make_int4(bad ? 0 : (int)rx, bad ? 0 : (int)ry, __float_as_int(w), bad ? 1 : 0);
  nc[o] = make_float4(render_dot(R[0], R[1], R[2], nx, ny, nz), render_dot(R[3], R[4], R[5], nx, ny, nz), render_dot(R[6], R[7], R[8], nx, ny, nz), 0.f);
}

// ---- the oriented triangle of a face and its fragment at a pixel: the one statement the raster and resolve kernels share
struct RenderTri {
  int X0, Y0, X1, Y1, X2, Y2;             // snapped, oriented: A > 0
  float w0, w1, w2;
  long long A;
  bool swapped, ok;                       // ok: no bad vertex and A != 0
};
__device__ __forceinline__ RenderTri render_setup(const int4& a, const int4& b, const int4& c) {
  RenderTri T;
  T.X0 = a.x; T.Y0 = a.y; T.w0 = __int_as_float(a.z);
  const long long A = (long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x);
  T.swapped = A < 0;
  const int4& u = T.swapped ? c : b;
  const int4& v = T.swapped ? b : c;
  T.X1 = u.x; T.Y1 = u.y; T.w1 = __int_as_float(u.z);
  T.X2 = v.x; T.Y2 = v.y; T.w2 = __int_as_float(v.z);
  T.A = T.swapped ? -A : A;
  T.ok = !(a.w | b.w | c.w) && A != 0;
  return T;
}
// the edge function of the edge a -> b at (px, py), and whether the pixel centre on it belongs to the triangle (top-left rule: with
// A > 0 in x-right, y-down coordinates a left edge runs up, dy < 0, and a top edge runs right, dy == 0 and dx > 0)
__device__ __forceinline__ bool render_edge(int Xa, int Ya, int Xb, int Yb, int px, int py, long long& E) {
  const int dx = Xb - Xa, dy = Yb - Ya;
  E = (long long)dx * (py - Ya) - (long long)dy * (px - Xa);
  return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}
// covered at the sample position (px, py): E_i, l_i = (float)E_i / (float)A, iw = (l0 w0 + l1 w1) + l2 w2
__device__ __forceinline__ bool render_fragment_at(const RenderTri& T, int px, int py, float& l0, float& l1, float& l2, float& iw) {
  long long E0, E1, E2;
  const bool in0 = render_edge(T.X1, T.Y1, T.X2, T.Y2, px, py, E0);
  const bool in1 = render_edge(T.X2, T.Y2, T.X0, T.Y0, px, py, E1);
  const bool in2 = render_edge(T.X0, T.Y0, T.X1, T.Y1, px, py, E2);
  const float fA = (float)T.A;
  l0 = __fdiv_rn((float)E0, fA); l1 = __fdiv_rn((float)E1, fA); l2 = __fdiv_rn((float)E2, fA);
  iw = __fadd_rn(__fadd_rn(__fmul_rn(l0, T.w0), __fmul_rn(l1, T.w1)), __fmul_rn(l2, T.w2));
  return in0 && in1 && in2;
}
// the fragment of `face` at (px, py), if there is one, into the key at `slot`
__device__ __forceinline__ void render_hit_at(const RenderTri& T, int px, int py, int face, unsigned long long* slot) {
  float l0, l1, l2, iw;
  if (!render_fragment_at(T, px, py, l0, l1, l2, iw)) return;
  if (!(iw > 0.f) || !render_finite(iw)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(iw) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)face);
  atomicMax(slot, key);
}
// the pixels p0 .. p1 of one axis that have a sample of render_sample_offset<S> inside lo .. hi (snapped), clamped to 0 .. n - 1
template <int S> __device__ __forceinline__ void render_box(int lo, int hi, int n, int& p0, int& p1) {
  constexpr int O_LO = S == 1 ? 128 : 32, O_HI = S == 1 ? 128 : 224;      // the least and the largest offset of the pattern
  p0 = max((lo + 255 - O_HI) >> 8, 0);        // the first p with 256 p + O_HI >= lo
  p1 = min((hi - O_LO) >> 8, n - 1);          // the last p with 256 p + O_LO <= hi
}
// lane src's triangle, for every lane of the wavefront (A from the coordinates; swapped and ok do not travel: a box exists only if ok)
__device__ __forceinline__ RenderTri render_tri_of_lane(const RenderTri& T, int src) {
  RenderTri Q = {};
  Q.X0 = __shfl(T.X0, src); Q.Y0 = __shfl(T.Y0, src); Q.X1 = __shfl(T.X1, src); Q.Y1 = __shfl(T.Y1, src);
  Q.X2 = __shfl(T.X2, src); Q.Y2 = __shfl(T.Y2, src);
  Q.w0 = __shfl(T.w0, src); Q.w1 = __shfl(T.w1, src); Q.w2 = __shfl(T.w2, src);
  Q.A = (long long)(Q.X1 - Q.X0) * (Q.Y2 - Q.Y0) - (long long)(Q.Y1 - Q.Y0) * (Q.X2 - Q.X0);
  return Q;
}

// xyw: [n][V]; faces [F][3]; vis: [n][H][W][S] keys (0 = no fragment).  grid (blocks of RENDER_TB faces, chunk rows).
template <int S>
__global__ __launch_bounds__(RENDER_TB) void render_raster_kernel(const int4* xyw, const int* faces, int F, int V, int W, int H,
                                                                  unsigned long long* vis) {
  static_assert(S == 1 || S == 4 || S == 16, "the sample patterns of render_sample_offset");
  const int row = blockIdx.y, f = blockIdx.x * RENDER_TB + threadIdx.x;
  const int4* rec = xyw + (size_t)row * V;
  unsigned long long* img = vis + (size_t)row * W * H * S;
  RenderTri T = {};
  int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
  if (f < F) {
    const int* fv = faces + 3 * (size_t)f;
    T = render_setup(rec[fv[0]], rec[fv[1]], rec[fv[2]]);
    if (T.ok) {      // pixels with a sample inside the triangle's box, clamped to the viewport
      render_box<S>(min(T.X0, min(T.X1, T.X2)), max(T.X0, max(T.X1, T.X2)), W, x0, x1);
      render_box<S>(min(T.Y0, min(T.Y1, T.Y2)), max(T.Y0, max(T.Y1, T.Y2)), H, y0, y1);
    }
  }
  const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
  const int nitem = (bw > 0 && bh > 0) ? bw * bh * S : 0;      // <= W H S <= 2^26 (fdm_render_set)
  bool wide = nitem > 0;                  // at S > 1 every box goes to the wavefront (profiles/render_out/README.md)
  if constexpr (S == 1) {                 // a small box is walked by its own lane: one atomicMax per trip, not unrolled
    wide = nitem > RENDER_LANE_BOX;
    if (nitem > 0 && !wide)
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) render_hit_at(T, 256 * x + 128, 256 * y + 128, f, img + (size_t)y * W + x);
  }
  // the wide boxes of this wavefront, one after the other, by all 64 lanes (every lane of the wavefront comes here): item i is sample
  // i % S of the box's pixel i / S, so the lanes' keys lie next to each other along a pixel row
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(wide);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const RenderTri Q = render_tri_of_lane(T, src);
    const int sx0 = __shfl(x0, src), sy0 = __shfl(y0, src), sbw = __shfl(bw, src), sn = __shfl(nitem, src), sf = __shfl(f, src);
    for (int i = lane; i < sn; i += 64) {
      const int pix = i / S, s = i - pix * S;
      const int dy = pix / sbw;
      const int x = sx0 + (pix - dy * sbw), y = sy0 + dy;
      int ox, oy;
      render_sample_offset<S>(s, ox, oy);
      render_hit_at(Q, 256 * x + ox, 256 * y + oy, sf, img + ((size_t)y * W + x) * S + s);
    }
  }
}

// step 5 for one fragment of the oriented triangle T with the camera-space normals of its vertices 0, 1, 2: the Lambert factor k; the
// perspective weights b0, b1, b2 are handed out (a material interpolates its attributes with them: computed once)
__device__ __forceinline__ float render_shade(const RenderTri& T, const float4& n0, const float4& n1, const float4& n2, float l0, float l1, float l2,
                                              float iw, const RenderView& vw, float& b0, float& b1, float& b2) {
  b0 = __fdiv_rn(__fmul_rn(l0, T.w0), iw); b1 = __fdiv_rn(__fmul_rn(l1, T.w1), iw); b2 = __fdiv_rn(__fmul_rn(l2, T.w2), iw);
  float nx = __fadd_rn(__fadd_rn(__fmul_rn(b0, n0.x), __fmul_rn(b1, n1.x)), __fmul_rn(b2, n2.x));
  float ny = __fadd_rn(__fadd_rn(__fmul_rn(b0, n0.y), __fmul_rn(b1, n1.y)), __fmul_rn(b2, n2.y));
  float nz = __fadd_rn(__fadd_rn(__fmul_rn(b0, n0.z), __fmul_rn(b1, n1.z)), __fmul_rn(b2, n2.z));
  const float s = render_dot(nx, ny, nz, nx, ny, nz);
  if (s > 0.f) {
    const float r = sqrtf(s);           // the correctly rounded expansion, as in mesh_nrm_kernel
    nx = __fdiv_rn(nx, r); ny = __fdiv_rn(ny, r); nz = __fdiv_rn(nz, r);
  } else {
    nx = ny = nz = 0.f;
  }
  if (nz < 0.f) { nx = -nx; ny = -ny; nz = -nz; }
  float k = vw.ambient;
#pragma unroll
  for (int l = 0; l < RENDER_MAX_LIGHTS; ++l) {      // (unrolled: the view stays in scalar registers)
    if (l >= vw.n_lights) break;
    const float d = render_dot(nx, ny, nz, vw.dir[l][0], vw.dir[l][1], vw.dir[l][2]);
    k = __fadd_rn(k, __fmul_rn(vw.intensity[l], d > 0.f ? d : 0.f));
  }
  return k;
}

// ---- materials (DESIGN item 25): the colour m that stands where `base` stands in step 5
struct RenderNoMat {};                    // what render_pixel<S, false> is handed in place of a material: nothing
__device__ __forceinline__ RenderNoMat render_first_or_none() { return RenderNoMat(); }
template <typename T> __device__ __forceinline__ const T& render_first_or_none(const T& t) { return t; }
struct RenderMat {                        // kernel argument (by value) of the MAT = true instances; the same in every lane
  int kind, unlit;                        // 0 base, 1 vertex colours, 2 scalar map, 3 texture
  const float* colors;                    // kind 1: [V][3]
  const float* u;                         // kind 2: [n][V] of the chunk, in [0, 1] (render_scalar_kernel)
  const float4* lut;                      // kind 2: [n_lut] {r, g, b, 0}
  int n_lut;
  const float2* uv;                       // kind 3: [F][3] per face corner
  const unsigned* tex;                    // kind 3: [tex_h][tex_w] texels r | g << 8 | b << 16 (the bytes r, g, b, 0), row 0 at the top
  int tex_w, tex_h, filter;               // 0 nearest, 1 bilinear
};
// The attributes of the held face's oriented corners i = 0, 1, 2 are nine floats a0 .. a8: kind 1 a(3 i + c), kind 2 a(i), kind 3 a(2 i),
// a(2 i + 1).  Nine variables of their own, not an array or a struct: the compiler merges the kinds' stores into one store at a
// run-time offset, and an aggregate then lives in scratch memory.
#define RENDER_ATTR_REFS float &a0, float &a1, float &a2, float &a3, float &a4, float &a5, float &a6, float &a7, float &a8
#define RENDER_ATTR_VALS float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7, float a8
#define RENDER_ATTR_ARGS a0, a1, a2, a3, a4, a5, a6, a7, a8

__device__ __forceinline__ float render_interp(float b0, float b1, float b2, float a0, float a1, float a2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(b0, a0), __fmul_rn(b1, a1)), __fmul_rn(b2, a2));
}
__device__ __forceinline__ float render_lerp(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(f, __fsub_rn(b, a))); }
// fmaxf / fminf return the operand that is not NaN: a NaN x gives lo
__device__ __forceinline__ float render_clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ void render_texel(const RenderMat& mt, int col, int row, float& r, float& g, float& b) {
  const unsigned t = mt.tex[(size_t)row * mt.tex_w + col];      // one 4-byte load
  r = __fdiv_rn((float)(t & 255u), 255.f); g = __fdiv_rn((float)((t >> 8) & 255u), 255.f); b = __fdiv_rn((float)((t >> 16) & 255u), 255.f);
}
// the attributes of face `won` whose oriented corners are the vertices v0, v1, v2 (corners 1 and 2 swapped where the setup swapped them)
__device__ __forceinline__ void render_attr_load(const RenderMat& mt, unsigned won, bool swapped, size_t r0, int v0, int v1, int v2, RENDER_ATTR_REFS) {
  if (mt.kind == 1) {
    const float *c0 = mt.colors + 3 * (size_t)v0, *c1 = mt.colors + 3 * (size_t)v1, *c2 = mt.colors + 3 * (size_t)v2;
    a0 = c0[0]; a1 = c0[1]; a2 = c0[2]; a3 = c1[0]; a4 = c1[1]; a5 = c1[2]; a6 = c2[0]; a7 = c2[1]; a8 = c2[2];
  } else if (mt.kind == 2) {
    a0 = mt.u[r0 + v0]; a1 = mt.u[r0 + v1]; a2 = mt.u[r0 + v2];
  } else if (mt.kind == 3) {
    const float2* q = mt.uv + 3 * (size_t)won;
    const float2 q0 = q[0], q1 = q[swapped ? 2 : 1], q2 = q[swapped ? 1 : 2];
    a0 = q0.x; a1 = q0.y; a2 = q1.x; a3 = q1.y; a4 = q2.x; a5 = q2.y;
  }
}
// m of one fragment with the perspective weights b0, b1, b2 (the switch is uniform over the wavefront: the kind is a kernel argument)
__device__ __forceinline__ void render_material(const RenderMat& mt, RENDER_ATTR_VALS, float b0, float b1, float b2, const RenderView& vw, float& mr,
                                                float& mg, float& mb) {
  mr = vw.base[0]; mg = vw.base[1]; mb = vw.base[2];
  if (mt.kind == 1) {
    mr = render_interp(b0, b1, b2, a0, a3, a6);
    mg = render_interp(b0, b1, b2, a1, a4, a7);
    mb = render_interp(b0, b1, b2, a2, a5, a8);
  } else if (mt.kind == 2) {
    const float u = render_clampf(render_interp(b0, b1, b2, a0, a1, a2), 0.f, 1.f);
    const float x = __fmul_rn(u, (float)(mt.n_lut - 1));      // in [0, n_lut - 1]
    const int i = min((int)x, mt.n_lut - 2);
    const float f = __fsub_rn(x, (float)i);
    const float4 p = mt.lut[i], q = mt.lut[i + 1];
    mr = render_lerp(p.x, q.x, f); mg = render_lerp(p.y, q.y, f); mb = render_lerp(p.z, q.z, f);
  } else if (mt.kind == 3) {
    const float tu = render_interp(b0, b1, b2, a0, a2, a4), tv = render_interp(b0, b1, b2, a1, a3, a5);
    const float fw = (float)mt.tex_w, fh = (float)mt.tex_h, cw = (float)(mt.tex_w - 1), ch = (float)(mt.tex_h - 1);
    if (mt.filter == 0) {                 // the clamps are made in float: no index leaves the texture, whatever the bits of uv
      const int col = (int)render_clampf(floorf(__fmul_rn(tu, fw)), 0.f, cw);
      const int row = (int)render_clampf(floorf(__fmul_rn(__fsub_rn(1.f, tv), fh)), 0.f, ch);
      render_texel(mt, col, row, mr, mg, mb);
    } else {
      const float x = __fsub_rn(__fmul_rn(tu, fw), 0.5f), y = __fsub_rn(__fmul_rn(__fsub_rn(1.f, tv), fh), 0.5f);
      const float x0 = floorf(x), y0 = floorf(y);
      const float fx = __fsub_rn(x, x0), fy = __fsub_rn(y, y0);      // NaN for a NaN or infinite coordinate: the sample takes the background
      const int c0 = (int)render_clampf(x0, 0.f, cw), c1 = (int)render_clampf(__fadd_rn(x0, 1.f), 0.f, cw);
      const int r0 = (int)render_clampf(y0, 0.f, ch), r1 = (int)render_clampf(__fadd_rn(y0, 1.f), 0.f, ch);
      float ar, ag, ab, br, bg, bb;
      render_texel(mt, c0, r0, ar, ag, ab);
      render_texel(mt, c1, r0, br, bg, bb);
      const float tr = render_lerp(ar, br, fx), tg = render_lerp(ag, bg, fx), tb = render_lerp(ab, bb, fx);
      render_texel(mt, c0, r1, ar, ag, ab);
      render_texel(mt, c1, r1, br, bg, bb);
      mr = render_lerp(tr, render_lerp(ar, br, fx), fy);
      mg = render_lerp(tg, render_lerp(ag, bg, fx), fy);
      mb = render_lerp(tb, render_lerp(ab, bb, fx), fy);
    }
  }
}

// What the resolve of one pixel gives: the three 8-bit channels, the largest key over the pixel's samples (0: no fragment) and n, the
// number of its samples that have a fragment.  depth, face and alpha follow from best and n.
struct RenderPixel {
  unsigned char r, g, b;
  int n;
  unsigned long long best;
};
__device__ __forceinline__ float render_key_depth(unsigned long long best) {
  return best ? __fdiv_rn(1.f, __uint_as_float((unsigned)(best >> 32))) : 0.f;
}
__device__ __forceinline__ int render_key_face(unsigned long long best) {
  return best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : -1;
}

// Step 5 for the pixel (x, y) of the chunk's row whose vertex records start at r0 = row V and whose keys start at img: reads the
// pixel's 8 S contiguous bytes of keys (S = 1: one 8-byte load; S > 1: 16 bytes at a time) and writes 0 back (the buffer is clear for
// the next chunk); per sample recomputes the winning face's fragment, interpolates the normal, shades; sums the channels in sample
// order, scales by 1 / S.  At S = 1 the sum is the one sample's colour and the scale is 1.  MAT: the colour comes from the material mt
// (a RenderMat) in place of vw.base; with MAT = false mt is not read.
template <int S, bool MAT, typename M>
__device__ __forceinline__ RenderPixel render_pixel(const int4* xyw, const float4* nc, const int* faces, int F, size_t r0, int W, int x, int y,
                                                    const RenderView& vw, const M& mt, unsigned long long* img) {
  static_assert(S == 1 || S == 4 || S == 16, "the sample patterns of render_sample_offset");
  constexpr int PER = S == 1 ? 1 : 2;     // keys per load
  unsigned long long* slot = img + ((size_t)y * W + x) * S;      // 8 S bytes, at S > 1 16-byte aligned
  float ar = 0.f, ag = 0.f, ab = 0.f;
  RenderPixel p;
  p.n = 0; p.best = 0ull;
  unsigned held = 0xFFFFFFFFu;            // the face whose setup T, n0, n1, n2 hold
  RenderTri T = {};
  float4 n0 = {}, n1 = {}, n2 = {};
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f;      // (MAT alone)
#pragma unroll 1
  for (int h = 0; h < S / PER; ++h) {
    ulonglong2 two = make_ulonglong2(0ull, 0ull);
    if constexpr (S == 1) {
      two.x = *slot;
      *slot = 0ull;
    } else {
      ulonglong2* pair = reinterpret_cast<ulonglong2*>(slot) + h;
      two = *pair;
      *pair = make_ulonglong2(0ull, 0ull);
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const unsigned long long key = e ? two.y : two.x;
      const int s = PER * h + e;
      float cr = vw.background[0], cg = vw.background[1], cb = vw.background[2];
      const unsigned won = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
      if (key && won < (unsigned)F) {     // (a key names a face of the list: the raster kernel wrote it)
        if (S == 1 || won != held) {
          const int* fv = faces + 3 * (size_t)won;
          T = render_setup(xyw[r0 + fv[0]], xyw[r0 + fv[1]], xyw[r0 + fv[2]]);
          n0 = nc[r0 + fv[0]]; n1 = nc[r0 + fv[T.swapped ? 2 : 1]]; n2 = nc[r0 + fv[T.swapped ? 1 : 2]];
          if constexpr (MAT) render_attr_load(mt, won, T.swapped, r0, fv[0], fv[T.swapped ? 2 : 1], fv[T.swapped ? 1 : 2], RENDER_ATTR_ARGS);
          held = won;
        }
        int ox, oy;
        render_sample_offset<S>(s, ox, oy);
        float l0, l1, l2, iw;             // (the recomputed iw has the key's bits: the same expressions on the same integers)
        (void)render_fragment_at(T, 256 * x + ox, 256 * y + oy, l0, l1, l2, iw);
        float b0, b1, b2;
        if constexpr (!MAT) {
          const float k = render_shade(T, n0, n1, n2, l0, l1, l2, iw, vw, b0, b1, b2);
          cr = __fmul_rn(vw.base[0], k); cg = __fmul_rn(vw.base[1], k); cb = __fmul_rn(vw.base[2], k);
        } else {
          float k = render_shade(T, n0, n1, n2, l0, l1, l2, iw, vw, b0, b1, b2);
          if (mt.unlit) k = 1.f;
          float mr, mg, mb;
          render_material(mt, RENDER_ATTR_ARGS, b0, b1, b2, vw, mr, mg, mb);
          cr = __fmul_rn(mr, k); cg = __fmul_rn(mg, k); cb = __fmul_rn(mb, k);
        }
        if (cr != cr) cr = vw.background[0];
        if (cg != cg) cg = vw.background[1];
        if (cb != cb) cb = vw.background[2];
        cr = cr < 1.f ? cr : 1.f; cg = cg < 1.f ? cg : 1.f; cb = cb < 1.f ? cb : 1.f;
        p.best = key > p.best ? key : p.best;
        ++p.n;
      }
      ar = s ? __fadd_rn(ar, cr) : cr; ag = s ? __fadd_rn(ag, cg) : cg; ab = s ? __fadd_rn(ab, cb) : cb;
    }
  }
  const float inv = 1.f / (float)S;       // a power of two: the product is exact
  p.r = (unsigned char)(int)__fadd_rn(__fmul_rn(255.f, __fmul_rn(ar, inv)), 0.5f);
  p.g = (unsigned char)(int)__fadd_rn(__fmul_rn(255.f, __fmul_rn(ag, inv)), 0.5f);
  p.b = (unsigned char)(int)__fadd_rn(__fmul_rn(255.f, __fmul_rn(ab, inv)), 0.5f);
  return p;
}

struct RenderOut {                        // kernel argument (by value): the call's outputs, null where it writes none
  unsigned char* rgb; float* depth; int* face; unsigned char* alpha; unsigned char* yuv;
};
struct RenderYuv {                        // kernel argument (by value)
  int k[10];                              // fdm_render_yuv_coeffs_host's {yr, yg, yb, ur, ug, ub, vr, vg, vb, y0}
  int nv12;
};
__host__ __device__ __forceinline__ int render_clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// rgb / depth / face / alpha of the pixel at o = (output frame) W H + y W + x, where asked for
__device__ __forceinline__ void render_store_pixel(const RenderOut& out, size_t o, const RenderPixel& p, int S) {
  if (out.rgb) { unsigned char* px = out.rgb + 3 * o; px[0] = p.r; px[1] = p.g; px[2] = p.b; }
  if (out.depth) out.depth[o] = render_key_depth(p.best);
  if (out.face) out.face[o] = render_key_face(p.best);
  if (out.alpha) out.alpha[o] = (unsigned char)((255 * p.n + S / 2) / S);
}

// out: the call's outputs [B][Lo_max][H][W](3), any of them null.
// YUV = false: one lane per (chunk row, pixel).  grid (blocks of RENDER_TB pixels, chunk rows).
// YUV = true (W and H even): one lane per (chunk row, 2 x 2 block of pixels).  The lane resolves its four pixels one after the other
// (not unrolled: the registers of one pixel, three channel sums and one luma byte stay live), stores each row's two luma bytes in one
// 2-byte store -- the 64 lanes of a wavefront write 128 contiguous bytes of a luma row -- and the block's chroma once (NV12: one
// 2-byte store).  yuv: [B][Lo_max][3 W H / 2], 2-byte aligned.  grid (blocks of RENDER_TB blocks of pixels, chunk rows).
// MAT = false: no further argument (the kernel's signature and code are what they were), the object has no material; MAT = true: one
// more argument, the object's RenderMat (kinds 0 to 3 and unlit).
template <int S, bool YUV, bool MAT, typename... M>
__global__ __launch_bounds__(RENDER_TB) void render_resolve_kernel(const int4* xyw, const float4* nc, const int* faces, int F, int V, int W, int H,
                                                                   const int2* rowtab, int Lo_max, const RenderView vw, unsigned long long* vis,
                                                                   const RenderOut out, const RenderYuv yc, const M... mat) {
  static_assert(sizeof...(M) == (MAT ? 1 : 0), "one RenderMat with MAT, nothing without");
  const auto& mt = render_first_or_none(mat...);
  const int row = blockIdx.y, i = blockIdx.x * RENDER_TB + threadIdx.x;
  const size_t WH = (size_t)W * H, r0 = (size_t)row * V;
  unsigned long long* img = vis + (size_t)row * WH * S;
  if constexpr (!YUV) {
    if (i >= W * H) return;
    const int2 bt = rowtab[row];
    const int y = i / W, x = i - y * W;
    const RenderPixel p = render_pixel<S, MAT>(xyw, nc, faces, F, r0, W, x, y, vw, mt, img);
    render_store_pixel(out, ((size_t)bt.x * Lo_max + bt.y) * WH + i, p, S);
  } else {
    const int W2 = W >> 1;
    if (i >= W2 * (H >> 1)) return;
    const int2 bt = rowtab[row];
    const size_t frame = (size_t)bt.x * Lo_max + bt.y;
    const int by = i / W2, bx = i - by * W2;
    unsigned char* Yp = out.yuv + frame * (WH + WH / 2);
    const int* k = yc.k;
    int Rs = 0, Gs = 0, Bs = 0, left = 0;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      const int x = 2 * bx + (q & 1), y = 2 * by + (q >> 1);
      const RenderPixel p = render_pixel<S, MAT>(xyw, nc, faces, F, r0, W, x, y, vw, mt, img);
      render_store_pixel(out, frame * WH + (size_t)y * W + x, p, S);
      const int R = p.r, G = p.g, B = p.b;
      Rs += R; Gs += G; Bs += B;
      const int luma = render_clamp_u8(((k[0] * R + k[1] * G + k[2] * B + 32768) >> 16) + k[9]);
      if (q & 1) *reinterpret_cast<uchar2*>(Yp + (size_t)y * W + 2 * bx) = make_uchar2((unsigned char)left, (unsigned char)luma);
      else left = luma;
    }
    const unsigned char U = (unsigned char)render_clamp_u8(((k[3] * Rs + k[4] * Gs + k[5] * Bs + (1 << 17)) >> 18) + 128);
    const unsigned char Vv = (unsigned char)render_clamp_u8(((k[6] * Rs + k[7] * Gs + k[8] * Bs + (1 << 17)) >> 18) + 128);
    unsigned char* Cp = Yp + WH;
    if (yc.nv12) {
      *reinterpret_cast<uchar2*>(Cp + 2 * (size_t)i) = make_uchar2(U, Vv);
    } else {
      Cp[i] = U;
      Cp[WH / 4 + i] = Vv;
    }
  }
}

// Kind 2, per (chunk row, vertex): the scalar field on the input frames -> u of the row's output frame.  sc: [B][L_max][V]; rowtab,
// lens, resample as render_pos_kernel (its expressions, no template; rows at or past frames[b] are never read); u: [n][V].
// grid (blocks of RENDER_TB vertices, chunk rows).
__global__ __launch_bounds__(RENDER_TB) void render_scalar_kernel(const float* sc, const int* lens, const int2* rowtab, int L_max, int V, int resample,
                                                                  float lo, float span, float* u) {
  const int row = blockIdx.y, v = blockIdx.x * RENDER_TB + threadIdx.x;
  if (v >= V) return;
  const int2 bt = rowtab[row];
  const int b = bt.x, t = bt.y;
  int i0 = t, i1 = t;
  float l0 = 1.f, l1 = 0.f;
  if (resample) interp_taps(lens[2 * b], lens[2 * b + 1], t, i0, i1, l0, l1);
  const float s0 = sc[((size_t)b * L_max + i0) * V + v];
  float s = s0;
  if (resample) s = __fadd_rn(__fmul_rn(l0, s0), __fmul_rn(l1, sc[((size_t)b * L_max + i1) * V + v]));
  u[(size_t)row * V + v] = render_clampf(__fdiv_rn(__fsub_rn(s, lo), span), 0.f, 1.f);
}

// fdm_op_vertex_dist: out[r][v] = sqrtf((dx dx + dy dy) + dz dz) of a - b over [rows][3 V].  n = rows V lanes.
__global__ __launch_bounds__(256) void vertex_dist_kernel(const float* a, const float* b, float* out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *p = a + 3 * i, *q = b + 3 * i;
  const float dx = __fsub_rn(p[0], q[0]), dy = __fsub_rn(p[1], q[1]), dz = __fsub_rn(p[2], q[2]);
  out[i] = sqrtf(render_dot(dx, dy, dz, dx, dy, dz));      // the correctly rounded expansion, as in mesh_nrm_kernel
}

}  // namespace fdm
