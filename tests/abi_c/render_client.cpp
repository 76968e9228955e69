// One frame of a small seeded mesh drawn without Python or torch: fdm_render_create -> fdm_render_forward, the face-id image compared
// with the integer coverage rule of include/fdm_hip.h computed here.  The mesh is a jittered grid in the plane at distance 1 whose
// vertices sit on whole sub-pixel counts (fx = fy = 64 and w = 1: the projection is exact), so the snapped coordinates are known to
// the program; its triangles do not overlap, so a covered pixel names exactly one face.  Built and run by tests/test_render_abi_gpu.py:
//   hipcc render_client.cpp -I include -L <dir> -lfdm_hip ; render_client
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fdm_hip.h"

#define CK(x) do { if ((x) != 0) { printf("FAIL %s: %s\n", #x, fdm_last_error()); return 1; } } while (0)
#define HK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static bool inside(long long Xa, long long Ya, long long Xb, long long Yb, long long px, long long py) {
  const long long dx = Xb - Xa, dy = Yb - Ya, E = dx * (py - Ya) - dy * (px - Xa);
  return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

int main() {
  if (!fdm_device_ok()) { printf("no gfx950 device\n"); return 2; }
  const int W = 40, H = 32, G = 9, V = G * G, F = 2 * (G - 1) * (G - 1);
  const float camera[6] = {64.f, 64.f, 16.f, 12.f, 0.01f, 3.f}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, -1};
  const float lights[4] = {0, 0, 1, 0.5f}, base[3] = {0.3f, 0.3f, 0.3f}, background[3] = {1, 1, 1};
  // snapped coordinates: a grid of 5-pixel cells from (-2, -3) pixels, jittered by up to +-1.5 pixels (cells keep their orientation),
  // some of it left of and above the viewport, some of it past the right edge
  std::vector<long long> X(V), Y(V);
  std::vector<float> pos(3 * V);
  srand(20261020);
  for (int r = 0; r < G; ++r)
    for (int c = 0; c < G; ++c) {
      const int v = r * G + c;
      X[v] = 256 * (5 * c - 2) + (rand() % 769) - 384;
      Y[v] = 256 * (5 * r - 3) + (rand() % 769) - 384;
      if (r == 4 && c == 4) { X[v] = 256 * 18 + 128; Y[v] = 256 * 17 + 128; }      // a vertex on a pixel centre
      pos[3 * v] = ((float)X[v] / 256.f - camera[2]) / camera[0];                   // exact: sx = fx x + cx, sy = cy - fy y
      pos[3 * v + 1] = (camera[3] - (float)Y[v] / 256.f) / camera[1];
      pos[3 * v + 2] = 0.f;
    }
  std::vector<int> faces;
  for (int r = 0; r + 1 < G; ++r)
    for (int c = 0; c + 1 < G; ++c) {
      const int a = r * G + c;
      const int q[6] = {a, a + 1, a + G, a + 1, a + G + 1, a + G};
      faces.insert(faces.end(), q, q + 6);
    }
  // the rule, in 64-bit ints
  std::vector<int> want(W * H, -1);
  for (int f = 0; f < F; ++f) {
    int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const long long A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a]);
    if (A == 0) continue;
    if (A < 0) { const int s = b; b = c; c = s; }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const long long px = 256 * x + 128, py = 256 * y + 128;
        if (inside(X[b], Y[b], X[c], Y[c], px, py) && inside(X[c], Y[c], X[a], Y[a], px, py) && inside(X[a], Y[a], X[b], Y[b], px, py)) {
          if (want[y * W + x] != -1) { printf("FAIL: the program's own rule covers pixel (%d, %d) twice (faces %d and %d)\n", x, y, want[y * W + x], f); return 1; }
          want[y * W + x] = f;
        }
      }
  }
  int covered = 0;
  for (int i = 0; i < W * H; ++i) covered += want[i] >= 0;

  hipStream_t st;
  HK(hipStreamCreate(&st));
  float* d_pos = nullptr;
  unsigned char* d_rgb = nullptr;
  int* d_face = nullptr;
  HK(hipMalloc(&d_pos, pos.size() * 4));
  HK(hipMalloc(&d_rgb, (size_t)W * H * 3));
  HK(hipMalloc(&d_face, (size_t)W * H * 4));
  HK(hipMemcpy(d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
  HK(hipMemset(d_rgb, 0x5a, (size_t)W * H * 3));
  HK(hipMemset(d_face, 0x5a, (size_t)W * H * 4));
  fdm_render* r = nullptr;
  // refusals come back as codes
  if (fdm_render_create(faces.data(), F, V, 0, H, camera, R, t, lights, 1, 0.2f, base, background, &r) != FDM_ERR_ARG || r) { printf("FAIL: W = 0 accepted\n"); return 1; }
  if (fdm_render_create(faces.data(), F, V - 1, W, H, camera, R, t, lights, 1, 0.2f, base, background, &r) != FDM_ERR_ARG || r) { printf("FAIL: a face index out of range accepted\n"); return 1; }
  CK(fdm_render_create(faces.data(), F, V, W, H, camera, R, t, lights, 1, 0.2f, base, background, &r));
  const int one = 1;
  int got_frames = -1;
  if (fdm_render_forward(r, d_pos, &one, 1, 1, nullptr, 1, 0.0, 0.0, nullptr, d_rgb, nullptr, d_face, 1, &got_frames, st) != FDM_ERR_ARG) { printf("FAIL: a null template accepted\n"); return 1; }
  CK(fdm_render_set(r, "chunk_frames", 1));
  CK(fdm_render_forward(r, d_pos, &one, 1, 1, nullptr, 0, 0.0, 0.0, nullptr, d_rgb, nullptr, d_face, 1, &got_frames, st));
  HK(hipStreamSynchronize(st));
  std::vector<int> face(W * H);
  std::vector<unsigned char> rgb((size_t)W * H * 3);
  HK(hipMemcpy(face.data(), d_face, face.size() * 4, hipMemcpyDeviceToHost));
  HK(hipMemcpy(rgb.data(), d_rgb, rgb.size(), hipMemcpyDeviceToHost));
  if (got_frames != 1) { printf("FAIL: %d frames out\n", got_frames); return 1; }
  for (int i = 0; i < W * H; ++i) {
    if (face[i] != want[i]) { printf("FAIL: pixel (%d, %d) shows face %d, the rule says %d\n", i % W, i / W, face[i], want[i]); return 1; }
    // a plane facing the camera under one head-on light: (int)(255 * 0.3 * (0.2 + 0.5) + 0.5) = 54; the background is white
    const int shade = want[i] >= 0 ? 54 : 255;
    if (rgb[3 * i] != shade || rgb[3 * i + 1] != shade || rgb[3 * i + 2] != shade) { printf("FAIL: pixel (%d, %d) has colour %d %d %d, expected %d\n", i % W, i / W, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], shade); return 1; }
  }
  CK(fdm_render_destroy(r));
  HK(hipFree(d_pos)); HK(hipFree(d_rgb)); HK(hipFree(d_face));
  printf("render_client ok (%d faces, %d x %d pixels, %d covered, libfdm_hip version %d)\n", F, W, H, covered, fdm_version());
  return 0;
}
