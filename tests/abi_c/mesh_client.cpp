// Quantised latent to renderer-ready frames without Python or torch: fdm_vq_decode_ragged -> fdm_mesh_forward (template add, time
// resampling, vertex normals) for two clips of unequal length, compared bit for bit with the positions and normals passed in.  The
// decoder's weights arrive by state-dict name from a flat record file; the case file holds the geometry, the inputs and the expected
// outputs.  Built and run by tests/test_mesh_out_gpu.py:
//   hipcc mesh_client.cpp -I include -L <dir> -lfdm_hip ; mesh_client weights.bin case.bin
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fdm_hip.h"

#define CK(x) do { if ((x) != 0) { printf("FAIL %s: %s\n", #x, fdm_last_error()); return 1; } } while (0)
#define HK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <typename T> static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 3) { printf("usage: mesh_client weights.bin case.bin\n"); return 2; }
  if (!fdm_device_ok()) { printf("no gfx950 device\n"); return 2; }
  hipStream_t st;
  HK(hipStreamCreate(&st));

  FILE* f = fopen(argv[2], "rb");
  if (!f) { printf("cannot open %s\n", argv[2]); return 2; }
  int hd[14];
  double fps[2];
  int want_frames[2];
  if (fread(hd, 4, 14, f) != 14 || fread(fps, 8, 2, f) != 2 || fread(want_frames, 4, 2, f) != 2) { printf("truncated case header\n"); return 2; }
  const fdm_vq_desc desc = {hd[0], hd[1], hd[2], hd[3], hd[4], hd[5]};
  const int dtype = hd[6], B = hd[7], L_max = hd[8], F = hd[11], V = hd[12], Lo_max = hd[13];
  const int frames[2] = {hd[9], hd[10]};
  if (B != 2 || desc.V3 != 3 * V) { printf("bad case file\n"); return 2; }
  const size_t R = (size_t)L_max * desc.G, n_out = (size_t)B * Lo_max * V * 3;
  std::vector<float> zq, tmpl, want_pos, want_nrm;
  std::vector<int> faces;
  if (!rd(f, zq, B * desc.c * R) || !rd(f, tmpl, (size_t)B * 3 * V) || !rd(f, faces, (size_t)F * 3) || !rd(f, want_pos, n_out) || !rd(f, want_nrm, n_out)) {
    printf("truncated case file\n");
    return 2;
  }
  fclose(f);

  fdm_vq* vq = nullptr;
  CK(fdm_vq_create(&desc, dtype, &vq));
  f = fopen(argv[1], "rb");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  int n_weights = 0;
  for (;;) {
    unsigned nl = 0;
    if (fread(&nl, 4, 1, f) != 1) break;
    std::string name(nl, '\0');
    unsigned long long cnt = 0;
    if (fread(&name[0], 1, nl, f) != nl || fread(&cnt, 8, 1, f) != 1) { printf("truncated record\n"); return 2; }
    std::vector<float> v(cnt);
    if (fread(v.data(), 4, cnt, f) != cnt) { printf("truncated record %s\n", name.c_str()); return 2; }
    CK(fdm_vq_set_weights(vq, name.c_str(), v.data(), (long long)cnt, st));
    HK(hipStreamSynchronize(st));          // (v is host memory that goes away)
    ++n_weights;
  }
  fclose(f);

  float *d_zq = nullptr, *d_off = nullptr, *d_tmpl = nullptr, *d_pos = nullptr, *d_nrm = nullptr;
  HK(hipMalloc(&d_zq, zq.size() * 4));
  HK(hipMalloc(&d_off, (size_t)B * L_max * 3 * V * 4));
  HK(hipMalloc(&d_tmpl, tmpl.size() * 4));
  HK(hipMalloc(&d_pos, n_out * 4));
  HK(hipMalloc(&d_nrm, n_out * 4));
  HK(hipMemcpy(d_zq, zq.data(), zq.size() * 4, hipMemcpyHostToDevice));
  HK(hipMemcpy(d_tmpl, tmpl.data(), tmpl.size() * 4, hipMemcpyHostToDevice));
  HK(hipMemset(d_pos, 0xff, n_out * 4));          // NaN everywhere: the call writes both outputs whole
  HK(hipMemset(d_nrm, 0xff, n_out * 4));

  fdm_mesh* m = nullptr;
  CK(fdm_mesh_create(faces.data(), F, V, &m));
  int got_frames[2] = {0, 0};
  // refusals come back as codes, before any launch
  if (fdm_mesh_forward(m, d_off, frames, B, L_max, d_tmpl, 3, fps[0], fps[1], FDM_MESH_NORMALS, d_pos, d_nrm, Lo_max, got_frames, st) != FDM_ERR_ARG) { printf("FAIL: tmpl_rows = 3 accepted\n"); return 1; }
  if (fdm_mesh_forward(m, d_off, frames, B, L_max, d_tmpl, B, fps[0], fps[1], FDM_MESH_NORMALS | 32, d_pos, d_nrm, Lo_max, got_frames, st) != FDM_ERR_ARG) { printf("FAIL: unknown flag accepted\n"); return 1; }
  if (fdm_mesh_forward(m, d_off, frames, B, L_max, d_tmpl, B, fps[0], fps[1], FDM_MESH_NORMALS, d_pos, d_nrm, Lo_max - 1, got_frames, st) != FDM_ERR_SHAPE) { printf("FAIL: an output too short accepted\n"); return 1; }
  if (got_frames[0] != 0 || got_frames[1] != 0) { printf("FAIL: a refused call wrote lengths\n"); return 1; }

  CK(fdm_vq_decode_ragged(vq, d_zq, frames, B, (int)R, d_off, st));
  CK(fdm_mesh_forward(m, d_off, frames, B, L_max, d_tmpl, B, fps[0], fps[1], FDM_MESH_NORMALS, d_pos, d_nrm, Lo_max, got_frames, st));
  HK(hipStreamSynchronize(st));
  std::vector<float> pos(n_out), nrm(n_out);
  HK(hipMemcpy(pos.data(), d_pos, n_out * 4, hipMemcpyDeviceToHost));
  HK(hipMemcpy(nrm.data(), d_nrm, n_out * 4, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    int lo = 0;
    CK(fdm_mesh_frames(frames[b], fps[0], fps[1], &lo));
    if (got_frames[b] != want_frames[b] || lo != want_frames[b]) { printf("FAIL: clip %d: %d frames out (fdm_mesh_frames: %d), expected %d\n", b, got_frames[b], lo, want_frames[b]); return 1; }
  }
  if (memcmp(pos.data(), want_pos.data(), n_out * 4) != 0) { printf("FAIL: positions differ from the values passed in\n"); return 1; }
  if (memcmp(nrm.data(), want_nrm.data(), n_out * 4) != 0) { printf("FAIL: normals differ from the values passed in\n"); return 1; }
  CK(fdm_mesh_destroy(m));
  CK(fdm_vq_destroy(vq));
  HK(hipFree(d_zq)); HK(hipFree(d_off)); HK(hipFree(d_tmpl)); HK(hipFree(d_pos)); HK(hipFree(d_nrm));
  printf("mesh_client ok (%d weights, %d + %d frames -> %d + %d, libfdm_hip version %d)\n", n_weights, frames[0], frames[1], got_frames[0], got_frames[1], fdm_version());
  return 0;
}
