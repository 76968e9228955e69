// Host side of the render hand-off's materials under AddressSanitizer + UBSan, as a stand-alone CPU program (no GPU, no Python): the
// refusals of fdm_render_set_material on an object without a device, each a code and a message, with every array sized exactly (a read
// past one is the sanitizer's to find), and the scalars rules of fdm_render_forward_material and of the two older calls
// (csrc/render_out.hip, with the mesh unit it calls); the two symbols those units take from fdm_hip.hip are supplied here (no device is
// ever reported).
//   cd face-diffusion-model_amd/csrc && /opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
//     -x hip ../../tools/render_material_host_check.cpp render_out.hip mesh_out.hip -o ../../tools/_build/render_material_host_check
//   ../../tools/_build/render_material_host_check          -> "render_material_host_check ok", exit status 0
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/fdm_hip.h"

namespace fdm {
static std::string g_err;
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace fdm
extern "C" int fdm_device_ok(void) { return 0; }

#define EXPECT(cond) do { if (!(cond)) { printf("FAIL line %d: %s (last error: %s)\n", __LINE__, #cond, fdm::g_err.c_str()); return 1; } } while (0)
// the call is refused with `code` and a message that holds `word`
#define REFUSED_AS(call, code, word) do { fdm::g_err.clear(); EXPECT((call) == (code)); EXPECT(fdm::g_err.find(word) != std::string::npos); } while (0)
#define REFUSED(call, word) REFUSED_AS(call, FDM_ERR_ARG, word)

static const int V = 4, F = 2;
static int make(fdm_render** out) {
  static const int faces[6] = {0, 1, 2, 0, 2, 3};
  static const float cam[6] = {48.f, 48.f, 16.f, 16.f, 0.01f, 3.f}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, -1};
  static const float light[4] = {0.f, 0.6f, 0.8f, 0.25f}, base[3] = {0.3f, 0.3f, 0.3f}, bg[3] = {1.f, 1.f, 1.f};
  return fdm_render_create(faces, F, V, 32, 32, cam, R, t, light, 1, 0.2f, base, bg, out);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  fdm_render* r = nullptr;
  EXPECT(make(&r) == FDM_OK && r != nullptr);
  // exactly sized arrays on the heap
  std::vector<float> colors((size_t)V * 3, 0.5f), lut2(2 * 3, 0.25f), lut1024(1024 * 3, 1.f), uv((size_t)F * 3 * 2, nan);      // (uv: any bits)
  std::vector<unsigned char> tex1(1 * 1 * 3, 200), tex53(5 * 3 * 3, 7);
  fdm_render_material none;
  std::memset(&none, 0, sizeof(none));
  fdm_render_material m = none;

  // what is accepted (validated; nothing is uploaded without a device)
  EXPECT(fdm_render_set_material(r, nullptr) == FDM_OK && fdm_render_set_material(r, &none) == FDM_OK);
  m = none; m.unlit = 1;
  EXPECT(fdm_render_set_material(r, &m) == FDM_OK);
  m = none; m.kind = 1; m.colors = colors.data();
  EXPECT(fdm_render_set_material(r, &m) == FDM_OK);
  m = none; m.kind = 2; m.lut = lut2.data(); m.n_lut = 2; m.lo = -1.f; m.hi = 1.f;
  EXPECT(fdm_render_set_material(r, &m) == FDM_OK);
  m.lut = lut1024.data(); m.n_lut = 1024;
  EXPECT(fdm_render_set_material(r, &m) == FDM_OK);
  m = none; m.kind = 3; m.uv = uv.data(); m.texture = tex1.data(); m.tex_w = 1; m.tex_h = 1;
  EXPECT(fdm_render_set_material(r, &m) == FDM_OK);
  m.texture = tex53.data(); m.tex_w = 5; m.tex_h = 3; m.filter = 1;
  EXPECT(fdm_render_set_material(r, &m) == FDM_OK);
  const fdm_render_material tex_ok = m;

  // the refusals
  REFUSED(fdm_render_set_material(nullptr, &none), "null object");
  for (int kind : {-1, 4, 100}) { m = none; m.kind = kind; REFUSED(fdm_render_set_material(r, &m), "kind"); }
  for (int unlit : {-1, 2}) { m = none; m.unlit = unlit; REFUSED(fdm_render_set_material(r, &m), "unlit"); }
  m = none; m.kind = 1;
  REFUSED(fdm_render_set_material(r, &m), "null colors");
  m = none; m.kind = 2; m.n_lut = 2; m.hi = 1.f;
  REFUSED(fdm_render_set_material(r, &m), "null lut");
  m = tex_ok; m.uv = nullptr;
  REFUSED(fdm_render_set_material(r, &m), "null uv or texture");
  m = tex_ok; m.texture = nullptr;
  REFUSED(fdm_render_set_material(r, &m), "null uv or texture");
  for (int n : {-1, 0, 1, 1025}) {
    m = none; m.kind = 2; m.lut = lut2.data(); m.n_lut = n; m.hi = 1.f;
    REFUSED(fdm_render_set_material(r, &m), "n_lut");
  }
  const int sizes[5][2] = {{0, 3}, {5, 0}, {8193, 3}, {5, 8193}, {-5, -3}};
  for (const int* s : sizes) { m = tex_ok; m.tex_w = s[0]; m.tex_h = s[1]; REFUSED(fdm_render_set_material(r, &m), "texture of"); }
  for (int flt : {-1, 2}) { m = tex_ok; m.filter = flt; REFUSED(fdm_render_set_material(r, &m), "filter"); }
  const float ranges[6][2] = {{1.f, 1.f}, {2.f, 1.f}, {nan, 1.f}, {0.f, inf}, {-inf, 0.f}, {-3e38f, 3e38f}};
  for (const float* q : ranges) {
    m = none; m.kind = 2; m.lut = lut2.data(); m.n_lut = 2; m.lo = q[0]; m.hi = q[1];
    REFUSED(fdm_render_set_material(r, &m), "range");
  }
  for (float bad : {-0.25f, nan, inf}) {
    std::vector<float> c = colors, t = lut2;
    c.back() = bad;                       // the last element of each array: all of it is read
    t.back() = bad;
    m = none; m.kind = 1; m.colors = c.data();
    REFUSED(fdm_render_set_material(r, &m), "colors[3][2]");
    m = none; m.kind = 2; m.lut = t.data(); m.n_lut = 2; m.hi = 1.f;
    REFUSED(fdm_render_set_material(r, &m), "lut[1][2]");
  }

  // a refused set leaves the object as it was; scalars go with kind 2 and with no other (no pointer is dereferenced)
  const float* x = (const float*)0x1000;
  const float* sc = (const float*)0x3000;
  fdm_render_planes out = {(unsigned char*)0x2000, nullptr, nullptr, nullptr, nullptr};
  EXPECT(fdm_render_set_material(r, &tex_ok) == FDM_OK);
  m = none; m.kind = 2; m.lut = lut2.data(); m.n_lut = 1;
  REFUSED(fdm_render_set_material(r, &m), "n_lut");
  REFUSED_AS(fdm_render_forward(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, out.rgb, nullptr, nullptr, 1, nullptr, nullptr), FDM_ERR_STATE, "no gfx950 device");
  REFUSED(fdm_render_forward_material(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, &out, 1, nullptr, nullptr, sc), "scalars on an object");
  REFUSED_AS(fdm_render_forward_material(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, &out, 1, nullptr, nullptr, nullptr), FDM_ERR_STATE, "no gfx950 device");
  REFUSED(fdm_render_forward_material(nullptr, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, &out, 1, nullptr, nullptr, nullptr), "null");
  REFUSED(fdm_render_forward_material(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, nullptr, 1, nullptr, nullptr, nullptr), "null");
  m = none; m.kind = 2; m.lut = lut2.data(); m.n_lut = 2; m.hi = 1.f;
  EXPECT(fdm_render_set_material(r, &m) == FDM_OK);
  REFUSED(fdm_render_forward_material(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, &out, 1, nullptr, nullptr, nullptr), "null scalars");
  REFUSED_AS(fdm_render_forward(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, out.rgb, nullptr, nullptr, 1, nullptr, nullptr), FDM_ERR_STATE, "scalar-map");
  REFUSED_AS(fdm_render_forward_planes(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, &out, 1, nullptr, nullptr), FDM_ERR_STATE, "scalar-map");
  REFUSED_AS(fdm_render_forward_material(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, &out, 1, nullptr, nullptr, sc), FDM_ERR_STATE, "no gfx950 device");
  EXPECT(fdm_render_set_material(r, nullptr) == FDM_OK);
  REFUSED_AS(fdm_render_forward_planes(r, x, nullptr, 1, 1, nullptr, 0, 0, 0, nullptr, &out, 1, nullptr, nullptr), FDM_ERR_STATE, "no gfx950 device");
  EXPECT(fdm_render_destroy(r) == FDM_OK);

  REFUSED(fdm_op_vertex_dist(nullptr, x, (float*)0x2000, 1, 1, nullptr), "null");
  REFUSED_AS(fdm_op_vertex_dist(x, x, (float*)0x2000, 0, 1, nullptr), FDM_ERR_SHAPE, "rows = 0");
  REFUSED_AS(fdm_op_vertex_dist(x, x, (float*)0x2000, 1, 1, nullptr), FDM_ERR_STATE, "no gfx950 device");
  printf("render_material_host_check ok\n");
  return 0;
}
