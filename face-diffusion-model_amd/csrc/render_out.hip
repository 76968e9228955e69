// Render hand-off behind plain C calls (include/fdm_hip.h, fdm_render_*): positions as the mesh, wrap and head hand-offs write them ->
// shaded image frames, a depth image and a face-id image.  Kernels: render_out.hpp.  fdm_render_create checks and uploads the topology
// and keeps the view on the host (it travels to the kernels as an argument, so fdm_render_set_view touches no device memory); a forward
// call validates (every check before the first launch), lists the live output frames, grows the scratch to one chunk of them and loops
// over the chunks on the caller's stream.  The vertex normals are the mesh hand-off's own: an internal fdm_mesh over the same faces runs
// mesh_nrm_kernel on each chunk's positions, unless the caller brings normals.  A material (fdm_render_set_material, DESIGN item 25) is
// state of the object: its tables are checked and uploaded at set, and a forward call then launches the MAT instance of the resolve kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "host.hpp"
#include "render_out.hpp"

struct fdm_render : fdm::Handoff {        // lens: {L, L_out} per clip
  int F = 0, V = 0, W = 0, H = 0;
  long long chunk_frames = 0;             // 0: the default (scratch under RENDER_SCRATCH_BYTES)
  int samples = 1;                        // coverage samples per pixel: 1, 4 or 16
  int yuv_matrix = 709, yuv_range = 0, yuv_layout = 0;      // fdm_render_set "yuv_*": 601 | 709, 0 limited | 1 full, 0 I420 | 1 NV12
  fdm::RenderView view;
  fdm_mesh* mesh = nullptr;               // the normals of a chunk (fdm_mesh_forward on the chunk's positions)
  int* faces = nullptr;                   // device [F][3]
  int2* rowtab = nullptr;                 // device: the call's live rows {clip, output frame}
  float *P = nullptr, *N = nullptr;       // device scratch of one chunk: [n][3V] each
  int4* xyw = nullptr;                    // [n][V]
  float4* nc = nullptr;                   // [n][V]
  unsigned long long* vis = nullptr;      // [n][H][W][samples], zero between calls (the resolve kernel leaves it so)
  long long rowtab_cap = 0, P_cap = 0, N_cap = 0, xyw_cap = 0, nc_cap = 0, vis_cap = 0;
  std::vector<int2> rows;                 // host: the live rows of the call in flight (the asynchronous upload reads it)
  bool vis_dirty = false;                 // a call ended between raster and resolve: clear before the next use
  // the material (fdm_render_set_material): kind 0 and unlit 0 is none, and the call runs the MAT = false kernels
  int mat_kind = 0, mat_unlit = 0, n_lut = 0, tex_w = 0, tex_h = 0, tex_filter = 0;
  float mat_lo = 0.f, mat_span = 1.f;     // kind 2: span = hi - lo, rounded once
  float* colors = nullptr;                // device [V][3]
  float4* lut = nullptr;                  // device [n_lut] {r, g, b, 0}
  float2* uv = nullptr;                   // device [F][3]
  uchar4* tex = nullptr;                  // device [tex_h][tex_w] {r, g, b, 0}
  float* u = nullptr;                     // device scratch of one chunk, kind 2: [n][V]
  long long u_cap = 0;
};

namespace {
using namespace fdm;

constexpr long long RENDER_SCRATCH_BYTES = 256LL << 20;
constexpr long long RENDER_CHUNK_MAX = 4096;      // rows of one launch (grid y <= 65535)
constexpr long long RENDER_FRAME_KEYS_MAX = 1LL << 26;      // W H samples of one frame: 512 MB of keys (4096^2 at 4 samples, 2048^2 at 16)

bool finite_all(const float* x, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

// camera [6] = {fx, fy, cx, cy, near, far}, R [9] row-major world -> camera, t [3], lights [n][4] = {unit direction towards the light
// in camera space, intensity}: checked, then written into `vw` (untouched on a refusal)
int check_view(const char* who, const float* camera, const float* R, const float* t, const float* lights, int n_lights, float ambient,
               RenderView& vw) {
  if (!camera || !R || !t) return fail(FDM_ERR_ARG, "%s: null camera, R or t", who);
  if (!finite_all(camera, 6) || !finite_all(R, 9) || !finite_all(t, 3)) return fail(FDM_ERR_ARG, "%s: a non-finite camera number", who);
  if (!(camera[0] > 0.f) || !(camera[1] > 0.f)) return fail(FDM_ERR_ARG, "%s: focal lengths %g, %g (> 0)", who, (double)camera[0], (double)camera[1]);
  if (!(camera[4] > 0.f) || !(camera[4] < camera[5])) return fail(FDM_ERR_ARG, "%s: near = %g, far = %g (0 < near < far)", who, (double)camera[4], (double)camera[5]);
  if (n_lights < 0 || n_lights > RENDER_MAX_LIGHTS) return fail(FDM_ERR_ARG, "%s: %d lights (0 .. %d)", who, n_lights, RENDER_MAX_LIGHTS);
  if (n_lights && !lights) return fail(FDM_ERR_ARG, "%s: %d lights with a null array", who, n_lights);
  if (!(ambient >= 0.f) || !std::isfinite(ambient)) return fail(FDM_ERR_ARG, "%s: ambient = %g (finite, >= 0)", who, (double)ambient);
  for (int l = 0; l < n_lights; ++l) {
    const float* q = lights + 4 * l;
    if (!finite_all(q, 4) || !(q[3] >= 0.f)) return fail(FDM_ERR_ARG, "%s: light %d is not finite or has a negative intensity", who, l);
    const double n2 = (double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2];
    if (std::fabs(n2 - 1.0) > 1e-4) return fail(FDM_ERR_ARG, "%s: the direction of light %d has squared length %g (a unit vector)", who, l, n2);
  }
  vw.fx = camera[0]; vw.fy = camera[1]; vw.cx = camera[2]; vw.cy = camera[3]; vw.znear = camera[4]; vw.zfar = camera[5];
  std::memcpy(vw.R, R, sizeof(vw.R));
  std::memcpy(vw.t, t, sizeof(vw.t));
  vw.n_lights = n_lights;
  std::memset(vw.dir, 0, sizeof(vw.dir));
  std::memset(vw.intensity, 0, sizeof(vw.intensity));
  for (int l = 0; l < n_lights; ++l) {
    for (int k = 0; k < 3; ++k) vw.dir[l][k] = lights[4 * l + k];
    vw.intensity[l] = lights[4 * l + 3];
  }
  vw.ambient = ambient;
  return FDM_OK;
}

long long frame_bytes(const fdm_render& R) {
  return (long long)R.V * (12 + 12 + 16 + 16 + (R.mat_kind == 2 ? 4 : 0)) + (long long)R.W * R.H * R.samples * 8;
}

template <int S> void sample_pattern(int* xy) {
  for (int s = 0; s < S; ++s) render_sample_offset<S>(s, xy[2 * s], xy[2 * s + 1]);
}

}  // namespace

extern "C" {

int fdm_render_create(const int* faces, int F, int V, int W, int H, const float* camera, const float* R, const float* t, const float* lights,
                      int n_lights, float ambient, const float* base, const float* background, fdm_render** out) {
  if (!out) return fail(FDM_ERR_ARG, "render_create: null out");
  if (!faces || !base || !background) return fail(FDM_ERR_ARG, "render_create: null faces, base or background");
  if (F < 1 || V < 1) return fail(FDM_ERR_ARG, "render_create: F = %d, V = %d", F, V);
  if (F > 0x7fffffff / 3 || V > 0x7fffffff / 6) return fail(FDM_ERR_ARG, "render_create: F = %d, V = %d (3 F and 6 V are 32-bit ints)", F, V);
  if (W < 1 || W > 4096 || H < 1 || H > 4096) return fail(FDM_ERR_ARG, "render_create: a viewport of %d x %d (1 .. 4096 each)", W, H);
  for (long long i = 0; i < 3LL * F; ++i)
    if (faces[i] < 0 || faces[i] >= V) return fail(FDM_ERR_ARG, "render_create: face %lld names vertex %d of %d", i / 3, faces[i], V);
  for (int k = 0; k < 3; ++k) {
    if (!(base[k] >= 0.f) || !std::isfinite(base[k])) return fail(FDM_ERR_ARG, "render_create: base[%d] = %g (finite, >= 0)", k, (double)base[k]);
    if (!(background[k] >= 0.f && background[k] <= 1.f)) return fail(FDM_ERR_ARG, "render_create: background[%d] = %g (in [0, 1])", k, (double)background[k]);
  }
  RenderView vw;
  std::memset(&vw, 0, sizeof(vw));
  FCK(check_view("render_create", camera, R, t, lights, n_lights, ambient, vw));
  for (int k = 0; k < 3; ++k) { vw.base[k] = base[k]; vw.background[k] = background[k]; }
  fdm_render* r = new (std::nothrow) fdm_render();
  if (!r) return fail(FDM_ERR_STATE, "render_create: out of memory");
  r->F = F; r->V = V; r->W = W; r->H = H; r->view = vw;
  const int rc = fdm_mesh_create(faces, F, V, &r->mesh);
  if (rc != FDM_OK) { delete r; return rc; }
  fdm_mesh* m = r->mesh;
  const int rf = handoff_finish(r, out, [&]() { return put(r->mem, &r->faces, faces, (size_t)F * 3); });
  if (rf != FDM_OK) (void)fdm_mesh_destroy(m);      // (handoff_finish has deleted r)
  return rf;
}

int fdm_render_destroy(fdm_render* r) {
  if (!r) return FDM_OK;
  fdm_mesh* m = r->mesh;
  (void)handoff_destroy(r);                         // (waits for the device)
  return fdm_mesh_destroy(m);
}

int fdm_render_set_view(fdm_render* r, const float* camera, const float* R, const float* t, const float* lights, int n_lights, float ambient) {
  if (!r) return fail(FDM_ERR_ARG, "render_set_view: null argument");
  RenderView vw = r->view;
  FCK(check_view("render_set_view", camera, R, t, lights, n_lights, ambient, vw));
  r->view = vw;
  return FDM_OK;
}

int fdm_render_set(fdm_render* r, const char* key, long long value) {
  if (!r || !key) return fail(FDM_ERR_ARG, "render_set: null argument");
  if (std::strcmp(key, "samples") == 0) {
    if (value != 1 && value != 4 && value != 16) return fail(FDM_ERR_ARG, "render_set: samples = %lld (1, 4 or 16)", value);
    if ((long long)r->W * r->H * value > RENDER_FRAME_KEYS_MAX)
      return fail(FDM_ERR_ARG, "render_set: samples = %lld on %d x %d pixels is %lld keys per frame (at most 2^26; samples is 1, 4 or 16)", value, r->W,
                  r->H, (long long)r->W * r->H * value);
    r->samples = (int)value;
    return FDM_OK;
  }
  if (std::strcmp(key, "yuv_matrix") == 0) {
    if (value != 601 && value != 709) return fail(FDM_ERR_ARG, "render_set: yuv_matrix = %lld (601 or 709)", value);
    r->yuv_matrix = (int)value;
    return FDM_OK;
  }
  if (std::strcmp(key, "yuv_range") == 0) {
    if (value != 0 && value != 1) return fail(FDM_ERR_ARG, "render_set: yuv_range = %lld (0 limited, 1 full)", value);
    r->yuv_range = (int)value;
    return FDM_OK;
  }
  if (std::strcmp(key, "yuv_layout") == 0) {
    if (value != 0 && value != 1) return fail(FDM_ERR_ARG, "render_set: yuv_layout = %lld (0 I420, 1 NV12)", value);
    r->yuv_layout = (int)value;
    return FDM_OK;
  }
  if (std::strcmp(key, "chunk_frames") != 0)
    return fail(FDM_ERR_ARG, "render_set: unknown key %s (chunk_frames, samples, yuv_matrix, yuv_range, yuv_layout)", key);
  if (value < 0 || value > RENDER_CHUNK_MAX) return fail(FDM_ERR_ARG, "render_set: chunk_frames = %lld (0 = the default, at most %lld)", value, RENDER_CHUNK_MAX);
  r->chunk_frames = value;
  return FDM_OK;
}

int fdm_render_sample_pattern_host(int samples, int* xy) {
  if (!xy) return fail(FDM_ERR_ARG, "render_sample_pattern_host: null xy");
  if (samples == 1) sample_pattern<1>(xy);
  else if (samples == 4) sample_pattern<4>(xy);
  else if (samples == 16) sample_pattern<16>(xy);
  else return fail(FDM_ERR_ARG, "render_sample_pattern_host: samples = %d (1, 4 or 16)", samples);
  return FDM_OK;
}

int fdm_render_yuv_coeffs_host(int matrix, int full_range, int* coeffs) {
  if (!coeffs) return fail(FDM_ERR_ARG, "render_yuv_coeffs_host: null coeffs");
  if (matrix != 601 && matrix != 709) return fail(FDM_ERR_ARG, "render_yuv_coeffs_host: matrix = %d (601 or 709)", matrix);
  const double Kr = matrix == 601 ? 0.299 : 0.2126, Kb = matrix == 601 ? 0.114 : 0.0722;
  const double sy = full_range ? 1.0 : 219.0 / 255.0, sc = full_range ? 1.0 : 224.0 / 255.0;
  auto q = [](double x) { return (int)std::floor(65536.0 * x + 0.5); };
  const int yr = q(Kr * sy), yb = q(Kb * sy), yg = q(sy) - yr - yb;      // the green terms from the other two: every grey is exact
  const int ub = q(sc / 2.0), ur = q(-Kr * sc / (2.0 * (1.0 - Kb))), ug = -(ur + ub);
  const int vr = q(sc / 2.0), vb = q(-Kb * sc / (2.0 * (1.0 - Kr))), vg = -(vr + vb);
  const int all[10] = {yr, yg, yb, ur, ug, ub, vr, vg, vb, full_range ? 0 : 16};
  std::memcpy(coeffs, all, sizeof(all));
  return FDM_OK;
}

}  // extern "C"

namespace {

// raster and resolve of a chunk of n rows at S samples per pixel; with yuv one resolve lane per 2 x 2 block of pixels
template <int S> void launch_raster_resolve(const fdm_render* r, int n, const int2* tab, int L_out_max, const RenderOut& out, const RenderYuv& yc,
                                            hipStream_t s) {
  const auto blocks = [](long long lanes) { return (unsigned)((lanes + RENDER_TB - 1) / RENDER_TB); };
  const long long WH = (long long)r->W * r->H;
  hipLaunchKernelGGL(render_raster_kernel<S>, dim3(blocks(r->F), (unsigned)n), dim3(RENDER_TB), 0, s, (const int4*)r->xyw, (const int*)r->faces, r->F,
                     r->V, r->W, r->H, r->vis);
  const dim3 grid(blocks(out.yuv ? WH / 4 : WH), (unsigned)n);
  if (!r->mat_kind && !r->mat_unlit) {    // no material: the kernels as they were
    const auto resolve = out.yuv ? render_resolve_kernel<S, true, false> : render_resolve_kernel<S, false, false>;
    hipLaunchKernelGGL(resolve, grid, dim3(RENDER_TB), 0, s, (const int4*)r->xyw, (const float4*)r->nc, (const int*)r->faces, r->F, r->V, r->W, r->H,
                       tab, L_out_max, r->view, r->vis, out, yc);
    return;
  }
  RenderMat mt;
  mt.kind = r->mat_kind; mt.unlit = r->mat_unlit;
  mt.colors = r->colors; mt.u = r->u; mt.lut = r->lut; mt.n_lut = r->n_lut;
  mt.uv = r->uv; mt.tex = reinterpret_cast<const unsigned*>(r->tex); mt.tex_w = r->tex_w; mt.tex_h = r->tex_h; mt.filter = r->tex_filter;
  const auto resolve = out.yuv ? render_resolve_kernel<S, true, true, RenderMat> : render_resolve_kernel<S, false, true, RenderMat>;
  hipLaunchKernelGGL(resolve, grid, dim3(RENDER_TB), 0, s, (const int4*)r->xyw, (const float4*)r->nc, (const int*)r->faces, r->F, r->V, r->W, r->H, tab,
                     L_out_max, r->view, r->vis, out, yc, mt);
}

// The body of fdm_render_forward (out.rgb set, alpha and yuv null) and of fdm_render_forward_planes: render_resolve_kernel writes
// whichever outputs are not null.  r, positions and the outputs have been checked by the caller.  scalars: the field of a scalar-map
// object [B][L_max][V] (fdm_render_forward_material), null on every other object; takes_scalars: the call has the argument at all.
int render_run(const char* who, fdm_render* r, const float* positions, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows,
               double fps_in, double fps_out, const float* normals, const RenderOut& out, int L_out_max, int* frames_out, void* stream,
               const float* scalars = nullptr, bool takes_scalars = false) {
  if (r->mat_kind == 2 && !takes_scalars)
    return fail(FDM_ERR_STATE, "%s: the object has a scalar-map material: fdm_render_forward_material brings the scalars", who);
  if (r->mat_kind == 2 && !scalars) return fail(FDM_ERR_ARG, "%s: null scalars on an object with a scalar-map material", who);
  if (r->mat_kind != 2 && scalars) return fail(FDM_ERR_ARG, "%s: scalars on an object whose material is of kind %d (a scalar map is kind 2)", who, r->mat_kind);
  if (tmpl_rows != 0 && tmpl_rows != 1 && tmpl_rows != B) return fail(FDM_ERR_ARG, "%s: tmpl_rows = %d (0, 1 or B = %d)", who, tmpl_rows, B);
  if (tmpl_rows && !tmpl) return fail(FDM_ERR_ARG, "%s: tmpl_rows = %d with a null template", who, tmpl_rows);
  FCK(check_fps(who, fps_in, fps_out));
  if (B < 1 || L_max < 1 || L_out_max < 1) return fail(FDM_ERR_SHAPE, "%s: B = %d, L_max = %d, L_out_max = %d", who, B, L_max, L_out_max);
  std::vector<int> hl;
  const ClipLens c = clip_lens(frames, B, L_max, fps_in, fps_out, L_out_max, hl);
  if (c.bad == ClipLens::LENGTH) return fail(FDM_ERR_SHAPE, "%s: clip %d has %d frames, the batch is %d long", who, c.clip, c.L, L_max);
  if (c.bad == ClipLens::OUTPUT) return fail(FDM_ERR_SHAPE, "%s: clip %d gives %lld frames, the output is %d long", who, c.clip, c.Lo, L_out_max);
  const long long V3 = 3LL * r->V, WH = (long long)r->W * r->H;
  if ((long long)B * L_out_max > 0x7fffffffLL || (V3 + RENDER_POS_TILE - 1) / RENDER_POS_TILE > 65535)
    return fail(FDM_ERR_SHAPE, "%s: %lld output rows of %d vertices exceed one launch", who, (long long)B * L_out_max, r->V);
  RenderYuv yc;
  std::memset(&yc, 0, sizeof(yc));
  if (out.yuv) {
    FCK(fdm_render_yuv_coeffs_host(r->yuv_matrix, r->yuv_range, yc.k));
    yc.nv12 = r->yuv_layout;
  }
  FCK(handoff_device(*r, who));
  hipStream_t s = (hipStream_t)stream;
  std::vector<int2>& rows = r->rows;      // the live output frames, in (clip, frame) order
  rows.clear();
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < hl[2 * b + 1]; ++t) rows.push_back(make_int2(b, t));
  const long long live = (long long)rows.size();
  long long chunk = r->chunk_frames ? r->chunk_frames : std::max(1LL, RENDER_SCRATCH_BYTES / frame_bytes(*r));
  chunk = std::min(std::min(chunk, RENDER_CHUNK_MAX), std::max(live, 1LL));
  FCK(grow(r->mem, &r->rowtab, &r->rowtab_cap, std::max(live, 1LL)));
  FCK(grow(r->mem, &r->P, &r->P_cap, chunk * V3));
  if (!normals) FCK(grow(r->mem, &r->N, &r->N_cap, chunk * V3));
  FCK(grow(r->mem, &r->xyw, &r->xyw_cap, chunk * r->V));
  FCK(grow(r->mem, &r->nc, &r->nc_cap, chunk * r->V));
  if (r->mat_kind == 2) FCK(grow(r->mem, &r->u, &r->u_cap, chunk * r->V));
  const long long vis_before = r->vis_cap;
  FCK(grow(r->mem, &r->vis, &r->vis_cap, chunk * WH * r->samples));
  if (r->vis_cap != vis_before || r->vis_dirty) {
    HIPCK(hipMemsetAsync(r->vis, 0, (size_t)r->vis_cap * sizeof(unsigned long long), s));
    r->vis_dirty = false;
  }
  FCK(handoff_lens(*r, hl, s));
  if (live) HIPCK(hipMemcpyAsync(r->rowtab, rows.data(), (size_t)live * sizeof(int2), hipMemcpyHostToDevice, s));
  // rows at or past a clip's L_out: zeros in every output
  for (int b = 0; b < B; ++b) {
    const long long lo = hl[2 * b + 1], n = (L_out_max - lo) * WH, at = ((long long)b * L_out_max + lo) * WH;
    if (!n) continue;
    if (out.rgb) HIPCK(hipMemsetAsync(out.rgb + 3 * at, 0, (size_t)(3 * n), s));
    if (out.depth) HIPCK(hipMemsetAsync(out.depth + at, 0, (size_t)n * sizeof(float), s));
    if (out.face) HIPCK(hipMemsetAsync(out.face + at, 0, (size_t)n * sizeof(int), s));
    if (out.alpha) HIPCK(hipMemsetAsync(out.alpha + at, 0, (size_t)n, s));
    if (out.yuv) HIPCK(hipMemsetAsync(out.yuv + at + at / 2, 0, (size_t)(n + n / 2), s));      // (W H is a multiple of 4 here)
  }
  const int rs = resamples(fps_in, fps_out) ? 1 : 0, tstride = tmpl_rows == B && B > 1 ? (int)V3 : 0;
  const float* tp = tmpl_rows ? tmpl : nullptr;
  const unsigned vblocks = (unsigned)((r->V + RENDER_TB - 1) / RENDER_TB);
  const auto raster_resolve = r->samples == 1 ? launch_raster_resolve<1> : r->samples == 4 ? launch_raster_resolve<4> : launch_raster_resolve<16>;
  for (long long r0 = 0; r0 < live; r0 += chunk) {
    const int n = (int)std::min(chunk, live - r0);
    const int2* tab = r->rowtab + r0;
    hipLaunchKernelGGL(render_pos_kernel, dim3((unsigned)n, (unsigned)((V3 + RENDER_POS_TILE - 1) / RENDER_POS_TILE)), dim3(256), 0, s, positions, tp,
                       tstride, (const int*)r->lens, tab, L_max, (int)V3, rs, r->P);
    if (!normals) {      // one clip of n frames, no template, no rates: positions in place, normals to N
      const int rc = fdm_mesh_forward(r->mesh, r->P, nullptr, 1, n, nullptr, 0, 0.0, 0.0, FDM_MESH_NORMALS, r->P, r->N, n, nullptr, stream);
      if (rc != FDM_OK) return rc;
    }
    hipLaunchKernelGGL(render_vertex_kernel, dim3(vblocks, (unsigned)n), dim3(RENDER_TB), 0, s, (const float*)r->P, normals ? normals : (const float*)r->N,
                       normals ? tab : (const int2*)nullptr, L_out_max, r->V, r->view, r->xyw, r->nc);
    if (r->mat_kind == 2)
      hipLaunchKernelGGL(render_scalar_kernel, dim3(vblocks, (unsigned)n), dim3(RENDER_TB), 0, s, scalars, (const int*)r->lens, tab, L_max, r->V, rs,
                         r->mat_lo, r->mat_span, r->u);
    r->vis_dirty = true;
    raster_resolve(r, n, tab, L_out_max, out, yc, s);
    HIPCK(hipGetLastError());
    r->vis_dirty = false;
  }
  if (frames_out) for (int b = 0; b < B; ++b) frames_out[b] = hl[2 * b + 1];
  return FDM_OK;
}

// The planes form behind fdm_render_forward_planes and fdm_render_forward_material: the checks of the output set, written once.
int render_planes_run(const char* who, fdm_render* r, const float* positions, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows,
                      double fps_in, double fps_out, const float* normals, const fdm_render_planes* planes, int L_out_max, int* frames_out,
                      void* stream, const float* scalars, bool takes_scalars) {
  if (!r || !positions || !planes) return fail(FDM_ERR_ARG, "%s: null argument", who);
  const RenderOut out = {planes->rgb, planes->depth, planes->face, planes->alpha, planes->yuv};
  if (!out.rgb && !out.depth && !out.face && !out.alpha && !out.yuv) return fail(FDM_ERR_ARG, "%s: every output is null", who);
  if (out.yuv && ((r->W | r->H) & 1))
    return fail(FDM_ERR_ARG, "%s: yuv 4:2:0 needs an even width and height, the viewport is %d x %d", who, r->W, r->H);
  if (out.yuv && ((size_t)out.yuv & 1)) return fail(FDM_ERR_ARG, "%s: yuv must be 2-byte aligned", who);
  return render_run(who, r, positions, frames, B, L_max, tmpl, tmpl_rows, fps_in, fps_out, normals, out, L_out_max, frames_out, stream, scalars,
                    takes_scalars);
}

}  // namespace

extern "C" {

int fdm_render_forward(fdm_render* r, const float* positions, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows, double fps_in,
                       double fps_out, const float* normals, unsigned char* rgb, float* depth, int* face, int L_out_max, int* frames_out,
                       void* stream) {
  if (!r || !positions || !rgb) return fail(FDM_ERR_ARG, "render_forward: null argument");
  const RenderOut out = {rgb, depth, face, nullptr, nullptr};
  return render_run("render_forward", r, positions, frames, B, L_max, tmpl, tmpl_rows, fps_in, fps_out, normals, out, L_out_max, frames_out, stream);
}

int fdm_render_forward_planes(fdm_render* r, const float* positions, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows,
                              double fps_in, double fps_out, const float* normals, const fdm_render_planes* planes, int L_out_max,
                              int* frames_out, void* stream) {
  return render_planes_run("render_forward_planes", r, positions, frames, B, L_max, tmpl, tmpl_rows, fps_in, fps_out, normals, planes, L_out_max,
                           frames_out, stream, nullptr, false);
}

int fdm_render_forward_material(fdm_render* r, const float* positions, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows,
                                double fps_in, double fps_out, const float* normals, const fdm_render_planes* planes, int L_out_max,
                                int* frames_out, void* stream, const float* scalars) {
  return render_planes_run("render_forward_material", r, positions, frames, B, L_max, tmpl, tmpl_rows, fps_in, fps_out, normals, planes, L_out_max,
                           frames_out, stream, scalars, true);
}

int fdm_render_set_material(fdm_render* r, const fdm_render_material* m) {
  const char* who = "render_set_material";
  if (!r) return fail(FDM_ERR_ARG, "%s: null object", who);
  fdm_render_material none;
  std::memset(&none, 0, sizeof(none));
  if (!m) m = &none;
  if (m->kind < 0 || m->kind > 3) return fail(FDM_ERR_ARG, "%s: kind = %d (0 base, 1 vertex colours, 2 scalar map, 3 texture)", who, m->kind);
  if (m->unlit != 0 && m->unlit != 1) return fail(FDM_ERR_ARG, "%s: unlit = %d (0 or 1)", who, m->unlit);
  float span = 1.f;
  if (m->kind == 1) {
    if (!m->colors) return fail(FDM_ERR_ARG, "%s: null colors for vertex colours", who);
    for (long long i = 0; i < 3LL * r->V; ++i)
      if (!std::isfinite(m->colors[i]) || !(m->colors[i] >= 0.f))
        return fail(FDM_ERR_ARG, "%s: colors[%lld][%lld] = %g (finite, >= 0)", who, i / 3, i % 3, (double)m->colors[i]);
  }
  if (m->kind == 2) {
    if (!m->lut) return fail(FDM_ERR_ARG, "%s: null lut for a scalar map", who);
    if (m->n_lut < 2 || m->n_lut > 1024) return fail(FDM_ERR_ARG, "%s: n_lut = %d (2 .. 1024)", who, m->n_lut);
    for (int i = 0; i < 3 * m->n_lut; ++i)
      if (!std::isfinite(m->lut[i]) || !(m->lut[i] >= 0.f))
        return fail(FDM_ERR_ARG, "%s: lut[%d][%d] = %g (finite, >= 0)", who, i / 3, i % 3, (double)m->lut[i]);
    if (!std::isfinite(m->lo) || !std::isfinite(m->hi) || !(m->lo < m->hi))
      return fail(FDM_ERR_ARG, "%s: the range lo = %g, hi = %g (finite, lo < hi)", who, (double)m->lo, (double)m->hi);
    span = m->hi - m->lo;
    if (!std::isfinite(span)) return fail(FDM_ERR_ARG, "%s: the range lo = %g, hi = %g has no finite fp32 span", who, (double)m->lo, (double)m->hi);
  }
  if (m->kind == 3) {
    if (!m->uv || !m->texture) return fail(FDM_ERR_ARG, "%s: null uv or texture for a texture", who);
    if (m->tex_w < 1 || m->tex_w > 8192 || m->tex_h < 1 || m->tex_h > 8192)
      return fail(FDM_ERR_ARG, "%s: a texture of %d x %d (1 .. 8192 each)", who, m->tex_w, m->tex_h);
    if (m->filter != 0 && m->filter != 1) return fail(FDM_ERR_ARG, "%s: filter = %d (0 nearest, 1 bilinear)", who, m->filter);
  }
  if (r->on_device) {                     // the new tables first: a failed upload leaves the object as it was
    float* colors = nullptr; float4* lut = nullptr; float2* uv = nullptr; uchar4* tex = nullptr;
    int rc = FDM_OK;
    if (m->kind == 1) rc = put(r->mem, &colors, m->colors, (size_t)r->V * 3);
    if (m->kind == 2) {
      std::vector<float4> t((size_t)m->n_lut);
      for (int i = 0; i < m->n_lut; ++i) t[i] = make_float4(m->lut[3 * i], m->lut[3 * i + 1], m->lut[3 * i + 2], 0.f);
      rc = put(r->mem, &lut, t.data(), t.size());
    }
    if (m->kind == 3) {
      const size_t n = (size_t)m->tex_w * m->tex_h;
      std::vector<uchar4> t(n);           // rgb padded to 4-byte texels
      for (size_t i = 0; i < n; ++i) t[i] = make_uchar4(m->texture[3 * i], m->texture[3 * i + 1], m->texture[3 * i + 2], 0);
      rc = put(r->mem, &tex, t.data(), n);
      if (rc == FDM_OK) rc = put(r->mem, &uv, reinterpret_cast<const float2*>(m->uv), (size_t)r->F * 3);
    }
    if (rc != FDM_OK) {
      for (void* p : {(void*)colors, (void*)lut, (void*)uv, (void*)tex}) if (p) r->mem.free_one(p);
      return rc;
    }
    if (const hipError_t e = hipDeviceSynchronize(); e != hipSuccess) {      // a call in flight may still read the old tables
      for (void* p : {(void*)colors, (void*)lut, (void*)uv, (void*)tex}) if (p) r->mem.free_one(p);      // (nothing reads the new ones yet)
      return fail(FDM_ERR_HIP, "%s: hipDeviceSynchronize: %s", who, hipGetErrorString(e));
    }
    for (void* p : {(void*)r->colors, (void*)r->lut, (void*)r->uv, (void*)r->tex}) if (p) r->mem.free_one(p);
    r->colors = colors; r->lut = lut; r->uv = uv; r->tex = tex;
  }
  r->mat_kind = m->kind; r->mat_unlit = m->unlit;
  r->n_lut = m->kind == 2 ? m->n_lut : 0;
  r->mat_lo = m->kind == 2 ? m->lo : 0.f; r->mat_span = span;
  r->tex_w = m->kind == 3 ? m->tex_w : 0; r->tex_h = m->kind == 3 ? m->tex_h : 0; r->tex_filter = m->kind == 3 ? m->filter : 0;
  return FDM_OK;
}

int fdm_op_vertex_dist(const float* a, const float* b, float* out, int rows, int V, void* stream) {
  if (!a || !b || !out) return fail(FDM_ERR_ARG, "vertex_dist: null operand");
  if (rows < 1 || V < 1) return fail(FDM_ERR_SHAPE, "vertex_dist: rows = %d, V = %d", rows, V);
  if (!fdm_device_ok()) return fail(FDM_ERR_STATE, "vertex_dist: no gfx950 device visible (there is no CPU fallback)");
  const long long n = (long long)rows * V;
  if ((n + 255) / 256 > 0x7fffffffLL) return fail(FDM_ERR_SHAPE, "vertex_dist: %lld vertices exceed one launch", n);
  hipLaunchKernelGGL(vertex_dist_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
  HIPCK(hipGetLastError());
  return FDM_OK;
}

}  // extern "C"
