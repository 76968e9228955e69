// Mesh hand-off behind plain C calls (include/fdm_hip.h, fdm_mesh_*): vertex offsets as fdm_vq_decode(_ragged) writes them -> positions
// (+ template, at the consumer's frame rate) and area-weighted vertex normals.  Kernels: mesh_out.hpp.  The topology (faces and the
// vertex -> incident-face lists) is built and uploaded in fdm_mesh_create; a forward call validates (every check before the first
// launch), grows the scratch when a call is larger than any before it, and launches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "host.hpp"
#include "mesh_out.hpp"

struct fdm_mesh : fdm::Handoff {          // lens: {L, L_out} per clip
  int F = 0, V = 0;
  int *faces = nullptr, *adj_off = nullptr, *adj = nullptr;      // device: [F][3], [V + 1], [3F]
  float* P = nullptr;           // fp32 positions of the call in flight when no fp32 planar output holds them
  long long P_cap = 0;
};

namespace {
using namespace fdm;

const int MESH_FLAGS = FDM_MESH_INTERLEAVED | FDM_MESH_F16 | FDM_MESH_NORMALS;

// a triangle list over V vertices: every index inside [0, V), 3 F and 6 V inside an int
int check_topology(const char* who, const int* faces, int F, int V) {
  if (!faces) return fail(FDM_ERR_ARG, "%s: null faces", who);
  if (F < 0 || V <= 0) return fail(FDM_ERR_ARG, "%s: F = %d, V = %d", who, F, V);
  if (F > 0x7fffffff / 3 || V > 0x7fffffff / 6) return fail(FDM_ERR_ARG, "%s: F = %d, V = %d (3 F and 6 V are 32-bit ints)", who, F, V);
  for (long long i = 0; i < 3LL * F; ++i)
    if (faces[i] < 0 || faces[i] >= V) return fail(FDM_ERR_ARG, "%s: face %lld names vertex %d of %d", who, i / 3, faces[i], V);
  return FDM_OK;
}

}  // namespace

extern "C" {

int fdm_mesh_adjacency_host(const int* faces, int F, int V, int* offsets, int* items) {
  if (!offsets || !items) return fail(FDM_ERR_ARG, "mesh_adjacency: null argument");
  FCK(check_topology("mesh_adjacency", faces, F, V));
  for (int v = 0; v <= V; ++v) offsets[v] = 0;
  for (long long i = 0; i < 3LL * F; ++i) ++offsets[faces[i] + 1];
  for (int v = 0; v < V; ++v) offsets[v + 1] += offsets[v];
  std::vector<int> at(offsets, offsets + V);
  for (int f = 0; f < F; ++f)                // ascending face index, one entry per corner
    for (int c = 0; c < 3; ++c) items[at[faces[3LL * f + c]]++] = f;
  return FDM_OK;
}

int fdm_mesh_create(const int* faces, int F, int V, fdm_mesh** out) {
  if (!out) return fail(FDM_ERR_ARG, "mesh_create: null out");
  FCK(check_topology("mesh_create", faces, F, V));
  std::vector<int> off((size_t)V + 1), items((size_t)F * 3 + 1);
  FCK(fdm_mesh_adjacency_host(faces, F, V, off.data(), items.data()));
  fdm_mesh* M = new (std::nothrow) fdm_mesh();
  if (!M) return fail(FDM_ERR_STATE, "mesh_create: out of memory");
  M->F = F; M->V = V;
  return handoff_finish(M, out, [&]() {
    FCK(put(M->mem, &M->faces, faces, (size_t)F * 3));
    FCK(put(M->mem, &M->adj, items.data(), (size_t)F * 3));
    FCK(put(M->mem, &M->adj_off, off.data(), (size_t)V + 1));
    return (int)FDM_OK;
  });
}

int fdm_mesh_destroy(fdm_mesh* M) { return handoff_destroy(M); }

int fdm_mesh_frames(int frames_in, double fps_in, double fps_out, int* frames_out) {
  if (!frames_out) return fail(FDM_ERR_ARG, "mesh_frames: null frames_out");
  if (frames_in < 0) return fail(FDM_ERR_ARG, "mesh_frames: frames_in = %d", frames_in);
  FCK(check_fps("mesh_frames", fps_in, fps_out));
  const long long n = frames_out_of(frames_in, fps_in, fps_out);
  if (n < 0) return fail(FDM_ERR_SHAPE, "mesh_frames: %d frames at %g -> %g fps do not fit an int", frames_in, fps_in, fps_out);
  *frames_out = (int)n;
  return FDM_OK;
}

int fdm_mesh_forward(fdm_mesh* M, const float* offsets, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows, double fps_in,
                     double fps_out, int flags, void* pos, void* nrm, int L_out_max, int* frames_out, void* stream) {
  if (!M || !offsets || !pos) return fail(FDM_ERR_ARG, "mesh_forward: null argument");
  if (flags & ~MESH_FLAGS) return fail(FDM_ERR_ARG, "mesh_forward: unknown flag bits 0x%x", flags & ~MESH_FLAGS);
  const bool inter = flags & FDM_MESH_INTERLEAVED, half = flags & FDM_MESH_F16, normals = flags & FDM_MESH_NORMALS;
  if (inter && !normals) return fail(FDM_ERR_ARG, "mesh_forward: the interleaved layout holds normals (set FDM_MESH_NORMALS)");
  if (inter && nrm) return fail(FDM_ERR_ARG, "mesh_forward: the interleaved layout has one output (nrm must be NULL)");
  if (!inter && normals && !nrm) return fail(FDM_ERR_ARG, "mesh_forward: FDM_MESH_NORMALS without nrm");
  if (tmpl_rows != 0 && tmpl_rows != 1 && tmpl_rows != B) return fail(FDM_ERR_ARG, "mesh_forward: tmpl_rows = %d (0, 1 or B = %d)", tmpl_rows, B);
  if (tmpl_rows && !tmpl) return fail(FDM_ERR_ARG, "mesh_forward: tmpl_rows = %d with a null template", tmpl_rows);
  FCK(check_fps("mesh_forward", fps_in, fps_out));
  if (B < 1 || L_max < 1 || L_out_max < 1) return fail(FDM_ERR_SHAPE, "mesh_forward: B = %d, L_max = %d, L_out_max = %d", B, L_max, L_out_max);
  std::vector<int> hl;
  const ClipLens c = clip_lens(frames, B, L_max, fps_in, fps_out, L_out_max, hl);
  if (c.bad == ClipLens::LENGTH) return fail(FDM_ERR_SHAPE, "mesh_forward: clip %d has %d frames, the batch is %d long", c.clip, c.L, L_max);
  if (c.bad == ClipLens::OUTPUT) return fail(FDM_ERR_SHAPE, "mesh_forward: clip %d gives %lld frames, the output is %d long", c.clip, c.Lo, L_out_max);
  const long long rows = (long long)B * L_out_max, V3 = 3LL * M->V;
  const int nblk = (M->V + MESH_VB - 1) / MESH_VB;
  if (rows > 0x7fffffffLL || (rows + 7) / 8 * 8 * nblk > 0x7fffffffLL || (V3 + MESH_POS_TILE - 1) / MESH_POS_TILE > 65535)
    return fail(FDM_ERR_SHAPE, "mesh_forward: %lld output rows of %d vertices exceed one launch", rows, M->V);
  FCK(handoff_device(*M, "mesh_forward"));
  hipStream_t s = (hipStream_t)stream;
  // fp32 positions for the normals: the planar fp32 output itself, scratch otherwise
  const bool own = normals && (inter || half);
  if (own) FCK(grow(M->mem, &M->P, &M->P_cap, rows * V3));
  FCK(handoff_lens(*M, hl, s));
  const int rs = resamples(fps_in, fps_out) ? 1 : 0, tstride = tmpl_rows == B && B > 1 ? (int)V3 : 0;
  const float* tp = tmpl_rows ? tmpl : nullptr;
  const dim3 gp((unsigned)rows, (unsigned)((V3 + MESH_POS_TILE - 1) / MESH_POS_TILE));
  float* P = own ? M->P : (float*)pos;
  if (inter)
    hipLaunchKernelGGL(mesh_pos_kernel<float>, gp, dim3(256), 0, s, offsets, tp, tstride, (const int*)M->lens, L_max, L_out_max, (int)V3, rs, (float*)nullptr, P);
  else if (half)
    hipLaunchKernelGGL(mesh_pos_kernel<_Float16>, gp, dim3(256), 0, s, offsets, tp, tstride, (const int*)M->lens, L_max, L_out_max, (int)V3, rs, (_Float16*)pos, own ? P : (float*)nullptr);
  else
    hipLaunchKernelGGL(mesh_pos_kernel<float>, gp, dim3(256), 0, s, offsets, tp, tstride, (const int*)M->lens, L_max, L_out_max, (int)V3, rs, (float*)pos, (float*)nullptr);
  if (normals) {
    const dim3 gn((unsigned)((rows + 7) / 8 * 8 * nblk));
    void* o = inter ? pos : nrm;
    if (half)
      hipLaunchKernelGGL(mesh_nrm_kernel<_Float16>, gn, dim3(MESH_VB), 0, s, (const float*)P, (const int*)M->lens, L_out_max, M->V, (const int*)M->faces, (const int*)M->adj_off, (const int*)M->adj, (int)rows, nblk, (_Float16*)o, inter ? 1 : 0);
    else
      hipLaunchKernelGGL(mesh_nrm_kernel<float>, gn, dim3(MESH_VB), 0, s, (const float*)P, (const int*)M->lens, L_out_max, M->V, (const int*)M->faces, (const int*)M->adj_off, (const int*)M->adj, (int)rows, nblk, (float*)o, inter ? 1 : 0);
  }
  HIPCK(hipGetLastError());
  if (frames_out) for (int b = 0; b < B; ++b) frames_out[b] = hl[2 * b + 1];
  return FDM_OK;
}

}  // extern "C"
