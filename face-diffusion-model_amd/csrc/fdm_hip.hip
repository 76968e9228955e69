// libfdm_hip.so: C ABI (include/fdm_hip.h) over the gfx950 kernels.  No torch, no exceptions across
// the boundary, no allocation or synchronisation inside fdm_op_* (so a caller may capture them).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <functional>

#include "elementwise.hpp"
#include "window.hpp"
#include "slots.hpp"
#include "host.hpp"
#include "gemm_tiles.hpp"

namespace fdm {
thread_local std::string g_err;
// records the message returned by fdm_last_error() on this thread and hands back `code` (kernels.hpp: shared by every host unit)
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

namespace {
using namespace fdm;

int hip_fail(hipError_t e, const char* what) {
  return fail(FDM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

using Op = std::function<hipError_t(hipStream_t)>;

}  // namespace

struct fdm_prog {
  std::vector<Op> ops;
  hipGraph_t graph = nullptr;                // the captured sequence
  hipGraphExec_t exec = nullptr;
};

namespace {

thread_local fdm_prog* g_rec = nullptr;

// Either record the launch closure into the program being built or launch it now.
int submit(Op op, void* stream, const char* what) {
  if (g_rec) {
    g_rec->ops.push_back(std::move(op));
    return FDM_OK;
  }
  hipError_t e = op((hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, what);
  return FDM_OK;
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// The kernel type behind a dtype code, handed to a generic lambda as a value (`using T = decltype(tag)`).
// with_move_type: a pure move -- every 2-byte kind (one plane of a split operand included: the caller passes each plane) moves as
// bf16 bit patterns, FDM_F32 as float.
template <typename F>
void with_move_type(int dtype, F&& f) {
  if (kind(dtype).bytes == 2) f(fdm::bf16{});
  else f(float{});
}
// with_out_kind: the operand copy y_t of a time norm -- f(tag, lo_off) with bf16, f16x3_t (the only kind that has a lo plane) or float
template <typename F>
void with_out_kind(int dtype, long long lo_off, F&& f) {
  if (dtype == FDM_BF16) f(fdm::bf16{}, 0LL);
  else if (dtype == FDM_F16X3) f(fdm::f16x3_t{}, lo_off);
  else f(float{}, 0LL);
}

}  // namespace

extern "C" {

const char* fdm_last_error(void) { return g_err.c_str(); }
int fdm_version(void) { return 105; }      // 1.05: round 5 (fdm_gemm_args.ksplit / batch2, fdm_ln_args.x_planes, plan keys ksplit.*; lanes, FDM_BF16X3 and three tile ids removed); additions since keep the number: fdm_frontend_* / fdm_pcm / fdm_resample_*_host (audio front end) and fdm_mesh_* (mesh hand-off) among them

// sizeof() of a public struct as THIS build sees it: a binding compares it with its own mirror before the first call
int fdm_abi_struct_size(const char* name) {
  if (!name) return fdm::fail(FDM_ERR_ARG, "abi_struct_size: null name");
  const std::string n(name);
  if (n == "fdm_sched_args") return (int)sizeof(fdm_sched_args);
  if (n == "fdm_gemm_args") return (int)sizeof(fdm_gemm_args);
  if (n == "fdm_attn_args") return (int)sizeof(fdm_attn_args);
  if (n == "fdm_ln_args") return (int)sizeof(fdm_ln_args);
  if (n == "fdm_model_desc") return (int)sizeof(fdm_model_desc);
  if (n == "fdm_sample_args") return (int)sizeof(fdm_sample_args);
  if (n == "fdm_vq_desc") return (int)sizeof(fdm_vq_desc);
  if (n == "fdm_slot_group_args") return (int)sizeof(fdm_slot_group_args);
  if (n == "fdm_slot_bank_args") return (int)sizeof(fdm_slot_bank_args);
  if (n == "fdm_pcm") return (int)sizeof(fdm_pcm);
  if (n == "fdm_flame_model") return (int)sizeof(fdm_flame_model);
  if (n == "fdm_render_planes") return (int)sizeof(fdm_render_planes);
  if (n == "fdm_render_material") return (int)sizeof(fdm_render_material);
  return fdm::fail(FDM_ERR_ARG, "abi_struct_size: unknown struct '%s'", name);
}

int fdm_device_ok(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 0;
  return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

static bool gemm_act_heavy_host(int act) { return act == FDM_ACT_MISH || act == FDM_ACT_GELU_ERF || act == FDM_ACT_GELU_TANH; }

int fdm_op_gemm(const fdm_gemm_args* a, void* stream) {
  if (!a || !a->A || !a->W) return fail(FDM_ERR_ARG, "gemm: null operand");
  if (a->M <= 0 || a->N <= 0 || a->K <= 0) return fail(FDM_ERR_SHAPE, "gemm: M,N,K must be positive (%d,%d,%d)", a->M, a->N, a->K);
  if (!kind_ok(a->dtype)) return fail(FDM_ERR_ARG, "gemm: bad dtype %d", a->dtype);
  const bool split = kind(a->dtype).planes == 2;
  const int bk = kind(a->dtype).bk, epc = kind(a->dtype).epc;
  if (split && (a->a_lo_off <= 0 || a->w_lo_off <= 0 || a->a_lo_off % epc || a->w_lo_off % epc))
    return fail(FDM_ERR_ARG, "gemm: split operands need positive a_lo_off / w_lo_off (multiples of 8 elements)");
  if (split && a->out_t && a->out_t_lo_off <= 0) return fail(FDM_ERR_ARG, "gemm: split out_t needs out_t_lo_off");
  if (a->K % bk) return fail(FDM_ERR_SHAPE, "gemm: K=%d not a multiple of %d", a->K, bk);
  if (a->lda % epc || a->ldw % epc || !aligned16(a->A) || !aligned16(a->W)) return fail(FDM_ERR_ARG, "gemm: operands need 16-byte aligned rows");
  if (a->lda < 0 || a->ldw < 0 || a->lda > 0x7fffffffLL || a->ldw > 0x7fffffffLL) return fail(FDM_ERR_SHAPE, "gemm: lda / ldw are passed to the kernel as 32-bit element counts");
  if (a->a_batch_stride % epc || a->w_batch_stride % epc) return fail(FDM_ERR_ARG, "gemm: batch strides need 16-byte alignment");
  if (!a->out_f32 && !a->out_t && !a->out_vp && !a->out_kp) return fail(FDM_ERR_ARG, "gemm: no output");
  if (a->out_kp || a->out_vp) {
    const int hi = a->out_vp ? a->vp_col0 : a->N;
    if (a->kv_hd <= 0 || a->kv_hd % 16 || a->kv_L <= 0 || a->kv_Lpad < a->kv_L || a->kv_Lpad % 32 || a->M % a->kv_L)
      return fail(FDM_ERR_SHAPE, "gemm: bad packed K/V geometry (hd %d, L %d, Lpad %d)", a->kv_hd, a->kv_L, a->kv_Lpad);
    if (a->out_vp && (a->vp_col0 < 0 || a->vp_col0 % 4 || (a->N - a->vp_col0) % a->kv_hd)) return fail(FDM_ERR_SHAPE, "gemm: bad packed V column range");
    if (a->out_kp && (a->kp_col0 < 0 || a->kp_col0 % 4 || hi < a->kp_col0 || (hi - a->kp_col0) % a->kv_hd)) return fail(FDM_ERR_SHAPE, "gemm: bad packed K column range");
    if (!aligned16(a->out_kp) || !aligned16(a->out_vp)) return fail(FDM_ERR_ARG, "gemm: packed K/V buffers must be 16-byte aligned");
    if (a->dtype == FDM_F16X3 && (a->kv_lo_off <= 0 || a->kv_lo_off % 8)) return fail(FDM_ERR_ARG, "gemm: split packed K/V outputs need kv_lo_off");
  }
  if (a->bias && !aligned16(a->bias)) return fail(FDM_ERR_ARG, "gemm: bias must be 16-byte aligned");
  if (a->ln_stat_in && (a->ln_nparts <= 0 || a->ln_dim <= 0)) return fail(FDM_ERR_ARG, "gemm: ln_stat_in needs ln_nparts and ln_dim");
  if ((a->ln_colsum || a->rln_gamma) && !a->ln_stat_in) return fail(FDM_ERR_ARG, "gemm: LayerNorm folding needs ln_stat_in");
  if (a->rln_gamma && (!a->rln_beta || !a->resid)) return fail(FDM_ERR_ARG, "gemm: rln_gamma needs rln_beta and resid");
  if ((a->stat_out || a->ln_stat_in) && (a->batch > 1 || a->out_batch_stride)) return fail(FDM_ERR_ARG, "gemm: LayerNorm folding is not batched");
  if (a->tile < 0 || (a->tile & FDM_TILE_ID_MASK) > FDM_TILE_MAX) return fail(FDM_ERR_ARG, "gemm: unknown tile %d", a->tile);
  if (a->sched_fuse) {
    const fdm_sched_args& sc = a->sched;
    if (sc.mode != 0 && sc.mode != 1 && sc.mode != 3) return fail(FDM_ERR_ARG, "gemm: fused scheduler supports mode 0 (DDPM), 1 (DDIM) and 3 (table-driven)");
    if (!a->resid || !a->out_f32 || a->N % 64 || a->ldo_f32 != a->N || a->ldr != a->N || a->resid_row_mod || a->batch > 1 ||
        !aligned16(a->resid) || !aligned16(a->out_f32) || (a->out_t && (a->ldo_t != a->N || !aligned16(a->out_t))))
      return fail(FDM_ERR_SHAPE, "gemm: fused scheduler needs resid = x_t and out_f32 = x_{t-1} as dense [M, N] arrays, N %% 64 == 0");
    if (gemm_act_heavy_host(a->act) || a->stat_out || a->out_kp || a->out_vp || a->rln_gamma)
      return fail(FDM_ERR_ARG, "gemm: fused scheduler cannot be combined with Mish/GELU, stat_out, packed K/V or rln outputs");
    if (sc.mode == 0 && (!sc.c1 || !sc.c2 || !sc.sigma)) return fail(FDM_ERR_ARG, "gemm: fused DDPM needs c1, c2, sigma");
    if (sc.mode == 1 && (!sc.sra || !sc.srm1 || !sc.sqrt_an || !sc.c_n)) return fail(FDM_ERR_ARG, "gemm: fused DDIM needs sra, srm1, sqrt_an, c_n");
    if (sc.mode == 0 && !sc.noise && sc.n_per_clip <= 0) return fail(FDM_ERR_ARG, "gemm: fused DDPM with Philox noise needs n_per_clip");
    if (sc.mode == 3 && (!sc.lm_a || !sc.lm_b || !sc.lm_c || !sc.lm_s || !sc.x0_hist || !aligned16(sc.x0_hist)))
      return fail(FDM_ERR_ARG, "gemm: fused table-driven sampler needs lm_a, lm_b, lm_c, lm_s and a 16-byte aligned x0_hist [M, N]");
    if (sc.mode == 3 && !sc.noise && sc.n_per_clip <= 0) return fail(FDM_ERR_ARG, "gemm: fused table-driven sampler with Philox noise needs n_per_clip");
  }
  if (a->ksplit < 0 || a->ksplit > 4) return fail(FDM_ERR_ARG, "gemm: ksplit %d outside 0..4", a->ksplit);
  if (a->ksplit > 1) {
    const int tl = a->tile & FDM_TILE_ID_MASK;
    if (a->batch > 1 || a->out_batch_stride || a->act != FDM_ACT_NONE || !a->out_f32 || a->out_t || a->out_kp || a->out_vp || a->stat_out || a->ln_stat_in ||
        a->sched_fuse || a->resid_row_mod || (a->tile & FDM_TILE_GENERAL))
      return fail(FDM_ERR_ARG, "gemm: ksplit needs a plain launch (one batch, no activation, out_f32 as the only output, no folds)");
    if ((a->K / bk) % a->ksplit) return fail(FDM_ERR_SHAPE, "gemm: ksplit %d does not divide the %d k-tiles of K=%d", a->ksplit, a->K / bk, a->K);
    if (a->N % 64 || a->ldo_f32 % 4 || !aligned16(a->out_f32) || a->ksplit_stride % 4 || a->ksplit_stride < (long long)(a->M - 1) * a->ldo_f32 + a->N ||
        (a->resid && (a->ldr % 4 || !aligned16(a->resid))))
      return fail(FDM_ERR_SHAPE, "gemm: ksplit needs N %% 64 == 0, 16-byte aligned rows and ksplit_stride >= one output plane");
    if (tl != 0 && !gemm_tile_can(tl, TILE_KSPLIT))
      return fail(FDM_ERR_ARG, "gemm: ksplit runs on the 64-column tiles (FDM_TILE_64x64, FDM_TILE_64x64_S2, FDM_TILE_32x64_S3), not tile %d", tl);
  }
  if (a->batch2 < 0) return fail(FDM_ERR_ARG, "gemm: negative batch2");
  if (a->batch2 >= 1) {
    const int tl = a->tile & FDM_TILE_ID_MASK;
    if (a->ksplit > 1 || a->out_kp || a->out_vp || a->stat_out || a->ln_stat_in || a->sched_fuse || a->resid_row_mod || a->incr_counter)
      return fail(FDM_ERR_ARG, "gemm: batch2 cannot be combined with ksplit, packed K/V, LayerNorm folds, the fused scheduler or resid_row_mod");
    if (a->a_batch_stride2 % epc) return fail(FDM_ERR_ARG, "gemm: a_batch_stride2 needs 16-byte alignment");
    if (tl != 0 && !gemm_tile_can(tl, TILE_BATCH2))
      return fail(FDM_ERR_ARG, "gemm: batch2 runs on the 64-column tiles (FDM_TILE_64x64, FDM_TILE_64x64_S2, FDM_TILE_128x64), not tile %d", tl);
    if (a->batch < 1) return fail(FDM_ERR_ARG, "gemm: batch2 needs batch >= 1 (the group count of the second batch level)");
  }
  fdm_gemm_args c = *a;
  return submit([c](hipStream_t s) { return fdm::gemm_launch(c, s); }, stream, "gemm");
}

int fdm_gemm_heuristic_tile(const fdm_gemm_args* a) {
  if (!a) return fail(FDM_ERR_ARG, "gemm_heuristic_tile: null argument");
  fdm_gemm_args b = *a;
  b.tile = 0;
  // (the query has always named the forced tile for a second-batch-level launch too, although the launch itself is exempt from FDM_GEMM_TILE)
  if (b.batch2 >= 1 && b.ksplit <= 1 && !b.sched_fuse && gemm_tile_override() > 0) return gemm_tile_override();
  return gemm_requested_tile(b);
}

int fdm_op_attention(const fdm_attn_args* a, void* stream) {
  if (!a || !a->Q || !a->Kp || !a->Vp || !a->O) return fail(FDM_ERR_ARG, "attention: null operand");
  if (a->hd != 64 && a->hd != 128 && a->hd != 256) return fail(FDM_ERR_SHAPE, "attention: head_dim %d unsupported (64, 128, 256)", a->hd);
  if (a->B <= 0 || a->H <= 0 || a->L <= 0) return fail(FDM_ERR_SHAPE, "attention: B,H,L must be positive");
  if (a->Lpad < a->L || a->Lpad % 32) return fail(FDM_ERR_SHAPE, "attention: Lpad=%d must be a multiple of 32 >= L", a->Lpad);
  if (!kind_ok(a->dtype)) return fail(FDM_ERR_ARG, "attention: bad dtype %d (FDM_F32, FDM_BF16, FDM_F16X3, FDM_F16)", a->dtype);
  if (a->o_split && (a->dtype != FDM_F32 || a->o_split != FDM_F16X3 || a->o_lo_off <= 0))
    return fail(FDM_ERR_ARG, "attention: o_split needs dtype FDM_F32, a split kind and o_lo_off");
  if (a->dtype == FDM_F16X3 && (a->q_lo_off <= 0 || a->kv_lo_off <= 0 || a->o_lo_off <= 0 || a->q_lo_off % 8 || a->kv_lo_off % 8 || a->o_lo_off % 4))
    return fail(FDM_ERR_ARG, "attention: split operands need q_lo_off, kv_lo_off and o_lo_off");
  if (a->q_lo_off > 0x7fffffffLL || a->kv_lo_off > 0x7fffffffLL || a->ldq > 0x7fffffffLL)
    return fail(FDM_ERR_SHAPE, "attention: q_lo_off, kv_lo_off and ldq are passed to the kernel as 32-bit element counts");
  const int epc = kind(a->dtype).epc;
  if (a->ldq % epc || a->ldo % 4 || !aligned16(a->Q) || !aligned16(a->Kp) || !aligned16(a->Vp) || !aligned16(a->O))
    return fail(FDM_ERR_ARG, "attention: operands need 16-byte aligned rows");
  if (a->slopes && a->period <= 0) return fail(FDM_ERR_ARG, "attention: period must be positive");
  if (a->lens && (a->causal || (a->hd != 64 && a->hd != 128)))
    return fail(FDM_ERR_ARG, "attention: per-clip lengths need causal = 0 and head_dim 64 or 128");
  fdm_attn_args c = *a;
  return submit([c](hipStream_t s) { return fdm::attn_launch(c, s); }, stream, "attention");
}

int fdm_op_pack_kv(const void* K, long long ldk, const void* V, long long ldv, void* Kp, void* Vp,
                   int B, int H, int L, int Lpad, int hd, int dtype, void* stream) {
  if (!K || !V || !Kp || !Vp) return fail(FDM_ERR_ARG, "pack_kv: null operand");
  if (B <= 0 || H <= 0 || L <= 0 || Lpad < L || Lpad % 32 || hd <= 0 || hd % 16) return fail(FDM_ERR_SHAPE, "pack_kv: bad geometry");
  if (dtype != FDM_F32 && dtype != FDM_BF16) return fail(FDM_ERR_ARG, "pack_kv: bad dtype %d", dtype);
  return submit([=](hipStream_t s) {
    return dtype == FDM_BF16 ? fdm::pack_kv_launch_bf16(K, ldk, V, ldv, Kp, Vp, B, H, L, Lpad, hd, s)
                             : fdm::pack_kv_launch_f32(K, ldk, V, ldv, Kp, Vp, B, H, L, Lpad, hd, s);
  }, stream, "pack_kv");
}

int fdm_op_layernorm(const fdm_ln_args* a, void* stream) {
  if (!a || !a->x || !a->gamma || !a->beta) return fail(FDM_ERR_ARG, "layernorm: null operand");
  if (a->d != 256 && a->d != 512 && a->d != 768 && a->d != 1024) return fail(FDM_ERR_SHAPE, "layernorm: d=%d unsupported (256, 512, 768, 1024)", a->d);
  if (a->M <= 0) return fail(FDM_ERR_SHAPE, "layernorm: M must be positive");
  if (!a->y_f32 && !a->y_t) return fail(FDM_ERR_ARG, "layernorm: no output");
  if (!kind_ok(a->dtype)) return fail(FDM_ERR_ARG, "layernorm: bad dtype %d", a->dtype);
  if (a->y_t && a->dtype == FDM_F16X3 && (a->y_t_lo_off <= 0 || a->y_t_lo_off % 4)) return fail(FDM_ERR_ARG, "layernorm: split y_t needs y_t_lo_off");
  if (a->add_mat_group < 0 || a->add_mat_wrap < 0 ||
      (a->add_mat_group > 0 && (a->add_mat_L <= 0 || a->add_mat_group % a->add_mat_L || (a->add_mat_wrap > 0 && a->add_mat_wrap % a->add_mat_group))))
    return fail(FDM_ERR_SHAPE, "layernorm: shared add_mat needs add_mat_L | add_mat_group | add_mat_wrap (got %d, %d, %d)", a->add_mat_L, a->add_mat_group, a->add_mat_wrap);
  if (a->x_planes < 0 || a->x_planes > 4 || (a->x_planes > 1 && (a->x_plane_stride < (long long)a->M * a->d || a->x_plane_stride % 4)))
    return fail(FDM_ERR_ARG, "layernorm: x_planes %d (0..4) needs x_plane_stride >= M * d, a multiple of 4", a->x_planes);
  if (a->clip_step && (a->clip_rows <= 0 || a->clip_step_stride <= 0 || a->clip_wrap < 0 || (a->clip_wrap > 0 && a->clip_wrap % a->clip_rows)))
    return fail(FDM_ERR_SHAPE, "layernorm: clip_step needs clip_rows > 0, clip_step_stride > 0 and clip_rows | clip_wrap (got %d, %d, %d)", a->clip_rows, a->clip_step_stride, a->clip_wrap);
  if (a->clip_step && a->act != FDM_ACT_NONE && a->act != FDM_ACT_RELU) return fail(FDM_ERR_ARG, "layernorm: clip_step runs with FDM_ACT_NONE / FDM_ACT_RELU only");
  fdm_ln_args c = *a;
  return submit([c](hipStream_t s) {
    switch (c.dtype) {
      case FDM_BF16: return fdm::ln_launch_t<fdm::bf16>(c, s);
      case FDM_F16X3: return fdm::ln_launch_t<fdm::f16x3_t>(c, s);
      case FDM_F16: return fdm::ln_launch_t<fdm::f16>(c, s);
      default: return fdm::ln_launch_t<float>(c, s);
    }
  }, stream, "layernorm");
}

int fdm_op_sched_step(const fdm_sched_args* a, void* stream) {
  if (!a || !a->x0 || !a->x_out) return fail(FDM_ERR_ARG, "sched: null operand");
  if (a->n <= 0 || a->n % 4) return fail(FDM_ERR_SHAPE, "sched: n=%lld must be a positive multiple of 4", a->n);
  if (a->mode == 0 && (!a->x || !a->c1 || !a->c2 || !a->sigma)) return fail(FDM_ERR_ARG, "sched: DDPM tables missing");
  if (a->mode == 1 && (!a->x || !a->sra || !a->srm1 || !a->sqrt_an || !a->c_n)) return fail(FDM_ERR_ARG, "sched: DDIM tables missing");
  if (a->mode == 3 && (!a->x || !a->lm_a || !a->lm_b || !a->lm_c || !a->lm_s || !a->x0_hist)) return fail(FDM_ERR_ARG, "sched: table-driven sampler needs lm_a, lm_b, lm_c, lm_s, x0_hist");
  if (a->mode < 0 || a->mode > 3) return fail(FDM_ERR_ARG, "sched: bad mode %d", a->mode);
  if (a->mode == 3 && !a->noise && (a->n_per_clip <= 0 || a->n_per_clip % 4)) return fail(FDM_ERR_SHAPE, "sched: n_per_clip must be a positive multiple of 4");
  if (a->mode == 0 && !a->noise && (a->n_per_clip <= 0 || a->n_per_clip % 4)) return fail(FDM_ERR_SHAPE, "sched: n_per_clip must be a positive multiple of 4");
  if (a->x_out_t && !kind_ok(a->out_dtype)) return fail(FDM_ERR_ARG, "sched: bad out_dtype %d", a->out_dtype);
  if (a->x_out_t && a->out_dtype == FDM_F16X3 && (a->x_out_t_lo_off <= 0 || a->x_out_t_lo_off % 4)) return fail(FDM_ERR_ARG, "sched: split x_out_t needs x_out_t_lo_off");
  fdm_sched_args c = *a;
  return submit([c](hipStream_t s) { return fdm::sched_launch(c, s); }, stream, "sched");
}

// what the two bank operators share: the bank's own pointers and sizes (the kernel checks every row against them)
static int check_bank(const fdm_slot_bank_args* b, const char* who) {
  if (!b || !b->req || !b->desc || !b->t) return fail(FDM_ERR_ARG, "%s: null bank table", who);
  if (b->n_samplers < 1 || b->n_t < 1 || b->n_coef < 0 || (b->n_coef > 0 && !b->coef)) return fail(FDM_ERR_SHAPE, "%s: bank sizes (%d samplers, %d timesteps, %d coefficients)", who, b->n_samplers, b->n_t, b->n_coef);
  if (!aligned16(b->req) || !aligned16(b->desc)) return fail(FDM_ERR_ARG, "%s: request rows and descriptors must be 16-byte aligned", who);
  return FDM_OK;
}

// The argument checks of the four slot scheduler passes, in one order.  g = the group tables of the group forms (null: plain slots
// only), b = the bank of the bank forms (null: the mode and the step-indexed tables are a's, and are checked here).
static int check_slot_pass(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots, const fdm_slot_group_args* g,
                           const fdm_slot_bank_args* b, const char* who) {
  if (!a || !a->x_out || !state || !keys || (!g && (!a->x0 || !a->x))) return fail(FDM_ERR_ARG, "%s: null operand", who);
  if (b) FCK(check_bank(b, who));
  if (g) {
    if (!g->member || !g->frames || !g->entries || !g->groups || !g->x_long) return fail(FDM_ERR_ARG, "%s: null table or arena", who);
    if (!g->init && (!a->x0 || !a->x)) return fail(FDM_ERR_ARG, "%s: null operand", who);
    if (g->init && g->plain) return fail(FDM_ERR_ARG, "%s: init loads the arena into the window rows only (plain must be 0)", who);
  }
  const bool own_sampler = !b && !(g && g->init);      // a's mode and tables are read: no bank holds them, and the launch updates
  if (a->noise) return fail(FDM_ERR_ARG, "%s: injected noise is not supported (Philox keyed per slot%s)", who, g ? " / group" : "");
  if (own_sampler && a->mode != 0 && a->mode != 1 && a->mode != 3) return fail(FDM_ERR_ARG, "%s: mode %d (0 DDPM, 1 DDIM, 3 table-driven)", who, a->mode);
  if (n_slots < 1 || a->n_per_clip <= 0 || a->n_per_clip % 4 || a->n != (long long)n_slots * a->n_per_clip)
    return fail(FDM_ERR_SHAPE, "%s: n=%lld must be n_slots=%d x n_per_clip=%lld (a multiple of 4)", who, a->n, n_slots, a->n_per_clip);
  if (g) {
    if (g->L < 1 || g->d < 4 || g->d % 4 || (long long)g->L * g->d != a->n_per_clip)
      return fail(FDM_ERR_SHAPE, "%s: L=%d x d=%d (a multiple of 4) must be n_per_clip=%lld", who, g->L, g->d, a->n_per_clip);
    if (g->arena_frames < 1 || g->n_groups < 1 || g->n_entries < 1 || g->frame0 < 0 || g->frame1 < g->frame0 || g->frame1 > g->arena_frames)
      return fail(FDM_ERR_SHAPE, "%s: arena frames [%d, %d) outside [0, %d), or no groups / entries", who, g->frame0, g->frame1, g->arena_frames);
  }
  if (own_sampler) {
    if (a->mode == 0 && (!a->c1 || !a->c2 || !a->sigma)) return fail(FDM_ERR_ARG, "%s: DDPM tables missing", who);
    if (a->mode == 1 && (!a->sra || !a->srm1 || !a->sqrt_an || !a->c_n)) return fail(FDM_ERR_ARG, "%s: DDIM tables missing", who);
    if (a->mode == 3 && (!a->lm_a || !a->lm_b || !a->lm_c || !a->lm_s || !a->x0_hist || (g && !g->hist_long)))
      return fail(FDM_ERR_ARG, "%s: table-driven sampler needs lm_a, lm_b, lm_c, lm_s, x0_hist%s", who, g ? " and hist_long" : "");
  }
  if (a->x_out_t && !kind_ok(a->out_dtype)) return fail(FDM_ERR_ARG, "%s: bad out_dtype %d", who, a->out_dtype);
  if (a->x_out_t && a->out_dtype == FDM_F16X3 && (a->x_out_t_lo_off <= 0 || a->x_out_t_lo_off % 4)) return fail(FDM_ERR_ARG, "%s: split x_out_t needs x_out_t_lo_off", who);
  if (!aligned16(a->x0) || !aligned16(a->x0u) || !aligned16(a->x) || !aligned16(a->x_out) || !aligned16(a->x_out_t) || !aligned16(a->x0_hist) || !aligned16(state) ||
      (g && (!aligned16(g->frames) || !aligned16(g->entries) || !aligned16(g->groups) || !aligned16(g->x_long) || !aligned16(g->hist_long))))
    return fail(FDM_ERR_ARG, "%s: operands%s and the state words must be 16-byte aligned", who, g ? ", table rows" : "");
  return FDM_OK;
}
// a bank form called without a bank: the null-operand check comes first, then check_bank refuses this one ("null bank table")
static const fdm_slot_bank_args no_bank = {};

// the pass's copy of the arguments: the fields no slot pass reads are cleared, and with a bank the step-indexed tables it holds
static fdm_sched_args slot_pass_args(const fdm_sched_args* a, bool bank) {
  fdm_sched_args c = *a;
  c.noise = nullptr; c.step = nullptr; c.tseq = nullptr; c.seed_dev = nullptr; c.arrive = nullptr;
  if (bank) { c.sqrt_an = c.c_n = nullptr; c.lm_a = c.lm_b = c.lm_c = c.lm_s = nullptr; }
  return c;
}

int fdm_op_slot_sched(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots, void* stream) {
  FCK(check_slot_pass(a, state, keys, n_slots, nullptr, nullptr, "slot_sched"));
  const fdm_sched_args c = slot_pass_args(a, false);
  return submit([c, state, keys](hipStream_t s) { return fdm::slot_sched_launch(c, state, keys, nullptr, s); }, stream, "slot_sched");
}

int fdm_op_slot_group_sched(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots,
                            const fdm_slot_group_args* g, void* stream) {
  if (!g) return fail(FDM_ERR_ARG, "slot_group_sched: null operand");
  FCK(check_slot_pass(a, state, keys, n_slots, g, nullptr, "slot_group_sched"));
  const fdm_sched_args c = slot_pass_args(a, false);
  const fdm_slot_group_args gg = *g;
  return submit([c, state, keys, gg, n_slots](hipStream_t s) { return fdm::slot_group_sched_launch(c, state, keys, gg, n_slots, nullptr, s); }, stream, "slot_group_sched");
}

int fdm_op_slot_sched_bank(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots,
                           const fdm_slot_bank_args* b, void* stream) {
  FCK(check_slot_pass(a, state, keys, n_slots, nullptr, b ? b : &no_bank, "slot_sched_bank"));
  const fdm_sched_args c = slot_pass_args(a, true);
  const fdm_slot_bank_args bb = *b;
  return submit([c, state, keys, bb](hipStream_t s) { return fdm::slot_sched_launch(c, state, keys, &bb, s); }, stream, "slot_sched_bank");
}

int fdm_op_slot_group_sched_bank(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots,
                                 const fdm_slot_group_args* g, const fdm_slot_bank_args* b, void* stream) {
  if (!g) return fail(FDM_ERR_ARG, "slot_group_sched_bank: null operand");
  FCK(check_slot_pass(a, state, keys, n_slots, g, b ? b : &no_bank, "slot_group_sched_bank"));
  const fdm_sched_args c = slot_pass_args(a, true);
  const fdm_slot_group_args gg = *g;
  const fdm_slot_bank_args bb = *b;
  return submit([c, state, keys, gg, n_slots, bb](hipStream_t s) { return fdm::slot_group_sched_launch(c, state, keys, gg, n_slots, &bb, s); }, stream,
                "slot_group_sched_bank");
}

}  // extern "C"

// the two small launches of the slot program that are not public operators (slots.hpp): recorded like any fdm_op_*
int fdm::slot_advance_op(int* state, const int* tseq, int n_steps, int n_slots, void* stream) {
  if (!state || !tseq || n_steps < 1 || n_slots < 1) return fail(FDM_ERR_ARG, "slot_advance: bad argument");
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::slot_advance_kernel, dim3(1), dim3(64), 0, s, (fdm::SlotState*)state, tseq, n_steps, n_slots);
    return hipGetLastError();
  }, stream, "slot_advance");
}
int fdm::slot_set_op(int* state, int slot, int k, int t, int live, int run, unsigned long long* keys, unsigned long long seed, int clip_id, void* stream) {
  if (!state || !keys || slot < 0) return fail(FDM_ERR_ARG, "slot_set: bad argument");
  const fdm::SlotState v{k, t, live, run};
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::slot_set_kernel, dim3(1), dim3(64), 0, s, (fdm::SlotState*)state + slot, v, keys + 2 * (size_t)slot, seed, (unsigned long long)(unsigned)clip_id);
    return hipGetLastError();
  }, stream, "slot_set");
}

// ... and their forms on a plan with a sampler bank
int fdm::slot_advance_bank_op(int* state, const fdm_slot_bank_args& b, int n_slots, void* stream) {
  if (!state || !b.req || !b.desc || !b.t || b.n_samplers < 1 || b.n_t < 1 || n_slots < 1) return fail(FDM_ERR_ARG, "slot_advance_bank: bad argument");
  const fdm_slot_bank_args bb = b;
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::slot_advance_bank_kernel, dim3(1), dim3(64), 0, s, (fdm::SlotState*)state, (const fdm::SlotReq*)bb.req, (const fdm::BankDesc*)bb.desc,
                       bb.t, bb.n_samplers, bb.n_t, n_slots);
    return hipGetLastError();
  }, stream, "slot_advance_bank");
}
int fdm::slot_set_bank_op(int* state, int slot, int k, int t, int live, int run, unsigned long long* keys, unsigned long long seed, int clip_id,
                          void* req, int sampler, float cfg_scale, void* stream) {
  if (!state || !keys || !req || slot < 0 || sampler < 0) return fail(FDM_ERR_ARG, "slot_set_bank: bad argument");
  const fdm::SlotState v{k, t, live, run};
  const fdm::SlotReq r{sampler, cfg_scale, 0, 0};
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::slot_set_bank_kernel, dim3(1), dim3(64), 0, s, (fdm::SlotState*)state + slot, v, keys + 2 * (size_t)slot, seed,
                       (unsigned long long)(unsigned)clip_id, (fdm::SlotReq*)req + slot, r);
    return hipGetLastError();
  }, stream, "slot_set_bank");
}
int fdm::slot_park_op(int* state, int slot, void* stream) {
  if (!state || slot < 0) return fail(FDM_ERR_ARG, "slot_park: bad argument");
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::slot_park_kernel, dim3(1), dim3(64), 0, s, (fdm::SlotState*)state + slot);
    return hipGetLastError();
  }, stream, "slot_park");
}

// windowed sampling's blend + scheduler pass (window.hpp): not a public operator -- the plan layer records it into the step program
// of a windowed plan (fdm_sample_windows)
int fdm::window_sched_op(const fdm_sched_args& a, const fdm::WinArgs& w, void* stream) {
  if (!a.x || !w.off || !w.ent || !w.xw || (!w.init && (!a.x0 || !a.x_out))) return fail(FDM_ERR_ARG, "window_sched: null operand");
  if (!w.init && a.mode == 3 && (!a.lm_a || !a.lm_b || !a.lm_c || !a.lm_s || !a.x0_hist)) return fail(FDM_ERR_ARG, "window_sched: table-driven sampler needs its tables and x0_hist");
  if (a.n <= 0 || a.n % 4 || w.d % 4 || w.L_total < 1 || w.W < 1 || w.n_win < 1 || a.n % ((long long)w.L_total * w.d))
    return fail(FDM_ERR_SHAPE, "window_sched: n=%lld is not a whole number of long clips of %d x %d", a.n, w.L_total, w.d);
  fdm_sched_args c = a;
  fdm::WinArgs ww = w;
  return submit([c, ww](hipStream_t s) { return fdm::window_launch(c, ww, s); }, stream, "window_sched");
}

extern "C" {

int fdm_op_cast(const float* src, void* dst, long long n, int dtype, void* stream) {
  if (!src || !dst || n <= 0) return fail(FDM_ERR_ARG, "cast: bad argument");
  if (!kind_ok(dtype)) return fail(FDM_ERR_ARG, "cast: bad dtype %d", dtype);
  return submit([=](hipStream_t s) {
    const dim3 g(grid_for(n)), b(256);
    if (dtype == FDM_BF16) hipLaunchKernelGGL((fdm::cast_kernel<fdm::bf16>), g, b, 0, s, src, (fdm::bf16*)dst, n);
    else if (dtype == FDM_F16X3) hipLaunchKernelGGL((fdm::cast_kernel<fdm::f16x3_t>), g, b, 0, s, src, (fdm::f16*)dst, n);
    else if (dtype == FDM_F16) hipLaunchKernelGGL((fdm::cast_kernel<fdm::f16>), g, b, 0, s, src, (fdm::f16*)dst, n);
    else hipLaunchKernelGGL((fdm::cast_kernel<float>), g, b, 0, s, src, (float*)dst, n);
    return hipGetLastError();
  }, stream, "cast");
}

int fdm_op_bias_act(const float* in, const float* vec, float* out, long long rows, int d, int act, void* stream) {
  if (!in || !out || rows <= 0 || d <= 0) return fail(FDM_ERR_ARG, "bias_act: bad argument");
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::bias_act_kernel, dim3(grid_for(rows * d)), dim3(256), 0, s, in, vec, out, rows, d, act);
    return hipGetLastError();
  }, stream, "bias_act");
}

int fdm_op_add_rows(const float* a, int a_div, int a_mod, const float* b, int b_div, int b_mod,
                    const float* c, int c_div, int c_mod, float* out, long long M, int d, void* stream) {
  if (!a || !out || M <= 0 || d <= 0 || a_div <= 0 || a_mod <= 0) return fail(FDM_ERR_ARG, "add_rows: bad argument");
  if ((b && (b_div <= 0 || b_mod <= 0)) || (c && (c_div <= 0 || c_mod <= 0))) return fail(FDM_ERR_ARG, "add_rows: bad div/mod");
  fdm::AddRowsArgs p{a, a_div, a_mod, b, b ? b_div : 1, b ? b_mod : 1, c, c ? c_div : 1, c ? c_mod : 1, out, M, d};
  return submit([p](hipStream_t s) {
    hipLaunchKernelGGL(fdm::add_rows_kernel, dim3(grid_for(p.M * p.d)), dim3(256), 0, s, p);
    return hipGetLastError();
  }, stream, "add_rows");
}

int fdm_op_small_linear(const float* x, const float* W, const float* bias, float* out, int B, int K, int d, int act, void* stream) {
  if (!x || !W || !out || B <= 0 || K <= 0 || d <= 0) return fail(FDM_ERR_ARG, "small_linear: bad argument");
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::small_linear_kernel, dim3((B * d + 255) / 256), dim3(256), 0, s, x, W, bias, out, B, K, d, act);
    return hipGetLastError();
  }, stream, "small_linear");
}

int fdm_op_cond_rows(const float* pe, const float* style, const float* emo, const float* sw, const float* sb, const float* ew,
                     const float* eb, float* out, long long uncond_off, int B, int L, int L_clip, int L_track, int d, int n_style,
                     int n_emo, int act, void* stream) {
  if (!pe || !style || !sw || !out) return fail(FDM_ERR_ARG, "cond_rows: null operand (pe, style track, style weight, out)");
  if (emo && !ew) return fail(FDM_ERR_ARG, "cond_rows: an emotion track needs the emotion weight");
  if (act < FDM_ACT_NONE || act > FDM_ACT_LEAKY02) return fail(FDM_ERR_ARG, "cond_rows: bad activation %d", act);
  if (B <= 0 || L <= 0 || d <= 0 || (long long)B * L > 0x7fffffffLL) return fail(FDM_ERR_SHAPE, "cond_rows: bad shape (B %d, L %d, d %d)", B, L, d);
  if (L_clip < 1 || L_clip > L || L_track < L_clip) return fail(FDM_ERR_SHAPE, "cond_rows: L_clip=%d outside [1, L %d] or beyond the track's %d rows per clip", L_clip, L, L_track);
  if (n_style < 1 || n_style > fdm::COND_ROWS_MAX_K || (emo && (n_emo < 1 || n_emo > fdm::COND_ROWS_MAX_K)))
    return fail(FDM_ERR_SHAPE, "cond_rows: vector widths (%d, %d) outside [1, %d]", n_style, n_emo, fdm::COND_ROWS_MAX_K);
  if (uncond_off < 0 || uncond_off % d || (uncond_off && uncond_off < (long long)B * L * d))
    return fail(FDM_ERR_SHAPE, "cond_rows: uncond_off=%lld is not a whole number of rows past the cond half", uncond_off);
  fdm::CondRowsArgs p{pe, style, emo, sw, sb, ew, eb, out, uncond_off, B * L, L, L_clip, L_track, d, n_style, emo ? n_emo : 0, act};
  return submit([p](hipStream_t s) {
    hipLaunchKernelGGL(fdm::cond_rows_kernel, dim3((unsigned)p.rows), dim3(256), 0, s, p);
    return hipGetLastError();
  }, stream, "cond_rows");
}

// The ops that exist in a fixed and a ragged (`_lens`) form share one implementation each: `ragged` chooses the kernel instantiation
// (lens is null and unread in the fixed form) and `name` is the entry's name in its messages.
static int pad_rows_impl(const char* name, const void* in, void* out, int B, int L, int d, int pad, int dtype, int zero, bool ragged, const int* lens,
                         void* stream) {
  if (!in || !out || (ragged && !lens) || B <= 0 || L <= 0 || d <= 0 || pad < 0) return fail(FDM_ERR_ARG, "%s: bad argument", name);
  if (!kind_ok(dtype)) return fail(FDM_ERR_ARG, "%s: bad dtype %d", name, dtype);
  const long long n = (long long)B * (L + 2 * pad) * d;
  return submit([=](hipStream_t s) {
    with_move_type(dtype, [&](auto tag) {
      using T = decltype(tag);
      const auto k = ragged ? fdm::pad_rows_kernel<T, true> : fdm::pad_rows_kernel<T, false>;
      hipLaunchKernelGGL(k, dim3(grid_for(n)), dim3(256), 0, s, (const T*)in, (T*)out, B, L, d, pad, zero, lens);
    });
    return hipGetLastError();
  }, stream, name);
}
int fdm_op_pad_rows(const void* in, void* out, int B, int L, int d, int pad, int dtype, int zero, void* stream) {
  return pad_rows_impl("pad_rows", in, out, B, L, d, pad, dtype, zero, false, nullptr, stream);
}
int fdm_op_pad_rows_lens(const void* in, void* out, int B, int L, int d, int pad, int dtype, const int* lens, void* stream) {
  return pad_rows_impl("pad_rows_lens", in, out, B, L, d, pad, dtype, 0, true, lens, stream);
}

int fdm_op_zero_pad_rows(float* x, int B, int L, int d, const int* lens, void* stream) {
  if (!x || !lens || B <= 0 || L <= 0 || d <= 0) return fail(FDM_ERR_ARG, "zero_pad_rows: bad argument");
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::zero_pad_rows_kernel, dim3(grid_for((long long)B * L * d)), dim3(256), 0, s, x, B, L, d, lens);
    return hipGetLastError();
  }, stream, "zero_pad_rows");
}

static int group_pad_impl(const char* name, const void* in, void* out, int B, int T, int d, int groups, int pad, int dtype, bool ragged, const int* lens,
                          void* stream) {
  if (!in || !out || (ragged && !lens) || B <= 0 || T <= 0 || d <= 0 || groups <= 0 || d % groups || pad < 0) return fail(FDM_ERR_ARG, "%s: bad argument", name);
  if (!kind_ok(dtype)) return fail(FDM_ERR_ARG, "%s: bad dtype %d", name, dtype);
  const long long n = (long long)B * (T + 2 * pad) * d;
  return submit([=](hipStream_t s) {
    with_move_type(dtype, [&](auto tag) {
      using E = decltype(tag);
      const auto k = ragged ? fdm::group_pad_kernel<E, true> : fdm::group_pad_kernel<E, false>;
      hipLaunchKernelGGL(k, dim3(grid_for(n)), dim3(256), 0, s, (const E*)in, (E*)out, B, T, d, groups, pad, lens);
    });
    return hipGetLastError();
  }, stream, name);
}
int fdm_op_group_pad(const void* in, void* out, int B, int T, int d, int groups, int pad, int dtype, void* stream) {
  return group_pad_impl("group_pad", in, out, B, T, d, groups, pad, dtype, false, nullptr, stream);
}
int fdm_op_group_pad_lens(const void* in, void* out, int B, int T, int d, int groups, int pad, int dtype, const int* lens, void* stream) {
  return group_pad_impl("group_pad_lens", in, out, B, T, d, groups, pad, dtype, true, lens, stream);
}

int fdm_op_mask_samples(const float* wav, float* out, int B, int n, const int* lens, void* stream) {
  if (!wav || !out || !lens || B <= 0 || n <= 0) return fail(FDM_ERR_ARG, "mask_samples: bad argument");
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::mask_samples_kernel, dim3(grid_for((long long)B * n)), dim3(256), 0, s, wav, out, B, n, lens);
    return hipGetLastError();
  }, stream, "mask_samples");
}

int fdm_op_set_ints(int* dst, const int* src, int n, void* stream) {
  if (!dst || !src || n <= 0) return fail(FDM_ERR_ARG, "set_ints: bad argument");
  for (int i0 = 0; i0 < n; i0 += 64) {
    fdm::IntPack p;
    const int m = n - i0 < 64 ? n - i0 : 64;
    for (int i = 0; i < 64; ++i) p.v[i] = i < m ? src[i0 + i] : 0;
    int* d = dst + i0;
    const int r = submit([=](hipStream_t s) {
      hipLaunchKernelGGL(fdm::set_ints_kernel, dim3(1), dim3(64), 0, s, d, p, m);
      return hipGetLastError();
    }, stream, "set_ints");
    if (r != FDM_OK) return r;
  }
  return FDM_OK;
}

int fdm_op_conv0(const float* wav, const float* w, const float* bias, float* out, int B, int n, int T0, void* stream) {
  if (!wav || !w || !out || B <= 0 || n < 10 || T0 != (n - 10) / 5 + 1) return fail(FDM_ERR_SHAPE, "conv0: bad shape (n=%d, T0=%d)", n, T0);
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::conv0_kernel, dim3((T0 + 15) / 16, B), dim3(256), 0, s, wav, w, bias, out, n, T0);
    return hipGetLastError();
  }, stream, "conv0");
}

int fdm_op_conv0_ln_gelu(const float* wav, const float* w, const float* bias, const float* gamma, const float* beta, void* out,
                         long long out_lo_off, int B, int n, int T0, float eps, int dtype, void* stream) {
  if (!wav || !w || !gamma || !beta || !out || B <= 0 || n < 10 || T0 != (n - 10) / 5 + 1) return fail(FDM_ERR_SHAPE, "conv0_ln_gelu: bad shape (n=%d, T0=%d)", n, T0);
  if (dtype != FDM_F32 && dtype != FDM_BF16 && dtype != FDM_F16X3) return fail(FDM_ERR_ARG, "conv0_ln_gelu: dtype %d (fp32, bf16 or FDM_F16X3 output)", dtype);
  if (dtype == FDM_F16X3 && out_lo_off <= 0) return fail(FDM_ERR_ARG, "conv0_ln_gelu: split output needs out_lo_off");
  return submit([=](hipStream_t s) {
    const dim3 grid((T0 + 31) / 32, B);       // 4 waves x 8 frames per workgroup
    if (dtype == FDM_BF16) hipLaunchKernelGGL((fdm::conv0_ln_gelu_kernel<fdm::bf16>), grid, dim3(256), 0, s, wav, w, bias, gamma, beta, (fdm::bf16*)out, 0LL, n, T0, eps);
    else if (dtype == FDM_F16X3) hipLaunchKernelGGL((fdm::conv0_ln_gelu_kernel<fdm::f16x3_t>), grid, dim3(256), 0, s, wav, w, bias, gamma, beta, (fdm::f16*)out, out_lo_off, n, T0, eps);
    else hipLaunchKernelGGL((fdm::conv0_ln_gelu_kernel<float>), grid, dim3(256), 0, s, wav, w, bias, gamma, beta, (float*)out, 0LL, n, T0, eps);
    return hipGetLastError();
  }, stream, "conv0_ln_gelu");
}

static int leaky_instnorm_impl(const char* name, const float* x, float* y_f32, void* y_t, int B, int L, int d, float eps, int dtype, bool ragged,
                               const int* lens, void* stream) {
  if (!x || (!y_f32 && !y_t) || (ragged && !lens) || B <= 0 || L <= 0 || d <= 0) return fail(FDM_ERR_ARG, "%s: bad argument", name);
  if (!kind_ok(dtype)) return fail(FDM_ERR_ARG, "%s: bad dtype %d", name, dtype);
  if (y_t && dtype != FDM_F32 && dtype != FDM_BF16) return fail(FDM_ERR_ARG, "%s: y_t dtype %d (fp32 or bf16 output)", name, dtype);
  return submit([=](hipStream_t s) {
    const dim3 grid((d + 63) / 64, B);
    const auto launch = [&](auto tag) {
      using T = decltype(tag);
      const auto k = ragged ? fdm::leaky_instnorm_kernel<T, true> : fdm::leaky_instnorm_kernel<T, false>;
      hipLaunchKernelGGL(k, grid, dim3(1024), 0, s, x, y_f32, (T*)y_t, L, d, eps, lens);
    };
    if (dtype == FDM_BF16) launch(fdm::bf16{});
    else launch(float{});
    return hipGetLastError();
  }, stream, name);
}
int fdm_op_leaky_instnorm(const float* x, float* y_f32, void* y_t, int B, int L, int d, float eps, int dtype, void* stream) {
  return leaky_instnorm_impl("leaky_instnorm", x, y_f32, y_t, B, L, d, eps, dtype, false, nullptr, stream);
}
int fdm_op_leaky_instnorm_lens(const float* x, float* y_f32, void* y_t, int B, int L, int d, float eps, int dtype, const int* lens, void* stream) {
  return leaky_instnorm_impl("leaky_instnorm_lens", x, y_f32, y_t, B, L, d, eps, dtype, true, lens, stream);
}

// Clips of TIME_CHUNKED_FROM frames or more take the chunked form (statistics and normalisation over time chunks: two launches, hundreds
// of workgroups), which needs scratch.  The two forms differ on purpose when the scratch is missing, too small or misaligned: the fixed
// form falls back to the three-pass kernel; the ragged form, whose clips must take the form of their own launch, refuses.
static int time_groupnorm_impl(const char* name, const float* x, const float* gamma, const float* beta, float* y_f32, void* y_t, long long y_t_lo_off,
                               int B, int T, int C, float eps, int act, int dtype, void* scratch, long long scratch_bytes, bool ragged, const int* lens,
                               void* stream) {
  if (!x || (!y_f32 && !y_t) || (ragged && !lens) || B <= 0 || T <= 0 || C <= 0) return fail(FDM_ERR_ARG, "%s: bad argument", name);
  if (!kind_ok(dtype)) return fail(FDM_ERR_ARG, "%s: bad dtype %d", name, dtype);
  if (y_t && dtype == FDM_F16) return fail(FDM_ERR_ARG, "%s: y_t dtype %d (fp32, bf16 or FDM_F16X3 output)", name, dtype);
  if (y_t && dtype == FDM_F16X3 && y_t_lo_off <= 0) return fail(FDM_ERR_ARG, "%s: split y_t needs y_t_lo_off", name);
  int chunk;
  const int nch = T >= fdm::TIME_CHUNKED_FROM ? fdm::time_chunks_of(T, &chunk) : 0;
  const long long need = (long long)B * nch * C * 2 * (long long)sizeof(double);
  const bool chunked = nch && scratch && scratch_bytes >= need && ((uintptr_t)scratch % 8) == 0;
  if (ragged && nch && !chunked) return fail(FDM_ERR_ARG, "%s: T = %d needs %lld bytes of 8-byte aligned scratch", name, T, need);
  double* part = (double*)scratch;
  return submit([=](hipStream_t s) {
    const dim3 g1((C + 63) / 64, B), g2((C + 63) / 64, nch ? nch : 1, B);
    with_out_kind(dtype, y_t_lo_off, [&](auto tag, long long lo) {
      using K = decltype(tag);
      auto* yt = (typename fdm::Opnd<K>::E*)y_t;
      if (ragged || !chunked) {      // (ragged: every form is launched, a workgroup whose clip belongs to the other form leaves at once)
        const auto k = ragged ? fdm::time_groupnorm_kernel<K, true> : fdm::time_groupnorm_kernel<K, false>;
        hipLaunchKernelGGL(k, g1, dim3(1024), 0, s, x, gamma, beta, y_f32, yt, lo, T, C, eps, act, lens);
      }
      if (chunked) {
        const auto ks = ragged ? fdm::time_stats_kernel<true> : fdm::time_stats_kernel<false>;
        const auto ka = ragged ? fdm::time_norm_apply_kernel<K, true> : fdm::time_norm_apply_kernel<K, false>;
        hipLaunchKernelGGL(ks, g2, dim3(1024), 0, s, x, part, T, C, lens);
        hipLaunchKernelGGL(ka, g2, dim3(1024), 0, s, x, (const double*)part, gamma, beta, y_f32, yt, lo, T, C, eps, act, lens);
      }
    });
    return hipGetLastError();
  }, stream, name);
}
int fdm_op_time_groupnorm(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_t, long long y_t_lo_off, int B, int T, int C,
                          float eps, int act, int dtype, void* scratch, long long scratch_bytes, void* stream) {
  return time_groupnorm_impl("time_groupnorm", x, gamma, beta, y_f32, y_t, y_t_lo_off, B, T, C, eps, act, dtype, scratch, scratch_bytes, false, nullptr, stream);
}
int fdm_op_time_groupnorm_lens(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_t, long long y_t_lo_off, int B, int T, int C,
                               float eps, int act, int dtype, void* scratch, long long scratch_bytes, const int* lens, void* stream) {
  return time_groupnorm_impl("time_groupnorm_lens", x, gamma, beta, y_f32, y_t, y_t_lo_off, B, T, C, eps, act, dtype, scratch, scratch_bytes, true, lens, stream);
}

int fdm_op_mean_diff(const float* a, const float* b, float* partial, float* out, long long n, int l1, void* stream) {
  if (!a || !b || !partial || !out || n <= 0) return fail(FDM_ERR_ARG, "mean_diff: bad argument");
  return submit([=](hipStream_t s) {
    const int nb = grid_for(n) > 1024 ? 1024 : grid_for(n);
    hipLaunchKernelGGL(fdm::diff_partial_kernel, dim3(nb), dim3(256), 0, s, a, b, partial, n, l1);
    hipLaunchKernelGGL(fdm::diff_final_kernel, dim3(1), dim3(256), 0, s, (const float*)partial, nb, 1.0f / (float)n, out);
    return hipGetLastError();
  }, stream, "mean_diff");
}

int fdm_op_vertex_err(const float* gt, const float* pred, const int* region, int R, int F, int V,
                      float* frame_max, double* frame_sum, double* out, void* stream) {
  if (!gt || !pred || !frame_max || !frame_sum || !out) return fail(FDM_ERR_ARG, "vertex_err: null operand");
  if (F <= 0 || V <= 0 || R <= 0 || (!region && R != V)) return fail(FDM_ERR_SHAPE, "vertex_err: bad shape (F %d, V %d, R %d)", F, V, R);
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::vertex_err_kernel, dim3(F), dim3(256), 0, s, gt, pred, region, R, V, frame_max, frame_sum);
    hipLaunchKernelGGL(fdm::vertex_err_final_kernel, dim3(1), dim3(256), 0, s, (const float*)frame_max, (const double*)frame_sum, F, R, out);
    return hipGetLastError();
  }, stream, "vertex_err");
}

int fdm_op_motion_std(const float* verts, const float* tmpl, const int* region, int R, int F, int V,
                      double* partial, double* out, void* stream) {
  if (!verts || !tmpl || !partial || !out) return fail(FDM_ERR_ARG, "motion_std: null operand");
  if (F <= 0 || V <= 0 || R <= 0 || (!region && R != V)) return fail(FDM_ERR_SHAPE, "motion_std: bad shape (F %d, V %d, R %d)", F, V, R);
  return submit([=](hipStream_t s) {
    const int FC = F < 64 ? F : 64;
    hipLaunchKernelGGL(fdm::motion_partial_kernel, dim3((R + 255) / 256, FC), dim3(256), 0, s, verts, tmpl, region, R, F, V, partial);
    hipLaunchKernelGGL(fdm::motion_final_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, FC, R, F, out);
    return hipGetLastError();
  }, stream, "motion_std");
}

int fdm_op_linear_interp(const float* x, float* y, int B, int Tin, int Tout, int C, void* stream) {
  if (!x || !y || B <= 0 || Tin <= 0 || Tout <= 0 || C <= 0) return fail(FDM_ERR_ARG, "linear_interp: bad argument");
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::linear_interp_kernel, dim3(grid_for((long long)B * Tout * C)), dim3(256), 0, s, x, y, B, Tin, Tout, C);
    return hipGetLastError();
  }, stream, "linear_interp");
}

int fdm_op_adain(const float* content, const float* style, float* out, int NC, int Lc, int Ls, float eps, void* stream) {
  if (!content || !style || !out || NC <= 0 || Lc < 2 || Ls < 2) return fail(FDM_ERR_ARG, "adain: bad argument");
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::adain_kernel, dim3((NC + 3) / 4), dim3(256), 0, s, content, style, out, NC, Lc, Ls, eps);
    return hipGetLastError();
  }, stream, "adain");
}

int fdm_op_vq_quant(const float* z, const float* codebook, const int* book, int B, int R, int c, int K,
                    float* zq_bcl, long long* idx, void* stream) {
  if (!z || !codebook || !zq_bcl || !idx) return fail(FDM_ERR_ARG, "vq_quant: null operand");
  if (B <= 0 || R <= 0 || K <= 0 || c <= 0 || c > 128) return fail(FDM_ERR_SHAPE, "vq_quant: bad shape (c=%d must be <= 128)", c);
  return submit([=](hipStream_t s) {
    const long long rows = (long long)B * R;
    hipLaunchKernelGGL(fdm::vq_quant_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, z, codebook, book, B, R, c, K, zq_bcl, idx);
    return hipGetLastError();
  }, stream, "vq_quant");
}

int fdm_op_vq_stats(const float* z, const float* codebook, const int* book, const long long* idx, int B, int R, int c, int K, float beta,
                    float* min_encodings, double* partial, int* hist, float* out, void* stream) {
  if (!z || !codebook || !idx || !partial || !hist || !out) return fail(FDM_ERR_ARG, "vq_stats: null operand");
  if (B <= 0 || R <= 0 || K <= 0 || c <= 0) return fail(FDM_ERR_SHAPE, "vq_stats: bad shape");
  const long long rows = (long long)B * R;
  const int nblk = (int)std::min<long long>(1024, (rows + 3) / 4);
  return submit([=](hipStream_t s) {
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)K * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fdm::vq_stats_partial_kernel, dim3(nblk), dim3(256), 0, s, z, codebook, book, idx, B, R, c, K, min_encodings, partial, hist);
    hipLaunchKernelGGL(fdm::vq_stats_final_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, nblk, (const int*)hist, K, rows, c, beta, out);
    return hipGetLastError();
  }, stream, "vq_stats");
}

// ---- per-row codebook (condition tracks): book has one entry per latent vector, [B * R] ------------------------------------------
int fdm_op_argmax_rows(const float* x, int* book, long long rows, int n, int rep, int n_books, void* stream) {
  if (!x || !book) return fail(FDM_ERR_ARG, "argmax_rows: null operand");
  if (rows <= 0 || n <= 0 || rep <= 0 || rows * rep > 0x7fffffffLL) return fail(FDM_ERR_SHAPE, "argmax_rows: bad shape (rows %lld, n %d, rep %d)", rows, n, rep);
  if (n_books < 1 || n > n_books) return fail(FDM_ERR_SHAPE, "argmax_rows: an argmax over %d columns can name a book outside the %d of the codebook", n, n_books);
  return submit([=](hipStream_t s) {
    hipLaunchKernelGGL(fdm::argmax_rows_rep_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, x, book, rows, n, rep);
    return hipGetLastError();
  }, stream, "argmax_rows");
}

int fdm_op_vq_quant_rows(const float* z, const float* codebook, const int* book_rows, int n_books, int B, int R, int c, int K,
                         float* zq_bcl, long long* idx, void* stream) {
  if (!z || !codebook || !book_rows || !zq_bcl || !idx) return fail(FDM_ERR_ARG, "vq_quant_rows: null operand");
  if (B <= 0 || R <= 0 || K <= 0 || c <= 0 || c > 128) return fail(FDM_ERR_SHAPE, "vq_quant_rows: bad shape (c=%d must be <= 128)", c);
  if (n_books < 1) return fail(FDM_ERR_SHAPE, "vq_quant_rows: n_books=%d", n_books);
  return submit([=](hipStream_t s) {
    const long long rows = (long long)B * R;
    hipLaunchKernelGGL(fdm::vq_quant_rowbook_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, z, codebook, book_rows, n_books, B, R, c, K, zq_bcl, idx);
    return hipGetLastError();
  }, stream, "vq_quant_rows");
}

int fdm_op_vq_stats_rows(const float* z, const float* codebook, const int* book_rows, int n_books, const long long* idx, int B, int R, int c,
                         int K, float beta, float* min_encodings, double* partial, int* hist, float* out, void* stream) {
  if (!z || !codebook || !book_rows || !idx || !partial || !hist || !out) return fail(FDM_ERR_ARG, "vq_stats_rows: null operand");
  if (B <= 0 || R <= 0 || K <= 0 || c <= 0) return fail(FDM_ERR_SHAPE, "vq_stats_rows: bad shape");
  if (n_books < 1) return fail(FDM_ERR_SHAPE, "vq_stats_rows: n_books=%d", n_books);
  const long long rows = (long long)B * R;
  const int nblk = (int)std::min<long long>(1024, (rows + 3) / 4);
  return submit([=](hipStream_t s) {
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)K * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fdm::vq_stats_partial_rowbook_kernel, dim3(nblk), dim3(256), 0, s, z, codebook, book_rows, n_books, idx, B, R, c, K, min_encodings, partial, hist);
    hipLaunchKernelGGL(fdm::vq_stats_final_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, nblk, (const int*)hist, K, rows, c, beta, out);
    return hipGetLastError();
  }, stream, "vq_stats_rows");
}

// ---------------------------------------------------------------------------------------------
// step programs
// ---------------------------------------------------------------------------------------------
int fdm_prog_create(fdm_prog** out) {
  if (!out) return fail(FDM_ERR_ARG, "prog_create: null out");
  *out = new (std::nothrow) fdm_prog();
  return *out ? FDM_OK : fail(FDM_ERR_STATE, "prog_create: out of memory");
}

int fdm_prog_destroy(fdm_prog* p) {
  if (!p) return FDM_OK;
  if (g_rec == p) g_rec = nullptr;
  if (p->exec) (void)hipGraphExecDestroy(p->exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  delete p;
  return FDM_OK;
}

int fdm_prog_begin(fdm_prog* p) {
  if (!p) return fail(FDM_ERR_ARG, "prog_begin: null program");
  if (g_rec) return fail(FDM_ERR_STATE, "prog_begin: another program is recording on this thread");
  if (p->exec) return fail(FDM_ERR_STATE, "prog_begin: program already instantiated");
  g_rec = p;
  return FDM_OK;
}

int fdm_prog_end(fdm_prog* p) {
  if (!p || g_rec != p) return fail(FDM_ERR_STATE, "prog_end: program is not recording");
  g_rec = nullptr;
  return FDM_OK;
}

int fdm_prog_num_ops(fdm_prog* p) { return p ? (int)p->ops.size() : 0; }

int fdm_prog_run(fdm_prog* p, void* stream) {
  if (!p) return fail(FDM_ERR_ARG, "prog_run: null program");
  if (g_rec) return fail(FDM_ERR_STATE, "prog_run: a program is still recording");
  for (auto& op : p->ops) {
    hipError_t e = op((hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "prog_run");
  }
  return FDM_OK;
}

int fdm_prog_instantiate(fdm_prog* p, void* stream) {
  if (!p) return fail(FDM_ERR_ARG, "prog_instantiate: null program");
  if (g_rec) return fail(FDM_ERR_STATE, "prog_instantiate: a program is still recording");
  if (p->exec) return FDM_OK;
  if (p->ops.empty()) return fail(FDM_ERR_STATE, "prog_instantiate: empty program");
  (void)stream;
  // Capture never executes anything, so it runs on a stream of the library's own: the caller's stream may be the legacy
  // default stream (torch's current stream usually is), which cannot be captured.  (Independent chains as parallel branches
  // of one graph, or as graphs on separate streams, were measured slower than one chain over all rows -- rounds 1 and 3,
  // profiles/README.md -- and are no longer offered.)
  hipStream_t cap = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&cap, hipStreamNonBlocking);
  if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
  struct CapGuard { hipStream_t s; ~CapGuard() { if (s) (void)hipStreamDestroy(s); } } guard{cap};
  e = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return hip_fail(e, "hipStreamBeginCapture");
  hipError_t opErr = hipSuccess;
  for (size_t i = 0; opErr == hipSuccess && i < p->ops.size(); ++i) opErr = p->ops[i](cap);
  hipGraph_t g = nullptr;
  e = hipStreamEndCapture(cap, &g);
  // a failure part-way leaves no half-built state behind: a later instantiate starts over, replay keeps failing loudly
  if (opErr != hipSuccess) { if (g) (void)hipGraphDestroy(g); return hip_fail(opErr, "prog_instantiate (launch during capture)"); }
  if (e != hipSuccess) return hip_fail(e, "hipStreamEndCapture");
  hipGraphExec_t x = nullptr;
  e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g); return hip_fail(e, "hipGraphInstantiate"); }
  p->graph = g;
  p->exec = x;
  return FDM_OK;
}

int fdm_prog_replay(fdm_prog* p, int n, void* stream) {
  if (!p || !p->exec) return fail(FDM_ERR_STATE, "prog_replay: program not instantiated");
  for (int i = 0; i < n; ++i) {
    const hipError_t e = hipGraphLaunch(p->exec, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipGraphLaunch");
  }
  return FDM_OK;
}

}  // extern "C"
