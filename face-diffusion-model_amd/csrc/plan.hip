// Plan layer of libfdm_hip.so (include/fdm_hip.h, "Plan layer"): the FDM denoiser + diffusion scheduler of one model
// behind plain C calls.  What the reference does in FDM.__init__ / FDM.forward (models/fdm_vocaset.py:9-91,
// models/fdm_vqvae_mead.py:9-104, models/fdm.py:10-99) and GaussianDiffusion.p_sample_loop / ddim_sample
// (video_diffusion_pytorch/diffusion_BIWI_encoder_decoder.py:649-710) is split here into
//   commit   (once per model)   operand-kind weight copies, tau table, folded cross-attention time tables, LayerNorm folds
//   prepare  (once per batch)   AF = audio_extract(features), per-layer tables C1_l, conditioning addend E0
//   step program (per step)     recorded once through fdm_op_*, captured into a hipGraph, replayed with t from a device counter
// All arithmetic runs in the library's own kernels (no torch, no vendor BLAS); host code only sequences launches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "common.hpp"
#include "plan.hpp"

std::string fdm::shape_key(const fdm_plan* P) {
  // (the K-slice factors belong to the key: a tile set tuned without slices holds tiles a sliced launch cannot run on, and the other
  //  way round -- in the in-process cache and in the FDM_TILE_CACHE file alike)
  char b[80];
  snprintf(b, sizeof(b), "%d,%d,%d,%d,%d,ks%d.%d", P->R, P->M, P->L, P->rep, P->S, P->ksplit_out, P->ksplit_ffn2);
  return b;
}

int fdm::drop_programs(fdm_plan* P, void* stream) {
  if (P->progs.empty()) return FDM_OK;
  // graph execs / kernarg storage may still be referenced by queued replays: drain the stream they were launched on first
  if (stream) HIPCK(hipStreamSynchronize((hipStream_t)stream));
  else HIPCK(hipDeviceSynchronize());
  for (auto& kv : P->progs) fdm_prog_destroy(kv.second);
  P->progs.clear();
  P->prog_order.clear();
  P->pinned.clear();
  return FDM_OK;
}

namespace {
using namespace fdm;

// ---------------------------------------------------------------------------------------------------------------------
// one-time weight preparation kernels (plan commit)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void transpose_kernel(const float* in, float* out, int rows, int cols) {      // out[c][r] = in[r][c]
  const long long n = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i / rows), r = (int)(i % rows);
    out[i] = in[(size_t)r * cols + c];
  }
}
__global__ void scale_cols_kernel(const float* W, const float* gamma, float* out, long long n, int K) {   // out[j][k] = W[j][k] * gamma[k]
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = W[i] * gamma[i % K];
}
// out[j] = sum_k (float) Wt[j][k]: one wavefront per row, fixed order (lane-strided partial sums, then the DPP tree)
__global__ __launch_bounds__(256) void rowsum_bf16_kernel(const fdm::bf16* W, float* out, int N, int K) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += (float)W[(size_t)row * K + k];
  s = fdm::wave_sum(s);
  if (lane == 0) out[row] = s;
}
// the same for a split operand: the value a GEMM sees is hi + lo / scale
template <typename E>
__global__ __launch_bounds__(256) void rowsum_split_kernel(const E* W, long long lo_off, float inv_scale, float* out, int N, int K) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += (float)W[(size_t)row * K + k] + (float)W[lo_off + (size_t)row * K + k] * inv_scale;
  s = fdm::wave_sum(s);
  if (lane == 0) out[row] = s;
}

// Every plan buffer starts zeroed (pad keys must be finite; counters, histories and partial planes start at 0).  Each allocation
// names the arena it lives in: P->mem (plan lifetime), P->ws (per capacity), P->cmem (per commit).
template <typename T> int zalloc(Arena& a, T** out, size_t n) { return a.alloc_t(out, n, true); }
// operand-kind matrix [rows, cols]: plain, or two consecutive planes for the split kinds
int zalloc_mat(const fdm_plan* P, Arena& a, Mat* out, size_t rows, size_t cols) {
  const size_t n = rows * cols;
  out->lo = kind(P->dtype).planes == 2 ? (long long)n : 0;
  return a.alloc(&out->p, n * kind(P->dtype).full(), true);
}

const Wt* weight(const fdm_plan* P, const std::string& name) {
  auto it = P->w.find(name);
  return it == P->w.end() ? nullptr : &it->second;
}
int need(const fdm_plan* P, const std::string& name, long long n, const float** out) { return need_weight(P->w, "plan: ", name, n, out); }

fdm_gemm_args gemm_op(const fdm_plan* P, const Mat& A, const Mat& W, int M, int N, int K) {
  fdm_gemm_args a = dense_gemm(P->dtype, A.p, W.p, M, N, K);
  a.a_lo_off = A.lo; a.w_lo_off = W.lo;
  return a;
}
void set_out_t(fdm_gemm_args& a, const Mat& o) { a.out_t = o.p; a.out_t_lo_off = o.lo; }

// a GEMM that applies the folded norm3 (fuse_ln3) reads the per-row partial sums the FFN2 GEMM left in ws.stats
void set_ln_stats(fdm_gemm_args& g, const fdm_plan* P) { g.ln_stat_in = P->stats; g.ln_nparts = P->m.d / 64; g.ln_dim = P->m.d; g.ln_eps = 1e-5f; }
// K slices of a GEMM whose fp32 output row a LayerNorm launch reads next: S partial planes of x1, summed by that launch
void set_ksplit(fdm_gemm_args& g, int S, long long plane) { if (S > 1) { g.ksplit = S; g.ksplit_stride = plane; } }
void set_ksplit(fdm_ln_args& ln, int S, long long plane) { if (S > 1) { ln.x_planes = S; ln.x_plane_stride = plane; } }

int plan_gemm(fdm_plan* P, const char* label, fdm_gemm_args a, void* stream) {
  if (P->tune_rec) (*P->tune_rec)[label].push_back(a);
  auto it = P->tiles.find(label);
  a.tile = (it == P->tiles.end() ? 0 : it->second) | (P->lockstep ? FDM_TILE_LOCKSTEP : 0);
  return fdm_op_gemm(&a, stream);
}

std::string lname(int l, const char* suffix) {
  char b[96];
  snprintf(b, sizeof(b), "transformer_decoder.layers.%d.%s", l, suffix);
  return b;
}

// ---------------------------------------------------------------------------------------------------------------------
// commit: per-model tables
// ---------------------------------------------------------------------------------------------------------------------
int commit_impl(fdm_plan* P, void* stream) {
  const fdm_model_desc& m = P->m;
  const int d = m.d;
  hipStream_t s = (hipStream_t)stream;
  FCK(drop_programs(P, stream));
  const float* p = nullptr;
  FCK(need(P, "audio_extract.0.weight", (long long)d * m.audio_in, &p));
  FCK(need(P, "audio_extract.0.bias", d, &p));
  FCK(need(P, "audio_extract.2.weight", (long long)d * d, &p));
  FCK(need(P, "audio_extract.2.bias", d, &p));
  FCK(need(P, "style_embedd.weight", (long long)d * m.n_style, &p));
  FCK(need(P, "style_embedd.bias", d, &p));
  if (m.n_emo) { FCK(need(P, "emotion_embedd.weight", (long long)d * m.n_emo, &p)); FCK(need(P, "emotion_embedd.bias", d, &p)); }
  FCK(need(P, "latent_encoder.0.bias", d, &p));
  FCK(need(P, "latent_decoder.bias", d, &p));
  // operand-kind copies of the per-step matrices
  std::vector<std::pair<std::string, long long>> mats = {{"latent_encoder.0.weight", (long long)d * d}, {"latent_decoder.weight", (long long)d * d}};
  for (int l = 0; l < m.n_layers; ++l) {
    mats.push_back({lname(l, "self_attn.in_proj_weight"), 3LL * d * d});
    mats.push_back({lname(l, "self_attn.out_proj.weight"), (long long)d * d});
    mats.push_back({lname(l, "linear1.weight"), (long long)m.ffn * d});
    mats.push_back({lname(l, "linear2.weight"), (long long)d * m.ffn});
    for (const char* b : {"self_attn.in_proj_bias", "self_attn.out_proj.bias", "linear1.bias", "linear2.bias", "norm1.weight", "norm1.bias",
                          "norm2.weight", "norm2.bias", "norm3.weight", "norm3.bias"}) {
      const long long nb = !strcmp(b, "self_attn.in_proj_bias") ? 3LL * d : (!strcmp(b, "linear1.bias") ? m.ffn : d);
      FCK(need(P, lname(l, b), nb, &p));
    }
  }
  for (auto& mt : mats) {
    FCK(need(P, mt.first, mt.second, &p));
    Mat o;
    FCK(to_operand(P->cmem, P->dtype, p, mt.second, &o, stream));
    P->wt[mt.first] = o;
  }
  // tau table [1000, d] = Mish(W_t^T + b_t): Linear(one_hot(t)) is a column gather (models/fdm_vocaset.py:71-72)
  const float *Wt_ = nullptr, *bt = nullptr;
  FCK(need(P, "time_embedd.0.weight", (long long)d * 1000, &Wt_));
  FCK(need(P, "time_embedd.0.bias", d, &bt));
  float* wtT = nullptr;
  FCK(zalloc(P->cmem, &wtT, (size_t)1000 * d));
  FCK(zalloc(P->cmem, &P->tau, (size_t)1000 * d));
  hipLaunchKernelGGL(transpose_kernel, dim3(grid_for(1000LL * d)), dim3(256), 0, s, Wt_, wtT, d, 1000);
  FCK(fdm_op_bias_act(wtT, bt, P->tau, 1000, d, FDM_ACT_MISH, stream));
  // folded cross-attention time tables TT_l = (tau Wv_l^T) Wo_l^T: fp32 MFMA, one-time
  float* tmp = nullptr;
  FCK(zalloc(P->cmem, &tmp, (size_t)1000 * d));
  P->TT.assign(m.n_layers, nullptr);
  P->Wv.assign(m.n_layers, nullptr); P->bv = P->Wo = P->bo = P->Wv;
  for (int l = 0; l < m.n_layers; ++l) {
    const float *ipw = nullptr, *ipb = nullptr;
    FCK(need(P, lname(l, "multihead_attn.in_proj_weight"), 3LL * d * d, &ipw));
    FCK(need(P, lname(l, "multihead_attn.in_proj_bias"), 3LL * d, &ipb));
    FCK(need(P, lname(l, "multihead_attn.out_proj.weight"), (long long)d * d, &P->Wo[l]));
    FCK(need(P, lname(l, "multihead_attn.out_proj.bias"), d, &P->bo[l]));
    P->Wv[l] = ipw + 2LL * d * d;
    P->bv[l] = ipb + 2LL * d;
    FCK(zalloc(P->cmem, &P->TT[l], (size_t)1000 * d));
    fdm_gemm_args g = dense_gemm(FDM_F32, P->tau, P->Wv[l], 1000, d, d);
    g.out_f32 = tmp;
    FCK(fdm_op_gemm(&g, stream));
    g = dense_gemm(FDM_F32, tmp, P->Wo[l], 1000, d, d);
    g.out_f32 = P->TT[l];
    FCK(fdm_op_gemm(&g, stream));
  }
  // Optional (fdm_plan_set "fuse_ln3"; bf16 and f16x3): norm3 of layer l-1 folded into the QKV / out-proj GEMMs of layer l and into the
  // latent decoder,   LN(x) W^T + b = rstd (x W'^T - mu colsum(W')) + (W beta + b),  W' = W o gamma   -- 8 launches fewer.
  // Off by default since the GEMM kernels were specialised: the plain GEMM + LayerNorm launch is now as fast or faster than
  // the three GEMMs that carry the fold (profiles/README.md, A/B of the final build).
  P->fuse_ln3 = (P->dtype == FDM_BF16 || P->dtype == FDM_F16X3) && P->want_fuse_ln3;     // fdm_plan_set(p, "fuse_ln3", 1) before the commit
  if (P->fuse_ln3) {
    auto make_fold = [&](const std::string& wname, const std::string& bname, int N, int l_prev, Fold* f) -> int {
      const float *W = nullptr, *b = nullptr, *gam = nullptr, *bet = nullptr;
      FCK(need(P, wname, (long long)N * d, &W));
      FCK(need(P, bname, N, &b));
      FCK(need(P, lname(l_prev, "norm3.weight"), d, &gam));
      FCK(need(P, lname(l_prev, "norm3.bias"), d, &bet));
      float* wg = nullptr;
      FCK(zalloc(P->cmem, &wg, (size_t)N * d));
      hipLaunchKernelGGL(scale_cols_kernel, dim3(grid_for((long long)N * d)), dim3(256), 0, s, W, gam, wg, (long long)N * d, d);
      FCK(to_operand(P->cmem, P->dtype, wg, (long long)N * d, &f->w, stream));
      FCK(zalloc(P->cmem, &f->colsum, (size_t)N));
      if (P->dtype == FDM_BF16)
        hipLaunchKernelGGL(rowsum_bf16_kernel, dim3((N + 3) / 4), dim3(256), 0, s, (const fdm::bf16*)f->w.p, f->colsum, N, d);
      else
        hipLaunchKernelGGL(rowsum_split_kernel<fdm::f16>, dim3((N + 3) / 4), dim3(256), 0, s, (const fdm::f16*)f->w.p, f->w.lo, 1.f / 2048.f, f->colsum, N, d);
      FCK(zalloc(P->cmem, &f->bias, (size_t)N));
      FCK(fdm_op_small_linear(bet, W, b, f->bias, 1, d, N, FDM_ACT_NONE, stream));      // W beta + b
      f->gamma = gam; f->beta = bet;
      return FDM_OK;
    };
    for (int l = 1; l < m.n_layers; ++l)
      FCK(make_fold(lname(l, "self_attn.in_proj_weight"), lname(l, "self_attn.in_proj_bias"), 3 * d, l - 1, &P->fold[l]));
    FCK(make_fold("latent_decoder.weight", "latent_decoder.bias", d, m.n_layers - 1, &P->fold[-1]));
  }
  HIPCK(hipGetLastError());
  // ALiBi slopes, positional table, schedule tables
  std::vector<float> hs(m.n_head);
  fdm_alibi_slopes_host(m.n_head, hs.data());
  FCK(zalloc(P->cmem, &P->slopes, (size_t)m.n_head));
  HIPCK(hipMemcpyAsync(P->slopes, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, s));
  const int pe_rows = m.max_len + 30;
  FCK(zalloc(P->cmem, &P->pe, (size_t)pe_rows * d));
  if (const Wt* pw = weight(P, "PE.pe")) {           // the reference's registered buffer [1, rows, d]
    if (pw->n < (long long)m.max_len * d) return fail(FDM_ERR_SHAPE, "plan: PE.pe has %lld elements, need >= %lld", pw->n, (long long)m.max_len * d);
    const long long n = pw->n < (long long)pe_rows * d ? pw->n : (long long)pe_rows * d;
    HIPCK(hipMemcpyAsync(P->pe, pw->p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  } else {
    std::vector<float> hp((size_t)pe_rows * d);
    fdm_pe_table_host(d, m.pe_periodic, m.period, pe_rows, hp.data());
    HIPCK(hipMemcpyAsync(P->pe, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, s));
    HIPCK(hipStreamSynchronize(s));
  }
  std::vector<float> sb((size_t)12 * 1000);
  fdm_schedule_host(1000, sb.data());
  std::vector<float> sg(1000);
  for (int i = 0; i < 1000; ++i) sg[i] = (float)std::exp((double)(0.5f * sb[9000 + i]));      // exp(0.5 logvar), p_sample :655
  struct { const char* name; float** dst; const float* host; } tabs[] = {
      {"sched.c1", &P->c1, &sb[10000]}, {"sched.c2", &P->c2, &sb[11000]}, {"sched.sigma", &P->sigma, sg.data()},
      {"sched.sra", &P->sra, &sb[6000]}, {"sched.srm1", &P->srm1, &sb[7000]}};
  for (auto& t : tabs) {
    FCK(zalloc(P->cmem, t.dst, (size_t)1000));
    if (const Wt* ow = weight(P, t.name)) {
      if (ow->n != 1000) return fail(FDM_ERR_SHAPE, "plan: %s must have 1000 elements", t.name);
      HIPCK(hipMemcpyAsync(*t.dst, ow->p, 4000, hipMemcpyDeviceToDevice, s));
    } else {
      HIPCK(hipMemcpyAsync(*t.dst, t.host, 4000, hipMemcpyHostToDevice, s));
    }
  }
  HIPCK(hipStreamSynchronize(s));         // host staging vectors go out of scope
  P->committed = true;
  return FDM_OK;
}

// Everything commit allocates (operand-kind weight copies, tau / TT tables, folds, schedule and PE tables) is derived from the
// weights: released when a weight changes under it (fdm_plan_set_weights) and rebuilt by the next commit.
int release_commit(fdm_plan* P, void* stream) {
  FCK(drop_programs(P, stream));           // recorded programs point into the tables
  if (!P->cmem.allocs.empty()) {
    if (stream) HIPCK(hipStreamSynchronize((hipStream_t)stream)); else HIPCK(hipDeviceSynchronize());
    P->cmem.release();
  }
  P->committed = false; P->prepared = false;
  P->wt.clear(); P->fold.clear(); P->TT.clear();
  P->tau = nullptr; P->slopes = P->pe = nullptr;
  P->c1 = P->c2 = P->sigma = P->sra = P->srm1 = nullptr;
  return FDM_OK;
}

int commit(fdm_plan* P, void* stream) {
  if (P->committed) return FDM_OK;
  if (!P->cmem.allocs.empty()) FCK(release_commit(P, stream));      // a commit that failed half way
  return commit_impl(P, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// workspaces
// ---------------------------------------------------------------------------------------------------------------------
int reserve(fdm_plan* P, int B, int L, int cfg) {
  const int rep = cfg ? 2 : 1;
  if (B <= P->capB && L <= P->capL && rep <= P->capRep) return FDM_OK;
  B = B > P->capB ? B : P->capB; L = L > P->capL ? L : P->capL;
  const int repc = rep > P->capRep ? rep : P->capRep;
  FCK(drop_programs(P, nullptr));
  P->ws.release();
  P->prepared = false;
  const fdm_model_desc& m = P->m;
  const size_t d = m.d, M = (size_t)B * L, R = M * repc;
  const size_t Lpad = ((size_t)L + 31) / 32 * 32;
  FCK(zalloc(P->ws, &P->h, R * d)); FCK(zalloc(P->ws, &P->h2, R * d)); P->x1_planes = std::max(1, std::max(P->ksplit_out, P->ksplit_ffn2));      // (x1: one fp32 plane per K slice of the plan's setting; plan_set grows it)
  FCK(zalloc(P->ws, &P->x1, R * d * P->x1_planes));
  FCK(zalloc(P->ws, &P->x0, R * d)); FCK(zalloc(P->ws, &P->x, M * d));
  FCK(zalloc(P->ws, &P->x0_hist, M * d));      // fp32 in every arithmetic mode
  if (P->dtype != FDM_F32) {
    FCK(zalloc_mat(P, P->ws, &P->xt, M, d)); FCK(zalloc_mat(P, P->ws, &P->ht, R, d)); FCK(zalloc_mat(P, P->ws, &P->h2t, R, d));
  } else {        // fp32 operands alias the fp32 residual-stream buffers
    P->xt = Mat{P->x, 0}; P->ht = Mat{P->h, 0}; P->h2t = Mat{P->h2, 0};
  }
  if (P->dtype != FDM_F32) {     // folded-norm3 buffers (raw rows, their operand copy, per-row partial sums)
    FCK(zalloc(P->ws, &P->x2, R * d)); FCK(zalloc_mat(P, P->ws, &P->x2t, R, d)); FCK(zalloc(P->ws, &P->stats, (d / 64) * R * 2));
  }
  // q: row-major queries; kp / vp: fragment-packed keys / values written by the QKV GEMM's epilogue (zeroed: pad keys must be
  // finite).  Split modes: attention runs in fp32, ctx returns as a plane pair.
  // (FDM_F16X3: fp16 plane pairs, the same bytes as fp32)
  const size_t ea = kind(P->dtype).full();
  FCK(P->ws.alloc(&P->q, R * d * ea, true));
  FCK(P->ws.alloc(&P->kp, (size_t)B * repc * Lpad * d * ea, true));
  FCK(P->ws.alloc(&P->vp, (size_t)B * repc * Lpad * d * ea, true));
  P->q_lo = (long long)(R * d);
  P->kv_lo = (long long)((size_t)B * repc * Lpad * d);
  P->kv_bytes = (size_t)B * repc * Lpad * d * ea;
  FCK(zalloc_mat(P, P->ws, &P->ctx, R, d));
  FCK(zalloc_mat(P, P->ws, &P->u, R, m.ffn));
  FCK(zalloc(P->ws, &P->AF, M * d)); FCK(zalloc(P->ws, &P->t1, M * d));
  FCK(zalloc(P->ws, &P->sty, (size_t)B * d)); FCK(zalloc(P->ws, &P->em, (size_t)B * d)); FCK(zalloc(P->ws, &P->emu, (size_t)B * d));
  FCK(zalloc(P->ws, &P->zeros, (size_t)B * (m.n_emo > 0 ? m.n_emo : 1)));
  FCK(zalloc(P->ws, &P->E0, R * d));
  P->C1.assign(m.n_layers, nullptr);
  for (int l = 0; l < m.n_layers; ++l) FCK(zalloc(P->ws, &P->C1[l], R * d));
  FCK(zalloc(P->ws, &P->step, (size_t)4));
  FCK(zalloc(P->ws, &P->seedbuf, (size_t)2));
  if (!P->tseq) { P->tseq_cap = 1024; FCK(zalloc(P->mem, &P->tseq, (size_t)P->tseq_cap)); }
  if (!P->lm_tab) { P->lm_cap = 1024; FCK(zalloc(P->mem, &P->lm_tab, (size_t)4 * P->lm_cap)); }
  P->capB = B; P->capL = L; P->capRep = repc;
  return FDM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the step program: one denoiser pass, ws.x (+ its operand copy) -> ws.x0, or -> x_{t-1} when the scheduler update is fused
// ---------------------------------------------------------------------------------------------------------------------
}  // namespace

int fdm::record_chain(fdm_plan* P, const fdm_sched_args* sched, void* stream) {
  const fdm_model_desc& m = P->m;
  const int d = m.d, M = P->M, R = P->R, L = P->L;
  const bool both = P->dtype != FDM_F32, split = kind(P->dtype).planes == 2, fuse = P->fuse_ln3;
  int* step = P->step; int* tcur = P->step + 1;
  const float *b = nullptr;
  {
    // latent encoder: h = act(x W^T + b) + E0.  A CFG plan's cond and uncond rows read the same x rows and differ only in
    // the addend, so both halves are one batched launch (batch index = half: A / W / bias strides 0, outputs and the
    // addend advance by M rows).  First kernel of the step: the step counter += 1 and tcur = tseq[counter].
    FCK(need(P, "latent_encoder.0.bias", d, &b));
    fdm_gemm_args g = gemm_op(P, P->xt, P->wt["latent_encoder.0.weight"], M, d, d);
    g.bias = b; g.act = m.latent_mish ? FDM_ACT_MISH : FDM_ACT_NONE;
    g.resid = P->E0; g.out_f32 = P->h;
    if (both) set_out_t(g, P->ht);
    g.batch = P->rep; g.out_batch_stride = (long long)M * d;
    if (!P->slots) { g.incr_counter = step; g.incr_table = P->tseq; }      // (slot mode: the advance launch moved every slot's own word)
    FCK(plan_gemm(P, "enc", g, stream));
  }
  const int BB = P->B * P->rep;
  const float eps = 1e-5f;
  for (int l = 0; l < m.n_layers; ++l) {
    const Fold* f = (fuse && l > 0) ? &P->fold[l] : nullptr;
    fdm_gemm_args g;
    if (!f) {
      FCK(need(P, lname(l, "self_attn.in_proj_bias"), 3LL * d, &b));
      g = gemm_op(P, P->ht, P->wt[lname(l, "self_attn.in_proj_weight")], R, 3 * d, d);
      g.bias = b;
    } else {          // layer input = LN3(x2) of the previous layer, never materialised
      g = gemm_op(P, P->x2t, f->w, R, 3 * d, d);
      g.bias = f->bias; g.ln_colsum = f->colsum; set_ln_stats(g, P);
    }
    // FDM_F16X3: split attention on plane pairs (head_dim 64 / 128 hold a key tile's fragments in registers, 256 -- BIWI --
    // streams them at one wave per SIMD).
    g.out_t = P->q; g.ldo_t = d; g.out_t_lo_off = split ? P->q_lo : 0;
    g.kv_lo_off = split ? P->kv_lo : 0;
    g.out_kp = P->kp; g.kp_col0 = d; g.out_vp = P->vp; g.vp_col0 = 2 * d; g.kv_L = L; g.kv_Lpad = P->Lpad; g.kv_hd = P->hd;
    FCK(plan_gemm(P, f ? "qkv_ln" : "qkv", g, stream));
    fdm_attn_args at;
    memset(&at, 0, sizeof(at));
    at.Q = P->q; at.ldq = d;
    at.Kp = P->kp; at.Vp = P->vp; at.Lpad = P->Lpad; at.O = P->ctx.p; at.ldo = d;
    at.B = BB; at.H = m.n_head; at.L = L; at.hd = P->hd; at.dtype = P->dtype;
    at.scale = 1.0f / std::sqrt((float)P->hd); at.causal = 1; at.slopes = P->slopes; at.period = m.period;
    if (split) { at.q_lo_off = P->q_lo; at.kv_lo_off = P->kv_lo; at.o_lo_off = P->ctx.lo; }
    FCK(fdm_op_attention(&at, stream));
    FCK(need(P, lname(l, "self_attn.out_proj.bias"), d, &b));
    g = gemm_op(P, P->ctx, P->wt[lname(l, "self_attn.out_proj.weight")], R, d, d);
    g.bias = b; g.out_f32 = P->x1;
    if (!f) {
      g.resid = P->h;
      set_ksplit(g, P->ksplit_out, (long long)R * d);
      FCK(plan_gemm(P, "out", g, stream));
    } else {
      g.resid = P->x2; g.rln_gamma = f->gamma; g.rln_beta = f->beta; set_ln_stats(g, P);
      FCK(plan_gemm(P, "out_ln", g, stream));
    }
    // norm1 and norm2 back to back in one kernel: h2 = LN2(LN1(x1) + C1_l + TT_l[t])
    fdm_ln_args ln;
    memset(&ln, 0, sizeof(ln));
    ln.x = P->x1; ln.M = R; ln.d = d; ln.add_mat = P->C1[l]; ln.add_tab = P->TT[l]; ln.tab_step = tcur; ln.eps = eps;
    if (P->S > 1) { ln.add_mat_L = L; ln.add_mat_group = P->S * L; ln.add_mat_wrap = M; }     // C1_l holds one block per audio clip
    if (P->slots) {      // every slot gathers TT_l by the t word of its own state (both CFG halves share it)
      ln.tab_step = nullptr; ln.clip_step = P->slot_state + 1; ln.clip_step_stride = 4; ln.clip_rows = L; ln.clip_wrap = M;
    }
    if (!f) set_ksplit(ln, P->ksplit_out, (long long)R * d);
    FCK(need(P, lname(l, "norm1.weight"), d, &ln.gamma)); FCK(need(P, lname(l, "norm1.bias"), d, &ln.beta));
    FCK(need(P, lname(l, "norm2.weight"), d, &ln.gamma2)); FCK(need(P, lname(l, "norm2.bias"), d, &ln.beta2));
    ln.y_f32 = P->h2; ln.dtype = P->dtype;
    if (both) { ln.y_t = P->h2t.p; ln.y_t_lo_off = P->h2t.lo; }
    FCK(fdm_op_layernorm(&ln, stream));
    FCK(need(P, lname(l, "linear1.bias"), m.ffn, &b));
    g = gemm_op(P, P->h2t, P->wt[lname(l, "linear1.weight")], R, m.ffn, d);
    g.bias = b; g.act = FDM_ACT_RELU; set_out_t(g, P->u);
    FCK(plan_gemm(P, "ffn1", g, stream));
    FCK(need(P, lname(l, "linear2.bias"), d, &b));
    g = gemm_op(P, P->u, P->wt[lname(l, "linear2.weight")], R, d, m.ffn);
    g.bias = b; g.resid = P->h2;
    if (fuse) {      // x2 = h2 + FFN(h2): fp32 + operand copy + per-row partial sums for the folded norm3
      g.out_f32 = P->x2; set_out_t(g, P->x2t); g.stat_out = P->stats;
      FCK(plan_gemm(P, "ffn2_stat", g, stream));
    } else {
      g.out_f32 = P->x1;
      set_ksplit(g, P->ksplit_ffn2, (long long)R * d);
      FCK(plan_gemm(P, "ffn2", g, stream));
      memset(&ln, 0, sizeof(ln));
      ln.x = P->x1; ln.M = R; ln.d = d; ln.eps = eps; ln.y_f32 = P->h; ln.dtype = P->dtype;
      set_ksplit(ln, P->ksplit_ffn2, (long long)R * d);
      FCK(need(P, lname(l, "norm3.weight"), d, &ln.gamma)); FCK(need(P, lname(l, "norm3.bias"), d, &ln.beta));
      if (both) { ln.y_t = P->ht.p; ln.y_t_lo_off = P->ht.lo; }
      FCK(fdm_op_layernorm(&ln, stream));
    }
  }
  fdm_gemm_args g;
  if (fuse) {
    const Fold& f = P->fold[-1];
    g = gemm_op(P, P->x2t, f.w, R, d, d);
    g.bias = f.bias; g.ln_colsum = f.colsum; set_ln_stats(g, P);
  } else {
    FCK(need(P, "latent_decoder.bias", d, &b));
    g = gemm_op(P, P->ht, P->wt["latent_decoder.weight"], R, d, d);
    g.bias = b;
  }
  if (sched) {       // x_{t-1} = update(x0_hat = this GEMM, x_t = ws.x) in the epilogue
    g.resid = P->x; g.out_f32 = P->x;
    if (both) set_out_t(g, P->xt);
    g.sched_fuse = 1; g.sched = *sched;
  } else {
    g.out_f32 = P->x0;
  }
  return plan_gemm(P, fuse ? "dec_ln" : "dec", g, stream);
}

namespace {

struct ProgSpec {
  int kind;                  // 0 pass (denoiser only, + CFG mix), 1 DDPM, 2 DDIM, 3 table-driven linear multistep (san = the device tables)
  const float* noise = nullptr; float cfg_scale = 0.f;
  const float* san = nullptr; const float* cn = nullptr;
  int reps = 1;              // diffusion steps recorded back to back (one graph launch runs them all)
  int slot_steps = 0;        // > 0: the slot program of a chain of that many steps (advance launch, chain, slot scheduler pass)
  int bank = 0;              // slot program with a sampler bank: the bank forms of the advance launch and of the scheduler pass
};

// Recorded programs are kept per (shape, tile set, program kind): a serving loop that alternates between shapes (clips of
// different lengths, one clip vs a batch) finds its graphs again instead of re-recording and re-instantiating them (~3 ms per
// switch).  What a program captured stays valid until the workspaces are re-allocated or the weights / tables change: those
// events drop every program.
std::string tiles_sig(const fdm_plan* P) {
  std::string s;
  for (auto& kv : P->tiles)
    if (kv.second) s += kv.first + "=" + std::to_string(kv.second) + ",";
  s += "ks" + std::to_string(P->ksplit_out) + std::to_string(P->ksplit_ffn2) + (P->lockstep ? "L" : "");
  return s;
}

fdm::WinArgs win_args(const fdm_plan* P, int init) {
  fdm::WinArgs w;
  w.off = P->win_off; w.ent = P->win_ent; w.xw = P->x;
  w.L_total = P->win_total; w.n_win = P->win_n; w.W = P->win_len; w.d = P->m.d; w.init = init;
  return w;
}

// the group tables and the arena of a slot plan with long capacity, visiting arena frames [f0, f1)
fdm_slot_group_args long_args(const fdm_plan* P, int f0, int f1, int plain, int init) {
  fdm_slot_group_args g;
  memset(&g, 0, sizeof(g));
  g.member = P->slot_member; g.frames = (const int*)P->long_frame; g.entries = P->long_ent; g.groups = (const int*)P->long_group;
  g.x_long = P->long_x; g.hist_long = P->long_hist;
  g.arena_frames = P->long_frames; g.n_entries = P->long_entries; g.n_groups = P->long_groups;
  g.L = P->L; g.d = P->m.d; g.frame0 = f0; g.frame1 = f1; g.plain = plain; g.init = init;
  return g;
}

// the sampler bank of a slot plan with bank capacity (fdm_slot_bank_args; sizes = what fdm_slots_open reserved)
fdm_slot_bank_args bank_args(const fdm_plan* P) {
  fdm_slot_bank_args b;
  memset(&b, 0, sizeof(b));
  b.req = P->slot_req; b.desc = P->bank_desc; b.t = P->bank_t; b.coef = P->bank_c;
  b.n_samplers = P->bank_rows; b.n_t = P->bank_t_cap; b.n_coef = P->bank_c_cap;
  return b;
}

int get_program(fdm_plan* P, const ProgSpec& sp, void* stream, fdm_prog** out) {
  char key[512];
  snprintf(key, sizeof(key), "%s#%s|%d|%p|%a|%p|%d", shape_key(P).c_str(), tiles_sig(P).c_str(), sp.kind, (const void*)sp.noise, (double)sp.cfg_scale,
           (const void*)sp.san, sp.reps);
  if (P->win_n) {            // a windowed plan's programs end in the blend pass over its long layout (plain keys unchanged)
    const size_t kl = strlen(key);
    snprintf(key + kl, sizeof(key) - kl, "|win%d,%d,%d,%d,%d", P->win_B, P->win_total, P->win_n, P->win_len, P->win_overlap);
  }
  if (P->slots) {            // slot mode: the chain gathers per slot and nothing advances P->step (plain keys unchanged)
    const size_t kl = strlen(key);
    snprintf(key + kl, sizeof(key) - kl, "|slot%d,%d,%p", sp.slot_steps, P->slots, (const void*)sp.cn);
    if (P->long_frames) {    // ... and with long capacity the scheduler pass also walks the arena (keys without capacity unchanged)
      const size_t k2 = strlen(key);
      snprintf(key + k2, sizeof(key) - k2, "|long%d,%d", P->long_frames, P->long_groups);
    }
    if (sp.bank) {           // ... and with a sampler bank both ends of the step read it (keys without a bank unchanged)
      const size_t k3 = strlen(key);
      snprintf(key + k3, sizeof(key) - k3, "|bank%d,%d,%d", P->bank_rows, P->bank_t_cap, P->bank_c_cap);
    }
  }
  auto it = P->progs.find(key);
  if (it != P->progs.end()) {            // hit: most recently used goes to the back, and the caller's handle stays valid for this call
    auto pos = std::find(P->prog_order.begin(), P->prog_order.end(), std::string(key));
    if (pos != P->prog_order.end()) { P->prog_order.erase(pos); P->prog_order.push_back(key); }
    P->pinned.push_back(key);
    if (sp.reps == 1) P->launches_per_step = fdm_prog_num_ops(it->second);
    *out = it->second;
    return FDM_OK;
  }
  if (P->progs.size() >= 16) {
    // programs are keyed by the pointers they captured (e.g. injected noise): cap the cache.  Victim = least recently used
    // program that was NOT handed out earlier in this API call (fdm_sample_graph holds two: the 1-step and the K-step one).
    auto victim = P->prog_order.end();
    for (auto v = P->prog_order.begin(); v != P->prog_order.end(); ++v)
      if (std::find(P->pinned.begin(), P->pinned.end(), *v) == P->pinned.end()) { victim = v; break; }
    if (victim != P->prog_order.end()) {
      HIPCK(hipStreamSynchronize((hipStream_t)stream));
      const std::string vk = *victim;
      P->prog_order.erase(victim);
      fdm_prog_destroy(P->progs[vk]);
      P->progs.erase(vk);
    }
  }
  const int d = P->m.d, M = P->M;
  const long long n = (long long)M * d;
  fdm_prog* prog = nullptr;
  FCK(fdm_prog_create(&prog));
  int rc = fdm_prog_begin(prog);
  const bool fuse_sched = !P->cfg && sp.kind != 0 && !sp.slot_steps;
  for (int rep = 0; rc == FDM_OK && rep < sp.reps; ++rep) {
    fdm_sched_args sc;
    memset(&sc, 0, sizeof(sc));
    sc.x0 = P->x0; sc.x0u = P->cfg ? P->x0 + n : nullptr; sc.cfg_scale = sp.cfg_scale;
    sc.x = P->x; sc.x_out = P->x; sc.n = n; sc.tseq = P->tseq; sc.step = P->step; sc.advance = 0;
    if (P->dtype != FDM_F32) { sc.x_out_t = P->xt.p; sc.out_dtype = P->dtype; sc.x_out_t_lo_off = P->xt.lo; }
    if (sp.kind == 1) {
      sc.mode = 0; sc.n_per_clip = (long long)P->L * d; sc.c1 = P->c1; sc.c2 = P->c2; sc.sigma = P->sigma;
      sc.noise = sp.noise; sc.noise_stride = n; sc.seed_dev = P->seedbuf;
    } else if (sp.kind == 2) {
      sc.mode = 1; sc.sra = P->sra; sc.srm1 = P->srm1; sc.sqrt_an = sp.san; sc.c_n = sp.cn;
    } else if (sp.kind == 3) {
      sc.mode = 3; sc.n_per_clip = (long long)P->L * d;
      sc.lm_a = P->lm_tab; sc.lm_b = P->lm_tab + P->lm_cap; sc.lm_c = P->lm_tab + 2 * (size_t)P->lm_cap; sc.lm_s = P->lm_tab + 3 * (size_t)P->lm_cap;
      sc.x0_hist = P->win_n ? P->hist_long : P->x0_hist;
      sc.noise = sp.noise; sc.noise_stride = n; sc.seed_dev = P->seedbuf;
    }
    if (sp.slot_steps) {
      // slot program: advance every slot's word, the chain with per-slot table rows and its scheduler update unfused, then the
      // pass that updates the live slots only -- two launches more than the plain program without guidance
      sc.n_per_clip = (long long)P->L * d; sc.noise = nullptr; sc.seed_dev = nullptr; sc.step = nullptr; sc.tseq = nullptr;
      const fdm_slot_bank_args bk = bank_args(P);
      if (sp.bank) {
        // sampler bank: both ends read every slot's own sampler; sc carries the t-indexed tables of every mode and the plain slots'
        // history (mode, scale and the step-indexed tables come from the bank)
        sc.mode = 0; sc.cfg_scale = 0.f;
        sc.c1 = P->c1; sc.c2 = P->c2; sc.sigma = P->sigma; sc.sra = P->sra; sc.srm1 = P->srm1; sc.x0_hist = P->x0_hist;
        rc = fdm::slot_advance_bank_op(P->slot_state, bk, P->slots, stream);
      } else {
        rc = fdm::slot_advance_op(P->slot_state, P->tseq, sp.slot_steps, P->slots, stream);
      }
      if (rc == FDM_OK) rc = record_chain(P, nullptr, stream);
      if (rc != FDM_OK) break;
      // long capacity: the same launch also updates the groups over the long arena; without it the pass is the plain slots' one
      const fdm_slot_group_args lg = long_args(P, 0, P->long_frames, 1, 0);
      if (sp.bank) rc = P->long_frames ? fdm_op_slot_group_sched_bank(&sc, P->slot_state, P->slot_keys, P->slots, &lg, &bk, stream)
                                       : fdm_op_slot_sched_bank(&sc, P->slot_state, P->slot_keys, P->slots, &bk, stream);
      else rc = P->long_frames ? fdm_op_slot_group_sched(&sc, P->slot_state, P->slot_keys, P->slots, &lg, stream)
                               : fdm_op_slot_sched(&sc, P->slot_state, P->slot_keys, P->slots, stream);
      continue;
    }
    if (sp.kind != 0 && P->win_n) {
      // windowed plan: the chain unfused, then one pass over the long layout -- blend the windows' x0 (after their CFG mix), update
      // each long-clip element once (noise keyed by the long clip), write back to the long buffer and every window holding the frame
      const long long nl = (long long)P->win_B * P->win_total * d;
      sc.x = P->xlong; sc.x_out = P->xlong; sc.n = nl; sc.n_per_clip = (long long)P->win_total * d; sc.noise_stride = nl;
      rc = record_chain(P, nullptr, stream);
      if (rc == FDM_OK) rc = fdm::window_sched_op(sc, win_args(P, 0), stream);
      continue;
    }
    if (sp.kind != 0 && fuse_sched) {
      // non-CFG samplers: the update runs in the latent decoder GEMM's epilogue (bit-identical, one launch less)
      fdm_sched_args fs2 = sc;
      fs2.x0 = fs2.x0u = fs2.x = nullptr; fs2.x_out = nullptr; fs2.x_out_t = nullptr;
      rc = record_chain(P, &fs2, stream);
      continue;
    }
    rc = record_chain(P, nullptr, stream);
    if (rc != FDM_OK) break;
    if (sp.kind != 0) {
      rc = fdm_op_sched_step(&sc, stream);
    } else if (P->cfg) {
      sc.mode = 2; sc.x = nullptr; sc.x_out = P->x0; sc.x_out_t = nullptr;
      rc = fdm_op_sched_step(&sc, stream);
    }
  }
  const int rc2 = fdm_prog_end(prog);
  if (rc != FDM_OK || rc2 != FDM_OK) { fdm_prog_destroy(prog); return rc != FDM_OK ? rc : rc2; }
  if (sp.reps == 1) P->launches_per_step = fdm_prog_num_ops(prog);
  P->progs[key] = prog;
  P->prog_order.push_back(key);
  P->pinned.push_back(key);
  *out = prog;
  return FDM_OK;
}

int set_steps(fdm_plan* P, const int* ts, int n, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n > P->tseq_cap) {
    FCK(drop_programs(P, stream));          // (drains the stream: nothing reads the old list any more)
    P->mem.free_one(P->tseq);
    P->tseq_cap = n;
    FCK(zalloc(P->mem, &P->tseq, (size_t)n));
  }
  HIPCK(hipMemcpyAsync(P->tseq, ts, (size_t)n * 4, hipMemcpyHostToDevice, s));
  const int init[2] = {-1, 0};       // the first GEMM of every step increments the counter before anything reads it
  HIPCK(hipMemcpyAsync(P->step, init, 8, hipMemcpyHostToDevice, s));
  HIPCK(hipStreamSynchronize(s));    // ts / init are caller / stack memory
  return FDM_OK;
}

// The operand-kind copy of the n fp32 elements at src (rows of P->x) into dst_t (the same rows of P->xt), whatever the plane distance
// P->xt.lo: the scheduler's mix-only mode (x_out = x0 = src) rewrites src in place and writes the copy through its store path.
int operand_copy(fdm_plan* P, float* src, void* dst_t, long long n, void* stream) {
  fdm_sched_args sc;
  memset(&sc, 0, sizeof(sc));
  sc.mode = 2; sc.x0 = src; sc.x_out = src; sc.n = n; sc.x_out_t = dst_t; sc.out_dtype = P->dtype; sc.x_out_t_lo_off = P->xt.lo;
  return fdm_op_sched_step(&sc, stream);
}

int load_x(fdm_plan* P, const float* x, void* stream) {
  const long long n = (long long)P->M * P->m.d;
  HIPCK(hipMemcpyAsync(P->x, x, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (P->dtype == FDM_F32) return FDM_OK;
  // fdm_op_cast's contract is lo = dst + n; the plane distance of xt is its capacity, so a plan below capacity takes the other path
  if (kind(P->dtype).planes == 1 || P->xt.lo == n) return fdm_op_cast(P->x, P->xt.p, n, P->dtype, stream);
  return operand_copy(P, P->x, P->xt.p, n, stream);
}

// windowed plan: x_T in long layout -> the long buffer, then the window rows (+ their operand copy) through the window pass's store path
int load_x_long(fdm_plan* P, const float* x, void* stream) {
  const long long n = (long long)P->win_B * P->win_total * P->m.d;
  HIPCK(hipMemcpyAsync(P->xlong, x, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  fdm_sched_args sc;
  memset(&sc, 0, sizeof(sc));
  sc.mode = 2; sc.x = P->xlong; sc.n = n;
  if (P->dtype != FDM_F32) { sc.x_out_t = P->xt.p; sc.out_dtype = P->dtype; sc.x_out_t_lo_off = P->xt.lo; }
  return fdm::window_sched_op(sc, win_args(P, 1), stream);
}

int check_ready(const fdm_plan* P) {
  if (!P) return fail(FDM_ERR_ARG, "plan: null plan");
  if (!P->prepared) return fail(FDM_ERR_STATE, "plan: call fdm_audio_prepare first");
  return FDM_OK;
}

// a plan-lifetime device buffer of at least `bytes` (windowed sampling): growing drains the stream and drops the recorded programs
int grow(fdm_plan* P, void** buf, size_t* cap, size_t bytes, void* stream) {
  if (*buf && *cap >= bytes) return FDM_OK;
  FCK(drop_programs(P, stream));
  if (*buf) {
    HIPCK(hipStreamSynchronize((hipStream_t)stream));
    P->mem.free_one(*buf);
    *buf = nullptr; *cap = 0;
  }
  FCK(P->mem.alloc(buf, bytes, true));
  *cap = bytes;
  return FDM_OK;
}

// the table-driven sampler's own arguments: checkable without a plan or a device
int check_tables_args(const fdm_sample_args* a) {
  if (a && a->kind == 2 && (!a->lm_tables || !a->t_list || a->n_steps < 1))
    return fail(FDM_ERR_ARG, "sample_graph: the table-driven sampler needs lm_tables [4][n_steps], t_list and n_steps >= 1");
  return FDM_OK;
}

// the caller's timestep list, checked (DDPM and the table-driven sampler)
int take_steps(const fdm_sample_args* a, std::vector<int>& ts) {
  for (int i = 0; i < a->n_steps; ++i) {
    if (a->t_list[i] < 0 || a->t_list[i] >= 1000) return fail(FDM_ERR_ARG, "sample_graph: timestep %d outside [0, 1000)", a->t_list[i]);
    ts.push_back(a->t_list[i]);
  }
  return FDM_OK;
}

// A sampler definition as the bank stores it (slots.hpp): the scheduler mode, the timestep list and the step-indexed coefficients
// in bank layout -- the values sampler_setup puts on the device for the same arguments, so a slot's bits match the solo path.
struct SamplerDef { int kind = 0, mode = 0; std::vector<int> ts; std::vector<float> coef; };
int sampler_def(const fdm_sample_args* a, const char* who, SamplerDef& o) {
  o.kind = a->kind;
  if (a->kind == 0) {
    if (!a->t_list || a->n_steps <= 0) return fail(FDM_ERR_ARG, "%s: DDPM needs t_list / n_steps", who);
    FCK(take_steps(a, o.ts));
    o.mode = 0;
  } else if (a->kind == 1) {
    if (a->ddim_steps <= 0) return fail(FDM_ERR_ARG, "%s: DDIM needs ddim_steps", who);
    std::vector<int> t(a->ddim_steps), tn(a->ddim_steps);
    std::vector<float> tab(2 * (size_t)a->ddim_steps);
    const int n = fdm_ddim_schedule_host(a->ddim_steps, 1000, t.data(), tn.data(), tab.data(), tab.data() + a->ddim_steps);
    if (n < 0) return n;
    o.mode = 1;              // (n == 0, only the dead pair: an empty list -- a solo call copies x_T through, the bank's callers refuse it)
    o.ts.assign(t.begin(), t.begin() + n);                                   // (the dead last pair is skipped)
    o.coef.assign(tab.begin(), tab.begin() + n);                             // sqrt_an[n] | c_n[n]
    o.coef.insert(o.coef.end(), tab.begin() + a->ddim_steps, tab.begin() + a->ddim_steps + n);
  } else if (a->kind == 2) {
    FCK(check_tables_args(a));
    FCK(take_steps(a, o.ts));
    o.mode = 3;
    o.coef.assign(a->lm_tables, a->lm_tables + 4 * (size_t)a->n_steps);      // a | b | c | s, each n_steps
  } else {
    return fail(FDM_ERR_ARG, "%s: kind %d (0 = DDPM, 1 = DDIM, 2 = table-driven)", who, a->kind);
  }
  return FDM_OK;
}

// the sampler of a call: its timestep list, its program kind and its device tables (DDIM: cached per step count; table-driven:
// uploaded per call, history zeroed).  Shared by fdm_sample_graph / fdm_sample_windows and fdm_slots_open.  The list and the DDIM
// tables are sampler_def's, so the solo path and the bank cannot drift.
int sampler_setup(fdm_plan* P, const fdm_sample_args* a, void* stream, std::vector<int>& ts, ProgSpec& sp) {
  hipStream_t s = (hipStream_t)stream;
  const bool cached = a->kind == 1 && P->ddim.count(a->ddim_steps);      // a DDIM step count seen before: list and tables are on the plan
  SamplerDef def;
  if (!cached) FCK(sampler_def(a, "sample_graph", def));
  if (a->kind == 0) {
    ts = def.ts;
    sp.kind = 1; sp.noise = a->noise;
  } else if (a->kind == 1) {
    if (!cached) {           // sqrt_an[n] | c_n[n] of the n live pairs (n = 0, e.g. ddim_steps = 1: an empty list, nothing is read)
      float* dv = nullptr;
      FCK(zalloc(P->mem, &dv, std::max<size_t>(def.coef.size(), 1)));
      if (!def.coef.empty()) HIPCK(hipMemcpyAsync(dv, def.coef.data(), def.coef.size() * 4, hipMemcpyHostToDevice, s));
      HIPCK(hipStreamSynchronize(s));
      P->ddim[a->ddim_steps] = {(int)def.ts.size(), dv};
      P->ddim_t[a->ddim_steps] = def.ts;
    }
    ts = P->ddim_t[a->ddim_steps];
    sp.kind = 2; sp.san = P->ddim[a->ddim_steps].second; sp.cn = sp.san + ts.size();
  } else {                   // table-driven (sampler_def refused every other kind)
    ts = def.ts;
    if (a->n_steps > P->lm_cap) {      // a longer table than any before: a new buffer (recorded programs point at the old one)
      FCK(drop_programs(P, stream));
      P->mem.free_one(P->lm_tab);
      P->lm_tab = nullptr; P->lm_cap = a->n_steps;
      FCK(zalloc(P->mem, &P->lm_tab, (size_t)4 * P->lm_cap));
    }
    for (int j = 0; j < 4; ++j)        // set_steps() below drains the copies (the tables are caller memory)
      HIPCK(hipMemcpyAsync(P->lm_tab + (size_t)j * P->lm_cap, a->lm_tables + (size_t)j * a->n_steps, (size_t)a->n_steps * 4, hipMemcpyHostToDevice, s));
    // a call never sees the history of the one before it (the shipped tables have c[0] = 0 and do not read it at step 0)
    if (P->win_n) HIPCK(hipMemsetAsync(P->hist_long, 0, (size_t)P->win_B * P->win_total * P->m.d * 4, s));
    else HIPCK(hipMemsetAsync(P->x0_hist, 0, (size_t)P->M * P->m.d * 4, s));
    sp.kind = 3; sp.noise = a->noise; sp.san = P->lm_tab;
  }
  return FDM_OK;
}

// n_steps steps of the program sp as graph launches: K steps per launch (the K-step program of the same spec; graph_steps, 10 when
// not set), then the remainder one step per launch on the 1-step program p1.  Shared by fdm_sample_graph / _windows and fdm_slots_run.
int replay_steps(fdm_plan* P, const ProgSpec& sp, fdm_prog* p1, int n_steps, int graph_steps, void* stream) {
  int K = graph_steps > 0 ? graph_steps : 10;
  if (K > n_steps) K = n_steps;
  int left = n_steps;
  if (K > 1) {
    ProgSpec spk = sp; spk.reps = K;
    fdm_prog* pk = nullptr;
    FCK(get_program(P, spk, stream, &pk));
    FCK(fdm_prog_instantiate(pk, stream));
    FCK(fdm_prog_replay(pk, left / K, stream));
    P->last_graph_launches += left / K;
    left %= K;
  }
  if (left) {
    FCK(fdm_prog_instantiate(p1, stream));
    FCK(fdm_prog_replay(p1, left, stream));
    P->last_graph_launches += left;
  }
  return FDM_OK;
}

// fdm_sample_graph (plain plan, x in plan layout) and fdm_sample_windows (windowed plan, x_T / out / noise / record in long layout)
int sample_impl(fdm_plan* P, const fdm_sample_args* a, void* stream) {
  P->pinned.clear();
  if (!a || !a->x_T || !a->out) return fail(FDM_ERR_ARG, "sample_graph: null argument");
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> ts;
  ProgSpec sp;
  sp.cfg_scale = a->cfg_scale;
  FCK(sampler_setup(P, a, stream, ts, sp));
  // {Philox seed, global index of clip 0} of the samplers that draw noise in-kernel (set_steps() below drains the copy)
  const unsigned long long sd[2] = {a->seed, (unsigned long long)(unsigned)a->clip0};
  if (a->kind != 1) HIPCK(hipMemcpyAsync(P->seedbuf, sd, 16, hipMemcpyHostToDevice, s));
  const int n_steps = (int)ts.size();
  const size_t nx = P->win_n ? (size_t)P->win_B * P->win_total * P->m.d : (size_t)P->M * P->m.d;     // elements of x in the caller's layout
  const size_t nb = nx * 4;
  float* xc = P->win_n ? P->xlong : P->x;
  P->last_graph_launches = 0;
  if (n_steps == 0) {        // e.g. ddim_steps = 1: only the dead pair
    if (a->out != a->x_T) HIPCK(hipMemcpyAsync(a->out, a->x_T, nb, hipMemcpyDeviceToDevice, s));
    return FDM_OK;
  }
  if (P->tune_lazy) tune_soft(P, stream);
  P->steps_seen[shape_key(P)] += n_steps;
  FCK(P->win_n ? load_x_long(P, a->x_T, stream) : load_x(P, a->x_T, stream));
  FCK(set_steps(P, ts.data(), n_steps, stream));
  fdm_prog* p1 = nullptr;
  FCK(get_program(P, sp, stream, &p1));
  if (a->record || a->eager) {
    for (int i = 0; i < n_steps; ++i) {
      if (a->eager) { FCK(fdm_prog_run(p1, stream)); }
      else { FCK(fdm_prog_instantiate(p1, stream)); FCK(fdm_prog_replay(p1, 1, stream)); ++P->last_graph_launches; }
      if (a->record) HIPCK(hipMemcpyAsync(a->record + (size_t)i * nx, xc, nb, hipMemcpyDeviceToDevice, s));
    }
  } else {
    FCK(replay_steps(P, sp, p1, n_steps, a->graph_steps, stream));
  }
  HIPCK(hipMemcpyAsync(a->out, xc, nb, hipMemcpyDeviceToDevice, s));
  return FDM_OK;
}
// The per-clip GEMMs of the prepare, shared by fdm_audio_prepare_conds (all clips at once) and fdm_slot_admit (one slot's rows).
// Every GEMM is row-independent and accumulates k in one order, so a clip's rows do not depend on how many rows ride the launch.
// clip_audio_in: t1[row0 .. row0 + rows) = Mish(audio_extract.0(hub rows of one clip)).
int clip_audio_in(fdm_plan* P, const float* hub_clip, int row0, int rows, void* stream) {
  const fdm_model_desc& m = P->m;
  const float *w0 = nullptr, *b0 = nullptr;
  FCK(need(P, "audio_extract.0.weight", (long long)m.d * m.audio_in, &w0)); FCK(need(P, "audio_extract.0.bias", m.d, &b0));
  fdm_gemm_args g = dense_gemm(FDM_F32, hub_clip, w0, rows, m.d, m.audio_in);
  g.bias = b0; g.act = FDM_ACT_MISH; g.out_f32 = P->t1 + (size_t)row0 * m.d;
  return fdm_op_gemm(&g, stream);
}
// clip_tables: AF = audio_extract.2(t1) and C1_l = Wo_l (Wv_l AF + bv_l) + bo_l for the rows [row0, row0 + rows) (t1's rows are
// reused as scratch); uncond_off > 0: every C1_l row block is copied that many elements on (the uncond half of a CFG plan).
int clip_tables(fdm_plan* P, int row0, int rows, size_t uncond_off, void* stream) {
  const fdm_model_desc& m = P->m;
  const int d = m.d;
  const size_t o = (size_t)row0 * d;
  const float *w2 = nullptr, *b2 = nullptr;
  FCK(need(P, "audio_extract.2.weight", (long long)d * d, &w2)); FCK(need(P, "audio_extract.2.bias", d, &b2));
  fdm_gemm_args g = dense_gemm(FDM_F32, P->t1 + o, w2, rows, d, d);
  g.bias = b2; g.out_f32 = P->AF + o;
  FCK(fdm_op_gemm(&g, stream));
  for (int l = 0; l < m.n_layers; ++l) {
    g = dense_gemm(FDM_F32, P->AF + o, P->Wv[l], rows, d, d);
    g.bias = P->bv[l]; g.out_f32 = P->t1 + o;
    FCK(fdm_op_gemm(&g, stream));
    g = dense_gemm(FDM_F32, P->t1 + o, P->Wo[l], rows, d, d);
    g.bias = P->bo[l]; g.out_f32 = P->C1[l] + o;
    FCK(fdm_op_gemm(&g, stream));
    if (uncond_off) HIPCK(hipMemcpyAsync(P->C1[l] + o + uncond_off, P->C1[l] + o, (size_t)rows * d * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return FDM_OK;
}

// zero n elements (per plane) of an operand-kind matrix starting at element `at`
int zero_mat(const fdm_plan* P, const Mat& mt, size_t at, size_t n, void* stream) {
  const size_t eb = kind(P->dtype).bytes;
  HIPCK(hipMemsetAsync((char*)mt.p + at * eb, 0, n * eb, (hipStream_t)stream));
  if (mt.lo) HIPCK(hipMemsetAsync((char*)mt.p + ((size_t)mt.lo + at) * eb, 0, n * eb, (hipStream_t)stream));
  return FDM_OK;
}

// One slot's rows of AF, C1_l (both CFG halves) and E0 for a clip (or a window of a long clip) of L_clip frames whose audio rows start
// at hub_clip: the per-clip GEMMs of fdm_audio_prepare_conds on L_clip rows, zero addends in the rows L_clip .. L.  Shared by
// fdm_slot_admit and fdm_slot_admit_long.
// the audio half of a slot's rows: AF and C1_l (both CFG halves) on L_clip rows, zero C1_l rows beyond (slot_rows, slot_rows_tracks)
int slot_audio_rows(fdm_plan* P, int slot, const float* hub_clip, int L_clip, void* stream) {
  const fdm_model_desc& m = P->m;
  const int d = m.d, L = P->L, M = P->M, row0 = slot * L, pad = L - L_clip;
  const size_t o = (size_t)row0 * d, nclip = (size_t)L_clip * d, npad = (size_t)pad * d;
  FCK(clip_audio_in(P, hub_clip, row0, L_clip, stream));
  FCK(clip_tables(P, row0, L_clip, P->rep == 2 ? (size_t)M * d : 0, stream));
  if (pad)        // rows L_clip .. L of the slot: zero addends (the denoiser is causal: they never reach the clip's own frames)
    for (int r = 0; r < P->rep; ++r)
      for (int l = 0; l < m.n_layers; ++l) HIPCK(hipMemsetAsync(P->C1[l] + (size_t)r * M * d + o + nclip, 0, npad * 4, (hipStream_t)stream));
  return FDM_OK;
}

int slot_rows(fdm_plan* P, int slot, const float* hub_clip, const float* style, const float* emo, int L_clip, void* stream) {
  const fdm_model_desc& m = P->m;
  hipStream_t s = (hipStream_t)stream;
  const int d = m.d, L = P->L, M = P->M, row0 = slot * L, pad = L - L_clip;
  const size_t o = (size_t)row0 * d, nclip = (size_t)L_clip * d, npad = (size_t)pad * d;
  FCK(slot_audio_rows(P, slot, hub_clip, L_clip, stream));
  const float *sw = nullptr, *sbias = nullptr, *ew = nullptr, *eb = nullptr;
  FCK(need(P, "style_embedd.weight", (long long)d * m.n_style, &sw)); FCK(need(P, "style_embedd.bias", d, &sbias));
  float *sty = P->sty + (size_t)slot * d, *em = P->em + (size_t)slot * d, *emu = P->emu + (size_t)slot * d;
  FCK(fdm_op_small_linear(style, sw, sbias, sty, 1, m.n_style, d, m.style_mish ? FDM_ACT_MISH : FDM_ACT_NONE, stream));
  if (m.n_emo) {
    FCK(need(P, "emotion_embedd.weight", (long long)d * m.n_emo, &ew)); FCK(need(P, "emotion_embedd.bias", d, &eb));
    FCK(fdm_op_small_linear(emo, ew, eb, em, 1, m.n_emo, d, FDM_ACT_NONE, stream));
    if (P->cfg) FCK(fdm_op_small_linear(P->zeros, ew, eb, emu, 1, m.n_emo, d, FDM_ACT_NONE, stream));
  }
  for (int r = 0; r < P->rep; ++r) {
    const float* e = m.n_emo ? (r == 1 ? emu : em) : nullptr;
    const size_t ro = (size_t)r * M * d + o;
    FCK(fdm_op_add_rows(P->pe, 1, L_clip, sty, L_clip, 1, e, L_clip, 1, P->E0 + ro, L_clip, d, stream));
    if (pad) HIPCK(hipMemsetAsync(P->E0 + ro + nclip, 0, npad * 4, s));      // (zero addends in the rows L_clip .. L, as the C1_l rows)
  }
  return FDM_OK;
}

// Condition tracks: the E0 rows (both CFG halves) of `clips` row blocks from block0 on, from per-frame tracks style [clips, L_track,
// n_style] / emo [clips, L_track, n_emo] of which the rows < L_clip are read; the rows L_clip .. L of every block become zeros.  One
// launch (fdm_op_cond_rows), bit for bit the small_linear + add_rows sequence of slot_rows / fdm_audio_prepare_conds per row.
int cond_tracks(fdm_plan* P, int block0, int clips, int L_clip, int L_track, const float* style, const float* emo, void* stream) {
  const fdm_model_desc& m = P->m;
  const int d = m.d;
  const float *sw = nullptr, *sbias = nullptr, *ew = nullptr, *eb = nullptr;
  FCK(need(P, "style_embedd.weight", (long long)d * m.n_style, &sw)); FCK(need(P, "style_embedd.bias", d, &sbias));
  if (m.n_emo) { FCK(need(P, "emotion_embedd.weight", (long long)d * m.n_emo, &ew)); FCK(need(P, "emotion_embedd.bias", d, &eb)); }
  return fdm_op_cond_rows(P->pe, style, m.n_emo ? emo : nullptr, sw, sbias, ew, eb, P->E0 + (size_t)block0 * P->L * d,
                          P->rep == 2 ? (long long)P->M * d : 0, clips, P->L, L_clip, L_track, d, m.n_style, m.n_emo,
                          m.style_mish ? FDM_ACT_MISH : FDM_ACT_NONE, stream);
}

// slot_rows with per-frame conditions: the slot's AF / C1_l rows as there, E0 (and its zero rows) through cond_tracks.  track0 = the
// first track row of this clip or window.  Shared by fdm_slot_admit_tracks and fdm_slot_admit_long_tracks.
int slot_rows_tracks(fdm_plan* P, int slot, const float* hub_clip, const float* style, const float* emo, int track0, int L_clip, void* stream) {
  const fdm_model_desc& m = P->m;
  FCK(slot_audio_rows(P, slot, hub_clip, L_clip, stream));
  return cond_tracks(P, slot, 1, L_clip, L_clip, style + (size_t)track0 * m.n_style, m.n_emo ? emo + (size_t)track0 * m.n_emo : nullptr, stream);
}

int check_slots(const fdm_plan* P, const char* who) {
  if (!P) return fail(FDM_ERR_ARG, "%s: null plan", who);
  if (!P->slots || !P->prepared) return fail(FDM_ERR_STATE, "%s: the plan is not in slot mode (fdm_slots_open)", who);
  return FDM_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
extern "C" {

int fdm_plan_create(const fdm_model_desc* desc, int B, int L, int cfg, int dtype, fdm_plan** out) {
  if (!desc || !out) return fail(FDM_ERR_ARG, "plan_create: null argument");
  if (!kind_ok(dtype)) return fail(FDM_ERR_ARG, "plan_create: bad dtype %d", dtype);
  const fdm_model_desc& m = *desc;
  if (m.d <= 0 || m.n_head <= 0 || m.d % m.n_head || m.n_layers <= 0 || m.ffn <= 0 || m.G * m.c != m.d || m.pair <= 0 || m.max_len <= 0)
    return fail(FDM_ERR_SHAPE, "plan_create: inconsistent model geometry (d %d, heads %d, G*c %d)", m.d, m.n_head, m.G * m.c);
  const int hd = m.d / m.n_head;
  if (hd != 64 && hd != 128 && hd != 256) return fail(FDM_ERR_SHAPE, "plan_create: head_dim %d unsupported (64, 128, 256)", hd);
  if (m.d != 256 && m.d != 512 && m.d != 768 && m.d != 1024) return fail(FDM_ERR_SHAPE, "plan_create: feature_dim %d unsupported (256, 512, 768, 1024)", m.d);
  if (B < 1 || L < 1 || L > m.max_len) return fail(FDM_ERR_SHAPE, "plan_create: B=%d, L=%d outside [1, .] x [1, %d] (models/fdm_vocaset.py:44)", B, L, m.max_len);
  if (!fdm_device_ok()) return fail(FDM_ERR_STATE, "plan_create: no gfx950 device visible (there is no CPU fallback)");
  fdm_plan* P = new (std::nothrow) fdm_plan();
  if (!P) return fail(FDM_ERR_STATE, "plan_create: out of memory");
  P->m = m; P->dtype = dtype; P->hd = hd;
  const int rc = reserve(P, B, L, cfg);
  if (rc != FDM_OK) { fdm_plan_destroy(P); return rc; }
  *out = P;
  return FDM_OK;
}

int fdm_plan_reserve(fdm_plan* P, int B, int L, int cfg) {
  if (!P) return fail(FDM_ERR_ARG, "plan_reserve: null plan");
  if (B < 1 || L < 1 || L > P->m.max_len) return fail(FDM_ERR_SHAPE, "plan_reserve: B=%d, L=%d outside [1, .] x [1, %d]", B, L, P->m.max_len);
  return reserve(P, B, L, cfg);
}

int fdm_plan_destroy(fdm_plan* P) {
  if (!P) return FDM_OK;
  (void)hipDeviceSynchronize();
  for (auto& kv : P->progs) fdm_prog_destroy(kv.second);
  P->ws.release(); P->cmem.release(); P->mem.release();
  delete P;
  return FDM_OK;
}

int fdm_plan_set_weights(fdm_plan* P, const char* name, const float* ptr, long long n, void* stream) {
  if (!P || !name || !ptr || n <= 0) return fail(FDM_ERR_ARG, "plan_set_weights: bad argument");
  // a weight changed under the derived tables (and under recorded programs that point at the fp32 masters): release them,
  // the next prepare / commit rebuilds
  if (P->committed || !P->cmem.allocs.empty()) FCK(release_commit(P, stream));
  Wt& w = P->w[name];
  if (w.n != n) {
    if (w.p) {                               // size change: the old tensor goes (nothing references it after release_commit)
      FCK(drop_programs(P, stream));
      HIPCK(hipStreamSynchronize((hipStream_t)stream));
      P->mem.free_one(w.p);
      w.p = nullptr;
    }
    w.n = n;
    FCK(zalloc(P->mem, &w.p, (size_t)n));
  }
  HIPCK(hipMemcpyAsync(w.p, ptr, (size_t)n * 4, hipMemcpyDefault, (hipStream_t)stream));
  return FDM_OK;
}

int fdm_plan_commit(fdm_plan* P, void* stream) {
  if (!P) return fail(FDM_ERR_ARG, "plan_commit: null plan");
  return commit(P, stream);
}

int fdm_audio_prepare(fdm_plan* P, const float* hub, int B, int N, int fw, const float* style, const float* emo, int L, int cfg, void* stream) {
  return fdm_audio_prepare_conds(P, hub, B, N, fw, 1, style, emo, L, cfg, stream);
}

// The part of a prepare that does not depend on the conditions: checks, workspaces, the plan's shape and the audio tables AF / C1_l.
// Shared by fdm_audio_prepare_conds (one vector per clip and condition) and fdm_audio_prepare_tracks (one vector per frame).
static int prepare_tables(fdm_plan* P, const float* hub, int B0, int N, int fw, int S, bool emo_missing, int L, int cfg, void* stream) {
  const fdm_model_desc& m = P->m;
  if (B0 < 1 || N < 1 || fw < 1) return fail(FDM_ERR_SHAPE, "audio_prepare: bad feature shape [%d, %d, %d]", B0, N, fw);
  if (S < 1) return fail(FDM_ERR_SHAPE, "audio_prepare: S=%d conditions per clip", S);
  P->win_n = 0;                              // plain mode (fdm_audio_prepare_windows sets the window mode after this call)
  P->slots = 0;                              // ... and out of slot mode (slot programs keep their own cache keys)
  P->long_frames = P->long_groups = P->long_entries = 0;
  P->bank_rows = P->bank_t_cap = P->bank_c_cap = 0;
  if (m.pair * fw != m.audio_in) return fail(FDM_ERR_SHAPE, "audio_prepare: audio feature width %d x pair %d != audio_extract input %d", fw, m.pair, m.audio_in);
  if (L < 1 || L > N / m.pair || L > m.max_len) return fail(FDM_ERR_SHAPE, "audio_prepare: latent frames L=%d outside [1, min(%d, %d)] (models/fdm_vocaset.py:44,64-66)", L, N / m.pair, m.max_len);
  if (m.n_emo && emo_missing) return fail(FDM_ERR_ARG, "audio_prepare: this model needs an emotion one-hot");
  const int B = B0 * S;                      // row blocks of the step program
  FCK(commit(P, stream));
  FCK(reserve(P, B, L, cfg));
  // recorded programs hold the workspace pointers and the shape, not the clip tables' contents: a new batch of a shape seen
  // before (serving) finds them and their instantiated graphs again (get_program keys them by shape and tile set)
  hipStream_t s = (hipStream_t)stream;
  const int d = m.d, M0 = B0 * L, M = B * L, rep = cfg ? 2 : 1;
  (void)d;
  P->B = B; P->S = S; P->L = L; P->M = M; P->rep = rep; P->R = M * rep; P->cfg = cfg ? 1 : 0; P->Lpad = (L + 31) / 32 * 32;
  // pad keys of the packed K / V buffers must be finite: the layout depends on (L, Lpad), so clear them per shape
  HIPCK(hipMemsetAsync(P->kp, 0, P->kv_bytes, s));
  HIPCK(hipMemsetAsync(P->vp, 0, P->kv_bytes, s));
  // audio rows: `pair` consecutive encoder frames per latent frame (models/fdm_vqvae_mead.py:73), cropped to L (:64-66);
  // the rows of a clip are contiguous in hub, so each clip's GEMM reads them in place (fp32: once per clip, parity)
  for (int b = 0; b < B0; ++b) FCK(clip_audio_in(P, hub + (size_t)b * N * fw, b * L, L, stream));
  // folded cross-attention tables C1_l = Wo_l (Wv_l AF + bv_l) + bo_l.  S = 1: layout [rep][M, d] (the uncond half is a copy);
  // S > 1: ONE block of [B0 * L, d] per layer, every condition (and both CFG halves) of a clip reads its clip's rows through
  // the LayerNorm kernel's row map (fdm_ln_args.add_mat_group) -- no table work per condition
  FCK(clip_tables(P, 0, M0, (rep == 2 && S == 1) ? (size_t)M * d : 0, stream));
  return FDM_OK;
}
// ... and its end: the plan is prepared, tiles chosen
static int prepare_done(fdm_plan* P, void* stream) {
  P->prepared = true;
  select_tiles(P);
  // A request path never tunes by itself: fdm_plan_tune does, when the caller schedules it (fdm_plan_get "needs_tune" says when a
  // shape has served >= 2000 steps on heuristic tiles).  Opt-in (fdm_plan_set "tune_lazy"): tune here / inside fdm_sample_graph
  // once that is the case -- and even then a tuner failure keeps the heuristic tiles instead of failing the request.
  if (P->tune_lazy) tune_soft(P, stream);
  return FDM_OK;
}

int fdm_audio_prepare_conds(fdm_plan* P, const float* hub, int B0, int N, int fw, int S, const float* style, const float* emo, int L, int cfg, void* stream) {
  if (!P || !hub || !style) return fail(FDM_ERR_ARG, "audio_prepare: null argument");
  FCK(prepare_tables(P, hub, B0, N, fw, S, !emo, L, cfg, stream));
  const fdm_model_desc& m = P->m;
  const int d = m.d, B = P->B, M = P->M, rep = P->rep;
  // conditioning addend E0 = PE[l] + style[b] (+ emotion[b]) (:75-84), one row block per (clip, condition)
  const float *sw = nullptr, *sbias = nullptr;
  FCK(need(P, "style_embedd.weight", (long long)d * m.n_style, &sw)); FCK(need(P, "style_embedd.bias", d, &sbias));
  FCK(fdm_op_small_linear(style, sw, sbias, P->sty, B, m.n_style, d, m.style_mish ? FDM_ACT_MISH : FDM_ACT_NONE, stream));
  const float *ew = nullptr, *eb = nullptr;
  if (m.n_emo) {
    FCK(need(P, "emotion_embedd.weight", (long long)d * m.n_emo, &ew)); FCK(need(P, "emotion_embedd.bias", d, &eb));
    FCK(fdm_op_small_linear(emo, ew, eb, P->em, B, m.n_emo, d, FDM_ACT_NONE, stream));
    // null condition = zeros_like(emotion one-hot) (models/fdm_vqvae_mead.py:56-57) -> bias only
    if (cfg) FCK(fdm_op_small_linear(P->zeros, ew, eb, P->emu, B, m.n_emo, d, FDM_ACT_NONE, stream));
  }
  for (int r = 0; r < rep; ++r) {
    const float* e = m.n_emo ? (r == 1 ? P->emu : P->em) : nullptr;
    FCK(fdm_op_add_rows(P->pe, 1, L, P->sty, L, B, e, L, B, P->E0 + (size_t)r * M * d, M, d, stream));
  }
  return prepare_done(P, stream);
}

// fdm_audio_prepare with one style / emotion vector per latent frame: the same tables, E0 from the tracks in one launch
int fdm_audio_prepare_tracks(fdm_plan* P, const float* hub, int B, int N, int fw, const float* style, const float* emo, int L, int cfg, void* stream) {
  if (!P || !hub) return fail(FDM_ERR_ARG, "audio_prepare_tracks: null argument");
  if (!style) return fail(FDM_ERR_ARG, "audio_prepare_tracks: null style track");
  if (P->m.n_emo && !emo) return fail(FDM_ERR_ARG, "audio_prepare_tracks: this model needs an emotion track");
  FCK(prepare_tables(P, hub, B, N, fw, 1, false, L, cfg, stream));
  FCK(cond_tracks(P, 0, P->B, P->L, P->L, style, emo, stream));
  return prepare_done(P, stream);
}

// fdm_audio_prepare_windows (tracks = false: one style / emotion vector per long clip) and fdm_audio_prepare_windows_tracks (tracks =
// true: [B, L_total, n] per-frame rows, window w is staged with the rows [s_w, s_w + W) of its clip)
static int prepare_windows_impl(fdm_plan* P, const float* hub, int B, int N, int fw, const float* style, const float* emo, bool tracks,
                                int L_total, int window, int overlap, int cfg, void* stream) {
  if (!P || !hub || !style) return fail(FDM_ERR_ARG, "audio_prepare_windows: null argument");
  const fdm_model_desc& m = P->m;
  P->win_n = 0;
  if (B < 1 || N < 1 || fw < 1) return fail(FDM_ERR_SHAPE, "audio_prepare_windows: bad feature shape [%d, %d, %d]", B, N, fw);
  if (window < 1 || window > m.max_len) return fail(FDM_ERR_SHAPE, "audio_prepare_windows: window %d outside [1, max_len %d]", window, m.max_len);
  if (overlap < 0 || overlap >= window) return fail(FDM_ERR_ARG, "audio_prepare_windows: overlap %d outside [0, window %d)", overlap, window);
  if (L_total < 1 || L_total > N / m.pair) return fail(FDM_ERR_SHAPE, "audio_prepare_windows: L_total=%d outside [1, %d] (N / pair)", L_total, N / m.pair);
  if (m.pair * fw != m.audio_in) return fail(FDM_ERR_SHAPE, "audio_prepare_windows: audio feature width %d x pair %d != audio_extract input %d", fw, m.pair, m.audio_in);
  if (m.n_emo && !emo) return fail(FDM_ERR_ARG, "audio_prepare_windows: this model needs an emotion one-hot");
  std::vector<int> starts;
  const int n = window_layout(L_total, window, overlap, starts);
  if (n < 0) return n;
  const int W = std::min(window, L_total), Bw = B * n, d = m.d;
  const size_t rows = (size_t)W * m.pair;                       // encoder frames per window
  const size_t per = tracks ? (size_t)W : 1;                     // condition rows per window
  const size_t n_hub = (size_t)Bw * rows * fw, n_sty = (size_t)Bw * per * m.n_style, n_emo = m.n_emo ? (size_t)Bw * per * m.n_emo : 0;
  hipStream_t s = (hipStream_t)stream;
  FCK(grow(P, (void**)&P->win_stage, &P->win_stage_cap, (n_hub + n_sty + n_emo) * 4, stream));
  FCK(grow(P, (void**)&P->xlong, &P->xlong_cap, (size_t)B * L_total * d * 4, stream));
  FCK(grow(P, (void**)&P->hist_long, &P->hist_long_cap, (size_t)B * L_total * d * 4, stream));
  // window w of long clip b = plan clip b * n + w: audio rows [s_w pair, (s_w + W) pair) of the clip, the clip's one-hots
  float *hw = P->win_stage, *sw = hw + n_hub, *ew = sw + n_sty;
  for (int b = 0; b < B; ++b)
    for (int w = 0; w < n; ++w) {
      const size_t k = (size_t)b * n + w;
      HIPCK(hipMemcpyAsync(hw + k * rows * fw, hub + ((size_t)b * N + (size_t)starts[w] * m.pair) * fw, rows * fw * 4, hipMemcpyDefault, s));
      const size_t src = tracks ? (size_t)b * L_total + starts[w] : (size_t)b;      // first condition row of the window
      HIPCK(hipMemcpyAsync(sw + k * per * m.n_style, style + src * m.n_style, per * m.n_style * 4, hipMemcpyDefault, s));
      if (m.n_emo) HIPCK(hipMemcpyAsync(ew + k * per * m.n_emo, emo + src * m.n_emo, per * m.n_emo * 4, hipMemcpyDefault, s));
    }
  // covering windows per frame (ascending window order) with their normalised weights
  std::vector<float> wt;
  window_weights(L_total, window, overlap, starts, wt);
  std::vector<int> off(1, 0);
  std::vector<fdm::WinEnt> ent;
  for (int f = 0; f < L_total; ++f) {
    for (int w = 0; w < n; ++w)
      if (starts[w] <= f && f < starts[w] + W) ent.push_back(fdm::WinEnt{w, starts[w], wt[(size_t)w * W + (f - starts[w])], 0});
    off.push_back((int)ent.size());
  }
  FCK(grow(P, (void**)&P->win_off, &P->win_off_cap, off.size() * sizeof(int), stream));
  FCK(grow(P, (void**)&P->win_ent, &P->win_ent_cap, ent.size() * sizeof(fdm::WinEnt), stream));
  HIPCK(hipMemcpyAsync(P->win_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCK(hipMemcpyAsync(P->win_ent, ent.data(), ent.size() * sizeof(fdm::WinEnt), hipMemcpyHostToDevice, s));
  HIPCK(hipStreamSynchronize(s));            // (off / ent are host vectors of this call)
  if (tracks) FCK(fdm_audio_prepare_tracks(P, hw, Bw, (int)rows, fw, sw, m.n_emo ? ew : nullptr, W, cfg, stream));
  else FCK(fdm_audio_prepare_conds(P, hw, Bw, (int)rows, fw, 1, sw, m.n_emo ? ew : nullptr, W, cfg, stream));
  P->win_n = n; P->win_len = W; P->win_total = L_total; P->win_overlap = overlap; P->win_B = B;
  return FDM_OK;
}

int fdm_audio_prepare_windows(fdm_plan* P, const float* hub, int B, int N, int fw, const float* style, const float* emo, int L_total,
                              int window, int overlap, int cfg, void* stream) {
  return prepare_windows_impl(P, hub, B, N, fw, style, emo, false, L_total, window, overlap, cfg, stream);
}

int fdm_audio_prepare_windows_tracks(fdm_plan* P, const float* hub, int B, int N, int fw, const float* style, const float* emo, int L_total,
                                     int window, int overlap, int cfg, void* stream) {
  if (!style) return fail(FDM_ERR_ARG, "audio_prepare_windows_tracks: null style track");
  if (P && P->m.n_emo && !emo) return fail(FDM_ERR_ARG, "audio_prepare_windows_tracks: this model needs an emotion track");
  return prepare_windows_impl(P, hub, B, N, fw, style, emo, true, L_total, window, overlap, cfg, stream);
}

int fdm_denoise_step(fdm_plan* P, const float* x_t, int t, float cfg_scale, float* x0_hat, float* x0_uncond, void* stream) {
  FCK(check_ready(P));
  if (P->slots) return fail(FDM_ERR_STATE, "denoise_step: the plan is in slot mode (fdm_slots_run)");
  P->pinned.clear();
  if (!x_t || !x0_hat || t < 0 || t >= 1000) return fail(FDM_ERR_ARG, "denoise_step: bad argument (t = %d)", t);
  FCK(load_x(P, x_t, stream));
  FCK(set_steps(P, &t, 1, stream));
  ProgSpec sp; sp.kind = 0; sp.cfg_scale = cfg_scale;
  fdm_prog* prog = nullptr;
  FCK(get_program(P, sp, stream, &prog));
  FCK(fdm_prog_run(prog, stream));
  const size_t nb = (size_t)P->M * P->m.d * 4;
  HIPCK(hipMemcpyAsync(x0_hat, P->x0, nb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (x0_uncond && P->cfg) HIPCK(hipMemcpyAsync(x0_uncond, P->x0 + (size_t)P->M * P->m.d, nb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return FDM_OK;
}

int fdm_sample_graph(fdm_plan* P, const fdm_sample_args* a, void* stream) {
  FCK(check_tables_args(a));
  FCK(check_ready(P));
  if (P->win_n) return fail(FDM_ERR_STATE, "sample_graph: the plan was prepared for windowed sampling (fdm_sample_windows)");
  if (P->slots) return fail(FDM_ERR_STATE, "sample_graph: the plan is in slot mode (fdm_slots_run)");
  return sample_impl(P, a, stream);
}

int fdm_sample_windows(fdm_plan* P, const fdm_sample_args* a, void* stream) {
  FCK(check_tables_args(a));
  FCK(check_ready(P));
  if (P->slots) return fail(FDM_ERR_STATE, "sample_windows: the plan is in slot mode (fdm_slots_run)");
  if (!P->win_n) return fail(FDM_ERR_STATE, "sample_windows: call fdm_audio_prepare_windows first");
  return sample_impl(P, a, stream);
}

int fdm_window_peek(fdm_plan* P, float* out, void* stream) {
  FCK(check_ready(P));
  if (!out) return fail(FDM_ERR_ARG, "window_peek: null output");
  if (!P->win_n) return fail(FDM_ERR_STATE, "window_peek: the plan is not in window mode (fdm_audio_prepare_windows)");
  HIPCK(hipMemcpyAsync(out, P->x, (size_t)P->M * P->m.d * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return FDM_OK;
}

// ---- in-flight batching (include/fdm_hip.h, "Slots") -------------------------------------------------------------------
int fdm_slots_open(fdm_plan* P, int B, int L, int cfg, const fdm_sample_args* a, void* stream) {
  if (!a) return fail(FDM_ERR_ARG, "slots_open: null sampler");
  if (a->noise || a->record) return fail(FDM_ERR_ARG, "slots_open: injected noise and record are not supported in slot mode");
  if (!P) return fail(FDM_ERR_ARG, "slots_open: null plan");
  FCK(check_tables_args(a));
  if (B < 1 || L < 1 || L > P->m.max_len) return fail(FDM_ERR_SHAPE, "slots_open: B=%d, L=%d outside [1, .] x [1, %d]", B, L, P->m.max_len);
  const fdm_model_desc& m = P->m;
  hipStream_t s = (hipStream_t)stream;
  P->pinned.clear();
  P->win_n = 0; P->slots = 0;
  P->long_frames = P->long_groups = P->long_entries = 0;
  P->bank_rows = P->bank_t_cap = P->bank_c_cap = 0;
  FCK(commit(P, stream));
  FCK(reserve(P, B, L, cfg));
  FCK(grow(P, (void**)&P->slot_state, &P->slot_state_cap, (size_t)B * 16, stream));
  FCK(grow(P, (void**)&P->slot_keys, &P->slot_keys_cap, (size_t)B * 16, stream));
  // long capacity asked for before this call: the arena (latent + history), one table row per arena frame, B * L entries (every slot
  // holds at most one window) and the group descriptors -- all reserved here, nothing per admit
  const int LF = (P->want_long_frames > 0 && P->want_long_groups > 0) ? P->want_long_frames : 0, LG = LF ? P->want_long_groups : 0;
  P->long_frames = 0; P->long_groups = 0; P->long_entries = 0;
  P->group_host.clear();
  if (LF) {
    const size_t na = (size_t)LF * m.d;
    FCK(grow(P, (void**)&P->long_x, &P->long_x_cap, na * 4, stream));
    FCK(grow(P, (void**)&P->long_hist, &P->long_hist_cap, na * 4, stream));
    FCK(grow(P, (void**)&P->long_frame, &P->long_frame_cap, (size_t)LF * sizeof(fdm::LongFrame), stream));
    FCK(grow(P, (void**)&P->long_ent, &P->long_ent_cap, (size_t)B * L * sizeof(fdm::LongEnt), stream));
    FCK(grow(P, (void**)&P->long_group, &P->long_group_cap, (size_t)LG * sizeof(fdm::LongGroup), stream));
    FCK(grow(P, (void**)&P->slot_member, &P->slot_member_cap, (size_t)B * 4, stream));
    HIPCK(hipMemsetAsync(P->long_x, 0, na * 4, s));
    HIPCK(hipMemsetAsync(P->long_hist, 0, na * 4, s));
    HIPCK(hipMemsetAsync(P->long_frame, 0xff, (size_t)LF * sizeof(fdm::LongFrame), s));      // group = -1: every arena frame free
    HIPCK(hipMemsetAsync(P->long_ent, 0, (size_t)B * L * sizeof(fdm::LongEnt), s));
    HIPCK(hipMemsetAsync(P->long_group, 0, (size_t)LG * sizeof(fdm::LongGroup), s));
    HIPCK(hipMemsetAsync(P->slot_member, 0xff, (size_t)B * 4, s));                            // -1: every slot plain
  }
  // bank capacity asked for before this call: request rows, 1 + S descriptors, sampler 0's steps + N timesteps, four coefficients per
  // step -- all reserved here, nothing per fdm_slot_sampler_add
  const bool want_bank = P->want_samplers > 0 && P->want_sampler_steps > 0;
  SamplerDef def0;
  P->bank_rows = 0; P->bank_t_cap = 0; P->bank_c_cap = 0;
  P->sampler_host.clear();
  if (want_bank) {
    FCK(sampler_def(a, "slots_open", def0));
    if (def0.ts.empty()) return fail(FDM_ERR_ARG, "slots_open: the sampler has no live step (ddim_steps = %d)", a->ddim_steps);
    const int rows = 1 + P->want_samplers, nt = (int)def0.ts.size() + P->want_sampler_steps;
    FCK(grow(P, &P->slot_req, &P->slot_req_cap, (size_t)B * 16, stream));
    FCK(grow(P, (void**)&P->bank_desc, &P->bank_desc_cap, (size_t)rows * 16, stream));
    FCK(grow(P, (void**)&P->bank_t, &P->bank_t_bytes, (size_t)nt * 4, stream));
    FCK(grow(P, (void**)&P->bank_c, &P->bank_c_bytes, (size_t)nt * 16, stream));
    HIPCK(hipMemsetAsync(P->slot_req, 0, (size_t)B * 16, s));
    HIPCK(hipMemsetAsync(P->bank_desc, 0, (size_t)rows * 16, s));             // n_steps = 0: every descriptor free
    HIPCK(hipMemsetAsync(P->bank_t, 0, (size_t)nt * 4, s));
    HIPCK(hipMemsetAsync(P->bank_c, 0, (size_t)nt * 16, s));
  }
  const int d = m.d, M = B * L, rep = cfg ? 2 : 1;
  P->B = B; P->S = 1; P->L = L; P->M = M; P->rep = rep; P->R = M * rep; P->cfg = cfg ? 1 : 0; P->Lpad = (L + 31) / 32 * 32;
  // every slot idle and holding zeros: tables, latent (+ operand copy), history, packed K / V pad keys, state words and keys
  HIPCK(hipMemsetAsync(P->kp, 0, P->kv_bytes, s));
  HIPCK(hipMemsetAsync(P->vp, 0, P->kv_bytes, s));
  const size_t nm = (size_t)M * d, nr = (size_t)P->R * d;
  HIPCK(hipMemsetAsync(P->AF, 0, nm * 4, s));
  HIPCK(hipMemsetAsync(P->E0, 0, nr * 4, s));
  for (int l = 0; l < m.n_layers; ++l) HIPCK(hipMemsetAsync(P->C1[l], 0, nr * 4, s));
  HIPCK(hipMemsetAsync(P->x, 0, nm * 4, s));
  HIPCK(hipMemsetAsync(P->x0_hist, 0, nm * 4, s));
  if (P->dtype != FDM_F32) FCK(zero_mat(P, P->xt, 0, nm, stream));
  HIPCK(hipMemsetAsync(P->slot_state, 0, (size_t)B * 16, s));
  HIPCK(hipMemsetAsync(P->slot_keys, 0, (size_t)B * 16, s));
  // the shared sampler: timestep list and tables on the device (drains the stream once, as a sampling call does)
  std::vector<int> ts;
  ProgSpec sp;
  FCK(sampler_setup(P, a, stream, ts, sp));
  if (ts.empty()) return fail(FDM_ERR_ARG, "slots_open: the sampler has no live step (ddim_steps = %d)", a->ddim_steps);
  if (want_bank) {           // sampler 0 at the start of the bank (set_steps below drains the copies: def0 is host memory)
    const int desc0[4] = {def0.mode, (int)def0.ts.size(), 0, 0};
    HIPCK(hipMemcpyAsync(P->bank_desc, desc0, 16, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(P->bank_t, def0.ts.data(), def0.ts.size() * 4, hipMemcpyHostToDevice, s));
    if (!def0.coef.empty()) HIPCK(hipMemcpyAsync(P->bank_c, def0.coef.data(), def0.coef.size() * 4, hipMemcpyHostToDevice, s));
  }
  FCK(set_steps(P, ts.data(), (int)ts.size(), stream));
  P->slot_kind = sp.kind; P->slot_nsteps = (int)ts.size(); P->slot_t0 = ts[0];
  P->slot_san = sp.san; P->slot_cn = sp.cn;
  P->slot_cfg_scale = a->cfg_scale; P->slot_graph_steps = a->graph_steps; P->slot_eager = a->eager;
  P->slot_host.assign(B, fdm_plan::SlotHost());
  P->slots = B;
  if (LF) { P->long_frames = LF; P->long_groups = LG; P->long_entries = B * L; P->group_host.assign(LG, fdm_plan::GroupHost()); }
  if (want_bank) {
    P->bank_rows = 1 + P->want_samplers; P->bank_t_cap = (int)def0.ts.size() + P->want_sampler_steps; P->bank_c_cap = 4 * P->bank_t_cap;
    P->sampler_host.assign(P->bank_rows, fdm_plan::SamplerHost());
    fdm_plan::SamplerHost& s0 = P->sampler_host[0];
    s0.used = true; s0.kind = def0.kind; s0.mode = def0.mode; s0.n_steps = (int)def0.ts.size(); s0.t0 = def0.ts[0]; s0.n_c = (int)def0.coef.size();
  }
  P->prepared = true;
  select_tiles(P);
  return FDM_OK;
}

// the sampler and guidance scale of a request, checked (fdm_slot_admit_as / fdm_slot_admit_long_as): steps and first timestep of its chain
static int request_sampler(const fdm_plan* P, const char* who, int sampler, float cfg_scale, int* n_steps, int* t0) {
  if (!P->bank_rows) {
    if (sampler != 0) return fail(FDM_ERR_ARG, "%s: sampler %d, the session has no sampler bank (fdm_plan_set slot_samplers / slot_sampler_steps before fdm_slots_open)", who, sampler);
    if (P->cfg && cfg_scale != P->slot_cfg_scale) return fail(FDM_ERR_ARG, "%s: a cfg_scale per request needs a sampler bank (the session's is %g)", who, (double)P->slot_cfg_scale);
    *n_steps = P->slot_nsteps; *t0 = P->slot_t0;
    return FDM_OK;
  }
  if (sampler < 0 || sampler >= P->bank_rows || !P->sampler_host[sampler].used) return fail(FDM_ERR_ARG, "%s: unknown sampler %d", who, sampler);
  *n_steps = P->sampler_host[sampler].n_steps; *t0 = P->sampler_host[sampler].t0;
  return FDM_OK;
}
// one slot's word and key (and, with a bank, its request row): {k = -1, running} at the first timestep of its sampler
static int slot_start(fdm_plan* P, int slot, int t0, unsigned long long seed, int clip_id, int sampler, float cfg_scale, void* stream) {
  if (P->bank_rows) return fdm::slot_set_bank_op(P->slot_state, slot, -1, t0, 0, 1, P->slot_keys, seed, clip_id, P->slot_req, sampler, cfg_scale, stream);
  return fdm::slot_set_op(P->slot_state, slot, -1, t0, 0, 1, P->slot_keys, seed, clip_id, stream);
}

int fdm_slot_admit(fdm_plan* P, int slot, const float* hub, int N, int fw, const float* style, const float* emo, int L_clip,
                   const float* x_T, unsigned long long seed, int clip_id, void* stream) {
  if (!P) return fail(FDM_ERR_ARG, "slot_admit: null argument");
  return fdm_slot_admit_as(P, slot, hub, N, fw, style, emo, L_clip, x_T, seed, clip_id, 0, P->slot_cfg_scale, stream);
}

// fdm_slot_admit_as (tracks = false: style / emo are the clip's one vector each) and fdm_slot_admit_tracks (tracks = true: [L_clip, n]
// per-frame rows): everything but the E0 rows is the same work
static int slot_admit_impl(fdm_plan* P, int slot, const float* hub, int N, int fw, const float* style, const float* emo, bool tracks, int L_clip,
                           const float* x_T, unsigned long long seed, int clip_id, int sampler, float cfg_scale, void* stream) {
  if (!P || !hub || !style || !x_T) return fail(FDM_ERR_ARG, "slot_admit: null argument");
  FCK(check_slots(P, "slot_admit"));
  const fdm_model_desc& m = P->m;
  if (slot < 0 || slot >= P->slots) return fail(FDM_ERR_ARG, "slot_admit: slot %d outside [0, %d)", slot, P->slots);
  if (m.n_emo && !emo) return fail(FDM_ERR_ARG, "slot_admit: this model needs an emotion one-hot");
  if (N < 1 || fw < 1 || m.pair * fw != m.audio_in) return fail(FDM_ERR_SHAPE, "slot_admit: audio feature width %d x pair %d != audio_extract input %d", fw, m.pair, m.audio_in);
  if (L_clip < 1 || L_clip > P->L || L_clip > N / m.pair) return fail(FDM_ERR_SHAPE, "slot_admit: L_clip=%d outside [1, min(%d, %d)]", L_clip, P->L, N / m.pair);
  fdm_plan::SlotHost& h = P->slot_host[slot];
  if (h.status != 0) return fail(FDM_ERR_STATE, "slot_admit: slot %d is %s", slot, h.status == 1 ? "running" : "finished and not read");
  int total = 0, t0 = 0;
  FCK(request_sampler(P, "slot_admit", sampler, cfg_scale, &total, &t0));
  hipStream_t s = (hipStream_t)stream;
  const int d = m.d, L = P->L, row0 = slot * L, pad = L - L_clip;
  const size_t o = (size_t)row0 * d, nclip = (size_t)L_clip * d, npad = (size_t)pad * d;
  if (tracks) FCK(slot_rows_tracks(P, slot, hub, style, emo, 0, L_clip, stream));
  else FCK(slot_rows(P, slot, hub, style, emo, L_clip, stream));
  // x_T (+ zero tail) and its operand copy into the slot's rows; the history starts at zero
  HIPCK(hipMemcpyAsync(P->x + o, x_T, nclip * 4, hipMemcpyDeviceToDevice, s));
  if (pad) HIPCK(hipMemsetAsync(P->x + o + nclip, 0, npad * 4, s));
  HIPCK(hipMemsetAsync(P->x0_hist + o, 0, (size_t)L * d * 4, s));
  if (P->dtype != FDM_F32) FCK(operand_copy(P, P->x + o, (char*)P->xt.p + o * kind(P->dtype).bytes, (long long)L * d, stream));
  // {k = -1, running}: the next step's advance launch makes it step 0 of this slot's chain
  FCK(slot_start(P, slot, t0, seed, clip_id, sampler, cfg_scale, stream));
  h.status = 1; h.done = 0; h.L = L_clip; h.sampler = sampler; h.total = total;
  return FDM_OK;
}

int fdm_slot_admit_as(fdm_plan* P, int slot, const float* hub, int N, int fw, const float* style, const float* emo, int L_clip,
                      const float* x_T, unsigned long long seed, int clip_id, int sampler, float cfg_scale, void* stream) {
  return slot_admit_impl(P, slot, hub, N, fw, style, emo, false, L_clip, x_T, seed, clip_id, sampler, cfg_scale, stream);
}

int fdm_slot_admit_tracks(fdm_plan* P, int slot, const float* hub, int N, int fw, const float* style, const float* emo, int L_clip,
                          const float* x_T, unsigned long long seed, int clip_id, int sampler, float cfg_scale, void* stream) {
  if (!style) return fail(FDM_ERR_ARG, "slot_admit_tracks: null style track");
  if (P && P->m.n_emo && !emo) return fail(FDM_ERR_ARG, "slot_admit_tracks: this model needs an emotion track");
  return slot_admit_impl(P, slot, hub, N, fw, style, emo, true, L_clip, x_T, seed, clip_id, sampler, cfg_scale, stream);
}

int fdm_slots_run(fdm_plan* P, int n_steps, void* stream) {
  FCK(check_slots(P, "slots_run"));
  if (n_steps < 0) return fail(FDM_ERR_ARG, "slots_run: n_steps = %d", n_steps);
  P->pinned.clear();
  P->last_graph_launches = 0;
  ProgSpec sp;
  sp.kind = P->slot_kind; sp.cfg_scale = P->slot_cfg_scale; sp.san = P->slot_san; sp.cn = P->slot_cn; sp.slot_steps = P->slot_nsteps;
  if (P->bank_rows) {        // the bank program serves every sampler and scale: none of them is part of its key
    sp = ProgSpec();
    sp.kind = 4; sp.slot_steps = 1; sp.bank = 1;
  }
  fdm_prog* p1 = nullptr;
  FCK(get_program(P, sp, stream, &p1));
  if (n_steps == 0) return FDM_OK;
  P->steps_seen[shape_key(P)] += n_steps;
  if (P->slot_eager) {
    for (int i = 0; i < n_steps; ++i) FCK(fdm_prog_run(p1, stream));
  } else {
    FCK(replay_steps(P, sp, p1, n_steps, P->slot_graph_steps, stream));
  }
  // the host mirror: a running slot does min(n_steps, what ITS chain has left) steps and freezes when the chain ends
  for (auto& h : P->slot_host)
    if (h.status == 1) {
      h.done = std::min(h.total, h.done + n_steps);
      if (h.done == h.total) h.status = 2;
    }
  return FDM_OK;
}

int fdm_slot_state(fdm_plan* P, int slot, int* steps_done, int* steps_total, int* status) {
  FCK(check_slots(P, "slot_state"));
  if (slot < 0 || slot >= P->slots) return fail(FDM_ERR_ARG, "slot_state: slot %d outside [0, %d)", slot, P->slots);
  const fdm_plan::SlotHost& h = P->slot_host[slot];
  if (steps_done) *steps_done = h.done;
  if (steps_total) *steps_total = h.status ? h.total : P->slot_nsteps;      // (an idle slot: sampler 0's)
  if (status) *status = h.status;
  return FDM_OK;
}

int fdm_slot_read(fdm_plan* P, int slot, float* out, void* stream) {
  FCK(check_slots(P, "slot_read"));
  if (!out) return fail(FDM_ERR_ARG, "slot_read: null output");
  if (slot < 0 || slot >= P->slots) return fail(FDM_ERR_ARG, "slot_read: slot %d outside [0, %d)", slot, P->slots);
  fdm_plan::SlotHost& h = P->slot_host[slot];
  if (h.group >= 0) return fail(FDM_ERR_STATE, "slot_read: slot %d holds a window of a long request (fdm_slot_read_long on its leader)", slot);
  if (h.status != 2) return fail(FDM_ERR_STATE, "slot_read: slot %d is %s, not finished", slot, h.status == 1 ? "running" : "idle");
  HIPCK(hipMemcpyAsync(out, P->x + (size_t)slot * P->L * P->m.d, (size_t)h.L * P->m.d * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (P->bank_rows) FCK(fdm::slot_park_op(P->slot_state, slot, stream));      // (its sampler may be dropped and the descriptor reused)
  h = fdm_plan::SlotHost();
  return FDM_OK;
}

int fdm_slot_peek(fdm_plan* P, int slot, float* out, void* stream) {
  FCK(check_slots(P, "slot_peek"));
  if (!out) return fail(FDM_ERR_ARG, "slot_peek: null output");
  if (slot < 0 || slot >= P->slots) return fail(FDM_ERR_ARG, "slot_peek: slot %d outside [0, %d)", slot, P->slots);
  HIPCK(hipMemcpyAsync(out, P->x + (size_t)slot * P->L * P->m.d, (size_t)P->L * P->m.d * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return FDM_OK;
}

// ---- long requests in slot mode (include/fdm_hip.h, "Long requests in slot mode") -----------------------------------------
int fdm_slot_admit_long(fdm_plan* P, const int* slots, int n, const float* hub, int N, int fw, const float* style, const float* emo,
                        int L_total, int overlap, const float* x_T, unsigned long long seed, int clip_id, void* stream) {
  if (!P) return fail(FDM_ERR_ARG, "slot_admit_long: null argument");
  return fdm_slot_admit_long_as(P, slots, n, hub, N, fw, style, emo, L_total, overlap, x_T, seed, clip_id, 0, P->slot_cfg_scale, stream);
}

// fdm_slot_admit_long_as (tracks = false) and fdm_slot_admit_long_tracks (tracks = true: style / emo are [L_total, n] per-frame rows and
// window w reads the rows [s_w, s_w + L)): everything but the E0 rows is the same work
static int slot_admit_long_impl(fdm_plan* P, const int* slots, int n, const float* hub, int N, int fw, const float* style, const float* emo,
                                bool tracks, int L_total, int overlap, const float* x_T, unsigned long long seed, int clip_id, int sampler,
                                float cfg_scale, void* stream) {
  if (!P || !slots || !hub || !style || !x_T) return fail(FDM_ERR_ARG, "slot_admit_long: null argument");
  FCK(check_slots(P, "slot_admit_long"));
  const fdm_model_desc& m = P->m;
  const int d = m.d, L = P->L;
  if (!P->long_frames) return fail(FDM_ERR_ARG, "slot_admit_long: the session has no long capacity (fdm_plan_set slot_long_frames / slot_long_groups before fdm_slots_open)");
  if (m.n_emo && !emo) return fail(FDM_ERR_ARG, "slot_admit_long: this model needs an emotion one-hot");
  if (N < 1 || fw < 1 || m.pair * fw != m.audio_in) return fail(FDM_ERR_SHAPE, "slot_admit_long: audio feature width %d x pair %d != audio_extract input %d", fw, m.pair, m.audio_in);
  if (overlap < 0 || overlap >= L) return fail(FDM_ERR_ARG, "slot_admit_long: overlap %d outside [0, slot capacity %d)", overlap, L);
  if (L_total <= L) return fail(FDM_ERR_SHAPE, "slot_admit_long: L_total=%d fits one slot of %d frames (fdm_slot_admit)", L_total, L);
  if (L_total > N / m.pair) return fail(FDM_ERR_SHAPE, "slot_admit_long: L_total=%d outside (%d, %d] (N / pair)", L_total, L, N / m.pair);
  if (L_total > P->long_frames) return fail(FDM_ERR_SHAPE, "slot_admit_long: L_total=%d exceeds the arena of %d long frames", L_total, P->long_frames);
  int total = 0, t0 = 0;
  FCK(request_sampler(P, "slot_admit_long", sampler, cfg_scale, &total, &t0));
  std::vector<int> starts;
  const int nw = window_layout(L_total, L, overlap, starts);
  if (nw < 0) return nw;
  if (n != nw) return fail(FDM_ERR_SHAPE, "slot_admit_long: %d slots for the %d windows of L_total=%d, window %d, overlap %d", n, nw, L_total, L, overlap);
  if (n > P->slots) return fail(FDM_ERR_SHAPE, "slot_admit_long: %d windows, the plan has %d slots", n, P->slots);
  for (int w = 0; w < n; ++w) {
    if (slots[w] < 0 || slots[w] >= P->slots) return fail(FDM_ERR_ARG, "slot_admit_long: slot %d outside [0, %d)", slots[w], P->slots);
    for (int v = 0; v < w; ++v)
      if (slots[v] == slots[w]) return fail(FDM_ERR_ARG, "slot_admit_long: slot %d is listed twice", slots[w]);
  }
  for (int w = 0; w < n; ++w) {
    const int st = P->slot_host[slots[w]].status;
    if (st != 0) return fail(FDM_ERR_STATE, "slot_admit_long: slot %d is %s", slots[w], st == 1 ? "running" : "finished and not read");
  }
  // a free descriptor, a contiguous arena range and a contiguous entry range, by first fit over what the live groups hold
  int gi = -1;
  for (int i = 0; i < P->long_groups && gi < 0; ++i)
    if (!P->group_host[i].used) gi = i;
  if (gi < 0) return fail(FDM_ERR_STATE, "slot_admit_long: all %d group descriptors are in use", P->long_groups);
  auto first_fit = [&](bool arena, int need, int cap) {
    std::vector<std::pair<int, int>> used;
    for (const auto& g : P->group_host)
      if (g.used) used.push_back(arena ? std::make_pair(g.first, g.L_total) : std::make_pair(g.e0, g.ne));
    std::sort(used.begin(), used.end());
    int at = 0;
    for (const auto& u : used) {
      if (u.first - at >= need) return at;
      at = u.first + u.second;
    }
    return cap - at >= need ? at : -1;
  };
  const int ne = n * L;
  const int a0 = first_fit(true, L_total, P->long_frames), e0 = first_fit(false, ne, P->long_entries);
  if (a0 < 0) return fail(FDM_ERR_STATE, "slot_admit_long: no free arena range of %d frames (arena %d)", L_total, P->long_frames);
  if (e0 < 0) return fail(FDM_ERR_STATE, "slot_admit_long: no free entry range of %d entries", ne);
  std::vector<int> off((size_t)L_total + 1), es(ne), est(ne);
  std::vector<float> ew(ne);
  const int got = fdm_slot_group_table_host(L_total, L, overlap, slots, n, off.data(), es.data(), est.data(), ew.data(), ne);
  if (got != ne) return got < 0 ? got : fail(FDM_ERR_STATE, "slot_admit_long: the group table has %d entries, expected %d", got, ne);
  std::vector<fdm::LongFrame> frames(L_total);
  std::vector<fdm::LongEnt> ents(ne);
  for (int f = 0; f < L_total; ++f) frames[f] = fdm::LongFrame{gi, e0 + off[f], e0 + off[f + 1], 0};
  for (int j = 0; j < ne; ++j) ents[j] = fdm::LongEnt{es[j], est[j], ew[j], 0};
  const fdm::LongGroup desc{slots[0], L_total, a0, 0};
  std::vector<int> member(n, gi);
  // ---- nothing above touched the plan; from here on the device work, in stream order between steps
  hipStream_t s = (hipStream_t)stream;
  HIPCK(hipMemcpyAsync(P->long_frame + a0, frames.data(), frames.size() * sizeof(fdm::LongFrame), hipMemcpyHostToDevice, s));
  HIPCK(hipMemcpyAsync(P->long_ent + e0, ents.data(), ents.size() * sizeof(fdm::LongEnt), hipMemcpyHostToDevice, s));
  HIPCK(hipMemcpyAsync(P->long_group + gi, &desc, sizeof(desc), hipMemcpyHostToDevice, s));
  for (int w = 0; w < n; ++w) HIPCK(hipMemcpyAsync(P->slot_member + slots[w], &member[w], 4, hipMemcpyHostToDevice, s));
  HIPCK(hipStreamSynchronize(s));            // (the tables are host vectors of this call)
  // every member's rows of AF, C1_l and E0: window w is an ordinary clip of L frames on the audio rows [s_w pair, (s_w + L) pair)
  for (int w = 0; w < n; ++w) {
    const float* hw = hub + (size_t)starts[w] * m.pair * fw;
    if (tracks) FCK(slot_rows_tracks(P, slots[w], hw, style, emo, starts[w], L, stream));
    else FCK(slot_rows(P, slots[w], hw, style, emo, L, stream));
  }
  // x_T into the arena, the group's history to zero, then the window rows (+ operand copies) through the pass's init form
  const size_t ao = (size_t)a0 * d, nl = (size_t)L_total * d;
  HIPCK(hipMemcpyAsync(P->long_x + ao, x_T, nl * 4, hipMemcpyDeviceToDevice, s));
  HIPCK(hipMemsetAsync(P->long_hist + ao, 0, nl * 4, s));
  fdm_sched_args sc;
  memset(&sc, 0, sizeof(sc));
  sc.mode = 2; sc.x_out = P->x; sc.n = (long long)P->M * d; sc.n_per_clip = (long long)L * d;
  if (P->dtype != FDM_F32) { sc.x_out_t = P->xt.p; sc.out_dtype = P->dtype; sc.x_out_t_lo_off = P->xt.lo; }
  const fdm_slot_group_args lg = long_args(P, a0, a0 + L_total, 0, 1);
  FCK(fdm_op_slot_group_sched(&sc, P->slot_state, P->slot_keys, P->slots, &lg, stream));
  // every member {k = -1, running} with the group's key (and request): the next step's advance launch makes it step 0 of the group's chain
  for (int w = 0; w < n; ++w) {
    FCK(slot_start(P, slots[w], t0, seed, clip_id, sampler, cfg_scale, stream));
    fdm_plan::SlotHost& h = P->slot_host[slots[w]];
    h.status = 1; h.done = 0; h.L = L; h.group = gi; h.sampler = sampler; h.total = total;
  }
  fdm_plan::GroupHost& gh = P->group_host[gi];
  gh.used = true; gh.L_total = L_total; gh.first = a0; gh.e0 = e0; gh.ne = ne; gh.slots.assign(slots, slots + n);
  return FDM_OK;
}

int fdm_slot_admit_long_as(fdm_plan* P, const int* slots, int n, const float* hub, int N, int fw, const float* style, const float* emo,
                           int L_total, int overlap, const float* x_T, unsigned long long seed, int clip_id, int sampler, float cfg_scale,
                           void* stream) {
  return slot_admit_long_impl(P, slots, n, hub, N, fw, style, emo, false, L_total, overlap, x_T, seed, clip_id, sampler, cfg_scale, stream);
}

int fdm_slot_admit_long_tracks(fdm_plan* P, const int* slots, int n, const float* hub, int N, int fw, const float* style, const float* emo,
                               int L_total, int overlap, const float* x_T, unsigned long long seed, int clip_id, int sampler,
                               float cfg_scale, void* stream) {
  if (!style) return fail(FDM_ERR_ARG, "slot_admit_long_tracks: null style track");
  if (P && P->m.n_emo && !emo) return fail(FDM_ERR_ARG, "slot_admit_long_tracks: this model needs an emotion track");
  return slot_admit_long_impl(P, slots, n, hub, N, fw, style, emo, true, L_total, overlap, x_T, seed, clip_id, sampler, cfg_scale, stream);
}

int fdm_slot_group(fdm_plan* P, int slot, int* leader, int* n, int* L_total) {
  FCK(check_slots(P, "slot_group"));
  if (slot < 0 || slot >= P->slots) return fail(FDM_ERR_ARG, "slot_group: slot %d outside [0, %d)", slot, P->slots);
  const int gi = P->slot_host[slot].group;
  const fdm_plan::GroupHost* g = gi >= 0 ? &P->group_host[gi] : nullptr;
  if (leader) *leader = g ? g->slots[0] : -1;
  if (n) *n = g ? (int)g->slots.size() : 0;
  if (L_total) *L_total = g ? g->L_total : 0;
  return FDM_OK;
}

int fdm_slot_read_long(fdm_plan* P, int leader, float* out, void* stream) {
  FCK(check_slots(P, "slot_read_long"));
  if (!out) return fail(FDM_ERR_ARG, "slot_read_long: null output");
  if (leader < 0 || leader >= P->slots) return fail(FDM_ERR_ARG, "slot_read_long: slot %d outside [0, %d)", leader, P->slots);
  const int gi = P->slot_host[leader].group;
  if (gi < 0 || P->group_host[gi].slots[0] != leader) return fail(FDM_ERR_STATE, "slot_read_long: slot %d does not lead a long request", leader);
  fdm_plan::GroupHost& g = P->group_host[gi];
  for (int sl : g.slots)
    if (P->slot_host[sl].status != 2) return fail(FDM_ERR_STATE, "slot_read_long: the group of slot %d is running, not finished", leader);
  hipStream_t s = (hipStream_t)stream;
  const int d = P->m.d;
  HIPCK(hipMemcpyAsync(out, P->long_x + (size_t)g.first * d, (size_t)g.L_total * d * 4, hipMemcpyDeviceToDevice, s));
  // the arena frames go back to free and the members to plain, so that a later clip in the leader's slot never wakes this group
  HIPCK(hipMemsetAsync(P->long_frame + g.first, 0xff, (size_t)g.L_total * sizeof(fdm::LongFrame), s));
  for (int sl : g.slots) {
    HIPCK(hipMemsetAsync(P->slot_member + sl, 0xff, 4, s));
    if (P->bank_rows) FCK(fdm::slot_park_op(P->slot_state, sl, stream));
    P->slot_host[sl] = fdm_plan::SlotHost();
  }
  g = fdm_plan::GroupHost();
  return FDM_OK;
}

// ---- samplers per request in slot mode (include/fdm_hip.h, "Samplers per request in slot mode") ---------------------------
int fdm_slot_sampler_add(fdm_plan* P, const fdm_sample_args* a, void* stream) {
  if (!a) return fail(FDM_ERR_ARG, "slot_sampler_add: null sampler");
  if (a->noise || a->record) return fail(FDM_ERR_ARG, "slot_sampler_add: injected noise and record are not supported in slot mode");
  if (!P) return fail(FDM_ERR_ARG, "slot_sampler_add: null plan");
  FCK(check_slots(P, "slot_sampler_add"));
  SamplerDef def;
  FCK(sampler_def(a, "slot_sampler_add", def));
  if (def.ts.empty()) return fail(FDM_ERR_ARG, "slot_sampler_add: the sampler has no live step (ddim_steps = %d)", a->ddim_steps);
  if (!P->bank_rows) return fail(FDM_ERR_STATE, "slot_sampler_add: the session has no sampler bank (fdm_plan_set slot_samplers / slot_sampler_steps before fdm_slots_open)");
  int id = -1;
  for (int i = 1; i < P->bank_rows && id < 0; ++i)
    if (!P->sampler_host[i].used) id = i;
  if (id < 0) return fail(FDM_ERR_STATE, "slot_sampler_add: all %d bank rows are in use", P->bank_rows - 1);
  // a timestep range and a coefficient range, by first fit over what the live samplers hold
  auto first_fit = [&](bool coef, int need, int cap) {
    std::vector<std::pair<int, int>> used;
    for (const auto& h : P->sampler_host)
      if (h.used && (coef ? h.n_c : h.n_steps) > 0) used.push_back(coef ? std::make_pair(h.c_off, h.n_c) : std::make_pair(h.t_off, h.n_steps));
    std::sort(used.begin(), used.end());
    int at = 0;
    for (const auto& u : used) {
      if (u.first - at >= need) return at;
      at = u.first + u.second;
    }
    return cap - at >= need ? at : -1;
  };
  const int nt = (int)def.ts.size(), nc = (int)def.coef.size();
  const int t_off = first_fit(false, nt, P->bank_t_cap), c_off = nc ? first_fit(true, nc, P->bank_c_cap) : 0;
  if (t_off < 0) return fail(FDM_ERR_STATE, "slot_sampler_add: no free range of %d timesteps (bank %d)", nt, P->bank_t_cap);
  if (c_off < 0) return fail(FDM_ERR_STATE, "slot_sampler_add: no free range of %d coefficients (bank %d)", nc, P->bank_c_cap);
  // ---- nothing above touched the plan.  The ranges are free: no running slot names them, so the upload is legal mid-chain
  hipStream_t s = (hipStream_t)stream;
  const int desc[4] = {def.mode, nt, t_off, c_off};
  HIPCK(hipMemcpyAsync(P->bank_t + t_off, def.ts.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
  if (nc) HIPCK(hipMemcpyAsync(P->bank_c + c_off, def.coef.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
  HIPCK(hipMemcpyAsync(P->bank_desc + 4 * (size_t)id, desc, 16, hipMemcpyHostToDevice, s));
  HIPCK(hipStreamSynchronize(s));            // (the tables are host memory of this call)
  fdm_plan::SamplerHost& h = P->sampler_host[id];
  h.used = true; h.kind = def.kind; h.mode = def.mode; h.n_steps = nt; h.t0 = def.ts[0]; h.t_off = t_off; h.c_off = c_off; h.n_c = nc;
  return id;
}

int fdm_slot_sampler_drop(fdm_plan* P, int id) {
  if (!P) return fail(FDM_ERR_ARG, "slot_sampler_drop: null plan");
  FCK(check_slots(P, "slot_sampler_drop"));
  if (id < 1 || id >= P->bank_rows || !P->sampler_host[id].used) return fail(FDM_ERR_ARG, "slot_sampler_drop: %s", id == 0 ? "sampler 0 belongs to the session" : "unknown sampler");
  for (size_t i = 0; i < P->slot_host.size(); ++i)
    if (P->slot_host[i].status != 0 && P->slot_host[i].sampler == id)
      return fail(FDM_ERR_STATE, "slot_sampler_drop: slot %d (%s) names sampler %d", (int)i, P->slot_host[i].status == 1 ? "running" : "finished and not read", id);
  // host only: every slot that named it has been read (its word is parked), and a descriptor nobody names is never loaded
  P->sampler_host[id] = fdm_plan::SamplerHost();
  return FDM_OK;
}

int fdm_slot_sampler_info(fdm_plan* P, int id, int* kind, int* n_steps) {
  if (!P) return fail(FDM_ERR_ARG, "slot_sampler_info: null plan");
  FCK(check_slots(P, "slot_sampler_info"));
  if (!P->bank_rows) {
    if (id != 0) return fail(FDM_ERR_ARG, "slot_sampler_info: unknown sampler %d", id);
    if (kind) *kind = P->slot_kind - 1;      // (program kind 1 / 2 / 3 = fdm_sample_args.kind 0 / 1 / 2)
    if (n_steps) *n_steps = P->slot_nsteps;
    return FDM_OK;
  }
  if (id < 0 || id >= P->bank_rows || !P->sampler_host[id].used) return fail(FDM_ERR_ARG, "slot_sampler_info: unknown sampler %d", id);
  if (kind) *kind = P->sampler_host[id].kind;
  if (n_steps) *n_steps = P->sampler_host[id].n_steps;
  return FDM_OK;
}

int fdm_plan_tune(fdm_plan* P, void* stream) {
  FCK(check_ready(P));
  return tune_tiles(P, 1, stream);
}

int fdm_plan_get(fdm_plan* P, const char* key, long long* out) {
  if (!P || !key || !out) return fail(FDM_ERR_ARG, "plan_get: null argument");
  const std::string k(key);
  if (k == "launches_per_step") *out = P->launches_per_step;
  else if (k == "graph_launches") *out = P->last_graph_launches;
  else if (k == "fuse_ln3") *out = P->fuse_ln3;
  else if (k == "rows") *out = P->R;
  else if (k == "ksplit.out") *out = P->ksplit_out;
  else if (k == "ksplit.ffn2") *out = P->ksplit_ffn2;
  else if (k == "tuned") *out = P->tile_cache.count(shape_key(P)) ? 1 : 0;
  else if (k == "needs_tune") *out = needs_tune(P, shape_key(P)) ? 1 : 0;
  else if (k == "tune_failed") *out = P->tune_failed;
  else if (k == "windows") *out = P->win_n;
  else if (k == "slots") *out = P->slots;
  else if (k == "slot_long_frames") *out = P->want_long_frames;
  else if (k == "slot_long_groups") *out = P->want_long_groups;
  else if (k == "slot_samplers") *out = P->want_samplers;
  else if (k == "slot_sampler_steps") *out = P->want_sampler_steps;
  else if (k == "window_len") *out = P->win_n ? P->win_len : P->L;
  else if (k == "L_total") *out = P->win_n ? P->win_total : P->L;
  else if (k.rfind("tile.", 0) == 0) { auto it = P->tiles.find(k.substr(5)); *out = it == P->tiles.end() ? 0 : it->second; }
  else return fail(FDM_ERR_ARG, "plan_get: unknown key '%s'", key);
  return FDM_OK;
}

int fdm_plan_set(fdm_plan* P, const char* key, long long value) {
  if (!P || !key) return fail(FDM_ERR_ARG, "plan_set: null argument");
  const std::string k(key);
  if (k == "tune") { P->tune_enabled = value != 0; return FDM_OK; }
  if (k == "tune_lazy") { P->tune_lazy = value != 0; return FDM_OK; }
  if (k == "slot_long_frames" || k == "slot_long_groups") {      // long capacity of the NEXT fdm_slots_open (both > 0 to have any)
    if (value < 0 || value > 0x3fffffffLL) return fail(FDM_ERR_ARG, "plan_set: %s = %lld", key, value);
    (k == "slot_long_frames" ? P->want_long_frames : P->want_long_groups) = (int)value;
    return FDM_OK;
  }
  if (k == "slot_samplers" || k == "slot_sampler_steps") {      // bank capacity of the NEXT fdm_slots_open (both > 0 to have any)
    if (value < 0 || value > 0xfffffLL) return fail(FDM_ERR_ARG, "plan_set: %s = %lld", key, value);
    (k == "slot_samplers" ? P->want_samplers : P->want_sampler_steps) = (int)value;
    return FDM_OK;
  }
  if (k == "fuse_ln3") {      // takes effect at the next commit (the folded weights are commit-time tables)
    if ((value != 0) != (P->want_fuse_ln3 != 0)) { P->want_fuse_ln3 = value != 0; P->committed = false; P->prepared = false; return drop_programs(P, nullptr); }
    return FDM_OK;
  }
  if (k == "ksplit.out" || k == "ksplit.ffn2") {      // K slices of the out-proj / FFN2 GEMMs (1 = none); tuned tiles of other split factors no longer apply
    const int kt = (k == "ksplit.out" ? P->m.d : P->m.ffn) / kind(P->dtype).bk;
    if (value < 1 || value > 4 || kt % value) return fail(FDM_ERR_ARG, "plan_set: %s = %lld must be 1..4 and divide the %d k-tiles", key, value, kt);
    int& cur = k == "ksplit.out" ? P->ksplit_out : P->ksplit_ffn2;
    if (cur == (int)value) return FDM_OK;
    cur = (int)value;
    P->tile_cache.clear(); P->tiles.erase(k == "ksplit.out" ? "out" : "ffn2");
    FCK(drop_programs(P, nullptr));
    if (P->capB > 0 && (int)value > P->x1_planes) {     // more partial planes than the workspace holds: a larger x1 (its contents do not outlive a step)
      P->x1_planes = (int)value;
      FCK(zalloc(P->ws, &P->x1, (size_t)P->capB * P->capL * P->capRep * P->m.d * P->x1_planes));
    }
    return FDM_OK;
  }
  if (k == "lockstep") { P->lockstep = value != 0; P->tile_cache.clear(); P->tiles.clear(); return drop_programs(P, nullptr); }
  if (k == "untune") {      // forget the tuned tiles of every shape (tests)
    P->tile_cache.clear(); P->steps_seen.clear(); P->tiles.clear(); P->tune_failed_shapes.clear();
    return drop_programs(P, nullptr);
  }
  if (k.rfind("tile.", 0) == 0) {
    if (value < 0 || value > FDM_TILE_MAX) return fail(FDM_ERR_ARG, "plan_set: unknown tile %lld", value);
    P->tiles[k.substr(5)] = (int)value;
    P->tile_cache[shape_key(P)] = P->tiles;      // an explicit choice counts as tuned: sampling calls keep it
    return drop_programs(P, nullptr);
  }
  return fail(FDM_ERR_ARG, "plan_set: unknown key '%s'", key);
}

}  // extern "C"