/* libfdm_hip.so -- C ABI of the MI355X-native FDM diffusion-sampling hot path.
 *
 * Drop-in boundary.  The reference is pure Python and has no FFI; the "plugin
 * boundary" it offers is the Python class surface (FDM.forward, GaussianDiffusion.sample /
 * ddim_sample / p_sample, HubertModel.forward, VQAutoEncoder.quant / decode).  Every entry point
 * below names the reference interface (file:line under /root/reference) whose arithmetic it
 * replaces.  All functions take raw device pointers, sizes and a hipStream_t (passed as void*),
 * return 0 on success or a negative error code (message via fdm_last_error()) and never throw.
 * Nothing here takes or returns a torch type.
 *
 * Synchronisation contract, per layer:
 *   fdm_op_*, fdm_prog_run / _replay     enqueue on the given stream and return: they never synchronise
 *   fdm_prog_instantiate / _destroy      graph capture / release (host work; _destroy expects the stream drained)
 *   fdm_plan_commit, _reserve, _tune, _set("tile.*"), fdm_plan_set_weights after a commit, fdm_audio_prepare when it
 *     has to commit, grow the workspaces or tune               PLAN-TIME: allocate and drain the stream
 *   fdm_sample_graph, fdm_denoise_step   ONE stream drain per call (the timestep list / seed are host memory of the
 *     caller and are uploaded before the loop), plus graph instantiation the first time a program shape is used and a
 *     drain when the 8-entry program cache evicts; NOTHING synchronises inside the T-step loop
 *   fdm_hubert_forward, fdm_vq_*         drain the stream when they grow their workspaces (first call at a larger shape)
 *
 * Three layers:
 *   fdm_op_*    single-kernel operators (one launch on the given stream)
 *   fdm_prog_*  a recorded sequence of operators = one "step program", captured into a hipGraph and
 *               replayed T times with the diffusion timestep read from a device-side counter
 *   fdm_plan_* / fdm_audio_prepare / fdm_denoise_step / fdm_sample_graph
 *               the denoiser + scheduler of one model (weights by reference state-dict name, per-model and
 *               per-clip tables, workspaces, the step program and its hipGraph): what FDM.__init__ / FDM.forward
 *               and GaussianDiffusion.sample / ddim_sample do in the reference, behind plain pointers
 */
#ifndef FDM_HIP_H
#define FDM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define FDM_F32 0
#define FDM_BF16 1
/* Split operands (GEMM inputs only): x = hi + lo / S held as two planes of a 16-bit type, the lo plane `*_lo_off`
 * ELEMENTS after the hi plane, and the product evaluated as hi.hi + (hi.lo + lo.hi) / S in three passes of the 16-bit
 * MFMA with fp32 accumulation.  FDM_F16X3: fp16 planes, S = 2^11 (22 significant bits per operand: fp32-class results,
 * the mode that meets the 1e-4 contract on the 16-bit matrix cores; |x| is clamped to 65504); its QKV projection writes Q and
 * the packed K / V as plane pairs too and attention runs split (fdm_attn_args).  Every producer of a GEMM input writes the plane
 * pair.  (A bf16-plane split -- 16 bits per operand, ~5e-5 per denoiser call, outside the contract over chains -- was built and
 * measured in rounds 2-4 as kind 3 and is no longer part of the library: tools/sim_split_precision.py) */
#define FDM_F16X3 2
/* Single-plane fp16 operands (round 6): the `hi` plane of the split kind alone -- the bf16 kind's bytes and MFMA rate with 11
 * significand bits instead of 8 (|x| clamped to 65504 when an operand copy is written).  The denoiser's step program only
 * (fdm_op_gemm / fdm_op_attention / fdm_op_layernorm / fdm_op_cast / fdm_op_sched_step, fdm_plan_create); the audio encoders and the
 * VQ stages take FDM_F32 / FDM_BF16 / FDM_F16X3. */
#define FDM_F16 3

#define FDM_ACT_NONE 0
#define FDM_ACT_RELU 1       /* nn.TransformerDecoderLayer default activation, models/fdm_vocaset.py:45 */
#define FDM_ACT_MISH 2       /* nn.Mish, models/fdm_vocaset.py:22,31,38 */
#define FDM_ACT_GELU_ERF 3   /* transformers HuBERT 'gelu' */
#define FDM_ACT_GELU_TANH 4  /* models/utils/base_model_util.py:81-94 */
#define FDM_ACT_LEAKY02 5    /* nn.LeakyReLU(0.2), models/vq_vae_vocaset.py:206 */

#define FDM_OK 0
#define FDM_ERR_ARG (-1)
#define FDM_ERR_SHAPE (-2)
#define FDM_ERR_HIP (-3)
#define FDM_ERR_STATE (-4)

const char* fdm_last_error(void);
int fdm_version(void);
/* sizeof() of a public struct of this header ("fdm_gemm_args", "fdm_ln_args", ...) in the loaded build: lets a binding in
 * another language check its mirror of the struct before the first call (negative = unknown name) */
int fdm_abi_struct_size(const char* name);
/* 1 if a gfx950 device is visible to this process, else 0 (no device is touched otherwise) */
int fdm_device_ok(void);

/* ------------------------------------------------------------------------------------------
 * Scheduler (GaussianDiffusion.q_posterior + p_sample, ddim_sample update, CFG mix):
 * video_diffusion_pytorch/diffusion_BIWI_encoder_decoder.py:632-656, 693-708;
 * utiles/classifierfree.py:20-21.  All clips of the batch share the timestep (a3).
 * tables are fp32 [T_train] arrays; the current step k = *step (device int, incremented by the
 * kernel when advance != 0), t = tseq[k].  x0u != NULL enables the CFG mix
 * x0 = x0u + cfg_scale*(x0 - x0u) before the update.
 * DDPM: x' = c1[t]*x0 + c2[t]*x + sigma[t]*z, z = 0 when t == 0.  z comes from `noise`
 * (+ k*n elements) if non-NULL, else Philox4x32-10/Box-Muller keyed by (seed, clip0 + clip, k).
 * DDIM (eta = 0): eps = (sra[t]*x - x0)/srm1[t]; x' = x0*sqrt_an[k] + c_n[k]*eps.
 * Table-driven linear multistep (mode 3): x' = lm_a[k]*x + lm_b[k]*x0 + lm_c[k]*x0_hist + lm_s[k]*z, then x0_hist = x0 (under
 * the CFG mix: the mixed x0).  Evaluated in _rn operations without contraction, in this order: o = b*x0 + a*x; if c[k] != 0:
 * o += c*x0_hist[e]; if s[k] != 0: o += s*z, z exactly as for DDPM (`noise`, or Philox keyed (seed, clip0 + clip, element, k)).
 * The four tables are device fp32 arrays indexed by the STEP k (not by t); x0_hist is n fp32 elements, read only when
 * c[k] != 0 and rewritten every step.  fdm_sampler_tables_host builds the tables of DPM-Solver++ 2M and of DDIM with eta; a
 * caller may bring its own.                                                                     */
typedef struct fdm_sched_args {
  const float* x0; const float* x0u; float cfg_scale;
  const float* x; float* x_out;
  long long n; long long n_per_clip;
  const int* tseq; int* step; int advance;
  const float* c1; const float* c2; const float* sigma;      /* DDPM tables, indexed by t */
  const float* sra; const float* srm1;                       /* DDIM tables, indexed by t */
  const float* sqrt_an; const float* c_n;                    /* DDIM tables, indexed by step k */
  const float* noise; long long noise_stride;               /* elements between steps (0 -> n) */
  void* x_out_t; int out_dtype;                              /* optional operand-dtype copy of x_out (next step's GEMM input) */
  unsigned int* arrive;                                      /* device word (zeroed once): lets the LAST block to read *step
                                                                advance it inside this kernel (no separate launch) */
  unsigned long long seed; int clip0;
  int mode;                                                  /* 0 DDPM, 1 DDIM, 2 CFG mix only (x_out = mix), 3 table-driven linear multistep */
  long long x_out_t_lo_off;                                  /* split out_dtype: elements between the hi and lo planes of x_out_t */
  const unsigned long long* seed_dev;                        /* optional device words {seed, clip0}: override `seed` / `clip0`, so a
                                                                captured graph serves every seed / shard (no re-capture per call) */
  const float* lm_a; const float* lm_b; const float* lm_c; const float* lm_s;   /* mode 3: device tables indexed by step k */
  float* x0_hist;                                            /* mode 3: fp32 [n], the previous step's x0 prediction (read, then rewritten) */
} fdm_sched_args;
int fdm_op_sched_step(const fdm_sched_args* a, void* stream);
/* The scheduler pass of the slot program (fdm_slots_open): the clips of x are n_slots SLOTS of n_per_clip elements, each at its own step.
 * state: one 16-byte word {int k, t, live, run} per slot; keys: {seed, clip id} (two 64-bit words) per slot.  A slot with live == 0
 * is skipped whole: nothing of its x_out, x_out_t or x0_hist rows is stored.  A live slot gets the optional CFG mix, then the update
 * of mode 0 / 1 / 3 at ITS (k, t) with fdm_op_sched_step's expressions -- the bits of that call on the slot's slice with step k,
 * seed = the slot's seed and clip0 = the slot's clip id (Philox keyed (seed, clip id, element inside the clip, k)).  n must be
 * n_slots * n_per_clip; a->step / tseq / advance / arrive / seed / clip0 / seed_dev are not read; a->noise must be NULL. */
int fdm_op_slot_sched(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots, void* stream);
/* The scheduler pass of a slot plan with long capacity (fdm_slot_admit_long): fdm_op_slot_sched over the plain slots and the group update
 * over the long arena, in ONE launch.  a / state / keys / n_slots as for fdm_op_slot_sched (a->x / x_out / x_out_t / x0 / x0u are the slot
 * rows, [n_slots, L * d]; a->x0_hist the plain slots' history); g points at device tables:
 *   member   [n_slots] ints: the group a slot belongs to, -1 = a plain slot.  A member slot is skipped by the plain part.
 *   frames   [arena_frames] rows {int group, int e0, int e1, int 0}: the group of an arena frame (-1 = free: skipped) and its covering
 *            entries [e0, e1), in ascending window order
 *   entries  [n_entries] rows {int slot, int window start, float weight, int 0} (fdm_slot_group_table_host)
 *   groups   [n_groups] rows {int leader slot, int L_total, int first arena frame, int 0}
 *   x_long / hist_long   the arena, fp32 [arena_frames * d]: the long clips' latents and (mode 3) their blended-x0 histories
 * Arena frames [frame0, frame1) are visited.  A frame of a group whose LEADER's word is live gets: the CFG mix per covering window, the
 * blend x0 = sum_w weight_w x0_w in ascending window order (the first term starts the sum), ONE update with fdm_op_sched_step's
 * expressions at the leader's (k, t), noise Philox (leader's seed, leader's clip id, element index inside the long clip, k), history
 * (mode 3) = the blended x0 at hist_long + first * d + element; the result is stored to x_long and to every window row holding the
 * frame (a->x_out, plus a->x_out_t).  These are the bits of window_sched_kernel (fdm_sample_windows) on that clip alone, B = 1.  A group
 * whose leader is not live is skipped whole.  init != 0: no update and no look at the state -- x_long is copied into the window rows
 * (+ operand copy): how fdm_slot_admit_long loads x_T.  plain == 0: the plain slots are not visited.  Every table row is checked against
 * n_slots / n_groups / n_entries / L / L_total before it is used as an index (a bad row stores nothing).  d % 4 == 0. */
typedef struct fdm_slot_group_args {
  const int* member; const int* frames; const void* entries; const int* groups;
  float* x_long; float* hist_long;
  int arena_frames, n_entries, n_groups;
  int L, d;                        /* frames per slot, elements per frame (n_per_clip == L * d) */
  int frame0, frame1;
  int plain, init;
} fdm_slot_group_args;
int fdm_op_slot_group_sched(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots,
                            const fdm_slot_group_args* g, void* stream);
/* The two passes above with a SAMPLER BANK (fdm_slot_sampler_add): every slot names its own sampler and guidance scale.  b points at
 * device tables:
 *   req     [n_slots] 16-byte rows {int sampler, float cfg_scale, int 0, int 0}: the request a slot runs
 *   desc    [n_samplers] 16-byte rows {int mode (0 DDPM / 1 DDIM / 3 table-driven), int n_steps, int t_off, int c_off}; n_steps = 0: free
 *   t       [n_t] ints: the timesteps of sampler i are t[t_off .. t_off + n_steps) (read by the advance launch of the slot program)
 *   coef    [n_coef] fp32, indexed by the STEP k from c_off:  mode 1: sqrt_an[n_steps] | c_n[n_steps];  mode 3: a[n_steps] | b[n_steps] |
 *           c[n_steps] | s[n_steps];  mode 0: nothing -- its tables (a->c1 / c2 / sigma) are indexed by t and shared, as are a->sra / srm1
 * a->mode, a->cfg_scale, a->sqrt_an / c_n and a->lm_* are NOT read.  A live slot gets fdm_op_slot_sched's update with mode, step tables
 * and cfg_scale of ITS request: the bits of fdm_op_sched_step on the slot's slice with that mode, those tables, step k, seed, clip id
 * and scale.  A group (fdm_op_slot_group_sched_bank) reads its LEADER's request row.  Mode 3 uses the slot's x0_hist rows (a group's
 * hist_long range) as before; modes 0 and 1 never touch them.  Every field of a request row and of a descriptor is checked against
 * n_samplers / n_t / n_coef (and k against n_steps, t against [0, 1000), the mode's shared tables against NULL) before it becomes an
 * index: a slot with a bad row stores nothing.  req and desc must be 16-byte aligned. */
typedef struct fdm_slot_bank_args {
  const void* req; const int* desc; const int* t; const float* coef;
  int n_samplers, n_t, n_coef;
  int reserved;
} fdm_slot_bank_args;
int fdm_op_slot_sched_bank(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots,
                           const fdm_slot_bank_args* b, void* stream);
int fdm_op_slot_group_sched_bank(const fdm_sched_args* a, const int* state, const unsigned long long* keys, int n_slots,
                                 const fdm_slot_group_args* g, const fdm_slot_bank_args* b, void* stream);

/* ------------------------------------------------------------------------------------------
 * C[M,N] = epilogue(A[M,K] * W[N,K]^T): every nn.Linear / Conv1d-as-GEMM on the path
 * (models/fdm_vocaset.py:20-24,36-39,45-51; transformers HubertAttention/FeedForward;
 * models/lib/base_models.py:71-87,138-174; models/vq_vae_vocaset.py:204,243).
 * A rows may overlap (lda < K) which expresses a strided Conv1d over a channels-last signal
 * without im2col.  v = acc + bias[n]; v = act(v); v += resid[m or m % mod][n]; stores fp32
 * and/or operand-dtype copies.  For a fused QKV projection the K columns [kp_col0, vp_col0) and the
 * V columns [vp_col0, N) can be written straight into the attention kernel's fragment-packed
 * buffers (see fdm_attn_args) instead of out_t/out_f32.  K must be a multiple of 32 (fp32) /
 * 64 (16-bit kinds); A, W 16-byte aligned with lda, ldw multiples of 4 (fp32) / 8 (16-bit kinds), 0 <= lda, ldw < 2^31 (they reach
 * the kernel as 32-bit preloaded arguments; FDM_ERR_SHAPE otherwise).   */
typedef struct fdm_gemm_args {
  const void* A; long long lda; long long a_batch_stride;
  const void* W; long long ldw; long long w_batch_stride;
  int M, N, K, batch;
  int dtype;                      /* FDM_F32 | FDM_BF16: type of A, W, out_t, out_kp, out_vp;
                                     FDM_F16X3: A, W, out_t, out_kp, out_vp are fp16 plane pairs */
  const float* bias; long long bias_batch_stride;
  int act;
  const float* resid; long long ldr; int resid_row_mod;
  float* out_f32; long long ldo_f32;
  void* out_t; long long ldo_t;
  long long out_batch_stride;     /* elements, applied to out_f32, out_t and resid (column offset) */
  /* packed K / V outputs: rows are (clip b = m / kv_L, key l = m % kv_L), columns h*kv_hd + e inside each range */
  void* out_kp; int kp_col0;
  void* out_vp; int vp_col0;
  int kv_L; int kv_Lpad; int kv_hd;
  /* --- LayerNorm folded into the GEMMs around it (bf16 step program; removes the norm3 launch) ---
   * producer: stat_out != NULL -> per-row partial (sum v, sum v^2) of the fp32 outputs of each 64-column
   *   group are written to stat_out[(n/64) * 2M + 2m + {0,1}] (plain stores; summed per 16-column fragment, fragments in
   *   column order: deterministic AND independent of the output tile, so `tile` never changes results).
   * consumer: ln_stat_in != NULL -> mu_m, rstd_m = f(sum over ln_nparts partials, ln_dim, ln_eps).
   *   ln_colsum != NULL: A holds the RAW (un-normalised) rows and W = W o gamma, so
   *     LN(x) W^T + b  ==  rstd_m (acc - mu_m colsum_n) + bias_n   with bias_n := beta.W_n + b_n;
   *   rln_gamma != NULL: `resid` holds the raw rows and the residual added is LN(resid) computed on the fly. */
  float* stat_out;
  const float* ln_stat_in; int ln_nparts; int ln_dim; float ln_eps;
  const float* ln_colsum;
  const float* rln_gamma; const float* rln_beta;
  /* optional device int incremented once (by one thread) when the kernel starts: the first GEMM of a diffusion
   * step advances the device-side step counter this way (no extra launch, no atomics on a hot word) */
  int* incr_counter;
  const int* incr_table;          /* optional: incr_counter[1] = incr_table[new counter value] (t = tseq[step] for the step) */
  /* output tile per workgroup: 0 = library heuristic, else FDM_TILE_*.  Results do not depend on it (every tile
   * accumulates k in the same order): callers time the candidates once per shape at plan build and pass the winner. */
  int tile;
  /* sched_fuse != 0: the epilogue applies fdm_op_sched_step's DDPM / DDIM / table-driven update (sched.mode 0 / 1 / 3, no CFG mix) to the
   * tile it just computed, v = x0_hat: `resid` is read as the current latent x_t (NOT added), and x_{t-1} goes to
   * out_f32 (may alias resid) and, if given, out_t (the next step's operand copy).  The latent-decoder GEMM of a
   * non-CFG sampler uses this: one launch less per diffusion step, bit-identical to the separate kernel.  Needs
   * N % 64 == 0, ldo_f32 == ldr == N, 16-byte aligned pointers; sched.x0 / x0u / x / x_out / x_out_t / arrive unused. */
  int sched_fuse;
  fdm_sched_args sched;
  /* split operand kind (dtype FDM_F16X3): elements between the hi and lo planes of A, W and out_t */
  long long a_lo_off, w_lo_off, out_t_lo_off;
  long long kv_lo_off;            /* FDM_F16X3 with out_kp / out_vp: elements between the hi and lo planes of the packed buffers */
  /* --- split K (round 5): ksplit = S > 1 runs S workgroups per output tile (blockIdx.z = slice s); slice s accumulates the
   * k-tiles [s nk / S, (s + 1) nk / S) in the usual order and stores its fp32 partial tile to out_f32 + s * ksplit_stride
   * (elements); slice 0 carries bias and residual, the others neither.  The consumer sums the S planes in plane order
   * (fdm_ln_args.x_planes): no atomics, no extra launch, deterministic.  A workgroup's dependent k chain is 1/S as long and S
   * chains share a CU.  Results depend on S (the k order changes), never on `tile`.  Needs batch <= 1, act NONE, out_f32 as the
   * only output, dense vectorisable rows (N % 64 == 0), (K / 64 [16-bit kinds] or K / 32 [fp32]) % S == 0, S <= 4 (8 measured: no further gain); tiles: the
   * 64-column tiles FDM_TILE_64x64, FDM_TILE_64x64_S2 and FDM_TILE_32x64_S3. */
  int ksplit; long long ksplit_stride;
  /* --- second batch level (round 5): batch2 = C >= 1 runs C x batch problems in one launch, z = (c, g): A advances by
   * a_batch_stride per g and by a_batch_stride2 per c, outputs and resid by out_batch_stride (a column offset) per g and by
   * out_batch_stride2 (elements: a row offset) per c; W and bias depend on g alone.  This is a grouped Conv1d over C clips
   * (HuBERT's positional conv: g = channel group, c = clip).  When batch % 8 == 0 the workgroups are dealt so that XCD x serves
   * the groups [x batch / 8, (x + 1) batch / 8) only, group-major: each L2 streams its 1 / 8 of W once for all clips and row
   * tiles.  Tiles: FDM_TILE_64x64, FDM_TILE_64x64_S2 and FDM_TILE_128x64; no ksplit, no LayerNorm folds, no packed K / V, no fused scheduler. */
  int batch2; long long a_batch_stride2, out_batch_stride2;
} fdm_gemm_args;
#define FDM_TILE_AUTO 0
/* Eight tiles (round 5; eleven before).  Every tile accumulates k in the same order: the choice changes speed, never results. */
#define FDM_TILE_64x64 1       /* 8 waves, 4-stage ring (64 KB; split kinds 128 KB) */
#define FDM_TILE_128x64 2      /* 4-stage ring while the launch is one round (<= 256 workgroups), else 3-stage (72 KB: two workgroups per CU);
                                  split kinds: 3-stage (144 KB) */
#define FDM_TILE_128x128 3
#define FDM_TILE_64x64_S2 8    /* 64x64 with a 2-stage ring (four workgroups per CU; split kinds two) */
#define FDM_TILE_32x64_S3 9    /* 32x64 on 4 waves, 3-stage ring: twice the workgroups of 64x64 for few-hundred-row GEMMs */
#define FDM_TILE_256x128_PP 10 /* 256x128, two wave groups half a period apart (one computes while the other loads): large M; split kinds: 128x128 */
#define FDM_TILE_80x128 11     /* 80x128: ten row tiles for 800 rows -> 240 workgroups at N = 3072 (the QKV projection of four 200-frame clips) */
#define FDM_TILE_64x128 12     /* 64x128: 13 row tiles for 800 rows -> 208 workgroups at N = 2048 in one round (FFN1 in the split modes) */
/* retired ids (accepted, resolve to a live tile; no heuristic rule returns them and the tuner does not time them):
 *   4  96x128 (round 4: never picked on 66 shapes)                         -> 128x128
 *   5  256x128 on the lockstep loop (round 5: 29.9 us against 29.4 for the ping-pong loop on its one heuristic site) -> 256x128_PP
 *   6  64x64 on a 3-stage ring (round 5: 3 tuner picks on 66 shapes, no heuristic rule) -> 64x64
 *   7  128x64 on a 3-stage ring (round 5: the ring depth follows the grid, see 128x64)  -> 128x64 */
#define FDM_TILE_96x128 4
#define FDM_TILE_256x128 5
#define FDM_TILE_64x64_S3 6
#define FDM_TILE_128x64_S3 7
#define FDM_TILE_MAX 12
/* or-ed into `tile`: run the general (edge-handling) kernel even where a specialised one would do -- the two must agree bit for
 * bit (tests/test_ops_gpu.py); not a tuning knob.  Honoured by every tile including the ping-pong one; the scheduler-fused latent
 * decoder (sched_fuse) has lean kernels only and ignores it. */
#define FDM_TILE_GENERAL 0x100
/* or-ed into `tile`: the lockstep k loop (every wave issues its own tile loads) instead of the loader-wave form the 16-bit kinds run
 * by default (round 5) -- the two are bit-identical (tests/test_ops_gpu.py); A/B measurements and tests, not a tuning knob */
#define FDM_TILE_LOCKSTEP 0x200
#define FDM_TILE_ID_MASK 0xff
int fdm_op_gemm(const fdm_gemm_args* a, void* stream);
/* The FDM_TILE_* value a launch of *a with tile = 0 resolves to (the library heuristic on M, N, K, batch and the operand kind;
 * no device work, a->tile is ignored).  What each id runs -- geometry, ring depths, launch forms, retired ids -- is the one table of
 * csrc/gemm_tiles.hpp; the plan-time tuner leaves the heuristic's own kernel out of its candidates with that header's resolver. */
int fdm_gemm_heuristic_tile(const fdm_gemm_args* a);

/* ------------------------------------------------------------------------------------------
 * Fused softmax(Q K^T * scale + bias) V for one [B, H, L, hd] problem.
 * nn.MultiheadAttention self-attention with the causal periodic-ALiBi mask generated in-kernel
 * (models/fdm_vocaset.py:85,95-116: mask[h,i,j] = -slope_h*floor((i-j)/period), -inf for j>i);
 * non-causal for HuBERT (hd 64, scale 1/8) and the VQ decoder (hd 128, scale hidden^-0.5,
 * models/lib/base_models.py:144).  Q: row (b*L + l), column h*hd + e, row stride ldq.
 * O: [B*L, ldo] operand dtype.
 * Kp, Vp: "fragment-packed" keys / values, one block of Lpad*hd elements per (b, h) (Lpad a
 * multiple of 32, pad keys must hold finite values, e.g. zeros), laid out so that every MFMA
 * operand fragment of a key tile is ONE contiguous 1 KB run (64 lanes x 16 B):
 *   EPC = 16 / sizeof(T) elements per chunk, key tile KT = 4*EPC keys (bf16 32, fp32 16)
 *   Kp[ ((((kt*NSUB + s)*NKS + ks)*4 + g)*16 + r)*EPC + e%EPC ]   NSUB = KT/16, NKS = hd/(4*EPC)
 *       key l = kt*KT + w;  bf16: s = (w>>2)&1, r = 4*(w>>3) + (w&3);  fp32: s = 0, r = w
 *       column e: chunk e/EPC = 4*ks + g
 *   Vp[ (((kt*(hd/16) + e/16)*4 + g)*16 + e%16)*EPC + w%EPC ]        g = w / EPC
 * Written by fdm_op_gemm (out_kp / out_vp) or by fdm_op_pack_kv from row-major K, V.          */
typedef struct fdm_attn_args {
  const void* Q; long long ldq;     /* ldq, q_lo_off, kv_lo_off < 2^31: 32-bit preloaded kernel arguments (FDM_ERR_SHAPE otherwise) */
  const void* Kp;
  const void* Vp; int Lpad;
  void* O; long long ldo;
  int B, H, L, hd;
  int dtype;
  float scale;
  int causal;
  /* slopes ([H] device floats or NULL) and causal are independent.  With slopes the score of (query i, key j) gets
   * -slopes[h] * floor((i - j) / period), floor towards -inf, for EVERY visible key: with causal = 0 the keys j > i are visible and
   * take the same formula, i.e. a bias >= 0 that grows with j - i (the first key after i already gets +slopes[h]).  causal = 1 hides
   * j > i whether or not there are slopes.  Any period >= 1 is taken, also one longer than L.  Pad keys (l >= L) are never seen,
   * whatever finite values they hold.  (tests/test_attention_edges_gpu.py) */
  const float* slopes;
  int period;
  /* o_split = FDM_F16X3 (with dtype FDM_F32): O is written as a split plane pair (the next GEMM's input),
   * lo plane o_lo_off elements after the hi plane; 0 = O has the dtype of Q */
  int o_split; long long o_lo_off;
  /* dtype FDM_F16X3: Q, Kp, Vp and O are fp16 plane pairs (the 16-bit packed layout, per plane); both products run as three
   * 16-bit MFMA passes with the probabilities split in registers: fp32-class results.  q_lo_off / kv_lo_off / o_lo_off =
   * elements between the hi and lo planes of Q / Kp and Vp / O. */
  long long q_lo_off, kv_lo_off;
  /* per-clip lengths ([B] device ints, 1 <= lens[b] <= L) or NULL = every clip is L long.  Clip b sees keys [0, lens[b]) and its key
   * tiles are counted, dealt to the waves and masked from lens[b] exactly as a launch with L = lens[b] does it: rows [0, lens[b]) of
   * clip b are bit for bit what that launch returns for the clip alone.  Rows at or beyond lens[b] are written as zeros; K / V
   * entries of key tiles wholly beyond lens[b] are never read (they may hold anything), those of the straddling tile must be
   * finite as pad keys are.  Non-causal only (causal = 0), head_dim 64 / 128.  (tests/test_ragged_gpu.py) */
  const int* lens;
} fdm_attn_args;
int fdm_op_attention(const fdm_attn_args* a, void* stream);
/* row-major K, V (row b*L + l, column h*hd + e, row strides ldk / ldv) -> the packed layouts above */
int fdm_op_pack_kv(const void* K, long long ldk, const void* V, long long ldv, void* Kp, void* Vp,
                   int B, int H, int L, int Lpad, int hd, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * y = act(LayerNorm(x + add_mat + add_tab[idx]) * gamma + beta), one wavefront per row
 * (nn.LayerNorm eps 1e-5: decoder norm1-3 models/fdm_vocaset.py:45; HuBERT; VQ Norm
 * models/lib/base_models.py:37-52).  add_tab row index = tab_index[*tab_step] if tab_step else
 * tab_index[0] (device ints) -- this is how the folded cross-attention time term enters
 * (SURVEY.md a11x).  d in {256, 512, 768, 1024}.                                                  */
typedef struct fdm_ln_args {
  const float* x; int M, d;
  const float* add_mat;               /* [M, d] or NULL */
  const float* add_tab;               /* [rows, d] or NULL */
  const int* tab_index; const int* tab_step;
  const float* gamma; const float* beta; float eps;
  int act;
  float* y_f32; void* y_t; int dtype;
  /* optional fused second LayerNorm (post-norm decoder: norm1 then norm2 back to back,
   * models/fdm_vocaset.py:45): y = LN2(LN1(x) + add_mat + add_tab[idx]); the addends then belong to
   * stage 2 and stage 1 sees x alone. */
  const float* gamma2; const float* beta2;
  long long y_t_lo_off;               /* split dtype: elements between the hi and lo planes of y_t */
  /* add_mat shared by the S conditions of a clip (fdm_audio_prepare_conds): add_mat_group > 0 -> row m reads add_mat row
   * ((m % add_mat_wrap) / add_mat_group) * add_mat_L + m % add_mat_L, i.e. rows are [wrap block][clip][condition][frame]
   * (add_mat_group = S * L, add_mat_L = L, add_mat_wrap = rows per cond/uncond half, 0 = no wrap) over an add_mat of
   * [clips * L, d]; 0 = row m reads add_mat row m */
  int add_mat_L, add_mat_group, add_mat_wrap;
  /* x given as x_planes (2..4) partial planes, x_plane_stride elements apart (a split-K GEMM's outputs, fdm_gemm_args.ksplit):
   * the row is ((x[0] + x[1]) + x[2]) + ..., summed in plane order before anything else; 0 / 1 = one plane */
  int x_planes; long long x_plane_stride;
  /* per-clip table row (the slot program, fdm_slots_open): clip_step != NULL -> the add_tab row of row m is
   * add_tab[tab_index ? tab_index[k_c] : k_c] with k_c = clip_step[clip * clip_step_stride], clip = (m % clip_wrap) / clip_rows
   * (clip_wrap = rows per cond / uncond half, 0 = no wrap; both halves of a clip share its word); tab_step is then not read.
   * Light activations only (NONE / RELU).  NULL = the single step word above. */
  const int* clip_step; int clip_step_stride, clip_rows, clip_wrap;
} fdm_ln_args;
int fdm_op_layernorm(const fdm_ln_args* a, void* stream);


/* ------------------------------------------------------------------------------------------
 * Small elementwise / layout operators.                                                      */
/* dst_t[i] = (dtype) src_f32[i]; split dtypes: hi plane at dst, lo plane at dst + n elements.  dst needs its element type's
 * alignment only.  The rule per kind (the operand copies out_t / y_t / x_out_t of the other operators follow it too):
 *   FDM_F32    the 32 bits are copied.
 *   FDM_BF16   round to nearest even; fp32 subnormals become bf16 subnormals; inf stays inf and a finite value at or above
 *              2^128 - 2^119 rounds to inf; a NaN stores a NaN (payload unspecified).
 *   FDM_F16    clamp to [-65504, 65504] first (+-inf store +-65504, -0 stays -0), then round to nearest even with gradual underflow.
 *              No NaN and no inf is ever stored: a quiet NaN stores -65504, a signalling NaN +65504.
 *   FDM_F16X3  hi = fp16(c), c the clamped value as for FDM_F16; lo = fp16((c - hi) * 2048), the subtraction and the scaling exact in
 *              fp32: |x - (hi + lo / 2048)| <= 2^-22 |x| + 2^-36 for |x| <= 65504.  lo = +0 where c is an fp16 number. */
int fdm_op_cast(const float* src, void* dst, long long n, int dtype, void* stream);
/* out[r, :] = act(in[r, :] + vec[:]) -- e.g. tau table = Mish(W_t^T + b_t), models/fdm_vocaset.py:71-72 */
int fdm_op_bias_act(const float* in, const float* vec, float* out, long long rows, int d, int act, void* stream);
/* out[m, :] = a[(m / a_div) % a_mod, :] (+ b[(m / b_div) % b_mod, :]) (+ c[...]) -- conditioning addend
 * table: PE[l] + style[b] (+ emotion[b]), models/fdm_vocaset.py:75-84 */
int fdm_op_add_rows(const float* a, int a_div, int a_mod, const float* b, int b_div, int b_mod,
                    const float* c, int c_div, int c_mod, float* out, long long M, int d, void* stream);
/* out[b, :] = act(W[d, K] x[b, :] + bias) for conditioning one-hots (K <= 64): style_embedd /
 * emotion_embedd, models/fdm_vocaset.py:34,75; models/fdm_vqvae_mead.py:34-36,85 */
int fdm_op_small_linear(const float* x, const float* W, const float* bias, float* out, int B, int K, int d,
                        int act, void* stream);
/* Condition tracks: the conditioning addend from PER-FRAME vectors, one launch for B clips of L rows each.  style [B, L_track,
 * n_style] and emo [B, L_track, n_emo] (or NULL) hold one vector per latent frame; only the rows l < L_clip of a clip are read.
 *   out[b L + l] = pe[l] + act(sw style[b, l] + sb) (+ ew emo[b, l] + eb)          l <  L_clip
 *   out[b L + l] = 0                                                                L_clip <= l < L
 * uncond_off > 0 (elements, a whole number of rows at or past B L d): the uncond half of a CFG plan goes out at out + uncond_off in
 * the same launch, with the row's style term and the emotion bias only (the null condition is a zero vector, models/fdm_vqvae_mead.py:
 * 56-57).  Every element is, bit for bit, what fdm_op_small_linear on the row's vectors followed by fdm_op_add_rows gives.
 * n_style, n_emo <= 128.  FDM_ERR_ARG for a null pe / style / sw / out or emo without ew; FDM_ERR_SHAPE for the lengths. */
int fdm_op_cond_rows(const float* pe, const float* style, const float* emo, const float* sw, const float* sb, const float* ew,
                     const float* eb, float* out, long long uncond_off, int B, int L, int L_clip, int L_track, int d, int n_style,
                     int n_emo, int act, void* stream);
/* out[b, k, :] = in[b, clamp(k - pad, 0, L-1), :] for k in [0, L + 2*pad): replicate padding, channels-last */
int fdm_op_pad_rows(const void* in, void* out, int B, int L, int d, int pad, int dtype, int zero, void* stream);
/* the replicate form with per-clip lengths ([B] device ints, 1 <= lens[b] <= L): out[b, k, :] = in[b, clamp(k - pad, 0, lens[b]-1), :],
 * so a clip's end padding copies its own last frame and rows of `in` at or beyond lens[b] are never read */
int fdm_op_pad_rows_lens(const void* in, void* out, int B, int L, int d, int pad, int dtype, const int* lens, void* stream);
/* x[b, l, :] = 0 for l >= lens[b] (x [B, L, d] fp32, lens [B] device ints): the pad rows of a batch of clips of unequal length */
int fdm_op_zero_pad_rows(float* x, int B, int L, int d, const int* lens, void* stream);
/* dst[i] = src[i], src a HOST array of n ints: the values travel inside kernel arguments (64 per launch), in stream order, so src is
 * not read after the call returns and need not be pinned -- how the per-clip lengths of the *_ragged calls reach the device */
int fdm_op_set_ints(int* dst, const int* src, int n, void* stream);
/* out[b, i] = wav[b, i] for i < lens[b], 0 beyond (wav, out [B, n] fp32; lens [B] device ints): a padded batch of waveforms with
 * its padding cleared, whatever it held */
int fdm_op_mask_samples(const float* wav, float* out, int B, int n, const int* lens, void* stream);
/* fdm_op_group_pad with per-clip lengths ([B] device ints): frames at or beyond lens[b] are written as zeros */
int fdm_op_group_pad_lens(const void* in, void* out, int B, int T, int d, int groups, int pad, int dtype, const int* lens, void* stream);
/* HuBERT / wav2vec2 conv layer 0: wav [B, n] -> out [B, T0, 512], Conv1d(1, 512, k=10, s=5) (+ bias if non-NULL) */
int fdm_op_conv0(const float* wav, const float* w, const float* bias, float* out, int B, int n, int T0, void* stream);
/* the same layer with the LayerNorm(512, eps) + GELU(erf) that follows it in HuBERT-large (feat_extract_norm = 'layer') applied
 * before the store: out [B, T0, 512] in fp32 or bf16 (dtype), nothing else written */
int fdm_op_conv0_ln_gelu(const float* wav, const float* w, const float* bias, const float* gamma, const float* beta, void* out,
                         long long out_lo_off, int B, int n, int T0, float eps, int dtype, void* stream);     /* dtype FDM_F16X3: a plane pair, lo plane out_lo_off elements on */
/* per-(clip, channel) InstanceNorm1d over L after LeakyReLU(0.2): models/vq_vae_vocaset.py:204-209 */
int fdm_op_leaky_instnorm(const float* x, float* y_f32, void* y_t, int B, int L, int d, float eps, int dtype, void* stream);
/* the same with per-clip lengths ([B] device ints, 1 <= lens[b] <= L): clip b's statistics run over its first lens[b] frames in the
 * order of a call with L = lens[b]; frames at or beyond lens[b] are written as zeros */
int fdm_op_leaky_instnorm_lens(const float* x, float* y_f32, void* y_t, int B, int L, int d, float eps, int dtype, const int* lens, void* stream);
/* GroupNorm(num_groups = C, affine) over time + activation, channels-last x [B, T, C]: first conv layer of
 * wav2vec2-base (transformers Wav2Vec2GroupNormConvLayer; BIWI audio encoder, models/wav2vec.py:69-143) */
/* scratch (optional, 8-byte aligned, >= B * min(64, ceil(T / 1024)) * C * 16 bytes): with it, clips of T >= 4096 frames are
 * normalised over time chunks in two launches of hundreds of workgroups (fp64 chunk statistics folded in chunk order); without
 * it one launch of C / 64 workgroups per clip does the three passes (fine for short clips; the operator never allocates) */
int fdm_op_time_groupnorm(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_t, long long y_t_lo_off, int B, int T, int C,
                          float eps, int act, int dtype, void* scratch, long long scratch_bytes, void* stream);
/* the same with per-clip lengths ([B] device ints, 1 <= lens[b] <= T): clip b is normalised over its first lens[b] frames in the form
 * and order of a call with T = lens[b] and scratch (three passes below 4096 frames, fp64 chunks of ITS length from there on);
 * frames at or beyond lens[b] are written as zeros.  scratch is required when T >= 4096 (FDM_ERR_ARG otherwise). */
int fdm_op_time_groupnorm_lens(const float* x, const float* gamma, const float* beta, float* y_f32, void* y_t, long long y_t_lo_off, int B, int T, int C,
                               float eps, int act, int dtype, void* scratch, long long scratch_bytes, const int* lens, void* stream);
/* out[0] = mean(|a - b|^p), p = 2 (l1 = 0) or 1: the forward value of p_losses' F.mse_loss / F.l1_loss
 * (diffusion_BIWI_encoder_decoder.py:744-749); partial: >= 1024 floats of scratch; deterministic order */
int fdm_op_mean_diff(const float* a, const float* b, float* partial, float* out, long long n, int l1, void* stream);
/* Evaluation metrics over vertex sequences gt, pred [F, V, 3] fp32 (computer_metrix.py:84-136, metric/metric.py:115-138).
 * region: R int32 vertex indices (NULL with R == V: all vertices).  Per frame: frame_max[f] = max_r d2 (bit-identical to
 * numpy's float32 value), frame_sum[2f] = sum_r d2, frame_sum[2f+1] = sum_r sqrt(d2) with d2 = |gt - pred|^2;
 * out[0] = mean_f frame_max ("Lip/Face Vertex Error"), out[1] = mean d2 ("Emotion Mean Error"), out[2] = mean |d|
 * ("Mean Vertex Error"; compute_diversity's pairwise distance).  Deterministic (fixed reduction order).
 * NaN propagates as in numpy: a NaN coordinate of a region vertex makes that frame's frame_max and sums NaN and with them
 * all of out[0..2]; other frames' frame_max keep their bits; a NaN at a vertex outside the region is never read.          */
int fdm_op_vertex_err(const float* gt, const float* pred, const int* region, int R, int F, int V,
                      float* frame_max, double* frame_sum, double* out, void* stream);
/* out[0] = mean_r std_f(|verts[f, region[r]] - tmpl[region[r]]|^2): the per-sequence motion statistic whose gt - pred
 * difference is FDD (computer_metrix.py:95-107).  partial: >= 2 * min(F, 64) * R doubles of scratch.                     */
int fdm_op_motion_std(const float* verts, const float* tmpl, const int* region, int R, int F, int V,
                      double* partial, double* out, void* stream);
/* F.interpolate(mode='linear', align_corners=True) over time, x [B, Tin, C] -> y [B, Tout, C] fp32
 * (linear_interpolation, models/hubert.py:62-69: optional 50 -> 30 fps resampling of the conv features)                  */
int fdm_op_linear_interp(const float* x, float* y, int B, int Tin, int Tout, int C, void* stream);
/* AdaIN (utiles/adaIN.py:4-22): content, style [N, C, Lc], [N, C, Ls] -> out [N, C, Lc] */
int fdm_op_adain(const float* content, const float* style, float* out, int NC, int Lc, int Ls, float eps, void* stream);
/* regroup [B, T, d] -> [groups, B, T + 2*pad, d/groups] zero padded (HuBERT positional conv input) */
int fdm_op_group_pad(const void* in, void* out, int B, int T, int d, int groups, int pad, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * VectorQuantizer.forward (models/lib/quantizer.py:35-64, models/vq_vae_emotion.py:221-252):
 * d_k = (sum z^2 + sum e_k^2) - 2 z.e_k, first-min argmin, z_q = z + (e - z), output
 * permuted to [B, c, R] (R = L*G rows per clip).  book[b] selects the 256-code slice.        */
int fdm_op_vq_quant(const float* z, const float* codebook, const int* book, int B, int R, int c, int K,
                    float* zq_bcl, long long* idx, void* stream);
/* The rest of VectorQuantizer.forward's return tuple (models/lib/quantizer.py:46-61; EVQ models/vq_vae_emotion.py:232-249) for the
 * indices idx [B*R] fdm_op_vq_quant chose: min_encodings [B*R, K] one-hot fp32 (optional), out[0] = loss =
 * beta * mean((e - z)^2) + mean((e - z)^2), out[1] = perplexity = exp(-sum_k p_k log(p_k + 1e-10)), p = column means of
 * min_encodings.  partial: >= 1024 doubles, hist: K ints of scratch.  Deterministic (fixed reduction order, integer histogram). */
int fdm_op_vq_stats(const float* z, const float* codebook, const int* book, const long long* idx, int B, int R, int c, int K, float beta,
                    float* min_encodings, double* partial, int* hist, float* out, void* stream);
/* The per-row forms (condition tracks): book_rows [B * R] holds one codebook slice per latent vector; an entry outside [0, n_books)
 * reads slice 0.  fdm_op_argmax_rows writes book[r * rep + g] = argmax(x[r, 0 .. n)) for g < rep: the first maximum as torch.argmax, but a
 * NaN never wins a comparison (torch.argmax returns a NaN's index; a row that starts with NaN gives 0), as the per-clip quantiser's
 * argmax; it refuses, on the host, n > n_books: an argmax over more columns than the codebook has slices could name a slice that does not exist. */
int fdm_op_argmax_rows(const float* x, int* book, long long rows, int n, int rep, int n_books, void* stream);
int fdm_op_vq_quant_rows(const float* z, const float* codebook, const int* book_rows, int n_books, int B, int R, int c, int K,
                         float* zq_bcl, long long* idx, void* stream);
int fdm_op_vq_stats_rows(const float* z, const float* codebook, const int* book_rows, int n_books, const long long* idx, int B, int R, int c,
                         int K, float beta, float* min_encodings, double* partial, int* hist, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Step programs: record fdm_op_* calls, run them eagerly or as a hipGraph replayed n times.  */
typedef struct fdm_prog fdm_prog;
int fdm_prog_create(fdm_prog** out);
int fdm_prog_destroy(fdm_prog* p);
int fdm_prog_begin(fdm_prog* p);            /* subsequent fdm_op_* calls on this thread are recorded, not launched */
int fdm_prog_end(fdm_prog* p);
int fdm_prog_run(fdm_prog* p, void* stream);                 /* eager: launch every recorded op */
int fdm_prog_instantiate(fdm_prog* p, void* stream);         /* capture into a hipGraph */
int fdm_prog_replay(fdm_prog* p, int n, void* stream);       /* launch the graph n times */
int fdm_prog_num_ops(fdm_prog* p);

/* ------------------------------------------------------------------------------------------
 * Plan layer.  A plan owns device copies of the model's weights, the tables derived from them,
 * its workspaces and the recorded step program; the caller owns every tensor it passes in.  Device memory is allocated only
 * by fdm_plan_create / _reserve / _commit (and by fdm_audio_prepare when it has to grow the workspaces or commit first);
 * fdm_sample_graph / fdm_denoise_step drain the stream once per call while uploading the timestep list (host memory of the
 * caller) and instantiate a graph the first time a program shape is used; nothing synchronises inside the T-step loop.
 * A plan is not thread-safe; one plan per device/stream.
 *
 * Model geometry = the reference constructors' numbers (models/fdm_vocaset.py:9-51, models/fdm_vqvae_mead.py:9-53,
 * models/fdm.py:10-48, models/utils/config.py): fdm_model_preset fills it for "vocaset", "mead", "biwi" (+ "_tiny" test twins). */
typedef struct fdm_model_desc {
  int d, n_head, n_layers, ffn;   /* feature_dim, heads, decoder layers, dim_feedforward (= 2 d) */
  int G, c;                       /* latent vectors per frame, their width (G * c == d) */
  int n_style, n_emo;             /* one-hot widths of style_embedd / emotion_embedd (0 = no emotion input) */
  int audio_in, pair;             /* input width of audio_extract.0; audio-encoder frames folded per latent frame */
  int pe_periodic, period;        /* PeriodicPositionalEncoding (period) or plain sinusoidal PE; ALiBi period */
  int latent_mish, style_mish;    /* Mish after latent_encoder / style_embedd */
  int max_len;                    /* init_biased_mask(max_seq_len = 600), models/fdm_vocaset.py:44 */
} fdm_model_desc;
int fdm_model_preset(const char* name, fdm_model_desc* out);

typedef struct fdm_plan fdm_plan;
/* Workspaces for up to B clips x L latent frames (x2 rows when cfg != 0: cond + uncond rows in one set of launches).
 * dtype: FDM_F32 | FDM_BF16 | FDM_F16X3 = the arithmetic mode of the step program. */
int fdm_plan_create(const fdm_model_desc* desc, int B, int L, int cfg, int dtype, fdm_plan** out);
int fdm_plan_reserve(fdm_plan* p, int B, int L, int cfg);           /* grow the workspaces (allocates; drops recorded programs) */
int fdm_plan_destroy(fdm_plan* p);
/* One fp32 tensor of the reference state dict (FDM.state_dict() names, e.g. "transformer_decoder.layers.0.linear1.weight",
 * "latent_decoder.bias", optional buffer "PE.pe"), n elements at ptr (host or device memory); copied into the plan.
 * Optional schedule overrides "sched.c1", "sched.c2", "sched.sigma", "sched.sra", "sched.srm1" ([1000] fp32 each: the
 * caller's own q_posterior / predict_noise tables; default = fdm_schedule_host's). */
int fdm_plan_set_weights(fdm_plan* p, const char* name, const float* ptr, long long n, void* stream);
/* Per-model tables: operand-kind weight copies, tau[t] = Mish(W_t[:, t] + b_t), folded cross-attention time tables
 * TT_l = Wo_l Wv_l tau, LayerNorm folds of the bf16 program.  Called implicitly by fdm_audio_prepare. */
int fdm_plan_commit(fdm_plan* p, void* stream);
/* Once per batch of clips (the hoisted, step-invariant part of FDM.forward, models/fdm_vocaset.py:59-84):
 * hub [B, N, fw] audio-encoder features (fw * pair == audio_in), style [B, n_style], emo [B, n_emo] or NULL, device fp32.
 * L <= N / pair latent frames.  Builds AF = audio_extract(hub), the per-layer tables C1_l = Wo_l (Wv_l AF + bv_l) + bo_l
 * and E0 = PE + style (+ emotion; the uncond rows of a CFG plan use emotion_embedd's bias only).                        */
int fdm_audio_prepare(fdm_plan* p, const float* hub, int B, int N, int fw, const float* style, const float* emo,
                      int L, int cfg, void* stream);
/* The same for S conditions per clip: the reference's sampler loops the style one-hots of a clip through ddim_sample one
 * B = 1 call at a time with the SAME audio (samples/sample_diffusion_vocaset.py:71-83; for 3D-MEAD any set of
 * (emotion, identity) pairs of one utterance).  Here the S conditions of each of the B clips run as B*S rows blocks of ONE step
 * program: row block (b, s) = "virtual clip" b*S + s.  style [B*S, n_style], emo [B*S, n_emo] or NULL (virtual-clip order);
 * AF and the C1_l tables are computed once per CLIP (B*L rows) and shared by its S conditions -- only E0 is per condition.
 * Afterwards the plan's batch is B*S clips: x_T / out / noise of fdm_sample_graph and fdm_denoise_step are
 * [B*S, L*G, c], Philox noise is keyed by clip0 + b*S + s, and every row block is bit-identical to the B = 1, S = 1 call
 * with that clip's audio and that condition.  S = 1 is fdm_audio_prepare. */
int fdm_audio_prepare_conds(fdm_plan* p, const float* hub, int B, int N, int fw, int S, const float* style, const float* emo,
                            int L, int cfg, void* stream);
/* One FDM.forward (models/fdm_vocaset.py:54-91): x_t [B, L*G, c] -> x0_hat [B, L*G, c], CFG-mixed
 * (x0u + cfg_scale (x0 - x0u), utiles/classifierfree.py:20-21) when prepared with cfg.  x0_uncond (optional) receives
 * the unconditional rows.  Eager launches of the recorded step program. */
int fdm_denoise_step(fdm_plan* p, const float* x_t, int t, float cfg_scale, float* x0_hat, float* x0_uncond, void* stream);
/* GaussianDiffusion.p_sample_loop / ddim_sample (diffusion_BIWI_encoder_decoder.py:649-710, diffusion_mead_encoder_decoder.py:
 * 649-667): the step program (denoiser + fused scheduler update) replayed n_steps times as a hipGraph, the timestep read
 * from a device-side counter; graph_steps (default 10) diffusion steps are captured per graph launch. */
typedef struct fdm_sample_args {
  int kind;                       /* 0 = DDPM over t_list, 1 = DDIM (eta = 0) with `ddim_steps` (the dead last pair is skipped),
                                     2 = table-driven linear multistep sampler over t_list with `lm_tables` (below) */
  const float* x_T; float* out;   /* [B, L*G, c] device fp32 (may alias) */
  const int* t_list; int n_steps; /* DDPM: host array of timesteps, descending */
  int ddim_steps;
  const float* noise;             /* DDPM: [n_steps, B, L*G, c] device fp32 injected z, or NULL: Philox(seed, clip0 + b, step) */
  unsigned long long seed; int clip0;
  float cfg_scale;
  int eager;                      /* != 0: launch the recorded ops directly instead of replaying the graph (bit-identical) */
  float* record;                  /* optional [n_steps, B, L*G, c]: the latent after every step */
  int graph_steps;                /* diffusion steps per graph launch; 0 = default */
  /* kind 2: HOST memory [4][n_steps] fp32 in the order a, b, c, s -- step k computes x' = a[k] x + b[k] x0 + c[k] x0_prev + s[k] z
   * (fdm_sched_args mode 3) with the denoiser run at t_list[k] (t_list need not be contiguous).  The plan uploads the tables
   * per call and owns the fp32 history buffer x0_prev (zeroed at the start of every call; LONG layout on a windowed plan).
   * noise, seed, clip0, cfg_scale, eager, record and graph_steps behave as for DDPM; the step program has DDPM's launch count
   * and its own cache key (the DDPM / DDIM programs of the plan are untouched).  fdm_sampler_tables_host builds t_list and
   * the tables of DPM-Solver++ 2M and of DDIM with eta.  FDM_ERR_ARG: lm_tables NULL, t_list NULL, n_steps < 1. */
  const float* lm_tables;
} fdm_sample_args;
int fdm_sample_graph(fdm_plan* p, const fdm_sample_args* a, void* stream);
/* Clips longer than max_len (windowed sampling).  A long clip of L_total latent frames (no cap) is sampled as n windows of exactly
 * W' = min(W, L_total) frames (1 <= W <= max_len), neighbours overlapping by >= O frames (0 <= O < W):
 *   layout   L_total <= W: one window of L_total frames; otherwise n = ceil((L_total - O) / (W - O)), s_w = floor(w (L_total - W) / (n - 1)).
 *            Every frame is covered; with 2 * stride < W three or more windows cover a frame (the blend takes any number).
 *   inputs   window w is an ordinary clip of the plan: audio rows [s_w pair, (s_w + W') pair) of the long encoder output, the long
 *            clip's style / emotion, window-local positions 0 .. W'-1 (ALiBi is relative: nothing else changes).
 *   blend    every diffusion step, in x0 space: omega_w(f) = min(1, (f - s_w + 0.5) / O, (s_w + W' - f - 0.5) / O) (no taper at the long
 *            clip's first and last frames; O = 0 -> 1), w_hat = omega / sum(omega), x0(f) = sum_w w_hat_w(f) x0_w(f - s_w) in ascending
 *            window order (fp32, _rn operations; CFG: each window's cond / uncond mix first).  The scheduler update (DDPM posterior sample
 *            / DDIM eta = 0) then runs ONCE per long-clip element and its result is written back to every window holding the frame, so
 *            overlapping rows are bitwise equal across windows at every step.  (The denoiser is causal: a window's FIRST frames lack
 *            context, hence the taper; the taper at the right edge keeps the weights continuous through the overlap.)
 *   noise    keyed by the long clip: Philox (seed, clip0 + long clip, element index inside the long clip, step); injected noise is
 *            [n_steps, B, L_total*G, c].  A one-window plan is bit-identical to fdm_sample_graph on the same clip.
 *   layout of x_T / out / noise / record: LONG, [B, L_total*G, c]; after the last step the long buffer is the stitched latent (the
 *            VQ quantiser / decoder then run on the whole L_total: the decoder is not causal).
 * fdm_window_layout_host: returns n and writes the starts when cap >= n (starts may be NULL: returns the needed cap);
 * fdm_window_weights_host: returns n and writes w_hat [n, W'] (w may be NULL).  FDM_ERR_ARG: W < 1, O < 0 or O >= W; FDM_ERR_SHAPE: L_total < 1. */
int fdm_window_layout_host(int L_total, int window, int overlap, int* starts, int cap);
int fdm_window_weights_host(int L_total, int window, int overlap, float* w);
/* hub [B, N, fw] features of B long clips (the audio encoder runs once over each whole waveform), style [B, n_style], emo [B, n_emo]
 * or NULL, device fp32; L_total <= N / pair.  The plan's batch becomes B * n windows of W' frames in (long clip, window) order (the
 * window audio rows are gathered on the device; workspaces are reserved as fdm_audio_prepare does).  FDM_ERR_SHAPE: window > max_len,
 * L_total > N / pair; FDM_ERR_ARG: overlap >= window.  fdm_plan_get: "windows" (n; 0 = plain plan), "window_len" (W'), "L_total".
 * Any fdm_audio_prepare* call returns the plan to plain mode; fdm_sample_graph on a windowed plan fails with FDM_ERR_STATE;
 * fdm_denoise_step stays per window (plan layout [B * n, W'*G, c], no blend). */
int fdm_audio_prepare_windows(fdm_plan* p, const float* hub, int B, int N, int fw, const float* style, const float* emo,
                              int L_total, int window, int overlap, int cfg, void* stream);
/* The sampler of a windowed plan: fdm_sample_args as for fdm_sample_graph (DDPM / DDIM / table-driven kind 2, eager, graph_steps, cfg_scale, seed, clip0),
 * with x_T / out / noise / record in LONG layout.  Step program: the denoiser chain with its scheduler update unfused, then the blend
 * + update pass (one launch more per step than a plain plan without guidance). */
int fdm_sample_windows(fdm_plan* p, const fdm_sample_args* a, void* stream);
/* Inspection: the window rows of a windowed plan as they stand, out [B * n_windows, W * d] fp32 (plan clip b * n + w = window w of long
 * clip b).  After fdm_sample_windows every frame that two windows cover holds the same bits in both, the long buffer's. */
int fdm_window_peek(fdm_plan* p, float* out, void* stream);
/* Slots (in-flight batching).  A plan in slot mode holds B SLOTS of up to L latent frames; every slot is a clip at ITS OWN step of one
 * shared sampler, so a clip joins a running batch at any step boundary and leaves when its own chain ends -- and its latent is, bit
 * for bit, what fdm_sample_graph returns for it on a (1, L_clip) plan with the same weights, x_T, seed and clip0 = clip_id.
 *   state    per slot on the device {k, t, live, run} and {seed, clip id}; zeroed = idle.  The host keeps a mirror of every slot's
 *            status and step count: no call below reads device memory.
 *   step     ONE recorded program for any mix of idle, running and finished slots, replayed as a hipGraph: a one-workgroup launch
 *            advances every slot's word (running with k + 1 < n_steps: k += 1, t = tseq[k], live; otherwise live = 0, t kept in
 *            range), the denoiser chain follows with every LayerNorm launch gathering TT_l by the row's clip (fdm_ln_args.clip_step) and
 *            its scheduler update unfused, then fdm_op_slot_sched updates the live slots only.  Two launches more per step than the
 *            plain program without guidance (fdm_plan_get "launches_per_step").
 *   exact    every kernel of the chain is row- or clip-independent, self-attention is causal (a clip padded at its end computes its
 *            own frames' bits), every GEMM tile accumulates k in one order, the unfused scheduler kernel gives the bits of the fused
 *            epilogue, and noise is keyed by (seed, clip id, element inside the clip, step of the clip).
 * fdm_slots_open: commits, reserves (B, L, cfg), sets the plan's shape, zeroes the clip tables, x and the state (every slot idle,
 *   holding zeros) and takes the shared sampler from `sampler`: kind, t_list / n_steps, ddim_steps, lm_tables, cfg_scale,
 *   graph_steps, eager (x_T, out, seed, clip0 are ignored; noise or record given: FDM_ERR_ARG).  Drains the stream once.  While in
 *   slot mode fdm_sample_graph, fdm_sample_windows and fdm_denoise_step fail with FDM_ERR_STATE; any fdm_audio_prepare* call returns
 *   the plan to plain mode.  fdm_plan_get "slots" = B (0 = not in slot mode).
 * fdm_slot_admit: hub [N, fw] features of ONE clip, style [n_style], emo [n_emo] or NULL, x_T [L_clip*G, c], device fp32.  Builds the
 *   slot's rows of AF, C1_l (both CFG halves) and E0 with the per-clip GEMMs of fdm_audio_prepare_conds, zero-pads rows L_clip..L,
 *   loads x_T (+ operand copy), zeroes the slot's history rows and sets {k = -1, running}, seed and clip id.  (The padding rows start
 *   at zero and are then updated with the slot like any row: finite, never read out, and -- the denoiser being causal -- without effect
 *   on the clip's own frames.)  Stream-ordered, between
 *   steps, while other slots are mid-chain.  FDM_ERR_STATE: the slot is running or finished and not read; FDM_ERR_SHAPE: L_clip outside
 *   [1, min(L, N / pair)]; FDM_ERR_ARG: slot outside [0, B).
 * fdm_slots_run: n_steps diffusion steps for every running slot; a slot whose chain ends part-way freezes there (finished).
 * fdm_slot_state: host only; status 0 idle, 1 running, 2 finished.  Any output may be NULL.
 * fdm_slot_read: copies the slot's L_clip rows to out [L_clip*G, c] (device fp32, stream-ordered) and marks the slot idle;
 *   FDM_ERR_STATE unless the slot is finished. */
#define FDM_SLOT_IDLE 0
#define FDM_SLOT_RUNNING 1
#define FDM_SLOT_FINISHED 2
int fdm_slots_open(fdm_plan* p, int B, int L, int cfg, const fdm_sample_args* sampler, void* stream);
int fdm_slot_admit(fdm_plan* p, int slot, const float* hub, int N, int fw, const float* style, const float* emo, int L_clip,
                   const float* x_T, unsigned long long seed, int clip_id, void* stream);
int fdm_slots_run(fdm_plan* p, int n_steps, void* stream);
int fdm_slot_state(fdm_plan* p, int slot, int* steps_done, int* steps_total, int* status);
int fdm_slot_read(fdm_plan* p, int slot, float* out, void* stream);
/* inspection: all L rows of a slot's latent, [L*G, c], whatever its status (an idle slot never admitted holds zeros); changes nothing */
int fdm_slot_peek(fdm_plan* p, int slot, float* out, void* stream);
/* Long requests in slot mode: a recording of L_total > L latent frames (L = the slot capacity) rides the slot program as a GROUP.
 *   rule     the request is n = fdm_window_layout_host(L_total, L, O) windows of exactly L frames, admitted into n idle slots at once:
 *            any slots, in any order, window w into slots[w]; slots[0] is the group's LEADER.  Every member carries the same state word
 *            and advances with the advance launch like any slot.  The denoiser chain treats a member as an ordinary slot holding its
 *            window's audio rows [s_w pair, (s_w + L) pair), the clip's style / emotion and window-local positions.  The scheduler pass
 *            (fdm_op_slot_group_sched) treats the group as fdm_sample_windows treats a windowed plan: CFG mix per window; the covering
 *            windows' x0 blended in ascending window order with fdm_window_weights_host's weights, the first term starting the sum; one
 *            update per long-clip element with fdm_op_sched_step's expressions at the leader's (k, t); noise Philox (seed, clip_id,
 *            element index inside the long clip, k); the table-driven sampler's history is the blended x0 in long layout; the result
 *            goes to the long buffer and to every window row holding the frame (fp32 + operand copy).  A group that is not live is
 *            skipped whole.
 *   exact    the group's latent is bit for bit what fdm_sample_windows returns for the clip alone on a B = 1 windowed plan (same weights,
 *            window = L, the same overlap, x_T, seed, clip0 = clip_id), in every arithmetic mode, for DDPM / DDIM / the table-driven
 *            sampler, with and without guidance, whatever the other slots hold and whenever the group was admitted.  Plain slots beside
 *            it keep their guarantee; overlapping rows of member slots are bitwise equal at every step.
 *   capacity fdm_plan_set(p, "slot_long_frames", F) and (p, "slot_long_groups", G) BEFORE fdm_slots_open (both default 0 = no long
 *            capacity: the recorded program and its launch count are exactly those of a plan without this feature).  fdm_slots_open then
 *            reserves an arena of F long frames (latent, history, per-frame table), B * L entries and G group descriptors; nothing is
 *            allocated per admit.  fdm_plan_get reads both keys back (a build without the feature does not know them).  With capacity the
 *            step has the same launch count: the group update rides the slot scheduler pass.
 * fdm_slot_admit_long: hub [N, fw] features of the WHOLE recording, style / emo as fdm_slot_admit, x_T [L_total*G, c] device fp32.  n must
 *   equal the layout's window count, every listed slot must be idle and distinct, L_total > L (a shorter clip is one window: use
 *   fdm_slot_admit) and L_total <= N / pair; a contiguous arena range, an entry range and a descriptor are taken by first fit.  Builds
 *   each member's rows with fdm_slot_admit's per-clip GEMMs, copies x_T into the arena and scatters it into the window rows (+ operand
 *   copies), zeroes the group's history, uploads the group's tables and sets every member's word to {k = -1, running} with the group's
 *   key.  The tables are host memory of this call: the call DRAINS THE STREAM ONCE after uploading them, as fdm_audio_prepare_windows
 *   does (no pinned staging buffer).  FDM_ERR_STATE: a listed slot is busy, or no arena range / entry range / descriptor is free -- the
 *   caller's cue to wait; FDM_ERR_SHAPE: L_total <= L, L_total > N / pair, n != the window count, n > B, bad feature width;
 *   FDM_ERR_ARG: null pointer, slot outside [0, B), a slot listed twice, overlap outside [0, L), no long capacity reserved.  Every
 *   check is made before the first launch: a failed call leaves the plan untouched.
 * fdm_slot_state reports the group's progress for every member.  fdm_slot_group (host only): leader = -1, n = 0, L_total = 0 for a plain
 *   or idle slot, else the group's leader, member count and L_total (any output may be NULL).  fdm_slot_read_long: copies the long buffer
 *   to out [L_total*G, c], frees the arena range, the entries and the descriptor and marks every member idle; FDM_ERR_STATE unless `leader`
 *   leads a finished group.  fdm_slot_read on a member fails with FDM_ERR_STATE; fdm_slot_peek stays per slot (a member's window rows). */
int fdm_slot_admit_long(fdm_plan* p, const int* slots, int n, const float* hub, int N, int fw, const float* style, const float* emo,
                        int L_total, int overlap, const float* x_T, unsigned long long seed, int clip_id, void* stream);
int fdm_slot_group(fdm_plan* p, int slot, int* leader, int* n, int* L_total);
int fdm_slot_read_long(fdm_plan* p, int leader, float* out, void* stream);
/* The tables of one group (host, no device): for a long clip of L_total > L frames as n = fdm_window_layout_host(L_total, L, overlap)
 * windows held by slots[0 .. n), off [L_total + 1] receives the per-frame offsets into the entries (off[0] = 0, monotone) and
 * ent_slot / ent_start / ent_wt [n * L] the entries: for frame f the covering windows in ascending window order, each with its slot
 * (slots[w]), its start s_w and its normalised weight -- bit for bit fdm_window_weights_host's.  Returns the number of entries (n * L);
 * nothing is written unless cap >= it (outputs may be NULL to ask for the count).  FDM_ERR_ARG: bad overlap, slots NULL;
 * FDM_ERR_SHAPE: L_total <= L, n != the window count.  fdm_slot_admit_long builds its tables with this function. */
int fdm_slot_group_table_host(int L_total, int L, int overlap, const int* slots, int n, int* off, int* ent_slot, int* ent_start,
                              float* ent_wt, int cap);
/* Samplers per request in slot mode: a plan in slot mode owns a BANK of sampler definitions, and every admitted request names one
 * (and, on a guidance plan, its own cfg_scale) -- a 10-step preview, a 100-step DDIM final and a DDPM chain share one step program.
 *   rule     sampler 0 is the one given to fdm_slots_open; further samplers are added (and dropped) between steps with the calls below.
 *            The guarantee of "Slots" and "Long requests" holds PER REQUEST: a slot's latent is bit for bit fdm_sample_graph on a
 *            (1, L_clip) plan with that request's sampler and scale (same x_T, seed, clip0 = clip_id), a group's latent bit for bit
 *            fdm_sample_windows with them -- in every arithmetic mode, whatever the other slots run.  Why: the denoiser chain reads only
 *            the slot's t word; the sampler is read by the advance launch (n_steps, timestep list) and by the scheduler pass (mode,
 *            step tables, scale), and both take them from the slot's own request row (fdm_slot_bank_args).
 *   capacity fdm_plan_set(p, "slot_samplers", S) = bank rows beyond sampler 0, (p, "slot_sampler_steps", N) = total steps those rows
 *            may hold, both BEFORE fdm_slots_open and both default 0 = no bank: the recorded program, its kernels, its launch count and
 *            its cache key are exactly those of a plan without this feature.  With both > 0 fdm_slots_open reserves the request rows,
 *            1 + S descriptors, n_steps(sampler 0) + N timesteps and four coefficients per step, and the step program records the bank
 *            forms of the advance launch and of the scheduler pass: the same launch count, its own cache key.  fdm_plan_get reads both
 *            keys back (a build without the feature does not know them).
 * fdm_slot_sampler_add: reads only kind, t_list / n_steps, ddim_steps and lm_tables of `sampler` (noise or record given: FDM_ERR_ARG);
 *   builds the tables as a sampling call does (kind 1: fdm_ddim_schedule_host, the dead last pair skipped), takes a descriptor, a
 *   timestep range and a coefficient range by first fit, uploads them and DRAINS THE STREAM ONCE (the tables are host memory of the
 *   call).  Legal between any two fdm_slots_run calls while slots are mid-chain.  Returns the sampler's id >= 1, or FDM_ERR_STATE when
 *   nothing fits (no bank, no free descriptor or range: the plan is untouched), FDM_ERR_ARG for a bad definition.
 * fdm_slot_sampler_drop: frees the descriptor and its ranges.  FDM_ERR_STATE while a running or finished-and-unread slot names the
 *   sampler; FDM_ERR_ARG for id 0 or an unknown id.
 * fdm_slot_sampler_info (host only): kind (0 / 1 / 2 as fdm_sample_args.kind) and steps of a chain; outputs untouched on error.
 * fdm_slot_admit_as / fdm_slot_admit_long_as: fdm_slot_admit / fdm_slot_admit_long plus the request's sampler and cfg_scale (ignored on a
 *   plan opened without guidance).  The slot's t word starts at the first timestep of ITS sampler.  An unknown sampler: FDM_ERR_ARG,
 *   nothing changed; without a bank only sampler 0 with the open's scale is accepted.  fdm_slot_admit / fdm_slot_admit_long are
 *   unchanged: on any plan they mean sampler 0 with the open's cfg_scale.  fdm_slots_run advances every slot to min(its own total,
 *   done + n) and fdm_slot_state reports the slot's own steps_total (an idle slot: sampler 0's). */
int fdm_slot_sampler_add(fdm_plan* p, const fdm_sample_args* sampler, void* stream);
int fdm_slot_sampler_drop(fdm_plan* p, int id);
int fdm_slot_sampler_info(fdm_plan* p, int id, int* kind, int* n_steps);
int fdm_slot_admit_as(fdm_plan* p, int slot, const float* hub, int N, int fw, const float* style, const float* emo, int L_clip,
                      const float* x_T, unsigned long long seed, int clip_id, int sampler, float cfg_scale, void* stream);
int fdm_slot_admit_long_as(fdm_plan* p, const int* slots, int n, const float* hub, int N, int fw, const float* style, const float* emo,
                           int L_total, int overlap, const float* x_T, unsigned long long seed, int clip_id, int sampler, float cfg_scale,
                           void* stream);
/* Condition tracks: one style and one emotion vector PER LATENT FRAME instead of one per clip ("neutral, happy from frame 210 on").
 * The conditions enter the denoiser through the addend table E0 only, one row per frame; these calls build that table from per-frame
 * rows in one fdm_op_cond_rows launch and are otherwise the calls they are named after -- the step program, its launch count and its
 * cached programs are the same, and a track whose rows are all equal gives the bits of the per-clip call.  Self-attention is causal
 * and every other kernel of the step is row-local, so a change of condition at frame f0 leaves the frames before f0 bit for bit what
 * they are without it, at every step of every sampler.  Tracks are device (or device-visible) float rows, read in stream order as
 * hub is.  A NULL style track, or a NULL emotion track on a model with emotions: FDM_ERR_ARG; lengths: FDM_ERR_SHAPE as the per-clip
 * call.  The S-conditions form has no track variant.
 *   fdm_audio_prepare_tracks:         fdm_audio_prepare, style [B, L, n_style], emo [B, L, n_emo].
 *   fdm_audio_prepare_windows_tracks: fdm_audio_prepare_windows, style [B, L_total, n_style], emo [B, L_total, n_emo]; window w reads the
 *                                     track rows [s_w, s_w + W') of its clip; positions stay window-local.
 *   fdm_slot_admit_tracks:            fdm_slot_admit_as, style [L_clip, n_style], emo [L_clip, n_emo].
 *   fdm_slot_admit_long_tracks:       fdm_slot_admit_long_as, style [L_total, n_style], emo [L_total, n_emo]. */
int fdm_audio_prepare_tracks(fdm_plan* p, const float* hub, int B, int N, int fw, const float* style, const float* emo, int L, int cfg,
                             void* stream);
int fdm_audio_prepare_windows_tracks(fdm_plan* p, const float* hub, int B, int N, int fw, const float* style, const float* emo,
                                     int L_total, int window, int overlap, int cfg, void* stream);
int fdm_slot_admit_tracks(fdm_plan* p, int slot, const float* hub, int N, int fw, const float* style, const float* emo, int L_clip,
                          const float* x_T, unsigned long long seed, int clip_id, int sampler, float cfg_scale, void* stream);
int fdm_slot_admit_long_tracks(fdm_plan* p, const int* slots, int n, const float* hub, int N, int fw, const float* style, const float* emo,
                               int L_total, int overlap, const float* x_T, unsigned long long seed, int clip_id, int sampler,
                               float cfg_scale, void* stream);
/* Plan-time tuning of the GEMM output tiles at the prepared shape (times candidates per call site; changes speed only, every
 * tile accumulates k in the same order).  This call is the ONLY place the library tunes by itself: request paths
 * (fdm_audio_prepare*, fdm_sample_graph) never do -- fdm_plan_get(p, "needs_tune") turns 1 once the prepared shape has served
 * >= 2000 diffusion steps on heuristic tiles, so a serving caller can schedule this call off the request path.  Opt-in
 * (fdm_plan_set(p, "tune_lazy", 1)): tune inside fdm_audio_prepare* / fdm_sample_graph once that is the case; a tuner failure
 * there keeps the heuristic tiles and is counted ("tune_failed"), it never fails the request.
 * The library reads five environment variables, all about tiles: FDM_TUNE=0 disables the tuner (heuristic tiles, or the pinned
 * set); FDM_TUNE_VERBOSE=1 prints its choices; FDM_TILE_OVERRIDE="qkv=3,ffn1=2" pins call sites (applied at fdm_audio_prepare*,
 * with or without the tuner); FDM_TILE_CACHE=<file> (opt-in) keeps tuned sets across processes: a tuning run appends
 * "<version|mode|geometry|shape>\t<site>=<tile>,..." (temporary file + rename), and fdm_audio_prepare* takes a stored set for its
 * shape without any timing launch; FDM_GEMM_TILE=<FDM_TILE_*> forces one tile for every fdm_op_gemm with tile = 0 (A/B sweeps);
 * FDM_GEMM_LOCKSTEP=1 = FDM_TILE_LOCKSTEP for every fdm_op_gemm of the process (A/B of the once-per-clip stages; the step has fdm_plan_set "lockstep"). */
int fdm_plan_tune(fdm_plan* p, void* stream);
/* Introspection / experiments: integer properties by name -- "launches_per_step", "graph_launches" (host graph launches of
 * the last fdm_sample_graph / fdm_slots_run), "rows", "slots", "slot_long_frames", "slot_long_groups", "slot_samplers", "slot_sampler_steps", "tuned", "needs_tune", "tune_failed", "fuse_ln3", "tile.<call site>" (qkv, out, ffn1, ffn2,
 * enc, dec, ...). */
int fdm_plan_get(fdm_plan* p, const char* key, long long* out);
/* "slot_long_frames" / "slot_long_groups" (long capacity of the NEXT fdm_slots_open, see fdm_slot_admit_long),
 * "slot_samplers" / "slot_sampler_steps" (bank capacity of the NEXT fdm_slots_open, see fdm_slot_sampler_add),
 * "tile.<call site>" (drops recorded programs), "tune" (0 = off), "tune_lazy" (1 = in-call tuning allowed), "untune" (forget every
 * tuned set), "fuse_ln3" (1 = fold norm3 into the GEMMs around it: 8 launches fewer per step, no longer faster; takes effect at
 * the next commit) */
int fdm_plan_set(fdm_plan* p, const char* key, long long value);

/* ------------------------------------------------------------------------------------------
 * Audio encoder (once per clip: it does not depend on (t, x_t), so the reference's per-step re-run, models/fdm_vocaset.py:59,
 * is hoisted).  kind 0 = HuBERT-large (models/hubert.py:75-146: 7 x {Conv1d, LayerNorm(512), GELU}, even crop, projection,
 * weight-normed grouped positional conv, 24 pre-LN layers, final LayerNorm); kind 1 = wav2vec2-base (models/wav2vec.py:
 * 69-143: GroupNorm on conv 0 only, no conv bias, 12 post-LN layers) -- the BIWI denoiser's encoder.  n_layers 0 = the
 * kind's depth.  Weights by transformers state-dict name ("feature_extractor.conv_layers.0.conv.weight", ...,
 * "encoder.pos_conv_embed.conv.parametrizations.weight.original0|1" or torch-2.0's "...conv.weight_g|weight_v").
 * forward: wav [B, n] processor-normalised fp32 -> out [B, N, D] fp32, *n_frames = N = fdm_hubert_frames(n) (the conv
 * stack's length, even-cropped, :95-96).  frame_num > 0 keeps at most 2 * frame_num frames (:97-98); interp_in_fps /
 * interp_out_fps > 0 resample the conv features (linear_interpolation, :62-69) to frame_num or int(T / in * out) frames
 * instead of the even crop.  The caller sizes `out` for fdm_hubert_frames(n) rows per clip (or the interpolated count).
 * dtype: FDM_F32, FDM_BF16, or FDM_F16X3 = the transformer layers (84 % of the FLOPs) on split-fp16 operands behind an fp32
 * conv front / projection / positional conv: inside the 1e-4 contract at 0.57x the fp32 encoder's time. */
typedef struct fdm_audio_encoder fdm_audio_encoder;
int fdm_hubert_create(int kind, int n_layers, int dtype, fdm_audio_encoder** out);
int fdm_hubert_set_weights(fdm_audio_encoder* e, const char* name, const float* ptr, long long n, void* stream);
int fdm_hubert_forward(fdm_audio_encoder* e, const float* wav, int B, int n_samples, int frame_num, int interp_in_fps, int interp_out_fps,
                       float* out, int* n_frames, void* stream);
int fdm_hubert_frames(int n_samples);
/* B clips of unequal length in one call, padded to the longest: wav [B, n_max], n_samples [B] HOST ints (copied to the device in
 * stream order, not read after the call returns) -> out [B, N_max, D] with N[b] = fdm_hubert_frames(n_samples[b]) (the even crop per
 * clip), N_max = max N[b]; n_frames [B] host ints receives N[b].  Rows [0, N[b]) of clip b are bit for bit what fdm_hubert_forward
 * returns for that clip alone (B = 1, n = n_samples[b], no frame_num, no interpolation), for both kinds and every dtype; rows at or
 * beyond N[b] are zeros; what wav holds at or beyond n_samples[b] never matters (it may be NaN).  Every check is made before the
 * first launch: FDM_ERR_ARG (null pointer), FDM_ERR_SHAPE (B < 1, a clip shorter than fdm_hubert_forward accepts, n_samples[b] > n_max). */
int fdm_hubert_forward_ragged(fdm_audio_encoder* e, const float* wav, const int* n_samples, int B, int n_max, float* out, int* n_frames, void* stream);
int fdm_hubert_destroy(fdm_audio_encoder* e);

/* ------------------------------------------------------------------------------------------
 * Audio front end: raw PCM -> the waveform the encoders take (16 kHz, mono, processor-normalised, padded), batched over clips of
 * unequal length, rate, format and channel count.  What the demos do on the host (librosa.load(sr=16000) + Wav2Vec2Processor + 1 s of
 * zeros, demo/demo_vocaset.py:84-90) in this project's definition: scipy.signal.resample_poly + (x - mean) / sqrt(var + 1e-7).
 * For a clip of `frames` sample frames of `channels` interleaved channels at `rate` Hz:
 *   convert   int16: x / 2^15, int32: x / 2^31, uint8: (x - 128) / 128, float32 as is                              (fp32, exact)
 *   downmix   ((c0 + c1) + c2 ...) / channels in fp32: numpy's x.mean(axis=1) bit for bit up to 7 channels (numpy adds 8 in pairs)
 *   resample  g = gcd(rate, 16000), up = 16000 / g, down = rate / g, m = max(up, down), half = 10 m;
 *             h[k], k = 0 .. 2 half: firwin(2 half + 1, 1 / m, window = ('kaiser', 5.0)) * up, i.e. sinc(k - half; cutoff 1 / m) times
 *             I0(5 sqrt(1 - ((k - half) / half)^2)) / I0(5), divided by its sum, times up; in double, stored as fp32;
 *             n_out = ceil(frames * up / down);  y[j] = sum_i x[i] h[half + j down - i up] over the i inside the clip whose tap index is
 *             in range, i ascending, products and sum in fp64, rounded once to fp32.  The value of y[j] depends on nothing but the
 *             clip (not on the batch, n_max or a tile size).  rate == 16000: no filter, y = x bit for bit.  64-bit indices.
 *   normalise (normalize != 0) (y - mean) / sqrt(var + 1e-7), mean and population variance over the clip's n_out samples in fp64,
 *             two passes over chunks whose count and width follow from n_out alone, partials folded in chunk order (no atomics);
 *             each element is formed in fp64 and rounded once.  A constant clip gives zeros.
 *   pad       `pad` zeros follow and count as samples: n_samples[b] = n_out + pad; everything from there to n_max is zero.
 * Rates with max(up, down) > 2048 are refused (FDM_ERR_SHAPE): their tap tables would run to megabytes.
 * fdm_frontend_create computes the tap tables of `rates` (laid out by phase: the taps one output needs are contiguous); with a
 * device visible it uploads them and allocates the statistics scratch -- nothing is allocated later; without one the object still
 * validates arguments and fdm_frontend_forward ends in FDM_ERR_STATE.  fdm_frontend_samples is host only: *n = n_out + pad.
 * fdm_frontend_forward: clips [B] HOST structs (data: DEVICE pointer, aligned to its sample type; the structs are not read after
 * the call returns) -> wav [B, n_max] fp32 device, n_samples [B] HOST ints: the input layout of fdm_hubert_forward_ragged.  Launches
 * on `stream`, never synchronises.  An object holds ONE statistics scratch, which every call with normalize != 0 writes: it serves one
 * stream at a time (calls on the same stream follow each other in stream order; use one object per stream for concurrent calls, or
 * order the streams with events).  Every check is made before the first launch: FDM_ERR_ARG (null pointer, unknown format, a rate
 * the object was not created for -- 16000 needs no table and is always taken --, channels outside 1..8, pad < 0, misaligned data),
 * FDM_ERR_SHAPE (B < 1, frames < 1, n_samples[b] > n_max, n_max > INT_MAX, the ratio cap).  Speed: unmeasured
 * (profiles/audio_frontend/README.md). */
#define FDM_PCM_S16 0
#define FDM_PCM_S32 1
#define FDM_PCM_U8 2
#define FDM_PCM_F32 3
typedef struct fdm_pcm { const void* data; int format; int channels; int rate; long long frames; } fdm_pcm;
typedef struct fdm_frontend fdm_frontend;
int fdm_frontend_create(const int* rates, int n_rates, fdm_frontend** out);
int fdm_frontend_samples(const fdm_pcm* clip, int pad, long long* n);
int fdm_frontend_forward(fdm_frontend* f, const fdm_pcm* clips, int B, int pad, int normalize, float* wav, long long n_max, int* n_samples,
                         void* stream);
int fdm_frontend_destroy(fdm_frontend* f);

/* ------------------------------------------------------------------------------------------
 * (E)VQ-VAE: quantise, decode, encode (models/vq_vae_vocaset.py:23-43, models/vq_vae_emotion.py:9-41, models/vq_vae.py).
 * Geometry from the reference's *_vq_vae_args (models/utils/config.py): G = face_quan_num, c = zquant_dim, K = 256 codes
 * per book, n_books = n_embed / 256 (emotion-sliced codebook), V3 = in_dim; pre = decoder_linear_embedding_pre /
 * encoder_linear_embedding_post present (3D-MEAD, BIWI).  Weights by reference state-dict name.
 * quant:  z [B, R, c] (+ emotion one-hot [B, n_books]) -> z_q [B, c, R] (the reference's permuted output), idx [B*R] int64;
 *         quant_stats: emb_loss, perplexity, min_encodings of that call
 * decode: z_q [B, c, L*G] -> vertex offsets [B, L, V3] (the caller adds the template: fdm_mesh_forward below does; every clip gets pe[0], a20)
 * encode: x [B, L, V3] (+ emotion one-hot [B, 7]) -> latent [B, L*G, c]
 * dtype: FDM_F32, FDM_BF16, or FDM_F16X3 = the two 6-layer transformers on split-fp16 operands, convolutions / embeddings /
 *        vertex map / quantiser in fp32 (indices and z_q identical to the fp32 object's; decode 1.4-4.6e-5 from the reference) */
typedef struct fdm_vq_desc { int G, c, K, n_books, V3, pre; } fdm_vq_desc;
typedef struct fdm_vq fdm_vq;
int fdm_vq_create(const fdm_vq_desc* desc, int dtype, fdm_vq** out);
int fdm_vq_set_weights(fdm_vq* v, const char* name, const float* ptr, long long n, void* stream);
int fdm_vq_quant(fdm_vq* v, const float* z, const float* emo_one_hot, int B, int R, float* zq_bcl, long long* idx, void* stream);
/* emb_loss, perplexity and min_encodings of the same call (the reference returns them from quant(): models/vq_vae_vocaset.py:31-33,
 * beta = 0.25 :16-18): out2 = {loss, perplexity} device floats, min_encodings [B*R, K] device fp32 or NULL. */
int fdm_vq_quant_stats(fdm_vq* v, const float* z, const float* emo_one_hot, const long long* idx, int B, int R, float beta,
                       float* min_encodings, float* out2, void* stream);
/* Condition tracks in the quantiser: emo [B, L, n_books] with L = R / G holds one emotion vector per latent FRAME, and every frame is
 * quantised in the codebook slice of its own emotion: argmax(emo[b, l, :]), the first maximum as torch.argmax except that a NaN never
 * wins (a cross-fade row of a track takes its heavier side).  A track whose rows are all equal gives the bits of fdm_vq_quant / fdm_vq_quant_stats.  A model
 * without emotion-sliced codebooks: the per-clip call (emo ignored).  NULL emo: FDM_ERR_ARG; R not a multiple of G: FDM_ERR_SHAPE. */
int fdm_vq_quant_tracks(fdm_vq* v, const float* z, const float* emo, int B, int R, float* zq_bcl, long long* idx, void* stream);
int fdm_vq_quant_stats_tracks(fdm_vq* v, const float* z, const float* emo, const long long* idx, int B, int R, float beta,
                              float* min_encodings, float* out2, void* stream);
int fdm_vq_decode(fdm_vq* v, const float* zq_bcl, int B, int R, float* out, void* stream);
/* B clips of unequal length in one call, padded to the longest: z_q [B, c, R_max], frames [B] HOST ints (2 <= frames[b] <= R_max / G;
 * copied into the object's workspace in stream order, not read after the call returns) -> out [B, L_max, V3], L_max = R_max / G.
 * Rows [0, frames[b]) of clip b are bit for bit what fdm_vq_decode returns for that clip alone (B = 1, R = frames[b] * G), in
 * every dtype; rows at or beyond frames[b] are zeros.  What the caller's latent holds beyond frames[b] * G never matters (it may
 * be NaN).  Every check is made before the first launch: FDM_ERR_ARG (null pointer), FDM_ERR_SHAPE (R_max, frames[b]). */
int fdm_vq_decode_ragged(fdm_vq* v, const float* zq_bcl, const int* frames, int B, int R_max, float* out, void* stream);
int fdm_vq_encode(fdm_vq* v, const float* x, const float* emo_one_hot, int B, int L, float* latent, void* stream);
int fdm_vq_destroy(fdm_vq* v);

/* ------------------------------------------------------------------------------------------
 * Mesh hand-off: the offsets fdm_vq_decode(_ragged) writes -> what a renderer or engine takes: positions (+ template) at its own
 * frame rate and area-weighted vertex normals, planar or interleaved, fp32 or fp16 (the reference's render/ recomputes normals per
 * frame on the CPU and takes --fps 30 / 25).  fp32 throughout, fixed order, no contraction.  For clip b of L = frames[b] frames
 * over a triangle list faces [F, 3] on V vertices:
 *   positions p = offset + template (one fp32 add; no template: p = offset): the vertices pipeline.animate returns.
 *   frame rate with fps_in, fps_out > 0 and different: L_out = max(1, (int)((double)L / fps_in * fps_out)) frames, each the reference's
 *             linear_interpolation (align_corners = True) of the clip's own templated frames in the expression of fdm_op_linear_interp:
 *             scale = (float)(L-1) / (float)(L_out-1) (0 when L_out = 1), src = scale * t, i0 = min((int)src, L-1), i1 = min(i0+1, L-1),
 *             l1 = src - i0, l0 = 1 - l1, y = l0 * p[i0] + l1 * p[i1], every operation rounded.  Otherwise (0 = not given, or equal
 *             rates) L_out = L and the positions pass through bit for bit.  L = 0 gives L_out = 0.
 *   normals   from the OUTPUT positions of the same frame (fp32, before any fp16 rounding).  Face f = (a, b, c): e1 = p_b - p_a,
 *             e2 = p_c - p_a, n_f = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x), two rounded products and
 *             one rounded subtraction each.  Vertex v: s = the sum of n_f over its incident faces in ascending face index, one term
 *             per corner occurrence, starting from the first term; d = (s.x s.x + s.y s.y) + s.z s.z; the normal is s / sqrtf(d) with
 *             correctly rounded square root and division when d > 0, else (0, 0, 0) (isolated vertices, degenerate faces).
 *   output    planar: pos [B, L_out_max, V, 3] and nrm the same; FDM_MESH_INTERLEAVED: pos [B, L_out_max, V, 6], position then normal
 *             (nrm = NULL; needs FDM_MESH_NORMALS).  FDM_MESH_F16: both outputs fp16, rounded to nearest even at the store.  Without
 *             FDM_MESH_NORMALS nrm is not touched.  Rows at or past L_out[b] are written as zeros; input rows at or past frames[b] are
 *             never read (they may be NaN).  No atomics: a clip's rows do not depend on the batch, L_max, L_out_max or a tile size.
 * fdm_mesh_adjacency_host (no device): the vertex -> incident-face lists in CSR form, offsets [V + 1] and items [3 F] = face indices,
 * ascending per vertex, one entry per corner.  FDM_ERR_ARG: a null pointer, F < 0, V <= 0, an index outside [0, V).
 * fdm_mesh_create checks the faces (HOST ints, not read after the call), builds the lists and, with a device visible, uploads both;
 * without one the object still validates and fdm_mesh_forward ends in FDM_ERR_STATE.  fdm_mesh_frames is host only: the L_out rule.
 * fdm_mesh_forward: offsets [B, L_max, 3 V] fp32 device, frames [B] HOST ints in [0, L_max] (NULL: every clip has L_max frames; copied
 * in stream order, not read after the call returns), tmpl [tmpl_rows, 3 V] fp32 device with tmpl_rows = 0 (none), 1 (shared) or B,
 * frames_out [B] HOST ints or NULL.  Launches on `stream`, never synchronises -- except that a call larger than any before it grows
 * the object's scratch first (fp32 positions for the normals whenever the planar fp32 output does not hold them; the lengths), which
 * waits for the device.  An object holds ONE such scratch: it serves one stream at a time (calls on the same stream follow each other
 * in stream order; use one object per stream for concurrent calls, or order the streams with events).  Every check is made before
 * the first launch: FDM_ERR_ARG (null m / offsets / pos, unknown flag bits, tmpl_rows not 0, 1 or B, a null template with tmpl_rows > 0,
 * interleaved with nrm or without normals, planar normals without nrm, a negative or non-finite rate), FDM_ERR_SHAPE (B, L_max or
 * L_out_max < 1, frames[b] outside [0, L_max], L_out_max below the largest L_out[b]).  Call times against torch and the byte floor: profiles/mesh_out/README.md. */
#define FDM_MESH_INTERLEAVED 1
#define FDM_MESH_F16 2
#define FDM_MESH_NORMALS 4
typedef struct fdm_mesh fdm_mesh;
int fdm_mesh_adjacency_host(const int* faces, int F, int V, int* offsets, int* items);
int fdm_mesh_create(const int* faces, int F, int V, fdm_mesh** out);
int fdm_mesh_frames(int frames_in, double fps_in, double fps_out, int* frames_out);
int fdm_mesh_forward(fdm_mesh* m, const float* offsets, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows, double fps_in,
                     double fps_out, int flags, void* pos, void* nrm, int L_out_max, int* frames_out, void* stream);
int fdm_mesh_destroy(fdm_mesh* m);

/* ------------------------------------------------------------------------------------------
 * Rig hand-off: the offsets fdm_vq_decode(_ragged) writes -> what an engine's face rig plays: blendshape coefficients per frame
 * (ARKit's 52 in [0, 1], FLAME expression coefficients, a studio's own set), at the consumer's frame rate.  The fit is the standard
 * one: ridge-regularised, box-constrained least squares of the offsets onto a basis.  Inputs: basis E [K, 3 V] of blendshape deltas
 * from the neutral face, 1 <= K <= 128; optional per-vertex weights w [V] >= 0 (NULL: all 1); ridge lambda >= 0; optional bounds
 * lo [K] <= hi [K] (both or neither); a sweep count S >= 0.  For a frame with offset row d (before the template is added):
 *   c = argmin 1/2 sum_i w_v(i) (sum_k E_ki c_k - d_i)^2 + 1/2 lambda |c|^2   subject to lo <= c <= hi.
 *   create    (host, fp64, no device needed) P = E diag(w) rounded to fp32 (the only large array uploaded); G = E diag(w) E^T + lambda I
 *             and its Cholesky factor L (G = L L^T, lower) in fp64, both then rounded to fp32.  A pivot <= 0 (to fp64 rounding: <= K 2^-52 G_ii) or a non-finite value:
 *             FDM_ERR_ARG, "basis is rank deficient under these weights: raise ridge".
 *   project   r[f, k] = sum_i P[k, i] d[f, i] in fp32.  3 V is cut into chunks of 768 elements; each chunk's partial sum is formed in
 *             an order that depends on nothing but the chunk (fused multiply-adds per lane, then a fixed tree over the lanes), and the
 *             partial sums are added in ascending chunk order starting from the first.  No atomics: a frame's r does not depend on
 *             the batch, L_max, its position in the launch or the workgroup that ran it.  |error| <= gamma_n sum_i |P_ki| |d_i| with
 *             n = 3 V + chunks.
 *   frame rate with fps_in, fps_out > 0 and different: L_out and (i0, i1, l0, l1) are exactly those of fdm_mesh_frames / fdm_mesh_forward,
 *             applied to r: r_out = l0 * r[i0] + l1 * r[i1], every operation rounded (projection is linear: this is the fit of the
 *             resampled offsets).  Otherwise r passes through bit for bit.
 *   solve     fp32, every product, subtraction and division rounded on its own, in a fixed column order (a function of K alone):
 *               forward   g = r; for i = 0..K-1: y_i = g_i / L_ii; for all k > i: g_k = g_k - (L_ki * y_i)
 *               backward  for i = K-1..0: x_i = y_i / L_ii; for all k < i: y_k = y_k - (L_ik * x_i)
 *               no bounds c = x
 *               bounds    c = min(max(x, lo), hi); g = r; for j = 0..K-1, all k: g_k = g_k - (G_kj * c_j); then S sweeps of projected
 *                         Gauss-Seidel, for j = 0..K-1: n = min(max(c_j + g_j / G_jj, lo_j), hi_j); delta = n - c_j; c_j = n;
 *                         for all k, j included: g_k = g_k - (G_kj * delta)
 *             (min / max keep a NaN operand: a non-finite live offset row gives NaN coefficients, never a bound)
 *   output    coef [B, L_out_max, K] fp32 and, when proj is not NULL, proj [B, L_out_max, K]: the r the solve consumed.  Rows at or past
 *             L_out[b] are written as zeros; input rows at or past frames[b] are never read (they may be NaN).
 * fdm_rig_gram_host (no device): gram [K, K] fp64 = G, chol [K, K] fp32 = L rounded (zeros above the diagonal).
 * fdm_rig_create: basis, vweight, lo, hi are HOST arrays, not read after the call; sweeps = S (16 is the library's default in Python;
 * how many an ill-conditioned artist rig needs is unmeasured; under the temporal fit below convergence also slows as mu grows, and
 * its table is there).  With a device visible it uploads P, G, L and the bounds; without one
 * the object still validates and fdm_rig_forward ends in FDM_ERR_STATE.  FDM_ERR_ARG: a null pointer, K outside [1, 128], V < 1, a
 * negative or non-finite weight or ridge, exactly one of lo and hi, lo_k > hi_k or a non-finite bound, sweeps < 0, a rank-deficient Gram.
 * fdm_rig_forward: offsets [B, L_max, 3 V] fp32 device, frames [B] HOST ints in [0, L_max] (NULL: every clip has L_max frames; copied
 * in stream order, not read after the call returns), coef and proj device, frames_out [B] HOST ints or NULL.  Launches on `stream`,
 * never synchronises -- except that a call larger than any before it grows the object's scratch first (the partial sums, the
 * lengths), which waits for the device.  An object holds ONE such scratch: it serves one stream at a time.  Every check is made
 * before the first launch: FDM_ERR_ARG (null r / offsets / coef, a negative or non-finite rate), FDM_ERR_SHAPE (B, L_max or
 * L_out_max < 1, frames[b] outside [0, L_max], L_out_max below the largest L_out[b]).  Not built: a per-frame fit residual, head and
 * jaw pose, fp16 output.  Call times: profiles/rig_out/README.md.
 *
 * Temporal fit (fdm_rig_set_temporal).  The per-frame fit above passes frame-to-frame decoder noise, the
 * null-space drift of an ill-conditioned rig and coefficients snapping on and off their bounds straight into the curves.  With
 * smooth = mu > 0 and optional sweights m [K] > 0 (NULL: all 1), M = mu diag(m), the frames of a clip are fitted together.  Everything
 * up to and including the frame-rate step is as above (P, G, r, L_out, the taps applied to r); then per clip with Lo = L_out[b] frames
 *   min over c_0..c_{Lo-1} of  sum_f (1/2 c_f^T G c_f - r_f^T c_f) + 1/2 sum_{f>=1} (c_f - c_{f-1})^T M (c_f - c_{f-1})   s.t. lo <= c_f <= hi.
 * The penalty is on OUTPUT frames: at another fps_out the same mu smooths over a different time span.  mu = 0 is the per-frame fit.
 * n_f = the number of neighbours of frame f inside its clip: 0 when Lo = 1, 1 at the two ends, 2 inside.
 *   tables    fdm_rig_temporal_tables_host (host, fp64, no device): D = diag(1 / sqrt(mu m_k)); A = D G D = U Lam U^T by cyclic Jacobi
 *             rotations (written in the library); eigenvalues ascending; each eigenvector's sign such that its largest-magnitude entry is
 *             positive (lowest index on a tie); Q = D U, so Q^T G Q = Lam and Q^T M Q = I.  lam [K], Q [K, K] (column k = mode k) fp64.
 *             The object keeps lam, Q, Q^T and mvec_k = mu m_k, each rounded once to fp32.  FDM_ERR_ARG: mu negative or non-finite (0
 *             too for the tables: there are none), m_k <= 0 or non-finite, lam_k <= 0 or a value that does not fit fp32.
 *   modal in  per output frame z_k = sum_j QT[k][j] r_j: j ascending, the first product starts the sum, every product and sum rounded.
 *   time      per (clip, k), fp32, every operation rounded on its own, with d_f = lam_k + (float)n_f:
 *               w_0 = d_0; iw_0 = 1 / w_0; u_0 = z_0; for f = 1..Lo-1: w_f = d_f - iw_{f-1}; iw_f = 1 / w_f; u_f = z_f + (u_{f-1} * iw_{f-1})
 *               y_{Lo-1} = u_{Lo-1} * iw_{Lo-1}; for f = Lo-2..0: y_f = (u_f + y_{f+1}) * iw_f
 *             (strictly diagonally dominant since lam_k > 0: no pivoting).  u and iw live in the object's scratch.
 *   modal out x_k = sum_j Q[k][j] y_j, the same order and rounding.  No bounds: c = x.  Bounds: c = min(max(x, lo), hi), a NaN kept.
 *   bounds    S sweeps of red-black projected Gauss-Seidel in place in coef; a sweep is colour 0 (even f inside the clip), then colour 1
 *             (odd f), one launch each.  For a frame of the current colour, reading its neighbours' current values:
 *               s = c_{f-1}, or c_{f+1}, or (c_{f-1} + c_{f+1}), or absent (n_f = 0); g = r_f when s is absent, else r_f + (mvec * s)
 *               for j = 0..K-1, all k: g_k = g_k - (G_kj * c_j);   e_k = (float)n_f * mvec_k;   g_k = g_k - (e_k * c_k)
 *               for j = 0..K-1: den = G_jj + e_j; n = min(max(c_j + g_j / den, lo_j), hi_j); delta = n - c_j; c_j = n;
 *                               for all k: g_k = g_k - (G_kj * delta); then g_j = g_j - (e_j * delta)
 *             Frames of one colour never read each other; the launch boundary is the only synchronisation between half-sweeps (no grid
 *             barrier, no atomics).  Convergence slows as mu grows against G.  Measured on the float32 restatement against fp64 bounded
 *             least squares of the stacked system (K = 12, 3 V = 96, Lo = 24, bounds [0, 1]; tests/test_rig_temporal_cpu.py), max-abs
 *             distance at 16 / 64 sweeps: mu = 0.1 tr(G)/K 2.3e-07 / 2.3e-07; mu = tr(G)/K 2.8e-05 / 4.8e-07; mu = 10 tr(G)/K
 *             2.1e-02 / 3.9e-04.  Raise S with mu.
 *   output    as above.  L_out[b] = 0 gives no rows; L_out[b] = 1 is the modal solve with n = 0: the per-frame answer mathematically,
 *             not bit for bit.  A non-finite live offset row makes every coefficient of ITS CLIP NaN (the frames are coupled), never a
 *             bound; other clips keep their bits.
 * A clip's bits do not depend on the batch: every step names only the clip's own rows, its own Lo and the frame's parity inside the
 * clip; B, L_max, L_out_max and the tiling only decide who computes it.
 * fdm_rig_set_temporal: builds the tables from the object's fp64 G, uploads them and waits for the device (before and after: a call in
 * flight may read the old ones); smooth = 0 returns the object to the per-frame path.  Without a device it still validates.  An object
 * on which it was never called, or was last called with 0, runs exactly the launches of the per-frame fit.  fdm_rig_forward keeps its
 * signature and fdm_version() its value: callers detect the feature by the symbol.  A bounded temporal call is 3 + 2 S launches after
 * the projection.  Call times: profiles/rig_temporal/README.md. */
typedef struct fdm_rig fdm_rig;
int fdm_rig_gram_host(const float* basis, const float* vweight, int K, int V, double ridge, double* gram, float* chol);
int fdm_rig_create(const float* basis, int K, int V, const float* vweight, double ridge, const float* lo, const float* hi, int sweeps,
                   fdm_rig** out);
int fdm_rig_forward(fdm_rig* r, const float* offsets, const int* frames, int B, int L_max, double fps_in, double fps_out, float* coef,
                    float* proj, int L_out_max, int* frames_out, void* stream);
int fdm_rig_destroy(fdm_rig* r);
int fdm_rig_temporal_tables_host(const double* gram, int K, double smooth, const float* sweights, double* lam, double* Q);
int fdm_rig_set_temporal(fdm_rig* r, double smooth, const float* sweights);

/* ------------------------------------------------------------------------------------------
 * Parametric head: parameters in, vertices out.  A head of the SMPL / FLAME family (Loper et al. 2015; Li et al. 2017): blend shapes,
 * pose correctives and linear blend skinning over a small kinematic tree.  The reverse direction of the rig hand-off, and the way a
 * sampled animation gets head, neck, jaw and eye motion: the decoder's offsets enter as `extra`.
 * Model (fdm_flame_model, HOST arrays, not read after the call): V vertices; J joints, 1 <= J <= 8; NB blend coefficients, 0 <= NB <= 512,
 *   of which [0, expr_at) are shape and [expr_at, NB) expression; v_template [V, 3]; shapedirs [V, 3, NB]; posedirs [9 (J - 1), 3 V]
 *   (NULL when J = 1); j_regressor [J, V] dense; parents [J] (entry 0 ignored, parents[j] in [0, j)); lbs_weights [V, J].  Optional
 *   landmarks: NL <= 256 vertex triples lmk_verts [NL, 3] with barycentric weights lmk_bary [NL, 3] (the static embedding, each face
 *   already resolved to its three vertices).
 * Per call: shape [shape_rows, NS] (shape_rows = 1 or B; NS <= expr_at), expr [B, L_max, NE] (NE <= NB - expr_at), pose [B, L_max, 3 J]
 *   axis-angle (FLAME: global, neck, jaw, left eye, right eye), optional transl [B, L_max, 3] and extra [B, L_max, 3 V] (the layout
 *   fdm_vq_decode_ragged writes), frames [B] HOST ints as in fdm_mesh_forward.  Coefficients not given are not accumulated (they are
 *   zeros: the result is that of the padded vector).
 *   create    (host, fp64, rounded once to fp32; fdm_flame_tables_host returns the same arrays, no device needed)
 *             D [NB + 9 (J - 1), 3 V]: D[k, 3 v + a] = shapedirs[v, a, k], then the posedirs rows; JT [J, 3] = j_regressor v_template;
 *             JD [NB, 3 J] = j_regressor shapedirs, sums over v ascending: joints are linear in the coefficients.
 *   pose      fp32, EVERY operation rounded on its own (no fused multiply-add), per frame:
 *             joints    Jf = JT; Jf += shape_k * JD[k] for k = 0..NS-1; Jf += expr_k * JD[expr_at + k] for k = 0..NE-1.
 *             rotation  per joint with r = its axis-angle: e = r + 1e-8 (each component), angle = sqrt((e.x e.x + e.y e.y) + e.z e.z),
 *                       (x, y, z) = r / angle, s = sinf(angle), m = 1 - cosf(angle), K = [0 -z y; z 0 -x; -y x 0],
 *                       KK = [-(yy + zz) xy xz; xy -(xx + zz) yz; xz yz -(xx + yy)], R = (I + s K) + m KK.  r = 0 gives R = I exactly.
 *             chain     G_0 = [R_0 | Jf_0]; for j >= 1 with p = parents[j] and d = Jf_j - Jf_p: G_j.R = G_p.R R_j, G_j.t = G_p.R d + G_p.t,
 *                       every 3-term product sum as (a0 b0 + a1 b1) + a2 b2.  Relative to the rest pose: A_j = [G_j.R | G_j.t - G_j.R Jf_j].
 *             feature   (R_j - I) for j >= 1, row-major, [9 (J - 1)].
 *             xforms [B, L_max, J, 12] (A_j as a row-major 3 x 4) and posefeat [B, L_max, 9 (J - 1)] live in the object's scratch and are
 *             copied out when the caller passes pointers.
 *   blend     fp32, FUSED multiply-adds (one rounding per term), fixed order.  Per clip v_id = v_template, then v_id = fma(shape_k, D[k],
 *             v_id) for k = 0..NS-1, stored once per shape row.  Per frame v = v_id; v = fma(expr_k, D[expr_at + k], v), k = 0..NE-1;
 *             v = fma(posefeat_p, D[NB + p], v), p = 0..9 (J - 1) - 1; then v = v + extra (one rounded add) when extra is given.
 *   skin      per vertex T = w_v0 * A_0 (a rounded product), T = fma(w_vj, A_j, T) for j = 1..J-1; out_c = fma(T_c2, v.z, fma(T_c1, v.y,
 *             T_c0 * v.x)) + T_c3, then + transl_c when transl is given (rounded adds).
 *   landmarks lmk [B, L_max, NL, 3] = fma(b2, out[v2], fma(b1, out[v1], b0 * out[v0])).  The dynamic contour is not built.
 *   output    verts [B, L_max, V, 3] fp32.  Rows at or past frames[b] come out as zeros in every output; input rows at or past
 *             frames[b] are never read (they may be NaN).  Every vertex of every frame follows the same operation sequence, a function
 *             of the model alone: no atomics, and a frame's values do not depend on the batch, L_max, its slot in a tile, the workgroup
 *             or which optional outputs were asked for.  extra of zeros equals no extra (x + 0 = x).
 * fdm_flame_create: FDM_ERR_ARG with a message naming the field for a null required pointer, V < 1, J outside [1, 8], NB outside
 * [0, 512], expr_at outside [0, NB], parents[j] outside [0, j), a non-finite model value, NL outside [0, 256], a landmark vertex outside
 * [0, V).  With a device visible it uploads the tables; without one the object still validates and fdm_flame_forward ends in
 * FDM_ERR_STATE.  fdm_flame_forward: device pointers except frames; lmk, xforms, posefeat, transl, extra, frames may be NULL (frames
 * NULL: every clip has L_max frames).  Launches on `stream`, never synchronises -- except that a call larger than any before it grows
 * the object's scratch first, which waits for the device.  An object holds ONE scratch: it serves one stream at a time.  Every check is
 * made before the first launch: FDM_ERR_ARG (null f / pose / verts, null shape with NS > 0 or expr with NE > 0, NS outside [0, expr_at],
 * NE outside [0, NB - expr_at], shape_rows not 1 or B, lmk without an embedding), FDM_ERR_SHAPE (B or L_max < 1, frames[b] outside
 * [0, L_max]).  Not built: the dynamic contour landmarks, fp16 output (fitting pose from vertices: fdm_flame_fit_* below).  Call times: profiles/flame_out/README.md. */
typedef struct fdm_flame_model {
  int V, J, NB, expr_at;
  const float* v_template; const float* shapedirs; const float* posedirs; const float* j_regressor;
  const int* parents; const float* lbs_weights;
} fdm_flame_model;
typedef struct fdm_flame fdm_flame;
int fdm_flame_tables_host(const fdm_flame_model* m, float* D, float* JT, float* JD);
int fdm_flame_create(const fdm_flame_model* m, const int* lmk_verts, const float* lmk_bary, int NL, fdm_flame** out);
int fdm_flame_forward(fdm_flame* f, const float* shape, int NS, int shape_rows, const float* expr, int NE, const float* pose, const float* transl,
                      const float* extra, const int* frames, int B, int L_max, float* verts, float* lmk, float* xforms, float* posefeat,
                      void* stream);
int fdm_flame_destroy(fdm_flame* f);

/* ------------------------------------------------------------------------------------------
 * Parametric head, the reverse direction: vertices in, expression and pose parameters out.  Frames are
 * independent.  Per live frame with target y [3 V] (absolute positions), fixed shape (per clip, or none) and the forward map F above,
 * `iters` damped Gauss-Newton steps on
 *     1/2 sum_v m_v |F(shape, expr, pose)_v + t - y_v|^2 + 1/2 ridge_expr |expr|^2 + 1/2 ridge_pose |pose_free - pose0_free|^2
 * over theta = (the first n_expr expression coefficients; the axis-angle of the joints free_joints[0..n_free), in that order; the
 * translation t when transl = 1), P = n_expr + 3 n_free + 3 transl in [1, 128], from theta = (0, pose0, 0).  Joints not in the free set
 * keep pose0's rotation (zeros without pose0).  m = vertex_weights [V] (HOST, at create; NULL: ones).  There is no line search and no
 * data-dependent branch: 2 + 5 iters launches, then the forward's own launches and one more for rms / verts.
 * A step at theta (all fp32, fixed order, no atomics; tests/flame_fit_cases.py restates every line in numpy):
 *   pose      the forward's pose stage at theta (its kernel): the transforms A_j, the pose feature, the blend coefficients.
 *   deriv     per row, every operation rounded, 3-term sums as (a0 b0 + a1 b1) + a2 b2.  With r a free joint's axis-angle,
 *             t2 = (r.x r.x + r.y r.y) + r.z r.z, K = hat(r), KK = r r^T - t2 I, S_c = e_c r^T + r e_c^T - 2 r_c I:
 *               t2 >= 1e-2: th = sqrt(t2), a = sinf(th) / th, b = (1 - cosf(th)) / t2, a1 = (cosf(th) - a) / t2, b1 = (a - 2 b) / t2;
 *               t2 <  1e-2 (the small-angle branch): a = 1 + t2 (-1/6 + t2 / 120), b = 1/2 + t2 (-1/24 + t2 / 720),
 *                           a1 = -1/3 + t2 (1/30 - t2 / 840), b1 = -1/12 + t2 (1/180 - t2 / 6720);
 *               dR_c = ((a hat(e_c) + b S_c) + (a1 r_c) K) + (b1 r_c) KK   (the closed-form derivative of I + a K + b K K).
 *             Pose column (joint f, component c), joints ascending: dG_0 = [dR_c if f = 0, else 0 | 0]; for j >= 1, p = parents[j],
 *             d = Jf_j - Jf_p: dG_j.R = G_p.R dR_c if j = f, else dG_p.R R_j; dG_j.t = dG_p.R d + dG_p.t; dA_j = [dG_j.R | dG_j.t - dG_j.R Jf_j].
 *             Expression column k, e = JD[expr_at + k]: h_0 = e_0, h_j = G_p.R (e_j - e_p) + h_p, dE_j = h_j - G_j.R e_j.
 *   columns   per vertex with T (the forward's blended transform), v (the forward's blended vertex before skinning), w its weights:
 *             expression k: fma(T_c2, d.z, fma(T_c1, d.y, T_c0 d.x)) + E_c with d = D[expr_at + k] at the vertex and
 *               E_c = w_0 dE_0c, then fma(w_j, dE_jc, E_c), j ascending -- exact for fixed rotations;
 *             pose q: U = w_0 dA_0, fma(w_j, dA_j, U); fma(U_c2, v.z, fma(U_c1, v.y, U_c0 v.x)) + U_c3 -- the derivative of the skinning;
 *               the derivative of the pose correctives is LEFT OUT (the Gauss-Newton approximation; a zero residual is still a fixed point);
 *             translation: the identity.  Residual r_c = (forward_c [+ t_c]) - y_c, the forward's own operation sequence.
 *   normal    with Z = [J | r] (P + 1 columns), per chunk of 256 vertices the upper triangle of Z^T M Z: s = fma(m Z_ia, Z_ib, s) over the
 *             chunk's elements i = 3 v + c ascending from s = 0 (m Z_ia a rounded product); then the chunks' sums added in ascending chunk
 *             order (rounded adds).  H = the P x P block, g = the last column.
 *   solve     A = H + diag(rho_q + lambda) (rho + lambda rounded, then one rounded add), b_q = -(g_q + rho_q (theta_q - theta0_q)); rho is
 *             ridge_expr on expression columns, ridge_pose on pose columns, 0 on the translation.  Right-looking Cholesky, columns
 *             ascending: the row FAILS at column j when its pivot is not > pivot_tol x the damped diagonal A_jj before elimination (this also
 *             catches NaN; pivot_tol = 0 is the plain test pivot > 0); l_jj = sqrt(pivot), l_ij = A_ij / l_jj, A_ik = fma(-l_ij, l_kj, A_ik) for j < k <= i.  y_j = b_j / l_jj,
 *             b_i = fma(-l_ij, y_j, b_i), j ascending; x_j = y_j / l_jj, y_i = fma(-l_ji, x_j, y_i), j descending; theta_q += x_q.
 *             A failed row sets status[row] = j + 1 and keeps its theta; it is evaluated again at the next step and fails again.
 * Outputs (device): expr [B, L_max, n_expr], pose [B, L_max, 3 J] (all joints: fixed ones carry pose0), transl [B, L_max, 3] (zeros when
 * the translation is not free), rms [B, L_max] = sqrt(S / sum m) with S the chunks' sums (ascending) of a 256-slot halving tree over
 * m ((dx dx + dy dy) + dz dz) of d = verts - y, verts [B, L_max, V, 3] = fdm_flame_forward of the returned parameters (that call), status
 * [B, L_max] ints.  Every output but expr and pose may be NULL (expr too when n_expr = 0).  Rows at or past frames[b] are zeros; target and pose0 rows there are
 * never read (they may be NaN).
 * fdm_flame_fit_create (HOST arrays, not kept; the head must outlive the fit and the two share one stream at a time: the fit uses the
 * head's tables and scratch): FDM_ERR_ARG for P outside [1, 128], n_expr > NE = NB - expr_at, a joint index out of range or given twice,
 * vertex weights negative, not finite or all zero.  fdm_flame_fit_set: "iters" (default 20, >= 1), "lambda" (1e-6), "ridge_expr" (0),
 * "ridge_pose" (0), each finite and not negative, "pivot_tol" (2^-18, in [0, 1]): settings, not measurements.  fdm_flame_fit_forward: checks as fdm_flame_forward; no
 * allocation after the first call at a given (B, L_max).  fdm_flame_fit_step: ONE step from the GIVEN parameters (copied; the caller's are
 * left alone), for tests and tools: H [B, L_max, (P + 1)(P + 2) / 2] (the reduced upper triangle, row-major packed; dead rows zeros), delta
 * [B, L_max, P], dX [B, L_max, 3 n_free, J, 12], dE [B, L_max, n_expr, J, 3], xforms [B, L_max, J, 12] (each may be NULL), status.
 * Not built: fitting shape, robust losses, temporal smoothing of the parameters, the derivative of the pose correctives, the dynamic
 * contour.  Call times are unmeasured: profiles/flame_fit/README.md. */
typedef struct fdm_flame_fit fdm_flame_fit;
int fdm_flame_fit_create(fdm_flame* f, const int* free_joints, int n_free, int n_expr, int transl, const float* vertex_weights, fdm_flame_fit** out);
int fdm_flame_fit_set(fdm_flame_fit* fit, const char* key, double value);
int fdm_flame_fit_forward(fdm_flame_fit* fit, const float* target, const float* shape, int NS, int shape_rows, const float* pose0, const int* frames,
                          int B, int L_max, float* expr, float* pose, float* transl, float* rms, float* verts, int* status, void* stream);
int fdm_flame_fit_step(fdm_flame_fit* fit, const float* target, const float* shape, int NS, int shape_rows, const float* pose0, const float* expr,
                       const float* pose, const float* transl, const int* frames, int B, int L_max, float* H, float* delta, float* dX, float* dE,
                       float* xforms, int* status, void* stream);
int fdm_flame_fit_destroy(fdm_flame_fit* fit);

/* ------------------------------------------------------------------------------------------
 * Wrap hand-off: the animated face drives a mesh of ANOTHER topology (a character head with its own vertex count and UV seams, another
 * LOD, a face patch of a body mesh).  A surface binding: every vertex of the target is bound once, at create, to one triangle of the
 * source's REST surface and follows that triangle in every frame.  The output has the layout fdm_mesh_forward and fdm_rig_forward read
 * ([B, L_max, 3 Vt]), so target normals, the frame rate, fp16 and a rig fit on the target's own blendshapes are those calls, AFTER this
 * one: there is no frame-rate step here (resample the wrapped frames with the mesh or rig hand-off).
 * Everything on the device is fp32, fixed order, no contraction, no atomics.  dot(x, y) = (x.x y.x + x.y y.y) + x.z y.z; cross(x, y) =
 * (x.y y.z - x.z y.y, x.z y.x - x.x y.z, x.x y.y - x.y y.x), two rounded products and one rounded subtraction per component (the mesh
 * hand-off's); vector sums and differences are per component.
 * Inputs at create (HOST arrays, not read after the call): source rest S [V, 3], source triangles faces [F, 3], target rest T [Vt, 3],
 *   optional face_idx [Vt] (a binding brought from a DCC tool or a cache), optional weights [Vt] in [0, 1].
 * Nearest face (device, fp32; only when face_idx is NULL).  Per face f = (a, b, c) of the rest surface, once: ab = b - a, ac = c - a,
 *   bc = c - b, n = cross(ab, ac), d = dot(n, n); the face is a candidate only when d > 0.  Per target vertex q and candidate face, the
 *   closest point by the region walk of Ericson, Real-Time Collision Detection 5.1.5, every operation rounded on its own:
 *     ap = q - a, bp = q - b, cp = q - c; d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp),
 *     d6 = dot(ac, cp); vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4 (two products, one subtraction); d43 = d4 - d3,
 *     d56 = d5 - d6.  The FIRST region in this order whose test holds:
 *       0 vertex a   d1 <= 0 and d2 <= 0                    P = a
 *       1 vertex b   d3 >= 0 and d4 <= d3                   P = b
 *       2 edge ab    vc <= 0 and d1 >= 0 and d3 <= 0        t1 = d1 / (d1 - d3),        P = a + t1 ab
 *       3 vertex c   d6 >= 0 and d5 <= d6                   P = c
 *       4 edge ac    vb <= 0 and d2 >= 0 and d6 <= 0        t2 = d2 / (d2 - d6),        P = a + t2 ac
 *       5 edge bc    va <= 0 and d43 >= 0 and d56 >= 0      t1 = d43 / (d43 + d56),     P = b + t1 bc
 *       6 interior   otherwise: s = (va + vb) + vc,         t1 = vb / s, t2 = vc / s,   P = a + t1 ab + t2 ac
 *     written as selects: P = (base + t1 dir) + t2 ac with base = a, b or c, dir = ab (bc in region 5), and t1 = 0 / 1, t2 = 0 / 1
 *     where the region states none (so a vertex region gives the vertex itself); divisions correctly rounded.  r = q - P,
 *     dist2 = dot(r, r).  q takes the face with the strictly smallest dist2 scanning f ascending from best = +inf: a tie keeps the
 *     lowest index and a NaN or infinite dist2 never wins.  A vertex left with no candidate fails the create (FDM_ERR_ARG, the message
 *     names the vertex).  The result is a function of q and the face list alone: not of Vt, the face tile of the kernel or how the
 *     faces are split over workgroups (partial minima combine to the lowest dist2, then the lowest index).
 * Coordinates (host, fp64, rounded once to fp32; fdm_wrap_coords_host, no device needed).  For q bound to face (a, b, c): e1 = b - a,
 *   e2 = c - a, r = q - a, n = cross(e1, e2), nn = dot(n, n), nh = n / sqrt(nn); g11 = dot(e1, e1), g12 = dot(e1, e2), g22 = dot(e2, e2),
 *   r1 = dot(e1, r), r2 = dot(e2, r), det = g11 g22 - g12 g12; u = (g22 r1 - g12 r2) / det, v = (g11 r2 - g12 r1) / det (the 2 x 2 normal
 *   equations), h = dot(r, nh): q = a + u e1 + v e2 + h nh.  (u, v) are plane coordinates and leave [0, 1] when the closest point is on
 *   an edge.  dist = sqrt(dist2) of the region walk above in fp64 for that face, rounded to fp32: the value a falloff reads, the same
 *   whichever way face_idx was obtained.  FDM_ERR_ARG: a null pointer, F, V or Vt < 1, an index outside its range, a face without area
 *   (nn or det not > 0), a non-finite coordinate.
 * Follow (device, fp32, per live frame row of clip b and target vertex j with face (a, b, c), (u, v, h), rest T_j, weight w_j):
 *   p = offset + template for the three source vertices (one fp32 add; no template: p = offset), as in fdm_mesh_forward;
 *   e1 = p_b - p_a, e2 = p_c - p_a, n = cross(e1, e2), d = dot(n, n); nh = n / sqrtf(d) with correctly rounded root and division when
 *   d > 0, else nh = 0 (a face that lost its area in this frame); y = ((p_a + u e1) + v e2) + h nh, every operation rounded on its own.
 *   With weights o = w_j (y - T_j), without o = y - T_j; the output is T_j + o, or o itself under FDM_WRAP_OFFSETS (the layout a rig
 *   fit on the target topology reads).  Without weights and without FDM_WRAP_OFFSETS the output is y: no subtract and add back.
 *   out [B, L_max, 3 Vt] fp32; rows at or past frames[b] are written as zeros, input rows at or past frames[b] are never read (they may
 *   be NaN); a clip's rows do not depend on the batch, L_max or a tile size.
 * Not built: scaling h with the triangle's area, smoothing across binding seams, binding to more than one face, fp16 output (the mesh
 * hand-off does that).
 * fdm_wrap_create: with face_idx given it validates (and computes the coordinates) without a device, and fdm_wrap_forward then ends in
 * FDM_ERR_STATE; with face_idx NULL and no device it returns FDM_ERR_STATE.  It may wait for the device.  FDM_ERR_ARG also for a weight
 * outside [0, 1] or non-finite.  fdm_wrap_binding copies face_idx [Vt], uvh [Vt, 3] and dist [Vt] to HOST arrays (any may be NULL).
 * fdm_wrap_forward: offsets [B, L_max, 3 V] fp32 device, frames [B] HOST ints (NULL: L_max each), tmpl [tmpl_rows, 3 V] fp32 device,
 * tmpl_rows = 0, 1 or B, out device.  Launches on `stream` and never synchronises, except to grow the lengths scratch; an object serves
 * one stream at a time.  Every check is made before the first launch: FDM_ERR_ARG (null w / offsets / out, unknown flag bits, tmpl_rows
 * not 0, 1 or B, a null template with tmpl_rows > 0), FDM_ERR_SHAPE (B or L_max < 1, frames[b] outside [0, L_max]).  fdm_version() keeps
 * its value: callers detect the feature by the symbol.  Call times: profiles/wrap_out/README.md. */
#define FDM_WRAP_OFFSETS 1
typedef struct fdm_wrap fdm_wrap;
int fdm_wrap_coords_host(const float* src_rest, const int* faces, int F, int V, const float* dst_rest, int Vt, const int* face_idx,
                         float* uvh /*[Vt,3]*/, float* dist /*[Vt]*/);
int fdm_wrap_create(const float* src_rest, const int* faces, int F, int V, const float* dst_rest, int Vt,
                    const int* face_idx /*or NULL: search on the device*/, const float* weights /*or NULL*/, fdm_wrap** out);
int fdm_wrap_binding(const fdm_wrap* w, int* face_idx, float* uvh, float* dist);      /* host copies; any may be NULL */
int fdm_wrap_forward(fdm_wrap* w, const float* offsets, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows, int flags,
                     float* out, void* stream);
int fdm_wrap_destroy(fdm_wrap* w);

/* ------------------------------------------------------------------------------------------
 * Time filter hand-off: a zero-phase FIR filter of the decoded offsets along time, per clip at its own
 * length, BEFORE any other hand-off reads them -- the VQ decoder writes every frame from its own code vector, so its output carries
 * frame-to-frame jitter, and the mesh, wrap, render, rig and head hand-offs all read the same [B, L_max, 3 V] offsets.  What a given
 * filter does to perceptual quality or to lip-sync metrics is UNMEASURED (there are no trained checkpoints here); it is off unless asked for.
 * Inputs: x [B, L_max, N] fp32 device, N = 3 V; lens [B] HOST ints, 1 <= L_b <= L_max (NULL: L_max each); half-taps h[0..R] fp32,
 *   0 <= R <= 32, the full kernel symmetric, h[-k] = h[k]; an edge rule; optionally a strength s [V] fp32, each in [0, 1].
 * Edge index e(i) of a clip of L frames.  FDM_TFILTER_MIRROR: L == 1: 0; otherwise p = 2 (L - 1), m = ((i mod p) + p) mod p,
 *   e = m < L ? m : p - m -- the end sample is not repeated, and the rule holds for any R against any L, clips shorter than the radius
 *   included.  FDM_TFILTER_NEAREST: e = min(max(i, 0), L - 1).
 * Filtered value of element (t, n) of a live frame, fp32, every operation rounded on its own (no contraction):
 *     acc = h[0] x[t][n];  for k = 1 .. R:  acc = acc + h[k] (x[e(t - k)][n] + x[e(t + k)][n]);  f = acc
 *   The pair is summed first: filtering a time-reversed clip gives the time-reversed result bit for bit.
 * Output: without a strength y = f.  With the strength s_v of column n's vertex: y = x (a copy, -0.0 included) where s_v == 0; otherwise
 *   d = f - x, y = x + s_v d, three rounded operations (s_v = 1 is NOT the call without a strength, bit for bit).
 * Rows at or past L_b are written as zeros; input rows at or past L_b are never read (they may be NaN).  y may not overlap x (refused).
 *   A clip's bits do not depend on the batch, on L_max or on a tile size: every element is the fixed chain above.  No atomics.
 * Taps are built on the host in fp64 and handed over as fp32 (the caller rounds; any taps of its own are as good):
 *   fdm_tfilter_taps_host, kind FDM_TFILTER_GAUSSIAN: w_k = exp(-k^2 / (2 sigma^2)) with sigma = param (finite, > 0), normalised so
 *   that h0 + 2 sum h_k = 1; kind FDM_TFILTER_SAVGOL: the Savitzky-Golay smoothing taps of window 2 R + 1 and polynomial order param
 *   in {2, 3, 4, 5}, the centre row of the least-squares fit (orders 2 and 3 share a row, as do 4 and 5; an order >= 2 R + 1 is
 *   refused).  taps holds R + 1 doubles.  Rounded to fp32 their sum is 1 only to rounding: a constant comes back to within the
 *   rounding bound of the chain above, not bit for bit, unless the taps are dyadic.
 * fdm_tfilter_create validates without a device (forward then ends in FDM_ERR_STATE) and uploads taps [R + 1] and strength [V] (HOST
 *   arrays, not read after the call); every launch of the object goes to `stream`: an object serves one stream at a time.  FDM_ERR_ARG:
 *   V < 1, R outside [0, 32], a NaN or infinite tap, a strength outside [0, 1] or NaN, an unknown edge rule, a null pointer.
 * fdm_tfilter_forward: ONE launch, never synchronises except to grow the lengths scratch.  Every check is made before it: FDM_ERR_ARG
 *   (a null pointer, y overlapping x), FDM_ERR_SHAPE (B < 1, L_max < 1, a length outside [1, L_max]).  fdm_version() keeps its value:
 *   callers detect the feature by the symbol.
 * Not built: asymmetric taps or velocity outputs, fp16 in or out, filtering after the frame-rate step, a filter per request.  Call
 *   times: profiles/time_filter/README.md.
 *
 * The recurrences: a one-pole low-pass (FDM_TFILTER_EMA) and the One Euro filter (FDM_TFILTER_ONE_EURO;
 * Casiez, Roussel, Vogel, CHI 2012: a one-pole low-pass whose cutoff rises with the smoothed speed of the vertex, so a slow vertex is
 * smoothed hard and a fast one passes almost untouched), causal with a state carried from call to call, or zero-phase.  Same x, lens,
 * strength rule, zero rows and no-overlap rule as above; every operation is one fp32 operation rounded on its own.
 * Constants, fdm_tfilter_recur_coeffs_host (device-free) -> coeffs [FDM_TFILTER_NCOEFF] = {k, c0, be, cd, fr, ad, a0, 0}:
 *   k = (float)(fps / (2 pi)) with the division in fp64; c0 = (float)cutoff (ema) or (float)min_cutoff; be = (float)beta;
 *   cd = (float)d_cutoff; fr = (float)fps; ad = cd / (cd + k) and a0 = c0 / (c0 + k) in fp32.  For FDM_TFILTER_EMA beta and d_cutoff
 *   are not read and be = cd = ad = 0.  Cutoffs are in Hz, > 0; fps > 0; beta >= 0, in Hz per (mesh unit per second): a sensible value
 *   depends on the mesh's scale.  What any setting does to perceptual quality or lip-sync metrics is UNMEASURED.
 * ema, per column:  y_0 = x_0;  y_t = y_{t-1} + a0 (x_t - y_{t-1}).
 * one_euro, per vertex (its three columns):  y_0 = x_0, dh_0 = 0;  for t >= 1, per column:  dx = (x_t - x_{t-1}) fr,
 *   dh_t = dh_{t-1} + ad (dx - dh_{t-1});  per vertex:  s = sqrt((dh.x dh.x + dh.y dh.y) + dh.z dh.z), fc = c0 + be s, a = fc / (fc + k);
 *   per column:  y_t = y_{t-1} + a (x_t - y_{t-1}).  x_{t-1} is the raw input, as in the paper.  A constant comes back bit for bit.
 * FDM_TFILTER_CAUSAL: f = y (it lags).  FDM_TFILTER_ZERO_PHASE: the causal filter, then the same causal filter over the result walked
 *   from frame L - 1 down to 0, starting afresh, each clip at its own L: flip(causal(flip(causal(x)))).
 * Strength: s_v == 0 copies the input bits, otherwise out = x + s_v (f - x) against the ORIGINAL x (under zero-phase once, after the
 *   second walk); the recurrence itself always runs on the unblended f.
 * fdm_tfilter_create_recur returns an fdm_tfilter: fdm_tfilter_forward (one launch, 1 <= L_b <= L_max) and fdm_tfilter_destroy serve
 *   both families.  FDM_ERR_ARG: an unknown kind or direction, a coefficient that is not finite, k, c0 or fr <= 0, be < 0, for one_euro
 *   cd or ad <= 0, a strength outside [0, 1], a null pointer.
 * fdm_tfilter_forward_state (causal only; FDM_ERR_ARG on an FIR object or on zero-phase): per clip seen [B] DEVICE ints (frames consumed
 *   so far, 0 = fresh) and st [B][3][N] DEVICE fp32 (y_prev, x_prev, dh; ema reads and writes row 0 alone).  0 <= L_b <= L_max.  A clip with
 *   seen > 0 continues exactly as if the frames had been contiguous: the chunks of a recording give the bits of the whole recording.  The
 *   state is written back and L_b added to seen (a second small launch); a clip with L_b == 0 is untouched, its state included.
 *   Nothing is read back.  Zero both arrays to start afresh.
 * fdm_tfilter_set_prefetch: how many frames the walk loads ahead (1, 4, 8 or 16; 16 unless set).  A tuning knob: no bit depends on it. */
#define FDM_TFILTER_GAUSSIAN 0
#define FDM_TFILTER_SAVGOL 1
#define FDM_TFILTER_MIRROR 0
#define FDM_TFILTER_NEAREST 1
#define FDM_TFILTER_EMA 0
#define FDM_TFILTER_ONE_EURO 1
#define FDM_TFILTER_CAUSAL 0
#define FDM_TFILTER_ZERO_PHASE 1
#define FDM_TFILTER_NCOEFF 8
typedef struct fdm_tfilter fdm_tfilter;
int fdm_tfilter_taps_host(int kind, int radius, double param, double* taps /*[radius + 1]*/);
int fdm_tfilter_create(int V, int radius, const float* taps, const float* strength /*[V] or NULL*/, int edge, void* stream, fdm_tfilter** out);
int fdm_tfilter_forward(fdm_tfilter* f, const float* x, const int* lens /*HOST [B] or NULL*/, int B, int L_max, float* y);
int fdm_tfilter_destroy(fdm_tfilter* f);
int fdm_tfilter_recur_coeffs_host(int kind, double fps, double cutoff_or_min_cutoff, double beta, double d_cutoff, float* coeffs /*[FDM_TFILTER_NCOEFF]*/);
int fdm_tfilter_create_recur(int V, int kind, const float* coeffs /*[FDM_TFILTER_NCOEFF]*/, const float* strength /*[V] or NULL*/, int direction,
                             void* stream, fdm_tfilter** out);
int fdm_tfilter_forward_state(fdm_tfilter* f, const float* x, const int* lens /*HOST [B] or NULL*/, int B, int L_max, float* st /*DEVICE [B][3][3V]*/,
                              int* seen /*DEVICE [B]*/, float* y);
int fdm_tfilter_set_prefetch(fdm_tfilter* f, int depth);

/* ------------------------------------------------------------------------------------------
 * Render hand-off: shaded image frames of the animated mesh.  The definition is this project's own: a
 * pinhole camera, exact integer coverage, a per-pixel maximum of 1 / depth, and a Lambert sum over directional lights.  It is not
 * pyrender's metallic-roughness material; there is no reference renderer to compare images with.  Everything on the device is fp32,
 * every operation rounded on its own, no contraction; dot and cross as in the wrap hand-off above; square roots are correctly rounded.
 * Inputs per call: positions [B, L_max, 3 V] fp32 device (what the mesh, wrap and head hand-offs write, or offsets with a template of 1 or
 *   B rows: p = offset + template, one fp32 add), frames [B] HOST ints (NULL: L_max each), fps_in / fps_out as in fdm_mesh_forward: with
 *   both > 0 and different the positions are resampled by that call's rule (L_out and the taps of fdm_mesh_frames, l0 p[i0] + l1 p[i1]).
 *   Vertex normals are those of fdm_mesh_forward on the same output frame (area-weighted, ascending face index) over the object's faces,
 *   or `normals` [B, L_out_max, V, 3] fp32 device when the caller brings them.
 * The object (HOST arrays at create, not read after the call): faces [F, 3] with fdm_mesh_create's index checks; W, H in 1 .. 4096;
 *   camera = {fx, fy, cx, cy, near, far} with fx, fy > 0 and 0 < near < far; world-to-camera R [3, 3] row-major and t [3]; up to 8
 *   directional lights [n, 4] = {unit direction TOWARDS the light in camera space (| |d|^2 - 1 | <= 1e-4), intensity >= 0}; ambient >= 0;
 *   base [3] >= 0; background [3] in [0, 1].  fdm_render_set_view replaces camera, R, t, lights and ambient without a new create.
 * 1 Vertex (per frame and vertex).  pc = R p + t, each component ((r0 p.x + r1 p.y) + r2 p.z) + t; d = -pc.z (the camera looks down -z);
 *   w = 1 / d; sx = fx (pc.x w) + cx; sy = cy - fy (pc.y w); X = (int)rintf(256 sx), Y = (int)rintf(256 sy): 8 sub-pixel bits.  The vertex
 *   is BAD when any of p, d, sx, sy is not finite, when d <= near or d >= far, or when |rintf(256 sx)| or |rintf(256 sy)| > 2^20.
 *   nc = R n in the same order (no t).
 * 2 Triangle.  One with a bad vertex is dropped: there is NO clipping (a limit: a head in front of the camera never straddles the near
 *   plane; a triangle that does vanishes whole).  A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) in 64-bit ints; A == 0 is dropped; A < 0:
 *   vertices 1 and 2 change places (both sides are drawn) and A = -A.
 * 3 Coverage (exact).  Pixel (x, y) has the centre (px, py) = (256 x + 128, 256 y + 128).  For the oriented triangle the edge function
 *   of a -> b is E = (Xb - Xa)(py - Ya) - (Yb - Ya)(px - Xa) in 64-bit ints; E0 belongs to the edge 1 -> 2, E1 to 2 -> 0, E2 to 0 -> 1
 *   (E0 + E1 + E2 = A).  The pixel is covered when for every edge E > 0, or E == 0 and the edge is a top or a left one: with
 *   (dx, dy) = (Xb - Xa, Yb - Ya), x to the right and y down, dy < 0 (left) or dy == 0 and dx > 0 (top).  Exactly one of an edge and its
 *   reverse qualifies, so two triangles that share an edge cover every pixel of their union once.  Only pixels of the triangle's
 *   box clamped to the viewport are visited.
 * 4 Depth.  l_i = (float)E_i / (float)A (64-bit int to float, round to nearest even, one division); iw = (l0 w0 + l1 w1) + l2 w2 (1 / d
 *   is linear on the screen).  The pixel's fragment is the one with the largest iw; among equal iw the lowest face index: the maximum
 *   of the 64-bit key (bits(iw) << 32) | (0xFFFFFFFF - face).  An iw that is not finite or not > 0 never enters.  A maximum does not
 *   depend on the order of the triangles: a clip's pixels do not depend on the batch, L_max, L_out_max or the chunk.
 * 5 Resolve (per pixel).  No fragment: the background, depth 0, face -1.  Else, with E_i, l_i, iw of the winning face recomputed:
 *   b_i = (l_i w_i) / iw; n = (b0 nc0 + b1 nc1) + b2 nc2 per component; s = dot(n, n); nh = n / sqrtf(s) when s > 0, else 0; nh = -nh
 *   when nh.z < 0 (the far side of a surface is lit like the near one); k = ambient + sum over lights l ascending of
 *   I_l max(0, dot(nh, dir_l)) (max(0, x) = x > 0 ? x : 0); per channel c = base_c k, a NaN c takes the background's channel, c = min(1, c),
 *   u8 = (int)(255 c + 0.5f); the background's channels go through the same two last steps.
 *   rgb [B, L_out_max, H, W, 3] uint8; depth [B, L_out_max, H, W] fp32 = 1 / iw (or NULL); face [B, L_out_max, H, W] int32 (or NULL).
 *   Rows at or past a clip's L_out are zeros in every output; input rows at or past frames[b] are never read.
 * A call works through its live output frames a chunk at a time on `stream`: per-vertex records and the visibility buffer exist for one
 * chunk (one scratch per object, grown when a call needs more; the call that grows waits for the device).  fdm_render_set(r,
 * "chunk_frames", n): n frames per chunk, 0 = the default, the largest chunk whose scratch stays under 256 MB (at least one frame).
 * Anti-aliasing: fdm_render_set(r, "samples", S) with S = 1 (the default: everything above as it stands), 4 or 16 coverage samples per
 *   pixel; any other S, or W H S > 2^26 keys per frame (4096^2 at 4 samples, 2048^2 at 16: 512 MB), is FDM_ERR_ARG.  The sample offsets
 *   (ox_s, oy_s) are integers on the same 256-units-per-pixel grid (fdm_render_sample_pattern_host writes them, no device needed):
 *     S = 1: (128, 128), the pixel centre;  S = 4 (rotated grid), in sample order: (96, 32), (224, 96), (32, 160), (160, 224);
 *     S = 16 (4 x 4 grid): sample s = 4 j + i at (32 + 64 i, 32 + 64 j).
 *   Steps 1 and 2 are unchanged.  Steps 3 and 4 hold per (triangle, pixel, sample) with (px, py) = (256 x + ox_s, 256 y + oy_s): the
 *   same edge functions and top-left rule, the same l_i, iw and key, and every sample keeps the maximum key of its own.  Which pixels a
 *   triangle is tried on is not part of the definition (a conservative box), nor does it show in the output.
 *   Resolve, per pixel: for s ascending the three channels c_s -- a sample with a fragment is shaded as in step 5 from its own l_i and
 *   iw (c = base_c k, a NaN c takes the background's channel, c = min(1, c)), a sample without one takes the background's channel --;
 *   the channel's sum ((c_0 + c_1) + c_2) + ... in fp32, one rounded multiplication by 1 / S (a power of two: exact), then
 *   u8 = (int)(255 c + 0.5f).  depth and face at S > 1 are a choice, made so that both images stay exact and independent of order:
 *   they come from the maximum key over the pixel's samples -- the nearest sampled surface, among equal iw the lowest face index --,
 *   depth = 1 / iw of that key, face its face; 0 and -1 when no sample has a fragment.  The visibility buffer holds 8 W H S bytes per
 *   frame of a chunk, and the default chunk counts them.
 * Planes for compositing and video (fdm_render_forward_planes; fdm_render_forward and everything it writes are unchanged).  `out` names
 *   any of rgb, depth, face (as above), alpha and yuv; a NULL member is not written, and rgb may be NULL too.  Every plane comes out of
 *   the one resolve pass (the keys are cleared as they are read) and no rgb image is written to memory that the caller did not ask for.
 *   alpha [B, L_out_max, H, W] uint8: with n the number of the pixel's S samples that have a fragment (the resolve's own test: a key
 *     that is not 0 and names a face < F), alpha = (255 n + S / 2) / S in integers: 0 or 255 at S = 1; 0, 64, 128, 191, 255 at S = 4.
 *     Alpha is coverage alone: it does not depend on shading, lights or background.  With background = (0, 0, 0) an uncovered sample adds
 *     0 to the channel sums, so rgb is then premultiplied by this coverage and rgb + alpha over black is a premultiplied RGBA frame (no
 *     new rgb mode is needed).  The one caveat: a sample whose shade is NaN takes the background's channel, as in step 5.
 *   yuv [B, L_out_max, 3 W H / 2] uint8, 2-byte aligned, W and H both even (else FDM_ERR_ARG; alpha has no such limit): Y'CbCr 4:2:0,
 *     each frame one contiguous block in the byte order of `ffmpeg -f rawvideo -pix_fmt yuv420p` (I420: Y [H][W], U [H/2][W/2],
 *     V [H/2][W/2]) or `-pix_fmt nv12` (NV12: Y [H][W], then [H/2][W/2][2] interleaved U, V).  The planes are a function of the frame's
 *     uint8 rgb as defined above (step 5 / the multi-sample resolve, after (int)(255 c + 0.5f)), whether or not rgb is stored.  All
 *     arithmetic is 32-bit signed integers, >> an arithmetic shift (floor).  With the ten numbers of fdm_render_yuv_coeffs_host (no
 *     device needed) {yr, yg, yb, ur, ug, ub, vr, vg, vb, y0}:
 *       per pixel        Y = clamp(((yr R + yg G + yb B + 32768) >> 16) + y0, 0, 255);
 *       per 2 x 2 block  Rs, Gs, Bs = the sums of its four uint8 values (0 .. 1020: the largest product sum is 6.7e7),
 *                        U = clamp(((ur Rs + ug Gs + ub Bs + (1 << 17)) >> 18) + 128, 0, 255), V likewise with vr, vg, vb:
 *       chroma sited at the block's centre (C420jpeg in Y4M terms).  Limited range stays in 16 .. 235 (Y) and 16 .. 240 (U, V) over all
 *       2^24 colours; full range reaches 256 for pure blue or red before the clamp.
 *     The numbers: (Kr, Kb) = (0.299, 0.114) for matrix 601, (0.2126, 0.0722) for 709; sy = 219 / 255 and sc = 224 / 255 for limited
 *       range, both 1 for full range; q(x) = floor(65536 x + 0.5) in fp64; yr = q(Kr sy), yb = q(Kb sy), yg = q(sy) - yr - yb;
 *       ub = q(sc / 2), ur = q(-Kr sc / (2 (1 - Kb))), ug = -(ur + ub); vr = q(sc / 2), vb = q(-Kb sc / (2 (1 - Kr))), vg = -(vr + vb);
 *       y0 = 16 limited, 0 full.  The green terms follow from the other two, so white, black and every grey are exact.
 *         601 limited  16829 33039 6416  -9714 -19070 28784  28784 -24103 -4681  16
 *         601 full     19595 38470 7471 -11058 -21710 32768  32768 -27439 -5329   0
 *         709 limited  11966 40254 4064  -6596 -22188 28784  28784 -26145 -2639  16
 *         709 full     13933 46871 4732  -7509 -25259 32768  32768 -29763 -3005   0
 *     fdm_render_set keys: "yuv_matrix" 601 or 709 (default 709), "yuv_range" 0 limited or 1 full (default 0), "yuv_layout" 0 I420 or
 *       1 NV12 (default 0); any other value is FDM_ERR_ARG.
 *   Rows at or past a clip's L_out are zero bytes in alpha and yuv as in every other output (zeros, not video black).  The call keeps
 *   fdm_render_forward's checks, chunks, scratch and one-stream rule; a null `out`, or one whose five members are all null, is FDM_ERR_ARG.
 * Materials (fdm_render_set_material).  A material is state of the object; it decides the colour m that stands
 *   where `base` stands in step 5: c = m_c k.  Coverage, depth, keys, ties, the sample patterns, the NaN-takes-background rule, min(1, c),
 *   the sample sum, the rounding to uint8, alpha, the yuv planes, depth, face, chunks and the clearing of the visibility buffer are as
 *   above; an object with no material set runs the code it ran before and gives the same bytes.  b_i = (l_i w_i) / iw are step 5's
 *   weights; "interpolated" means (b0 a0 + b1 a1) + b2 a2, each operation rounded, with the corners in the ORIENTED triangle's order:
 *   where A < 0 swapped vertices 1 and 2, the attributes of corners 1 and 2 swap with them, as the normals do.
 *   kind 0, base: m = base.
 *   kind 1, vertex colours: colors [V, 3] fp32, finite and >= 0, fixed per object; m_c is the interpolated colour.
 *   kind 2, scalar map: lut [n_lut, 3] fp32, 2 <= n_lut <= 1024, finite and >= 0; lo < hi, both finite, span = hi - lo rounded once to
 *     fp32 on the host (finite); per call scalars [B, L_max, V] fp32 device on the INPUT frames, resampled to the output frames as the
 *     positions are (l0 s[i0] + l1 s[i1] with fdm_mesh_frames' taps, no template; rows at or past frames[b] are never read).  Per vertex
 *     of an output frame u_v = fmin(fmax((s_v - lo) / span, 0), 1), fmax and fmin returning the operand that is not NaN, so a NaN scalar
 *     gives u = 0.  Per fragment: u interpolated, clamped to [0, 1] again the same way; x = u (float)(n_lut - 1); i = min((int)x, n_lut - 2);
 *     f = x - (float)i; m_c = lut[i][c] + f (lut[i + 1][c] - lut[i][c]).  The scalar is interpolated and then mapped, not the colours,
 *     so isolines are straight across a triangle.
 *   kind 3, texture: uv [F, 3, 2] fp32, one (u, v) pair per face corner (seams need no vertex splitting), any bits allowed; texture
 *     [tex_h, tex_w, 3] uint8, 1 <= tex_w, tex_h <= 8192, row 0 at the top; filter 0 nearest or 1 bilinear.  tu, tv are interpolated.  A
 *     texel channel is (float)u8 / 255.f (a rounded division).  Bilinear: x = tu (float)tex_w - 0.5f, y = (1 - tv) (float)tex_h - 0.5f (v
 *     points up, as in FLAME and OpenGL UV sets); x0 = floorf(x), fx = x - x0; the columns are (int)fmin(fmax(x0, 0), tex_w - 1) and the
 *     same of x0 + 1 (clamp to edge), the rows likewise from y0 = floorf(y), fy = y - y0; top = t00 + fx (t01 - t00), bot = t10 + fx
 *     (t11 - t10), m = top + fy (bot - top).  Nearest: column (int)fmin(fmax(floorf(tu tex_w), 0), tex_w - 1), row likewise from
 *     (1 - tv) tex_h.  The clamps are made in float before any conversion: no index leaves the texture for any bits of uv, NaN and
 *     infinities included.  Bilinear: a NaN or infinite coordinate makes fx or fy NaN, hence m NaN, hence the sample takes the
 *     background by step 5's rule.  Nearest has no fx: a NaN coordinate reads column or row 0, an infinite one the edge it points to.  There are no mip levels (a limit): a
 *     minified texture aliases, and samples = 16 is the remedy.
 *   unlit = 1, for any kind: k = 1.0f in place of the Lambert sum (heat maps are usually wanted flat).
 *   fdm_render_set_material(r, m) reads m's HOST arrays during the call and keeps none; NULL or kind 0 with unlit 0: back to base.
 *   FDM_ERR_ARG (the object is left as it was): a null r, an unknown kind or filter, unlit not 0 or 1, a null array that the kind needs,
 *   n_lut or a texture size out of range, lo >= hi, lo, hi, span, a colour or a table entry not finite, a negative colour or table entry.
 *   Without a device the set validates and a later forward ends in FDM_ERR_STATE.  The call waits for the device before it frees the
 *   tables it replaces.  fdm_render_forward and fdm_render_forward_planes draw objects of kinds 0, 1 and 3 (the material is object
 *   state); on a kind-2 object they return FDM_ERR_STATE.  fdm_render_forward_material is fdm_render_forward_planes with one more
 *   argument, scalars: FDM_ERR_ARG when it is null on a kind-2 object or not null on an object of another kind; u per (chunk row,
 *   vertex) is 4 V more bytes of scratch per frame, counted in the default chunk.
 * fdm_op_vertex_dist(a, b, out, rows, V, stream): out[r, v] = sqrtf((dx dx + dy dy) + dz dz) of a - b over [rows, 3 V] fp32 device, each
 *   operation rounded, the square root correctly rounded: a per-vertex error field for a scalar map, made on the device.  FDM_ERR_ARG: a
 *   null operand; FDM_ERR_SHAPE: rows or V < 1; FDM_ERR_STATE: no device.
 * Not built: the metallic-roughness material, clipping, mip levels, normal maps, per-frame vertex colours, 4:2:2 / 4:4:4 or 10-bit
 *   output, video encoding.
 * fdm_render_create validates without a device and fdm_render_forward then ends in FDM_ERR_STATE.  Every check is made before the first
 * launch: FDM_ERR_ARG (a null r / positions / rgb, tmpl_rows not 0, 1 or B, a null template with tmpl_rows > 0, frame rates not finite
 * or negative; at create and set_view: a null array, F or V < 1, a face index outside [0, V), W or H outside 1 .. 4096, more than 8
 * lights, a light direction that is not a unit vector, near >= far, anything not finite; in fdm_render_set an unknown key -- the keys
 * are chunk_frames, samples, yuv_matrix, yuv_range and yuv_layout --, chunk_frames outside 0 .. 4096, samples or a yuv_* value as
 * above; in the planes form rgb may be null, and a null out, five null members, yuv with an odd W or H or an odd yuv address are
 * refused), FDM_ERR_SHAPE (B, L_max or L_out_max < 1, frames[b] outside [0, L_max], a clip whose L_out exceeds L_out_max).
 * frames_out [B] HOST (or NULL) receives L_out per clip.  An object serves one stream at a time.  fdm_version() keeps its value: callers
 * detect the feature by the symbol.  Call times are unmeasured: profiles/render_out/README.md. */
typedef struct fdm_render fdm_render;
int fdm_render_create(const int* faces, int F, int V, int W, int H, const float* camera /*[6]*/, const float* R /*[9]*/, const float* t /*[3]*/,
                      const float* lights /*[n_lights,4] or NULL*/, int n_lights, float ambient, const float* base /*[3]*/,
                      const float* background /*[3]*/, fdm_render** out);
int fdm_render_set_view(fdm_render* r, const float* camera, const float* R, const float* t, const float* lights, int n_lights, float ambient);
int fdm_render_set(fdm_render* r, const char* key, long long value);
/* The sample offsets of `samples` = 1, 4 or 16 into xy [samples][2] HOST ints (no device needed); FDM_ERR_ARG for any other count or
 * a null xy.  Callers detect multi-sample rendering by this symbol. */
int fdm_render_sample_pattern_host(int samples, int* xy);
int fdm_render_forward(fdm_render* r, const float* positions, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows, double fps_in,
                       double fps_out, const float* normals /*or NULL*/, unsigned char* rgb, float* depth /*or NULL*/, int* face /*or NULL*/,
                       int L_out_max, int* frames_out, void* stream);
/* The planes form (the paragraph "Planes for compositing and video" above).  Callers detect it by the symbol. */
typedef struct fdm_render_planes {      /* any may be NULL, not all */
  unsigned char* rgb; float* depth; int* face; unsigned char* alpha; unsigned char* yuv;
} fdm_render_planes;
int fdm_render_forward_planes(fdm_render* r, const float* positions, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows,
                              double fps_in, double fps_out, const float* normals /*or NULL*/, const fdm_render_planes* out, int L_out_max,
                              int* frames_out, void* stream);
/* {yr, yg, yb, ur, ug, ub, vr, vg, vb, y0} of matrix = 601 or 709 and full_range = 0 or not into coeffs [10] HOST ints (no device
 * needed); FDM_ERR_ARG for any other matrix or a null coeffs. */
int fdm_render_yuv_coeffs_host(int matrix, int full_range, int* coeffs /*[10]*/);
/* Materials (the paragraph "Materials" above).  Callers detect them by the symbol. */
typedef struct fdm_render_material {
  int kind;                                   /* 0 base, 1 vertex colours, 2 scalar map, 3 texture */
  int unlit;
  const float* colors;                        /* HOST [V, 3], kind 1 */
  const float* lut; int n_lut; float lo, hi;  /* HOST [n_lut, 3], kind 2 */
  const float* uv;                            /* HOST [F, 3, 2], kind 3 */
  const unsigned char* texture;               /* HOST [tex_h, tex_w, 3], kind 3 */
  int tex_w, tex_h, filter;                   /* filter: 0 nearest, 1 bilinear */
} fdm_render_material;
int fdm_render_set_material(fdm_render* r, const fdm_render_material* m /* NULL or kind 0: back to base */);
int fdm_render_forward_material(fdm_render* r, const float* positions, const int* frames, int B, int L_max, const float* tmpl, int tmpl_rows,
                                double fps_in, double fps_out, const float* normals /*or NULL*/, const fdm_render_planes* out, int L_out_max,
                                int* frames_out, void* stream, const float* scalars /* DEVICE [B, L_max, V] or NULL */);
int fdm_op_vertex_dist(const float* a, const float* b, float* out, int rows, int V, void* stream);
int fdm_render_destroy(fdm_render* r);

/* Host-side tables (no device needed): the 12 GaussianDiffusion buffers in registration order, T floats each
 * (diffusion_BIWI_encoder_decoder.py:565-603: cosine schedule in fp64, fp32 cast); DDIM pairs and per-pair coefficients
 * (:684-708, eta = 0; returns the number of live pairs, the dead (t, -1) pair excluded); get_slopes (models/fdm_vocaset.py:96-106);
 * the positional tables (:150-184). */
int fdm_schedule_host(int T, float* out12);
int fdm_ddim_schedule_host(int steps, int T, int* t, int* t_next, float* sqrt_an, float* c_n);
/* Tables of the table-driven sampler (fdm_sample_args kind 2 / fdm_sched_args mode 3): `steps` entries of t, a, b, c, s each, fp64
 * math on the cosine schedule of fdm_schedule_host, fp32 cast.  Schedule overrides given to a plan ("sched.*") do not apply here.
 * Grid: the reference's own, reversed(linspace(-1, T-1, steps+1).astype(int32)), and ALL `steps` pairs are executed: for the last
 * pair (t_last, -1) alpha_bar(-1) := 1, i.e. a = 0, b = 1, c = 0, s = 0 -- the sampler ends in data (its output is the last x0
 * prediction), unlike the reference's DDIM, which skips that pair and returns a latent still at t_last.
 * With alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln(alpha / sigma), h_k = lambda(t_next) - lambda(t),
 * phi_k = alpha_next (1 - exp(-h_k)):
 *   FDM_SAMPLER_DPMPP_2M (DPM-Solver++ 2M, Lu et al. 2022; eta must be 0): a = sigma_next / sigma, s = 0; first step and final pair:
 *     b = phi, c = 0; otherwise with r = h_{k-1} / h_k: b = phi (1 + 1 / (2 r)), c = -phi / (2 r).
 *   FDM_SAMPLER_DDIM (Song et al. 2020, eta in [0, 1]): sigma_k = eta sqrt((1 - abar_n) / (1 - abar)) sqrt(1 - abar / abar_n),
 *     a = sqrt(1 - abar_n - sigma_k^2) / sqrt(1 - abar), b = sqrt(abar_n) - a sqrt(abar), c = 0, s = sigma_k.
 * FDM_ERR_ARG: steps < 1, steps > T, eta outside [0, 1] (or != 0 for 2M), unknown kind, a NULL output.  What 20 such steps do to
 * perceptual quality on trained checkpoints is unmeasured here. */
#define FDM_SAMPLER_DPMPP_2M 0
#define FDM_SAMPLER_DDIM 1
int fdm_sampler_tables_host(int kind, int steps, int T, double eta, int* t, float* a, float* b, float* c, float* s);
int fdm_alibi_slopes_host(int n_head, float* out);
int fdm_pe_table_host(int d, int periodic, int period, int rows, float* out);
/* Tables of the audio front end (fdm_frontend_*): the resampling ratio of `rate` -> 16 kHz (up = 16000 / gcd, down = rate / gcd;
 * FDM_ERR_ARG: rate < 1 or a NULL output, FDM_ERR_SHAPE: max(up, down) > 2048); n_out = ceil(frames * up / down) in 64 bits (negative:
 * the same errors, or frames < 1); the 20 max(up, down) + 1 taps in double, I0 by its power series (returns their count). */
int fdm_resample_ratio_host(int rate, int* up, int* down);
long long fdm_resample_len_host(int rate, long long frames);
int fdm_resample_taps_host(int up, int down, double* taps);

#ifdef __cplusplus
}
#endif
#endif
