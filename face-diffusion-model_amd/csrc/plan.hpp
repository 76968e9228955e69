// The plan object of the plan layer (include/fdm_hip.h, "Plan layer") and the few functions its units share:
//   plan.hip   commit, workspaces, the step recorder, the program cache, sampling, the plan C ABI
//   tune.hip   plan-time tile tuning, the on-disk tile store, FDM_TILE_OVERRIDE
#pragma once
#include <set>

#include "host.hpp"

struct Fold { fdm::Mat w; float* colsum = nullptr; float* bias = nullptr; const float* gamma = nullptr; const float* beta = nullptr; };

struct fdm_plan {
  fdm_model_desc m{};
  int dtype = FDM_F32, hd = 0;
  fdm::Arena mem, ws, cmem;                  // plan lifetime | per capacity | per commit (freed when weights change)
  std::map<std::string, fdm::Wt> w;          // fp32 weights / buffers by reference state-dict name (plan-owned copies)
  bool committed = false;
  // ---- per model
  std::map<std::string, fdm::Mat> wt;        // operand-kind copies of the step's matrices
  float* tau = nullptr;
  std::vector<float*> TT;
  std::vector<const float*> Wv, bv, Wo, bo;
  bool fuse_ln3 = false;
  std::map<int, Fold> fold;                  // layer l (1 .. n_layers-1) reads norm3 of layer l-1; -1 = latent decoder
  float *slopes = nullptr, *pe = nullptr;
  float *c1 = nullptr, *c2 = nullptr, *sigma = nullptr, *sra = nullptr, *srm1 = nullptr;
  // ---- per shape (capacity cap*, current B, L, ...)
  int capB = 0, capL = 0, capRep = 0;
  int B = 0, L = 0, M = 0, rep = 1, R = 0, Lpad = 0, cfg = 0;     // B = row blocks ("virtual clips") = audio clips x S
  int S = 1;                                 // conditions per audio clip sharing the clip's AF / C1_l tables (fdm_audio_prepare_conds)
  bool prepared = false;
  float *h = nullptr, *h2 = nullptr, *x1 = nullptr, *x0 = nullptr, *x = nullptr, *x2 = nullptr, *stats = nullptr;
  fdm::Mat xt, ht, h2t, x2t, ctx, u;
  void *q = nullptr, *kp = nullptr, *vp = nullptr;
  long long q_lo = 0, kv_lo = 0;             // FDM_F16X3: plane distances of q and of the packed K / V buffers
  size_t kv_bytes = 0;
  float *AF = nullptr, *t1 = nullptr, *sty = nullptr, *em = nullptr, *emu = nullptr, *zeros = nullptr, *E0 = nullptr;
  std::vector<float*> C1;
  int* step = nullptr;                       // [device step counter, t of the current step]
  unsigned long long* seedbuf = nullptr;     // {Philox seed, global index of clip 0}: read by the scheduler at run time
  int* tseq = nullptr; int tseq_cap = 0;
  // table-driven sampler (fdm_sample_args kind 2): device tables [4][lm_cap] (a | b | c | s, uploaded per call) and the fp32 history
  // of the previous step's x0 prediction -- plan layout, sized with the workspaces (a windowed plan keeps its own in long layout)
  float* lm_tab = nullptr; int lm_cap = 0;
  float* x0_hist = nullptr;
  std::map<int, std::pair<int, float*>> ddim;   // ddim_steps -> (live pairs, device [san | cn])
  std::map<int, std::vector<int>> ddim_t;
  // ---- programs and tiles
  std::map<std::string, fdm_prog*> progs;
  std::vector<std::string> prog_order;       // least recently used first
  std::vector<std::string> pinned;           // programs handed out during the current API call: never evicted by it
  std::map<std::string, int> tiles;
  std::map<std::string, std::map<std::string, int>> tile_cache;     // by shape key
  std::map<std::string, long long> steps_seen;
  std::map<std::string, std::vector<fdm_gemm_args>>* tune_rec = nullptr;
  int tune_enabled = 1;
  int tune_failed = 0;                       // opt-in request-path tuning runs that failed (heuristic tiles kept)
  std::set<std::string> tune_failed_shapes;  // ... and their shapes: the request path tries a shape once (fdm_plan_tune retries)
  int want_fuse_ln3 = 0;                     // fdm_plan_set "fuse_ln3": fold norm3 into the GEMMs around it at the next commit
  // K slices of the two GEMMs whose fp32 output row is read next by a LayerNorm launch (out-proj -> LN1+LN2, FFN2 -> LN3): S > 1 = S
  // partial planes of x1, summed by that launch (fdm_gemm_args.ksplit / fdm_ln_args.x_planes).  A property of the plan, NOT of the
  // shape: results depend on S, and a clip must compute the same bits in every batch composition.
  int ksplit_out = 1, ksplit_ffn2 = 1;
  int x1_planes = 0;                 // fp32 planes the workspace's x1 holds (one per K slice)
  int lockstep = 0;                          // fdm_plan_set "lockstep": the lockstep k loop in every GEMM of the step (A/B against the loader-wave form; same bits)
  int tune_lazy = 0;                         // 1: fdm_sample_graph may tune in-call once a shape has run 2000 steps (opt-in)
  long long last_graph_launches = 0, launches_per_step = 0;
  // ---- windowed sampling (fdm_audio_prepare_windows): win_B long clips of win_total latent frames run as the plan's B = win_B * win_n
  // clips ("windows") of L = win_len frames; win_n == 0 = plain mode.  Plan-lifetime buffers, grown on demand (growing drops programs).
  int win_n = 0, win_len = 0, win_total = 0, win_overlap = 0, win_B = 0;
  float* xlong = nullptr; size_t xlong_cap = 0;             // x_t in long layout [win_B, win_total * d]
  float* hist_long = nullptr; size_t hist_long_cap = 0;     // x0_hist of the table-driven sampler in long layout (the blended x0)
  int* win_off = nullptr; size_t win_off_cap = 0;           // CSR of the covering windows per frame (fdm::WinArgs)
  fdm::WinEnt* win_ent = nullptr; size_t win_ent_cap = 0;
  float* win_stage = nullptr; size_t win_stage_cap = 0;     // gathered window audio rows + repeated one-hots (read by the prepare)
  // ---- in-flight batching (fdm_slots_open): the plan's B clips are `slots` SLOTS of L frames, each at its own diffusion step of one
  // shared sampler (or, with a sampler bank, of its own: below); slots == 0 = not in slot mode.  Device: one {k, t, live, run} word and one {seed, clip id} key per slot
  // (plan-lifetime, grown on demand).  Host: a mirror of every slot's status and step count, so no call reads the device words.
  int slots = 0;
  int* slot_state = nullptr; size_t slot_state_cap = 0;
  unsigned long long* slot_keys = nullptr; size_t slot_keys_cap = 0;
  struct SlotHost { int status = 0, done = 0, L = 0, group = -1, sampler = 0, total = 0; };     // status: 0 idle, 1 running, 2 finished (not read yet); group: its long request, -1 = a plain clip; sampler / total: its request's bank row and chain length
  std::vector<SlotHost> slot_host;
  int slot_kind = 0, slot_nsteps = 0, slot_t0 = 0;          // program kind (1 DDPM, 2 DDIM, 3 table-driven), steps per chain, tseq[0]
  int slot_graph_steps = 0, slot_eager = 0;
  float slot_cfg_scale = 0.f;
  const float *slot_san = nullptr, *slot_cn = nullptr;      // DDIM per-step tables of the session
  // ---- long requests in slot mode (fdm_slot_admit_long): a recording longer than a slot occupies a GROUP of slots, one window each,
  // and a range of the long ARENA (its latent and blended-x0 history in long layout).  Capacity is asked for before fdm_slots_open
  // (fdm_plan_set "slot_long_frames" / "slot_long_groups") and reserved there; long_frames == 0 = a session without long capacity,
  // whose program is the plain slot program.  Device tables as fdm_slot_group_args describes them; the host mirrors every group.
  int want_long_frames = 0, want_long_groups = 0;
  int long_frames = 0, long_groups = 0, long_entries = 0;
  float* long_x = nullptr; size_t long_x_cap = 0;
  float* long_hist = nullptr; size_t long_hist_cap = 0;
  fdm::LongFrame* long_frame = nullptr; size_t long_frame_cap = 0;
  fdm::LongEnt* long_ent = nullptr; size_t long_ent_cap = 0;
  fdm::LongGroup* long_group = nullptr; size_t long_group_cap = 0;
  int* slot_member = nullptr; size_t slot_member_cap = 0;
  struct GroupHost { bool used = false; int L_total = 0, first = 0, e0 = 0, ne = 0; std::vector<int> slots; };      // slots[0] = the leader
  std::vector<GroupHost> group_host;
  // ---- samplers per request in slot mode (fdm_slot_sampler_add / fdm_slot_admit_as): a BANK of sampler definitions, sampler 0 = the one
  // given to fdm_slots_open.  Capacity is asked for before fdm_slots_open (fdm_plan_set "slot_samplers" / "slot_sampler_steps") and
  // reserved there; bank_rows == 0 = a session without a bank, whose program is the plain slot program.  Device tables as
  // fdm_slot_bank_args describes them (layout: slots.hpp); the host mirrors every descriptor.
  int want_samplers = 0, want_sampler_steps = 0;
  int bank_rows = 0, bank_t_cap = 0, bank_c_cap = 0;          // descriptors (1 + capacity), timesteps, coefficients of this session
  void* slot_req = nullptr; size_t slot_req_cap = 0;
  int* bank_desc = nullptr; size_t bank_desc_cap = 0;
  int* bank_t = nullptr; size_t bank_t_bytes = 0;
  float* bank_c = nullptr; size_t bank_c_bytes = 0;
  struct SamplerHost { bool used = false; int kind = 0, mode = 0, n_steps = 0, t0 = 0, t_off = 0, c_off = 0, n_c = 0; };      // kind as fdm_sample_args.kind
  std::vector<SamplerHost> sampler_host;
};

namespace fdm {
// ---- plan.hip
std::string shape_key(const fdm_plan* P);                 // key of the prepared shape in tile_cache / steps_seen / the tile store
int drop_programs(fdm_plan* P, void* stream);             // drain, then destroy every recorded program
int record_chain(fdm_plan* P, const fdm_sched_args* sched, void* stream);     // one denoiser pass through fdm_op_*
// ---- tune.hip
bool needs_tune(fdm_plan* P, const std::string& key);     // an untuned shape that has served >= 2000 steps, tuner enabled
int tune_tiles(fdm_plan* P, int force, void* stream);
void tune_soft(fdm_plan* P, void* stream);                // request-path tuning: a failure is counted, never returned
void select_tiles(fdm_plan* P);                           // P->tiles of a freshly prepared shape
}  // namespace fdm
