// Plan-time tile tuning of the plan layer (plan.hpp): the tuner, the tuned sets kept across processes (FDM_TILE_CACHE), FDM_TILE_OVERRIDE.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include <unistd.h>

#include "gemm_tiles.hpp"
#include "plan.hpp"

namespace {
using namespace fdm;

int time_prog(fdm_prog* prog, int warm, int reps, hipStream_t s, float* ms) {
  hipEvent_t e0, e1;
  HIPCK(hipEventCreate(&e0)); HIPCK(hipEventCreate(&e1));
  int rc = fdm_prog_instantiate(prog, s);
  if (rc == FDM_OK) rc = fdm_prog_replay(prog, warm, s);
  if (rc == FDM_OK) {
    (void)hipEventRecord(e0, s);
    rc = fdm_prog_replay(prog, reps, s);
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(ms, e0, e1);
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return rc;
}

// "site=tile,site=tile,...": the text form of a tile set (FDM_TILE_OVERRIDE, the lines of the tile store)
std::vector<std::pair<std::string, int>> parse_tiles(const std::string& v) {
  std::vector<std::pair<std::string, int>> out;
  size_t pos = 0;
  while (pos < v.size()) {
    const size_t comma = v.find(',', pos), eq = v.find('=', pos);
    const size_t end = comma == std::string::npos ? v.size() : comma;
    if (eq != std::string::npos && eq < end) out.push_back({v.substr(pos, eq - pos), atoi(v.substr(eq + 1, end - eq - 1).c_str())});
    pos = end + 1;
  }
  return out;
}

void apply_tile_override(std::map<std::string, int>& tiles) {      // FDM_TILE_OVERRIDE="qkv_ln=5,ffn1=3": force call sites (experiments, pinned profiles)
  if (const char* ov = getenv("FDM_TILE_OVERRIDE"))
    for (auto& kv : parse_tiles(ov)) tiles[kv.first] = kv.second;
}

// ---- tuned tiles kept across processes (opt-in: FDM_TILE_CACHE=<file>).  One text line per (library version, arithmetic mode,
// model geometry, shape): "<key>\t<site>=<tile>,...".  A plan whose shape is in the file takes the stored set at
// fdm_audio_prepare without a single timing launch; fdm_plan_tune / the serving-time tuning of fdm_audio_prepare add their
// result.  Written through a temporary file + rename: concurrent ranks may lose each other's additions, never corrupt the file.
std::string store_key(const fdm_plan* P) {
  const fdm_model_desc& m = P->m;
  char b[160];
  snprintf(b, sizeof(b), "v%d|dt%d|%d,%d,%d,%d,%d,%d,%d,%d|%s", fdm_version(), P->dtype, m.d, m.n_head, m.n_layers, m.ffn, m.G, m.c, m.audio_in, m.pair,
           shape_key(P).c_str());
  return b;
}

bool store_read(std::map<std::string, std::string>& lines) {
  const char* path = getenv("FDM_TILE_CACHE");
  if (!path || !*path) return false;
  std::ifstream f(path);
  std::string ln;
  while (f && std::getline(f, ln)) {
    const size_t tab = ln.find('\t');
    if (tab != std::string::npos) lines[ln.substr(0, tab)] = ln.substr(tab + 1);
  }
  return true;
}

bool store_lookup(const fdm_plan* P, std::map<std::string, int>& tiles) {
  std::map<std::string, std::string> lines;
  if (!store_read(lines)) return false;
  auto it = lines.find(store_key(P));
  if (it == lines.end()) return false;
  tiles.clear();
  for (auto& kv : parse_tiles(it->second)) {
    if (kv.second < 0 || kv.second > FDM_TILE_MAX) return false;      // a damaged line: tune again
    if (kv.second) tiles[kv.first] = kv.second;
  }
  return true;
}

void store_save(const fdm_plan* P, const std::map<std::string, int>& tiles) {
  std::map<std::string, std::string> lines;
  if (!store_read(lines)) return;
  std::string v;
  for (auto& kv : tiles)
    if (kv.second) v += (v.empty() ? "" : ",") + kv.first + "=" + std::to_string(kv.second);
  lines[store_key(P)] = v;
  const std::string path = getenv("FDM_TILE_CACHE"), tmp = path + ".tmp" + std::to_string((long long)getpid());
  {
    std::ofstream f(tmp, std::ios::trunc);
    if (!f) return;                                     // an unwritable location disables the store, never the plan
    for (auto& kv : lines) f << kv.first << '\t' << kv.second << '\n';
  }
  if (rename(tmp.c_str(), path.c_str()) != 0) remove(tmp.c_str());
}

bool tuning_on(const fdm_plan* P) {      // off: heuristic tiles, or the pinned set of FDM_TILE_OVERRIDE
  const char* env = getenv("FDM_TUNE");
  return P->tune_enabled && !(env && !strcmp(env, "0"));
}

int tune_tiles_impl(fdm_plan* P, void* stream) {
  const std::string key = shape_key(P);
  hipStream_t s = (hipStream_t)stream;
  const Kind& kd = kind(P->dtype);
  const bool split = kd.planes == 2;
  FCK(drop_programs(P, stream));
  P->tiles.clear();
  std::map<std::string, std::vector<fdm_gemm_args>> calls;
  {      // dry recording of one pass: captures each call site's arguments, runs nothing
    fdm_prog* dry = nullptr;
    FCK(fdm_prog_create(&dry));
    int rc = fdm_prog_begin(dry);
    P->tune_rec = &calls;
    if (rc == FDM_OK) rc = record_chain(P, nullptr, stream);
    P->tune_rec = nullptr;
    (void)fdm_prog_end(dry);
    fdm_prog_destroy(dry);
    FCK(rc);
  }
  auto timed = [&](const std::vector<fdm_gemm_args>& inst, int tile, float* best) -> int {
    *best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
      fdm_prog* prog = nullptr;
      FCK(fdm_prog_create(&prog));
      int rc = fdm_prog_begin(prog);
      for (size_t i = 0; rc == FDM_OK && i < inst.size(); ++i) { fdm_gemm_args a = inst[i]; a.tile = tile | (P->lockstep ? FDM_TILE_LOCKSTEP : 0); a.incr_counter = nullptr; a.incr_table = nullptr; rc = fdm_op_gemm(&a, stream); }
      (void)fdm_prog_end(prog);
      float ms = 0.f;
      if (rc == FDM_OK) rc = time_prog(prog, 2, 5, s, &ms);
      HIPCK(hipStreamSynchronize(s));
      fdm_prog_destroy(prog);
      FCK(rc);
      if (ms < *best) *best = ms;
    }
    return FDM_OK;
  };
  std::vector<int> cands;      // every kernel of the plan's operand kind, in table order; the ping-pong tile from 1024 rows
  for (const GemmTile& t : kGemmTiles)
    if (gemm_tile_runs(t.id, split) == t.id && !(t.pp && P->R < 1024)) cands.push_back(t.id);
  // Which of them are worth a stopwatch is decided by a wave-quantisation model first.  What bounds these GEMMs is the
  // bytes a CU pulls from L2 into LDS: a BM x BN tile costs (BM + BN) * K * bytes-per-element (x planes)
  // and the busiest CU runs ceil(tiles / 256) of them (the whole grid is resident, or queued behind, at <= 160 KB / ring per CU),
  // on top of a fixed cost per kernel (~5 us: boundary, ring fill, epilogue; in-situ timings of profiles/README.md fit
  // 5 us + bytes / 70 GB/s within ~15 % for tiles up to 128x64; larger tiles run above the model).  Candidates modelled
  // more than 35 % above the best one are not timed.
  auto modelled_us = [&](const fdm_gemm_args& a, int tile) {
    const GemmTile& g = gemm_tile(tile);
    const double planes = kd.planes, eb = kd.bytes;
    const long long tiles = (long long)((a.M + g.bm - 1) / g.bm) * ((a.N + g.bn - 1) / g.bn) * (a.batch > 0 ? a.batch : 1);
    const long long rounds = (tiles + 255) / 256;                                   // tiles on the busiest CU
    const double bytes = (double)rounds * (g.bm + g.bn) * a.K * eb * planes;
    return 5.0 + bytes / 70e3;          // us
  };
  std::map<std::string, int> tuned, runner_up;
  for (auto& kv : calls) {
    std::vector<fdm_gemm_args> inst = kv.second;
    while (inst.size() < 4) { auto c = inst; inst.insert(inst.end(), c.begin(), c.end()); }
    float base = 0.f;
    FCK(timed(inst, 0, &base));
    std::vector<std::pair<float, int>> cand = {{base * 0.97f, 0}};          // switch only for a > 3 % gain over the heuristic
    double best_model = 1e30;
    for (int tile : cands) best_model = std::min(best_model, modelled_us(kv.second[0], tile));
    // the heuristic's own tile is `base`: timing it again as a candidate only lets noise "pick" it (the split kinds alias
    // several ids to one kernel: compare what the ids launch)
    auto launched = [&](int tile) { fdm_gemm_args a = kv.second[0]; a.tile = tile; return gemm_resolve_tile(a); };
    const int heur = launched(0);
    const unsigned form = (kv.second[0].ksplit > 1 ? TILE_KSPLIT : 0) | (kv.second[0].sched_fuse ? TILE_SCHED : 0);
    for (int tile : cands) {
      if (launched(tile) == heur) continue;
      if (!gemm_tile_can(tile, form)) continue;      // K-sliced sites and the scheduler-fused decoder run on their own tile sets
      if (modelled_us(kv.second[0], tile) > 1.35 * best_model) continue;
      float t = 0.f;
      FCK(timed(inst, tile, &t));
      cand.push_back({t, tile});
    }
    std::sort(cand.begin(), cand.end());
    tuned[kv.first] = cand[0].second;
    if (cand.size() > 1 && cand[1].first < cand[0].first * 1.05f) runner_up[kv.first] = cand[1].second;   // settled inside the chain below
  }
  // the isolated timings can mislead (cache state inside the step differs): keep the tuned set only if one whole denoiser
  // pass is faster with it than with the heuristic
  auto chain_time = [&](const std::map<std::string, int>& tiles, float* best) -> int {
    *best = 1e30f;
    for (int rep = 0; rep < 2; ++rep) {
      P->tiles = tiles;
      const int init[2] = {-1, 0};
      HIPCK(hipMemcpyAsync(P->step, init, 8, hipMemcpyHostToDevice, s));
      fdm_prog* prog = nullptr;
      FCK(fdm_prog_create(&prog));
      int rc = fdm_prog_begin(prog);
      if (rc == FDM_OK) rc = record_chain(P, nullptr, stream);
      (void)fdm_prog_end(prog);
      float ms = 0.f;
      if (rc == FDM_OK) rc = time_prog(prog, 2, 4, s, &ms);
      HIPCK(hipStreamSynchronize(s));
      fdm_prog_destroy(prog);
      FCK(rc);
      if (ms < *best) *best = ms;
    }
    return FDM_OK;
  };
  bool any = !runner_up.empty();
  for (auto& kv : tuned) any = any || kv.second != 0;
  std::map<std::string, int> keep;
  if (any) {
    float t_h = 0.f, t_t = 0.f;
    FCK(chain_time({}, &t_h));
    FCK(chain_time(tuned, &t_t));
    for (auto& kv : runner_up) {            // close calls: try the runner-up in place, keep what the chain prefers
      std::map<std::string, int> trial = tuned;
      trial[kv.first] = kv.second;
      float t_a = 0.f;
      FCK(chain_time(trial, &t_a));
      if (t_a < 0.997f * t_t) { tuned = trial; t_t = t_a; }
    }
    if (t_t < 0.99f * t_h) {                    // (below 1 % the chain timing's own spread decides: keep the heuristic set)
      float t_h2 = 0.f;                         // the heuristic chain once more, AFTER the trials: a slow first measurement
      FCK(chain_time({}, &t_h2));               // (clock ramp, cold caches) must not make a neutral set look faster
      t_h = std::min(t_h, t_h2);
    }
    if (t_t < 0.99f * t_h) keep = tuned;
    if (getenv("FDM_TUNE_VERBOSE")) {
      std::string desc;
      for (auto& kv : tuned) desc += kv.first + "=" + std::to_string(kv.second) + ",";
      fprintf(stderr, "[fdm tune] rows=%d candidates: %s chain %.3f -> %.3f ms: %s\n", P->R, desc.c_str(), t_h / 4, t_t / 4, keep.empty() ? "rejected" : "kept");
    }
  }
  P->tiles = keep;
  apply_tile_override(P->tiles);
  P->tile_cache[key] = P->tiles;
  return FDM_OK;
}

}  // namespace

bool fdm::needs_tune(fdm_plan* P, const std::string& key) {      // (a failed request-path tune is not repeated per request)
  return !P->tile_cache.count(key) && tuning_on(P) && P->steps_seen.count(key) && P->steps_seen[key] >= 2000 && !P->tune_failed_shapes.count(key);
}

// Time the candidate output tiles of every GEMM call site of the step at this plan's shapes and keep the fastest.  Cached per
// shape.  Tuning is PLAN-TIME work (it records, instantiates and times dozens of graphs with stream drains in between):
//   force != 0          fdm_plan_tune
//   force == 0          fdm_audio_prepare, for a shape that earlier sampling calls have run >= 2000 steps at (serving)
// fdm_sample_graph itself only counts steps per shape, unless the caller opted in to in-call tuning
// (fdm_plan_set(p, "tune_lazy", 1)).  Every tile accumulates k in the same order, so the choice changes speed only, never results.
int fdm::tune_tiles(fdm_plan* P, int force, void* stream) {
  const std::string key = shape_key(P);
  if (P->tile_cache.count(key) || !tuning_on(P)) return FDM_OK;
  if (!force && !needs_tune(P, key)) return FDM_OK;
  const std::map<std::string, int> before = P->tiles;
  const int rc = tune_tiles_impl(P, stream);
  if (rc != FDM_OK) { P->tiles = before; (void)drop_programs(P, stream); if (!force) P->tune_failed_shapes.insert(key); }   // never leave a trial set behind
  else { store_save(P, P->tiles); P->tune_failed_shapes.erase(key); }
  return rc;
}

// opt-in tuning on a request path: a failure is remembered (fdm_plan_get "tune_failed"), never returned
void fdm::tune_soft(fdm_plan* P, void* stream) {
  if (tune_tiles(P, 0, stream) != FDM_OK) ++P->tune_failed;
}

// The tile set a freshly prepared shape runs with (programs are keyed by the tile set they were recorded with): the shape's tuned
// set, else a set tuned by an earlier process (FDM_TILE_CACHE: counts as tuned), else the heuristic tiles; FDM_TILE_OVERRIDE pins
// tiles with or without the tuner.
void fdm::select_tiles(fdm_plan* P) {
  const std::string key = shape_key(P);
  auto it = P->tile_cache.find(key);
  std::map<std::string, int> want;
  if (it != P->tile_cache.end()) {
    want = it->second;
  } else if (tuning_on(P) && store_lookup(P, want)) {
    apply_tile_override(want);
    P->tile_cache[key] = want;
  } else {
    want.clear();
    apply_tile_override(want);
  }
  P->tiles = want;
}
