// Which kernel a GEMM launch gets, host side only (no device code: gemm.hpp instantiates from it, tune.hip and fdm_hip.hip read it):
// the tile table, the retired ids, the heuristic and the resolver.  What an FDM_TILE_* id means is written here and nowhere else.
#pragma once
#include <cstdlib>
#include <initializer_list>

#include "../../include/fdm_hip.h"

namespace fdm {

// ---- the tile table ------------------------------------------------------------------------------------------------------
enum : unsigned { TILE_KSPLIT = 1, TILE_BATCH2 = 2, TILE_SCHED = 4 };      // launch forms beside the plain one (GemmTile::can)
struct GemmTile {
  int id;
  int bm, bn, wm, wn;      // output tile per workgroup, compute waves along M and N
  int lw;                  // loader waves of the 16-bit kinds (gemm.hpp: gemm_depth_launch); the ping-pong loop has none
  bool pp;                 // main loop: the ping-pong loop; else the LDS-DMA ring
  int nst, nst_many;       // one-plane kinds: ring stages while the grid is at most 256 workgroups (one round), and beyond
  int kch;                 // 16-byte chunks per row of a ring stage
  int nst2;                // two-plane kinds: ring stages (a stage is twice as large, hi and lo planes of both operands)
  int split_id;            // the live id a two-plane launch of this id runs
  unsigned can;            // TILE_KSPLIT: K-sliced launches, TILE_BATCH2: a second batch level, TILE_SCHED: the scheduler-fused decoder
};
// In the order the tuner times them (tune.hip: of two equal timings the earlier candidate wins).
constexpr GemmTile kGemmTiles[] = {
    {FDM_TILE_64x64, 64, 64, 2, 4, 4, false, 4, 4, 8, 4, FDM_TILE_64x64, TILE_KSPLIT | TILE_BATCH2 | TILE_SCHED},      // 8 waves, 32x16 per wave; 64 KB ring (split kinds 128 KB)
    {FDM_TILE_64x64_S2, 64, 64, 2, 4, 4, false, 2, 2, 8, 2, FDM_TILE_64x64_S2, TILE_KSPLIT | TILE_BATCH2},             // 32 KB -> 4 workgroups per CU (split kinds 64 KB -> 2)
    {FDM_TILE_32x64_S3, 32, 64, 2, 2, 2, false, 3, 3, 8, 3, FDM_TILE_32x64_S3, TILE_KSPLIT},                           // 4 waves, 16x32 per wave, 36 KB (split kinds 72 KB -> 2 workgroups per CU)
    // 8 waves, 32x32 per wave; 4-stage ring (96 KB, one per CU) while the grid is one round, beyond that the 3-stage ring (72 KB): two
    // workgroups per CU; split kinds 144 KB.
    // (Round 6, measured and not adopted: four compute waves of 64x32 instead of eight of 32x32 beyond one round -- fewer fragment bytes read
    //  from LDS per staged byte -- is 7-11 % faster on the isolated QKV / FFN1 shapes at 1992 rows with a plain epilogue and 1-1.7 % SLOWER
    //  inside cfg5's step program and HuBERT-large, where the epilogue's residual / packed-K,V operands share the registers:
    //  profiles/r6_loop_ablation/.)
    {FDM_TILE_128x64, 128, 64, 4, 2, 4, false, 4, 3, 8, 3, FDM_TILE_128x64, TILE_BATCH2},
    {FDM_TILE_128x128, 128, 128, 2, 4, 4, false, 3, 3, 8, 2, FDM_TILE_128x128, 0},      // 8 waves, 64x32 per wave; split kinds 128 KB, one tile in flight
    {FDM_TILE_80x128, 80, 128, 1, 8, 4, false, 4, 4, 8, 3, FDM_TILE_80x128, 0},         // 8 waves, 80x16 per wave: 800 rows x 3072 = 240 workgroups; split kinds 156 KB
    {FDM_TILE_64x128, 64, 128, 2, 4, 4, false, 4, 4, 8, 3, FDM_TILE_64x128, 0},         // 8 waves, 32x32 per wave; split kinds 144 KB
    // ping-pong loop, 64x64 per wave, 146 KB; one-plane kinds only (the split kinds run the nearest member of their set)
    {FDM_TILE_256x128_PP, 256, 128, 4, 2, 0, true, 3, 3, 8, 0, FDM_TILE_128x128, TILE_SCHED},
};
// Retired ids (still accepted) and the live id each one runs; an id in neither list runs FDM_TILE_64x64, as FDM_TILE_64x64_S3 does.
constexpr int kGemmRetiredTiles[][2] = {
    {FDM_TILE_96x128, FDM_TILE_128x128},         // nearest member
    {FDM_TILE_256x128, FDM_TILE_256x128_PP},     // the lockstep loop on this tile
    {FDM_TILE_64x64_S3, FDM_TILE_64x64},
    {FDM_TILE_128x64_S3, FDM_TILE_128x64},       // the tile picks its ring depth
};

constexpr const GemmTile* gemm_tile_find(int id) {
  for (const GemmTile& t : kGemmTiles)
    if (t.id == id) return &t;
  return nullptr;
}
constexpr const GemmTile& gemm_tile(int live_id) { return *gemm_tile_find(live_id); }
// whether `id` can run the launch forms `forms` (a retired id runs none of them but the plain one)
constexpr bool gemm_tile_can(int id, unsigned forms) { return gemm_tile_find(id) && (gemm_tile_find(id)->can & forms) == forms; }
// the live id that a launch asking for `id` runs on a kind with `split` (two-plane) operands
constexpr int gemm_tile_runs(int id, bool split) {
  if (!gemm_tile_find(id)) {
    int live = FDM_TILE_64x64;
    for (auto& r : kGemmRetiredTiles)
      if (r[0] == id) live = r[1];
    id = live;
  }
  return split ? gemm_tile(id).split_id : id;
}

// ---- tile choice -------------------------------------------------------------------------------------------------------
// fdm_gemm_args.tile (the caller's plan-time choice; FDM_TILE_GENERAL may be or-ed in), else the FDM_GEMM_TILE override (env, read
// once: the FDM_TILE_* value forced for every GEMM, for A/B measurements), else the heuristic below: gemm_heuristic_tile names the FDM_TILE_* a launch
// with tile = 0 resolves to (gemm_requested_tile with tile = 0 is exported as fdm_gemm_heuristic_tile).  Every tile accumulates k in
// the same order: the choice changes speed, never results.
static int gemm_tile_override() {
  static int v = [] { const char* e = getenv("FDM_GEMM_TILE"); return e ? atoi(e) : 0; }();
  return v;
}
static bool gemm_one_round(long long tiles) { return tiles > 192 && tiles <= 256; }
// 80x128 tiles that fill the chip in exactly one round (225..256 workgroups, e.g. 800 rows x 3072 columns = 240): every CU
// streams one (80 + 128)-row operand pair instead of two or three 64x64 ones (12.7 vs 14.6 us bf16, 22.2 vs 28.4 us f16x3
// on that shape; profiles/README.md round 3)
static bool gemm_one_round_80(const fdm_gemm_args& a) {
  const long long t80 = (long long)((a.M + 79) / 80) * ((a.N + 127) / 128) * (a.batch > 0 ? a.batch : 1);
  return t80 > 224 && t80 <= 256 && (a.M % 80 == 0 || a.M % 80 > 40);   // (a mostly empty last row tile wastes the round)
}

// 64x128 tiles that fill the chip in exactly one round for a wide projection (FFN1 at the step's 800 rows: 13 x 16 = 208 workgroups): with
// loader waves (round 5) the k loop runs at the CU's L2 -> LDS rate, so the tile with fewer bytes per CU wins -- 8.45 us against 9.71 for two
// co-resident 64x64 tiles per CU in bf16, 14.9 against 18.7 in f16x3 (profiles/r5_ldw/isolated.txt)
static bool gemm_one_round_64x128(const fdm_gemm_args& a) {
  const long long t = (long long)((a.M + 63) / 64) * ((a.N + 127) / 128) * (a.batch > 0 ? a.batch : 1);
  return gemm_one_round(t) && a.N >= 2048 && a.N % 128 == 0;
}

// elem_bytes: 4 (fp32) or 2; split: the two-plane kinds (a ring stage is twice as large there, so their tile set is the part
// of the one-plane set whose ring fits 160 KB of LDS)
static int gemm_heuristic_tile(const fdm_gemm_args& a, int elem_bytes, bool split) {
  if (a.batch2 >= 1) {       // grouped conv over clips: 128-row tiles once they fill the chip (one round of 256: 4 row tiles x 16 groups x 4 clips), else 64
    const long long t128b = (long long)((a.M + 127) / 128) * ((a.N + 63) / 64) * (a.batch > 0 ? a.batch : 1) * a.batch2;
    return t128b >= 192 ? FDM_TILE_128x64 : FDM_TILE_64x64;
  }
  const long long batch = a.batch > 0 ? a.batch : 1;
  const long long t128 = (long long)((a.M + 127) / 128) * ((a.N + 127) / 128) * batch;
  const long long t128x64 = (long long)((a.M + 127) / 128) * ((a.N + 63) / 64) * batch;
  const long long t64 = (long long)((a.M + 63) / 64) * ((a.N + 63) / 64) * batch;
  const long long t64x128 = (long long)((a.M + 63) / 64) * ((a.N + 127) / 128) * batch;
  // Round 5 (the loop runs at the CU's L2 -> LDS rate: fewer bytes on the busiest CU wins; rules from the tuner's picks over 66 shapes on
  // the loader-wave build, profiles/r5_tile_sweep/):
  //  * narrow outputs (N <= 512: MEAD's out-proj / FFN2 / decoder at 2400-4000 rows) whose 64x64 grid needs two workgroups per CU or two
  //    rounds while the 64x128 grid is one round: 64x128 (-4...-8 % on those chains)
  const bool narrow_one_round = elem_bytes == 2 && a.N <= 512 && a.N % 128 == 0 && t64 > 256 && t64x128 <= 256;
  //  * a few hundred rows and a wide projection whose 128x64 grid is (nearly) one round: 128x64 instead of two co-resident 64x64 tiles
  //    per CU (QKV at 400-600 rows, FFN1 at 600: -2.5...-4 %)
  const bool wide_128x64 = elem_bytes == 2 && a.M <= 1024 && a.N >= 2048 && t128x64 >= 160 && t128x64 <= 256;
  if (!split) {
    // Measured on MI355X (profiles/README.md): the biggest tile wins only once it still yields >= 2 blocks per CU;
    // below that the 64x64 tile's extra blocks beat its higher L2->LDS traffic.
    constexpr long long thr128 = 512, thr128x64 = 700;
    const long long t256 = (long long)((a.M + 255) / 256) * ((a.N + 127) / 128) * batch;
    // thousands of rows: the ping-pong loop on the 256x128 tile (the tuner's pick for the N <= 2048 sites from 6400 rows and
    // for FFN1 from 3200; `profiles/r3_rows_sweep`, `r3_tile_sweep`; bf16 only, whole column tiles)
    const bool pp_ok = elem_bytes == 2 && a.N % 128 == 0 && a.K >= 1024;
    if (pp_ok && a.M >= 6000 && a.N <= 2048 && t256 >= 150) return FDM_TILE_256x128_PP;
    // a wide projection whose 256x128 grid is exactly one round (HuBERT's FFN1 at 4 x 10 s: 1992 x 4096 = 8 x 32 tiles; 29.6 us
    // against 33.3 on the 512 tiles of 128x128, profiles/r4_pmc_hubert; the lockstep 256x128 kernel of rounds 2-4 measured 29.9 against
    // 29.4 for the ping-pong loop there and is retired: profiles/r5_xcd_band/gemm_tiles_hubert_ffn.txt)
    if (elem_bytes == 2 && a.M > 1024 && t128 >= thr128 && gemm_one_round(t256)) return FDM_TILE_256x128_PP;
    if (t128 >= thr128) {
      // 128x128 unless its last round is less than half full (600 tiles = 2.34 rounds: QKV at 3200 rows, MEAD's at 6400): 128x64 on the
      // 3-stage ring, two workgroups per CU, balances that tail (-4 % on those chains)
      const long long tail = t128 % 256;
      if (elem_bytes == 2 && t128 < 1024 && tail > 0 && tail < 128) return FDM_TILE_128x64;
      return FDM_TILE_128x128;
    }
    if (gemm_one_round_80(a)) return FDM_TILE_80x128;
    if (elem_bytes == 2 && gemm_one_round_64x128(a)) return FDM_TILE_64x128;
    if (wide_128x64) return FDM_TILE_128x64;
    if (narrow_one_round && a.M > 1024) return FDM_TILE_64x128;
    // one short clip (and MEAD's d = 512 sites up to ~800 rows): 64x64 tiles leave most CUs idle -> 32-row tiles, twice the workgroups
    // (the split kinds have had this rule since round 3; with loader waves it pays in bf16 too: -3.5...-5.5 % on MEAD's chains at 200-800 rows)
    if (elem_bytes == 2 && t64 <= 128 && a.N <= 1536) return FDM_TILE_32x64_S3;
    // (measured in bf16 only: the fp32 kind keeps its rules; short-K products whose 64x64 grid is resident in one round -- two
    //  64 KB rings per CU -- stay on it: MEAD's d = 512 sites at 1200-1600 rows lost 3-5 % on larger tiles)
    if (elem_bytes == 2 && a.M > 1024 && (t64 > 512 || a.K >= 1024)) {
      // 1100..4000 rows (batched clips, long clips, CFG): what the plan-time tuner picks there (profiles/r3_tile_sweep/), as rules.
      // A grid that fills the chip in exactly ONE round wins; else 128x64 -- on the 4-stage ring while its grid is one round, on the
      // 3-stage ring (72 KB: two workgroups per CU, all of <= 512 tiles resident) beyond.
      if (gemm_one_round(t128)) return FDM_TILE_128x128;
      if (gemm_one_round(t256)) return FDM_TILE_256x128_PP;
      if (t128x64 > 128) return FDM_TILE_128x64;          // (4-stage ring while its grid is one round, 3-stage beyond: the tile picks)
    }
    if (t128x64 >= thr128x64) return FDM_TILE_128x64;
    return FDM_TILE_64x64;
  }
  if (t128 >= 512) return FDM_TILE_128x128;
  if (gemm_one_round_80(a)) return FDM_TILE_80x128;
  if (gemm_one_round_64x128(a)) return FDM_TILE_64x128;
  if (wide_128x64) return FDM_TILE_128x64;
  if (a.M > 1024) {            // the tuner's picks at 1100..4000 rows as rules (see above)
    if (gemm_one_round(t128)) return FDM_TILE_128x128;
    if (narrow_one_round) return FDM_TILE_64x128;
    if (t128x64 > 128 && t128x64 <= 256) return FDM_TILE_128x64;     // (split kinds: 3-stage, 144 KB ring -- one per CU, so one round only)
    // Beyond the rules (1600+ rows in the split kinds, where every ring is one workgroup per CU): the tile with the fewest operand rows on
    // the busiest CU, rounds x (BM + BN) -- the model the tuner prunes with; it reproduces the tuner's picks at 1600-4800 rows (80x128 for
    // QKV at 1600 and FFN1 at 2400, 128x128 for QKV at 2400: -3.6...-8.6 % on those chains)
    int best = FDM_TILE_64x64; long long best_rows = -1;
    for (int id : {FDM_TILE_64x64, FDM_TILE_128x64, FDM_TILE_64x128, FDM_TILE_80x128, FDM_TILE_128x128}) {
      const GemmTile& c = gemm_tile(id);
      if (a.N % c.bn) continue;
      const long long tiles = (long long)((a.M + c.bm - 1) / c.bm) * (a.N / c.bn) * batch;
      const long long rows = ((tiles + 255) / 256) * (c.bm + c.bn);
      if (best_rows < 0 || rows < best_rows) { best = c.id; best_rows = rows; }
    }
    return best;
  } else {
    // a single short clip: 64x64 tiles leave half the CUs idle -> 32-row tiles (72 KB rings, two per CU); 257..512 tiles of a
    // wide projection: the 2-stage ring (64 KB) keeps all of them resident in one round instead of two
    if (t64 <= 128) return FDM_TILE_32x64_S3;
    // more than one round of 64x64 tiles (one 128 KB ring per CU) where the 64x128 grid is a single round: MEAD's QKV at 800 rows (-6...-8 %)
    if (t64 > 256 && t64x128 <= 256 && a.N % 128 == 0) return FDM_TILE_64x128;
    if (t64 > 256 && t64 <= 512 && a.N >= 2048) return FDM_TILE_64x64_S2;
  }
  if (t128x64 >= 700) return FDM_TILE_128x64;
  return FDM_TILE_64x64;
}

// the scheduler-fused latent decoder has two forms (64x64, ping-pong 256x128): the same rule as its unfused shape
static bool gemm_sched_fuse_heuristic_pp(const fdm_gemm_args& a, int elem_bytes) {
  fdm_gemm_args b = a;
  b.sched_fuse = 0;
  return gemm_heuristic_tile(b, elem_bytes, false) == FDM_TILE_256x128_PP;
}

// K-sliced launches (fdm_gemm_args.ksplit): the 64-column tiles, ring depth by tile id.  With S slices per output tile the grid
// is S times as large and a slice's chain 1 / S as long, so shallower rings (more co-resident slices per CU) are the candidates.
static int gemm_ksplit_heuristic_tile(const fdm_gemm_args& a) { return a.M <= 256 ? FDM_TILE_32x64_S3 : FDM_TILE_64x64; }   // (profiles/r5_splitk/; the tuner's pick at 249 rows on the loader-wave build)

// ---- the resolver ------------------------------------------------------------------------------------------------------
// The id a launch asks for: the caller's, else FDM_GEMM_TILE (plain launches only: K-sliced and second-batch-level launches run on
// their own tile sets), else the heuristic of its form.  May name a retired id, or a tile the split kinds map to another.
static int gemm_requested_tile(const fdm_gemm_args& a) {
  const int id = a.tile & FDM_TILE_ID_MASK, elem_bytes = a.dtype == FDM_F32 ? 4 : 2;
  const bool split = a.dtype == FDM_F16X3;
  if (a.ksplit > 1) {        // (ids outside the K-slice set run 64x64; fdm_op_gemm refuses them)
    const int want = id > 0 ? id : gemm_ksplit_heuristic_tile(a);
    return gemm_tile_can(want, TILE_KSPLIT) ? want : FDM_TILE_64x64;
  }
  if (a.sched_fuse) {        // two forms: 64x64, and the ping-pong tile (one-plane kinds, whole column tiles, no LayerNorm fold) when
                             // the plan's tuner picked it or, for thousands of rows, the heuristic does
    const bool pp = !split && !a.ln_stat_in && a.N % 128 == 0 &&
                    (id == FDM_TILE_256x128_PP || (id == 0 && gemm_tile_override() == 0 && gemm_sched_fuse_heuristic_pp(a, elem_bytes)));
    return pp ? FDM_TILE_256x128_PP : FDM_TILE_64x64;
  }
  const int want = id > 0 ? id : (a.batch2 >= 1 ? 0 : gemm_tile_override());
  return want > 0 ? want : gemm_heuristic_tile(a, elem_bytes, split);
}
// The live id the launch runs: the row of kGemmTiles that gemm_dispatch instantiates its kernel from.
static int gemm_resolve_tile(const fdm_gemm_args& a) { return gemm_tile_runs(gemm_requested_tile(a), a.dtype == FDM_F16X3); }

}  // namespace fdm
