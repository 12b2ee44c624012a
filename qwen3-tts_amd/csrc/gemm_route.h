// qt_gemm's planner: which kernel family serves an argument block, and every launch decision that goes with it.
// Pure host arithmetic (C++17, no HIP): gemm_plan() looks at sizes, dtype / epilogue codes and whether pointers are
// null or 16-byte aligned, never at memory.  qt_gemm (gemm.hip) launches what the plan says; qt_gemm_route reports it.
#pragma once
#include "../../include/qwen3tts_amd.h"
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace qt_gemm_impl {

enum class GemmRoute : int {
  NONE = QT_ROUTE_NONE,        // rejected arguments
  IM2COL = QT_ROUTE_IM2COL,    // im2col_k into the workspace, then the linear route `inner` on the image
  GEMV = QT_ROUTE_GEMV,        // gemv_wt: decode rows, or row groups of <= 16 rows
  SK = QT_ROUTE_SK,            // gemm_sk_k: 17..64 rows, every row in one block per column tile
  CONV_N1 = QT_ROUTE_CONV_N1,  // conv_n1_k: one output channel
  WT_1x8 = QT_ROUTE_WT_1x8,    // gemm_wt fallbacks: <= 16 rows / <= 32 rows / any
  WT_2x8 = QT_ROUTE_WT_2x8,
  WT_4x4 = QT_ROUTE_WT_4x4,
  PF2 = QT_ROUTE_PF2,          // gemm_pf2_k: bf16 x bf16 linears, K % 64 == 0
  PF = QT_ROUTE_PF,            // gemm_pf_k: the same linears with K % 64 != 0 or unaligned A
  IGEMM = QT_ROUTE_IGEMM,      // igemm_k: convs and the remaining linears of >= 128 rows
};

// Measurement knobs of the A/B tools (tools/*.sh): the product build runs on these defaults; a probe build fills
// them from the environment once (gemm_knobs() in gemm.hip).
struct GemmKnobs {
  int gemv_fold = 4;        // QT_GEMV_FOLD: 1 disables the row folds of the decode GEMV
  int gemv_u = 0;           // QT_GEMV_U: 4 / 8 forces the k tiles in flight per wave
  int gemv_max_m = 256;     // QT_GEMV_MAX_M: largest row count of the row-group GEMV (QT_SKINNY=0 rule; 16 = decode only)
  int gemv_nt = -1;         // QT_GEMV_NT: 0 / 1 forces non-temporal weight loads off / on
  int gemv_wpb = 0;         // QT_GEMV_WPB: waves-per-block cap
  int gemv_split_auto = 2;  // QT_GEMV_SPLIT_AUTO: the automatic split-K factor
  int gemv_rg = 0;          // QT_GEMV_RG: n forces n row groups, 1 = off, 0 = auto
  int skinny = 1;           // QT_SKINNY: 0 restores the round-2 rule for 17..256 rows
  int sk = 1;               // QT_SK: 0 disables gemm_sk_k
  int sk_max_m = 48;        // QT_SK_MAX_M (48 vs 64: bench --workload vd64 451 vs 442 audio-s/s)
  int im2col = 1;           // QT_IM2COL: 0 disables the im2col route
  // QT_IM2COL_MAX_M (first streamed window at B = 8: 256 rows 1.70 ms, 512 1.39, 1024 1.39, 2048 1.40;
  // profiles/r03_codec_first_window_im2col.txt)
  int im2col_max_m = 1024;
  int igemm_min_m = 128;    // QT_IGEMM_MIN_M: fewest rows of a linear on the LDS-tiled GEMMs
  int igemm_cfg = 0;        // QT_IGEMM_CFG = "NT,MI" as NT * 10 + MI: forces igemm_k's tiling
  int no_igemm = 0;         // QT_NO_IGEMM: 1 keeps large-M GEMMs on gemm_wt
  int pf = 1;               // QT_PF: 0 keeps the bf16 x bf16 linears on igemm_k
  int pf2_split = 1;        // QT_PF2_SPLIT: 0 disables gemm_pf2_k's narrow-output split-K
  int pf2_cfg = 0;          // QT_PF2_CFG = 3 / 4 / 9 / 11 / 21 / 22 / 23 forces a tile configuration
  int pf2_pp = 1;           // QT_PF2_PP: 0 leaves the ping-pong configurations out
};

struct GemmPlan {
  GemmRoute route = GemmRoute::NONE;
  int err = 0;                      // QT_ERR_ARG / QT_ERR_SHAPE / QT_ERR_DTYPE when route == NONE
  GemmRoute inner = GemmRoute::NONE;  // IM2COL: the route of the rewritten linear call; the fields below are its
  int kp = 0;                       // K padded to the weight's k tile (conv: taps * cin_pad)
  int ks = 1, mr = 0, wpb = 0, u = 0, fold = 0, nt_loads = 0;  // GEMV
  int pf2_cfg = 0, pf2_ks = 1;      // PF2, after the cfg 22 -> 21 fallback
  int ntb = 0, mi = 0;              // IGEMM tiling; PF: ntb
  int sk_mi = 0;                    // SK: 16-row tiles
  bool ws_split = false;            // the launch uses the workspace's arrival counters / partial records
};

// The workspace: [0, 16 KiB) arrival counters, then split-K partials / records; the im2col image lives in its upper
// half, so the linear call on the image keeps the lower half for its own split records.
constexpr long long WS_CNT_BYTES = 4096 * (long long)sizeof(unsigned);
constexpr long long IM2COL_WS = 16ll << 20, IM2COL_OFF = 8ll << 20;
constexpr int GEMV_PART = 64 * 4 + 16;  // floats of one GEMV split-K partial
constexpr int PF2_KS_MAX = 4;           // gemm_pf2_k's split-K factor bound (its merge is instantiated up to it)

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// short conv windows (<= 1024 rows: a streamed codec window's stages; tens of rows, K = taps x cin_pad up to ~7k): igemm_k's
// 128-row tiles leave a few dozen blocks each walking hundreds of k chunks (~110-130 us per conv at B = 8 x 1 frame);
// as im2col + the linear routes (decode GEMV / skinny GEMMs / split-K prefill GEMM) the weights stream over the chip.
inline bool im2col_applies(const qt_gemm_args& a, const GemmKnobs& k) {
  if (!k.im2col || a.taps <= 0 || a.w_dtype != QT_BF16 || a.M <= 0 || a.M > k.im2col_max_m || a.rmsnorm ||
      a.gamma != nullptr || a.a_index != nullptr || !a.ws || a.ws_bytes < IM2COL_WS || a.t_out <= 0 ||
      a.cin_pad % 32 || a.cin % 8 || a.splitk == 1)
    return false;
  const long long kp = (long long)a.taps * a.cin_pad;
  return kp <= (IM2COL_WS - IM2COL_OFF) / 2 / a.M && a.M % a.t_out == 0;  // the bf16 image fits its half
}
// the linear call on the bf16 image (prologue already applied by im2col_k)
inline qt_gemm_args im2col_linear_args(const qt_gemm_args& a) {
  qt_gemm_args b = a;
  const int kp = (int)((long long)a.taps * a.cin_pad);
  b.taps = 0; b.A = (const char*)a.ws + IM2COL_OFF; b.a_dtype = QT_BF16; b.lda = kp; b.K = kp;
  b.a_act = QT_AACT_NONE; b.snake_alpha = nullptr; b.snake_inv_beta = nullptr;
  b.ws_bytes = IM2COL_OFF;  // split records below the image
  return b;
}

// waves per block of the decode GEMV from the k tiles a block walks
inline int gemv_waves(int kts, int cap) { return (kts >= 48 && cap >= 16) ? 16 : ((kts >= 16 && cap >= 8) ? 8 : 4); }

// gemm_pf2_k tile configurations.
// tools/pf2_probe.hip timed every configuration on the 1.7B / 0.6B talker prefill shapes at M = 256 ... 4096
// (profiles/r03_pf2_probe_sweep.txt, profiles/r06_pf2_pingpong_probe.txt): a block's time is nearly independent of M
// and N (its loop runs K / 64 stages of a fixed tile), so launch time ~ ceil(blocks / resident slots) x block time,
// and the best tile is the one whose block count quantises best onto the 256 CUs.  Block cycles per 2048 of K and
// epilogue cycles below are those measurements; cfg 3 (72 KiB of LDS) runs 2 blocks per CU, the others 1.  The
// ping-pong configurations (pp, 8 waves in two staggered groups) are considered from 256 rows (long prefills: voice
// clone, non-streaming prompts); cfg 22 is cfg 21 with K split over two blocks (per-block K in its loop figure, its
// epilogue the record merge), only for <= 2048-column outputs whose two-fold grid fits the 256 CUs.
// (deeper pipelines of the two small-tile configurations -- 7 stages of 64 x 96, 6 of 128 x 64, one block per CU --
// measured slower at 24..680 rows: gate-up 160 rows 25.4 -> 37.9 us, qkv 680 rows 26.2 -> 37.1;
// profiles/r04_pf2_deep_ab.txt)
struct Pf2Cfg { int id, BM, BN, WM, WN, bpc; float loop1, loop2, epi; int pp, ks; };
constexpr Pf2Cfg PF2_CFGS[] = {
    {3, 128, 64, 2, 2, 2, 31000.f, 44000.f, 4000.f, 0, 1},    // 4 waves, wave tile 64 x 32
    {11, 64, 96, 2, 2, 1, 28000.f, 28000.f, 3000.f, 0, 1},    // 4 waves, wave tile 32 x 48
    {4, 256, 128, 4, 2, 1, 68000.f, 68000.f, 8000.f, 0, 1},   // 8 waves, wave tile 64 x 64
    {9, 256, 160, 4, 2, 1, 76500.f, 76500.f, 9000.f, 1, 1},   // ping-pong, 8 waves, wave tile 64 x 80 (4-wave form: 95000)
    {21, 128, 128, 4, 2, 1, 42600.f, 42600.f, 2500.f, 1, 1},  // ping-pong, 8 waves, wave tile 32 x 64
    {22, 128, 128, 4, 2, 1, 45000.f, 45000.f, 9500.f, 1, 2},  // cfg 21, split-K 2
    {23, 256, 256, 4, 2, 1, 97500.f, 97500.f, 10000.f, 1, 1}, // ping-pong, 8 waves, wave tile 64 x 128, 2 LDS stages
};
inline const Pf2Cfg& pf2_cfg(int id) {  // an id without a configuration runs cfg 3
  for (const Pf2Cfg& c : PF2_CFGS)
    if (c.id == id) return c;
  return PF2_CFGS[0];
}
inline long long pf2_tiles(const Pf2Cfg& c, int M, int N) {
  return cdiv(M, c.BM) * cdiv(N, c.BN);
}
// floats of one block's split record: NW x MI x CT x 256 accumulators + WN x BM row sums
inline long long pf2_rec(const Pf2Cfg& c) {
  return (long long)c.WM * c.WN * (c.BM / c.WM / 16) * (c.BN / 16 / c.WN) * 256 + c.WN * c.BM;
}
// the split records of ks blocks per tile fit the workspace's part_bytes of record room (0: no workspace)
inline bool pf2_split_fits(const Pf2Cfg& c, long long tiles, int ks, long long part_bytes) {
  return part_bytes > 0 && tiles <= 4096 && tiles * ks * pf2_rec(c) * 4 <= part_bytes;
}
inline int pf2_pick(int M, int N, int K, long long part_bytes, const GemmKnobs& k) {
  int best = 3;
  float best_t = 3.4e38f;
  for (const Pf2Cfg& c : PF2_CFGS) {
    if (c.pp && (M < 256 || !k.pf2_pp)) continue;
    const long long tiles = pf2_tiles(c, M, N);
    if (c.ks > 1 && (N > 2048 || tiles * c.ks > 256 || K / 64 < 32 || !pf2_split_fits(c, tiles, c.ks, part_bytes))) continue;
    const long long blocks = tiles * c.ks;
    const float kf = K / 2048.f / c.ks;
    float t;
    if (c.bpc == 2 && blocks > 256) t = (float)((blocks + 511) / 512) * (c.loop2 * kf + c.epi);
    else t = (float)((blocks + 255) / 256) * (c.loop1 * kf + c.epi);
    if (t < best_t) { best_t = t; best = c.id; }
  }
  return best;
}
// split-K factor of the 4-wave configurations (3, 11) for a launch of nwg tiles: narrow (<= 2048-column) outputs whose
// tiles leave most CUs idle split K (>= 16 stages of 64 per split; wide outputs measured slower split: 1.7B q/k/v at
// 80 rows 15.5 -> 17.9 us) when the caller's workspace holds the split records
inline int pf2_splits(const Pf2Cfg& c, int M, int N, int K, long long part_bytes, const GemmKnobs& k) {
  const long long nwg = pf2_tiles(c, M, N);
  const int S = K / 64;
  if (!k.pf2_split || part_bytes <= 0 || N > 2048 || nwg >= 192 || S < 32) return 1;
  int ks = std::min({PF2_KS_MAX, (int)(256 / nwg), S / 16});
  while (ks > 1 && nwg * ks * pf2_rec(c) * 4 > part_bytes) --ks;
  return std::max(ks, 1);
}

inline GemmPlan gemm_reject(int err) { GemmPlan pl; pl.err = err; return pl; }

// One call without the im2col rewrite (taps > 0 here means the implicit-im2col kernels).
inline GemmPlan gemm_plan_direct(const qt_gemm_args& a, const GemmKnobs& k) {
  const bool wbf = a.w_dtype == QT_BF16, abf = a.a_dtype == QT_BF16, lin = a.taps <= 0;
  const int E = wbf ? 8 : 4, KT = 4 * E;
  GemmPlan pl;
  long long kp;
  if (!lin) {
    if (a.cin_pad % KT || a.cin % E || a.t_out <= 0) return gemm_reject(QT_ERR_SHAPE);
    kp = (long long)a.taps * a.cin_pad;
  } else {
    if (a.K % E) return gemm_reject(QT_ERR_SHAPE);
    kp = ((long long)a.K + KT - 1) / KT * KT;
  }
  pl.kp = (int)kp;
  if (a.M <= 0 || a.N <= 0 || (a.epi == QT_EPI_SWIGLU && a.N % 16)) return gemm_reject(QT_ERR_SHAPE);
  if (a.epi == QT_EPI_SWIGLU && (a.bias || a.colscale)) return gemm_reject(QT_ERR_ARG);
  if (a.out2 && (!lin || a.epi == QT_EPI_SWIGLU || a.o_dtype != QT_F32)) return gemm_reject(QT_ERR_ARG);
  if ((a.snake_alpha == nullptr) != (a.snake_inv_beta == nullptr)) return gemm_reject(QT_ERR_ARG);
  if (a.a_act != QT_AACT_NONE && a.a_act != QT_AACT_ELU) return gemm_reject(QT_ERR_ARG);
  if (a.act < QT_ACT_NONE || a.act > QT_ACT_RELU_TANH) return gemm_reject(QT_ERR_ARG);

  const int dil = a.dil > 0 ? a.dil : 1;
  const int ntl = (int)(((long long)a.N + 15) / 16), ktl = pl.kp / KT;  // column tiles, k tiles
  const bool kt_whole = a.K % KT == 0, elu = a.a_act == QT_AACT_ELU;
  const bool plain_a = !elu && a.snake_alpha == nullptr;
  const bool ws_ok = a.ws && a.ws_bytes >= QT_GEMM_WS_MIN && a.splitk != 1;
  // room for gemm_pf2_k's split records (17+ rows); 0 = none
  const long long part_bytes = (a.M > 16 && ws_ok) ? a.ws_bytes - WS_CNT_BYTES : 0;

  // 17..256 rows of bf16 A x bf16 weights (prefills of streaming-text / voice-clone prompts, single-request refills):
  // three kernels, picked by the per-launch times of tools/prefill_gemm_bench.py at 1.7B / 0.6B dims
  // (profiles/r03_skinny_routes.txt).  The row-group GEMV grows linearly in M (each group re-reads the weights), the
  // tiled gemm_pf2_k is flat in M but has few blocks on narrow outputs, gemm_sk_k (every row in one block per column
  // tile) reads the weights once but every block re-reads A:
  //   outputs >= 4096 columns: gemm_sk_k at <= 48 rows of a <= 8 Mi-element weight (1.7B qkv 24 rows 11.5 -> 7.6 us,
  //     48 rows 16.5 -> 10.7), else gemm_pf2_k (gate-up 80 rows 51.4 -> 16.2, 112 rows 87.6 -> 16.9; qkv 112 rows
  //     35.1 -> 16.0);
  //   narrower outputs: the row-group GEMV while M x N x K <= 400 Mi (1.7B o up to 100 rows: 80 rows 12.2 vs 13.0 us
  //     on gemm_pf2_k; 1.7B down up to 33 rows: 24 rows 11.5 vs 16.9), else gemm_pf2_k with its narrow-output
  //     split-K (1.7B down 80 rows 29.0 -> 16.9, 112 rows 37.7 -> 17.7; o 112 rows 15.5 -> 13.8, 200 rows 24.3 -> 13.5;
  //     profiles/r03_skinny_routes.txt).
  const bool skinny = k.skinny != 0 && a.M > 16 && a.M <= 256 && lin && wbf && abf && a.K % 64 == 0 &&
                      a.a_index == nullptr && a.gamma == nullptr && plain_a && a.lda % 8 == 0 && aligned16(a.A) &&
                      a.N >= 32;
  bool sk = false, pf_small = false, skinny_gemv = false;
  if (skinny) {
    const int sk_max_m = k.sk ? std::min(k.sk_max_m, 64) : 0;
    if (a.N >= 4096) {
      if (a.M <= sk_max_m && (long long)a.N * a.K <= (8ll << 20)) sk = true;
      else pf_small = true;
    } else if ((long long)a.N * a.K <= (400ll << 20) / a.M) {  // M x N x K <= 400 Mi
      skinny_gemv = true;
    } else {
      pf_small = true;
    }
  }

  // rows per GEMV block, and whether the rows are split into groups over gridDim.z
  int mr = a.M;
  bool grouped = false;
  if (a.M <= 16 && lin && wbf && kt_whole && a.gamma == nullptr) {
    // decode GEMV row groups (bf16 weights): rows split over gridDim.z blocks instead of K over gridDim.y for
    // shapes with <= 128 column tiles (measured cold, M = 8, two groups of 4 rows with fold 4: talker o 6.0 -> 5.3,
    // talker down 10.9 (split-K 2) -> 9.4, CP down 7.6 -> 6.5, CP lm_head 4.9 -> 4.5 us; wider shapes lose:
    // talker qkv 6.7 -> 9.6); four groups of 2 rows for <= 64 tiles (CP down 6.5 -> 5.8 us; 128-tile shapes lose
    // with four)
    const int rg = k.gemv_rg > 0 ? k.gemv_rg : (a.M > 4 ? (ntl <= 64 ? 4 : (ntl <= 128 ? 2 : 1)) : 1);
    if (rg > 1) { mr = (int)cdiv(a.M, rg); grouped = true; }
  } else if (skinny ? skinny_gemv
                    : (a.M <= k.gemv_max_m && (a.M <= 96 || a.N <= 2048) && lin && wbf && kt_whole &&
                       a.gamma == nullptr && plain_a)) {
    // skinny GEMM (the rule above, or without it 17..96 rows / up to gemv_max_m rows of a <= 2048-column output: the
    // talker prefill of streaming-text prompts, short codec windows): the decode GEMV over row groups of 16 -- one
    // block per (column tile, row group), the weight tile streamed from HBM once and re-read from L2 by the other row
    // groups of its XCD.  Its time grows with the row groups; the tiled GEMMs' is flat in M but their grids are small
    // for narrow outputs (tools/prefill_gemm_bench.py: M=80 o 29.6 -> 12.2 us, down 93.7 -> 29.0, qkv 36.0 -> 30.0,
    // gate-up 79.0 -> 65.4; at M=160 gate-up 86 (igemm) vs 130, down 233 vs 48)
    mr = 16;
    grouped = true;
  }
  const bool gemv = mr <= 16 && lin && kt_whole && a.gamma == nullptr && !elu;

  // gemm_pf2_k / gemm_pf_k serve bf16-A linears (the bf16 residual shadow, attention / SwiGLU outputs); with fp32 A
  // the 32 KiB per-stage A fetch from beyond L2 is not hidden by one stage of prefetch (M=680 gate-up 184 vs 107 us on
  // igemm_k)
  const bool pf = wbf && abf && lin && k.pf && a.a_index == nullptr && a.gamma == nullptr && a.N >= 32 &&
                  (pf_small || a.M >= k.igemm_min_m) && mr > 16 && a.K % 8 == 0 && a.lda % 8 == 0 && plain_a &&
                  !k.no_igemm;

  if (sk) {
    pl.route = GemmRoute::SK;
    pl.sk_mi = (int)std::min(std::max(cdiv(a.M, 16), 2ll), 4ll);
  } else if (gemv) {
    pl.route = GemmRoute::GEMV;
    pl.mr = mr;
    // wide grids use smaller blocks so several fit per CU (fewer block rounds; measured: N=12288 K=2048
    // 14.7 us at 16 waves/block -> 12.0 at 4); deep-K row-group shapes (the down projections) prefer 8 waves per
    // block: talker down 9.4 -> 8.6, CP down 5.8 -> 5.6 us (o_proj / lm_head keep 16)
    int wpb_max = ntl > 512 ? 4 : (ntl > 256 ? 8 : 16);
    if (grouped && ktl >= 96) wpb_max = 8;
    if (k.gemv_wpb > 0) wpb_max = k.gemv_wpb;
    // split-K for the ungrouped decode GEMV when it has too few column tiles to fill 256 CUs twice.
    // auto: split only deep-K shapes on < 256 column tiles (the arrival / partial round trips pay only when they
    // remove weight round trips).  Measured cold, paired-A GEMV, partial loads of four splits in flight:
    // 2048x6144 11.4 (no split) / 10.9 (2) / 10.3 us (4), 1024x3072 8.5 / 7.6 / 7.1 us; other shapes lose.
    // In the frame graph split 2 wins (bench 158.6 vs 157.2 audio-s/s, same box)
    if (a.M <= 16 && !grouped && ws_ok && ntl <= 4096) {
      const int wpb1 = gemv_waves(ktl, 16), per1 = (ktl + wpb1 - 1) / wpb1;
      int ks = a.splitk > 1 ? a.splitk : ((per1 > 4 && ntl < 256) ? k.gemv_split_auto : 1);
      ks = std::max(1, std::min({ks, 16, ktl / 2}));
      const long long need = WS_CNT_BYTES + (long long)ntl * ks * GEMV_PART * (long long)sizeof(float);
      if (ks > 1 && need <= a.ws_bytes) { pl.ks = ks; pl.ws_split = true; }
    }
    const int kts = (ktl + pl.ks - 1) / pl.ks;  // k tiles per split
    pl.wpb = gemv_waves(kts, wpb_max);
    // k tiles in flight per wave: 8 when a wave owns 5..8 (one round trip instead of two).  Forcing 8 on every shape,
    // or 16, was measured slower (register pressure; profiles/r01_gemv_variants_ab.jsonl)
    const int per = (kts + pl.wpb - 1) / pl.wpb;
    pl.u = (k.gemv_u ? k.gemv_u : ((per > 4 && per <= 8) ? 8 : 4)) >= 8 ? 8 : 4;
    // fold factor from the rows per block (bf16 weights): 4 for <= 4 rows, 2 for <= 8
    pl.fold = !wbf ? 1 : ((k.gemv_fold >= 4 && mr <= 4) ? 4 : ((k.gemv_fold >= 2 && mr <= 8) ? 2 : 1));
    // weights streamed once per frame (talker-size matrices) bypass cache retention so the re-read code-predictor
    // weights stay in L2 / Infinity Cache
    pl.nt_loads = k.gemv_nt >= 0 ? k.gemv_nt : ((long long)ntl * 16 * kp >= (16ll << 20) / (wbf ? 2 : 4));  // >= 16 MiB
  } else if (a.N == 1 && !lin && kp <= 2048 && a.act == QT_ACT_NONE && a.epi != QT_EPI_SWIGLU && !a.rmsnorm &&
             a.colscale == nullptr && a.a_index == nullptr && a.gamma == nullptr &&
             ((long long)a.taps - 1) * dil <= 240) {
    pl.route = GemmRoute::CONV_N1;  // the window of 256 steps, 256 + (taps - 1) * dil rows of 33 floats, fits 64 KiB
  } else if (a.M <= 16) {
    pl.route = GemmRoute::WT_1x8;
  } else if (pf && a.K % 64 == 0 && kp == a.K && aligned16(a.A)) {
    pl.route = GemmRoute::PF2;
    int cfg = k.pf2_cfg ? k.pf2_cfg : pf2_pick(a.M, a.N, a.K, part_bytes, k);
    if (cfg == 22 && !pf2_split_fits(pf2_cfg(22), pf2_tiles(pf2_cfg(22), a.M, a.N), 2, part_bytes)) cfg = 21;
    const Pf2Cfg& c = pf2_cfg(cfg);
    pl.pf2_cfg = c.id;
    pl.pf2_ks = c.pp ? c.ks : (c.BM <= 128 ? pf2_splits(c, a.M, a.N, a.K, part_bytes, k) : 1);
    pl.ws_split = pl.pf2_ks > 1;
  } else if (pf) {
    // LDS-staged A and B, 128 x 128 tiles (128 x 64 when that leaves < 256 blocks)
    pl.route = GemmRoute::PF;
    pl.ntb = cdiv(a.M, 128) * cdiv(ntl, 8) < 256 ? 4 : 8;
  } else if (wbf && a.a_index == nullptr && a.gamma == nullptr && a.N >= 32 && a.M >= (lin ? k.igemm_min_m : 16) &&
             (lin ? a.K % 8 == 0 : ((long long)a.taps - 1) * dil <= 64) && !k.no_igemm) {
    // (convs: the staged window of a 128-row tile, 128 + (taps - 1) * dil rows, is at most 192 rows)
    pl.route = GemmRoute::IGEMM;
    // column tile per block: 6 x 16 for 96 / 192-channel layers (no idle tiles, the snake-staged window is
    // shared by all of a row tile's columns), else 8 x 16
    pl.ntb = (ntl % 6 == 0 && ntl <= 12) ? 6 : 8;
    pl.mi = 2;
    if (k.igemm_cfg) {
      pl.ntb = k.igemm_cfg / 10;
      pl.mi = k.igemm_cfg % 10;
    } else {
      // short windows (a streamed codec window, 1-3 frames x batch rows per conv): 64-row tiles and 4 (6) column
      // tiles per block when the default tiling leaves fewer than 256 blocks -- the first streamed window's feed
      // 2.53 -> 2.08 ms at B=8 (tools/codec_feed_prof.py)
      const long long tout = lin ? a.M : a.t_out, nb = lin ? 1 : a.M / a.t_out;
      const long long blocks = nb * cdiv(tout, 128) * cdiv(ntl, pl.ntb);
      if (blocks < 256) { pl.mi = 1; pl.ntb = pl.ntb == 6 ? 6 : 4; }
    }
    // the instantiated tilings; anything else runs 8 x 2
    const bool known = (pl.ntb == 6 || pl.ntb == 4 || pl.ntb == 8) && (pl.mi == 1 || pl.mi == 2);
    if (!known) { pl.ntb = 8; pl.mi = 2; }
  } else if (a.M <= 32) {
    pl.route = GemmRoute::WT_2x8;
  } else {
    pl.route = GemmRoute::WT_4x4;
  }

  // out2 is written by the decode GEMV's epilogue (M <= 16, or the row-group path above), gemm_sk_k and the two
  // bf16-A prefill GEMMs
  if (a.out2 && pl.route != GemmRoute::GEMV && pl.route != GemmRoute::SK && pl.route != GemmRoute::PF2 &&
      pl.route != GemmRoute::PF)
    return gemm_reject(QT_ERR_ARG);
  const bool abf_ok = a.a_dtype == QT_BF16 || a.a_dtype == QT_F32, obf_ok = a.o_dtype == QT_BF16 || a.o_dtype == QT_F32;
  if (!(wbf ? (abf_ok && obf_ok) : (a.w_dtype == QT_F32 && a.a_dtype == QT_F32 && a.o_dtype == QT_F32)))
    return gemm_reject(QT_ERR_DTYPE);
  return pl;
}

inline GemmPlan gemm_plan(const qt_gemm_args& a, const GemmKnobs& k) {
  if (!a.A || !a.W || !a.out) return gemm_reject(QT_ERR_ARG);
  if (!im2col_applies(a, k)) return gemm_plan_direct(a, k);
  if (a.a_dtype != QT_BF16 && a.a_dtype != QT_F32) return gemm_reject(QT_ERR_DTYPE);
  GemmPlan pl = gemm_plan_direct(im2col_linear_args(a), k);
  if (pl.route == GemmRoute::NONE) return pl;
  pl.inner = pl.route;
  pl.route = GemmRoute::IM2COL;
  return pl;
}

}  // namespace qt_gemm_impl
