// Fused matching-head retrieval at evaluation scale (aladin_retrieval_ranks): the COCO-protocol ranks and arg-maxima of both
// directions straight from the embeddings, bit for bit those of aladin_sim_matrix + aladin_recall_ranks (recall.hip).
// Replaces ims.mm(caps.t()) + numpy argsort/where, reference alad/recall_auxiliary.py:30-56.  The chain every score comes from is
// described in sim_common.hpp; this file SCREENS with the hi.hi prefix of that chain (a third of the work) and pays for the other
// two segments only where a decision needs them; see sim_screen_kernel.
#include "../../include/aladin_hip.h"
#include <type_traits>
#include <utility>

#include "sim_common.hpp"

// ------------------------------------------------------------------------------------------------
// Fused retrieval (aladin_retrieval_ranks): ranks and arg-maxima of both directions straight from the
// embeddings; the (n_img x n_cap) score matrix is never written (500 MB at COCO-5k).
//
// rank = #(scores strictly above the ground truth G): a DECISION per pair, and most pairs are decided by far
// less than an exact score.  The fused kernel therefore runs the hi.hi segment only -- s, bit for bit the
// PREFIX of the pair's exact chain -- and bounds what the two dropped segments can add:
//     |v - s| <= band = |lo_a||hi_b| + |hi_a||lo_b| + 2^-14 |s|
// (Cauchy-Schwarz per segment on the actual fp16 operands, norms rounded up by the packer; the last term
// covers the fp32 rounding of the 48 more accumulator steps, each within a few ulp of the running value,
// ~16 x what round-to-nearest gives; where |s| is tiny the roundings are bounded by a few ulp of the largest
// lo.hi product instead, ~2^-22 of the Cauchy-Schwarz terms, inside the 2^-9 by which the packer's rounded-up
// norms overstate them).  Rigorous per pair: no statistics, no tuning to the data.  Then
//     s - band >  G  : counted          s + band < G : not counted          otherwise: AMBIGUOUS
// and for the arg-maxima, with L = max(G, tile-local lower bound of the row / column maximum) <= the exact
// maximum, only pairs with s + band >= L can be the exact arg-max (the true one always is: v >= L).
// Per 256 x 384 tile:
//   * at most SIM_LIST_CAP ambiguous / arg-max candidate pairs: they go to the tile's list with their prefix s;
//     sim_rescore_kernel CONTINUES their chains (16 pairs on the diagonal of one 16 x 16 MFMA tile) and
//     patches the integer counters / packed maxima with the exact value;
//   * more than that: the tile itself continues the chain -- the same accumulators run the lo.hi and hi.lo
//     segments -- and takes the exact epilogue (round 3's kernel, for this tile only).
// Either way every decision is made on the exact chain's bits or is implied by the band, so the four outputs
// equal aladin_sim_matrix + aladin_recall_ranks bit for bit (tests), whatever the data; only the COST
// depends on it: a third of round 3's MFMA work when ground truths stand clear of the bulk, up to all of it
// when they sit inside.  Ground-truth pairs themselves (exact scores from sim_gt_kernel, which also enters
// them into the arg-maxima) are masked out of the tiles: they never beat their own threshold.
// Integer counters and packed-max atomics only: the result does not depend on the tile order.
// ------------------------------------------------------------------------------------------------
struct SimEntry { int row, col; float s; int flags; };
enum { SIM_F_ROWCNT = 1, SIM_F_COLCNT = 2, SIM_F_ROWARG = 4, SIM_F_COLARG = 8 };
constexpr int SIM_LIST_CAP = 512;
struct SimRaw { int rc; float s; };               // tile-local (row << 16 | column), prefix score
constexpr int SIM_RAW_WAVE = 192;                 // UNDECIDED scores and arg-max candidates of a wave's 128 x 96 block before the tile gives up screening
                                                  // (scores that beat their ground truth by more than the band are counted in registers: round 5)
// statistics words (int32, aladin_retrieval_stats_offset): [0] tiles continued in place, [1] pairs listed, [2..4] diagnostic build,
// [5] listed pairs whose chains sim_rescore_kernel continued (the others were ruled out by the certified bounds), [6] tiles that ran
// the analysis, [7] of those, tiles that overflowed their lists, [8] tiles that skipped the analysis (hopeless data, see sim_screen_kernel)
enum { SIM_ST_EXACT = 0, SIM_ST_LISTED = 1, SIM_ST_RESCORED = 5, SIM_ST_ANALYSED = 6, SIM_ST_OVERFLOW = 7, SIM_ST_SKIPPED = 8 };
constexpr int SIM_STATS_WORDS = 64;
constexpr int SIM_RESCORE_SPLIT = 4;

struct SimRankArgs {
  int cpi;
  const float* gt;                    // n_cap, in the accumulators' scale
  const float2* na;                   // Mp  (P, R)
  const float2* nb;                   // Np  (Q, T)
  int32_t* cnt_i2t;                   // n_img: scores beating the row's best ground truth = its i2t rank
  int32_t* cnt_t2i;                   // n_cap
  unsigned long long* best_i2t;       // n_img
  unsigned long long* best_t2i;       // n_cap
  SimEntry* list;                     // n_tiles x SIM_LIST_CAP
  int* list_cnt;                      // n_tiles
  int* stats;                         // SIM_ST_*
  unsigned* lob_i2t;                  // n_img: float_key of a certified lower bound of the row's exact maximum (0: none yet)
  unsigned* lob_t2i;                  // n_cap
};

template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }


// ALADIN_DIAG build (make diag): thread 0 of every tile leaves wall-clock stamps of its phases in the tile's list segment
// (its last 96 bytes: tools/retrieval_stamps.py reads them; a tile that lists more than 58 pairs overwrites them)
#ifdef ALADIN_DIAG
#define SIM_STAMP(k) do { if (threadIdx.x == 0) reinterpret_cast<long long*>(ra.list + (int64_t)(mb * n_nblk + nb) * SIM_LIST_CAP + (SIM_LIST_CAP - 6))[k] = wall_clock64(); } while (0)
#else
#define SIM_STAMP(k) do { } while (0)
#endif
// The exact epilogue (round 3): every accumulator holds the full chain.  Scores are compared in the accumulators' own
// scale (gt[] is kept in it).  The workgroup's partial results meet in LDS (free after the main loop) so that each row /
// column of the tile costs ONE global atomic per counter instead of one per wave.
// i2t: the reference's rank is the best of the image's cpi captions (recall_auxiliary.py:38-44);
// #(v > t) never grows with t, so that minimum is the count against the LARGEST ground truth.
__device__ __forceinline__ void sim_rank_epilogue_exact(f32x4 (&acc)[SIM_RT][SIM_CT], char* smem, int mb, int nb, int n_img, int n_cap,
                                                        const SimRankArgs& ra, int n_nblk) {
  using Cfg = SimCfg;
  constexpr int RT = SIM_RT, CT = SIM_CT;
  const int tid = fresh_tid();
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / Cfg::WGN, wn = wave % Cfg::WGN;
  const int row0 = mb * Cfg::BM + wm * (RT * 16) + 4 * (lane >> 4);
  const int col0 = nb * Cfg::BN + wn * (CT * 16) + (lane & 15);
  __syncthreads();                                                   // every wave is done with the operand stages
  int* l_row = reinterpret_cast<int*>(smem);                         // [BM] scores beating the row's best ground truth
  int* l_col = l_row + Cfg::BM;                                      // [BN]
  unsigned long long* l_brow = reinterpret_cast<unsigned long long*>(l_col + Cfg::BN);    // [BM]
  unsigned long long* l_bcol = l_brow + Cfg::BM;                     // [BN]
  float* l_grow = reinterpret_cast<float*>(l_bcol + Cfg::BN);        // [BM] max of the row's ground truths
  float* l_gcol = l_grow + Cfg::BM;                                  // [BN]
  for (int e = threadIdx.x; e < Cfg::BM + Cfg::BN; e += Cfg::THREADS) { l_row[e] = 0; l_brow[e] = 0ull; }
  for (int e = threadIdx.x; e < Cfg::BM; e += Cfg::THREADS) {
    const int row = mb * Cfg::BM + e;
    float g = INFINITY;
    if (row < n_img) {
      g = -INFINITY;
      for (int q = 0; q < ra.cpi; ++q) g = fmaxf(g, ra.gt[row * ra.cpi + q]);
    }
    l_grow[e] = g;
  }
  for (int e = threadIdx.x; e < Cfg::BN; e += Cfg::THREADS) {
    const int c = nb * Cfg::BN + e;
    l_gcol[e] = (c < n_cap) ? ra.gt[c] : INFINITY;
  }
  __syncthreads();
  SIM_STAMP(8);
  const int lrow0 = wm * (RT * 16) + 4 * (lane >> 4), lcol0 = wn * (CT * 16) + (lane & 15);
  // Reductions by DPP row rotations (the 16 lanes of a row) and permlane swaps (the 4 lane groups of a column): round 3
  // used __shfl_xor (ds_bpermute through the LDS crossbar, ~400 of them per wave) and this epilogue took as long as a
  // K = 768 main loop (26 us per tile, phase stamps).
  // ---- rows: lanes with the same lane >> 4 share a row; CT columns each
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = row0 + rt * 16 + reg, lrow = lrow0 + rt * 16 + reg;
      const float g = l_grow[lrow];
      int cnt = 0;
      float best = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const float v = acc[rt][ct][reg];               // pad rows / columns and ground-truth pairs are -inf since phase 0: never count, never win
        cnt += (v > g);
        best = fmax_nc(best, v);
      }
      cnt = row16_isum(cnt);
      best = row16_max(best);
      // the maximum's first column: this lane's first hit (columns ascend with ct), then the smallest over the 16 lanes
      int besti = 0x7fffffff;
#pragma unroll
      for (int ct = CT - 1; ct >= 0; --ct)
        if (acc[rt][ct][reg] == best) besti = col0 + ct * 16;
      besti = row16_imin(besti);
      if (row < n_img && (lane & 15) == 0) {
        if (cnt) atomicAdd(&l_row[lrow], cnt);
        if (besti != 0x7fffffff && best > -INFINITY) atomicMax(&l_brow[lrow], pack_best(best, besti));
      }
    }
  SIM_STAMP(9);
  // ---- columns: lanes with the same lane & 15 share a column; 16 rows each
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int col = col0 + ct * 16, lcol = lcol0 + ct * 16;
    const float g = l_gcol[lcol];
    int cnt = 0;
    float best = -INFINITY;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float v = acc[rt][ct][reg];
        cnt += (v > g);
        best = fmax_nc(best, v);
      }
    cnt += lane_xor16(cnt);
    cnt += lane_xor32(cnt);
    best = fmax_nc(best, lane_xor16(best));
    best = fmax_nc(best, lane_xor32(best));
    int besti = 0x7fffffff;
#pragma unroll
    for (int rt = RT - 1; rt >= 0; --rt)
#pragma unroll
      for (int reg = 3; reg >= 0; --reg)
        if (acc[rt][ct][reg] == best) besti = row0 + rt * 16 + reg;     // rows ascend with (rt, reg)
    { const int o = lane_xor16(besti); besti = o < besti ? o : besti; }
    { const int o = lane_xor32(besti); besti = o < besti ? o : besti; }
    if (col < n_cap && lane < 16) {
      if (cnt) atomicAdd(&l_col[lcol], cnt);
      if (besti != 0x7fffffff && best > -INFINITY) atomicMax(&l_bcol[lcol], pack_best(best, besti));
    }
  }
  SIM_STAMP(10);
  __syncthreads();
  SIM_STAMP(11);
  // ---- one global atomic per non-zero counter; arg-maxima only when they beat what is already there
  for (int e = threadIdx.x; e < Cfg::BM; e += Cfg::THREADS) {
    const int row = mb * Cfg::BM + e;
    if (row < n_img) {
      if (l_row[e]) atomicAdd(&ra.cnt_i2t[row], l_row[e]);
      const unsigned long long p = l_brow[e];
      if (p > __hip_atomic_load(&ra.best_i2t[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&ra.best_i2t[row], p);
    }
  }
  for (int e = threadIdx.x; e < Cfg::BN; e += Cfg::THREADS) {
    const int col = nb * Cfg::BN + e;
    if (col < n_cap) {
      if (l_col[e]) atomicAdd(&ra.cnt_t2i[col], l_col[e]);
      const unsigned long long p = l_bcol[e];
      if (p > __hip_atomic_load(&ra.best_t2i[col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&ra.best_t2i[col], p);
    }
  }
}

// MODE 0: screened; 1: every tile exact (no analysis code at all); 2: the screened kernel with every tile skipping its analysis
// (diagnostic build: is the exact path of the MODE-0 code as fast as MODE 1's?)
template <int MODE>
__global__ __launch_bounds__(512) void sim_screen_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b,
                                                         const float* __restrict__ scale, int n_img, int n_cap, int64_t ldk,
                                                         int kps, int n_nblk, int n_blocks, SimRankArgs ra) {
  using Cfg = SimCfg;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 4, mb, nb);
  constexpr int RT = SIM_RT, CT = SIM_CT;
  f32x4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const half_t* a_tile = a + (int64_t)mb * Cfg::BM * ldk;
  const half_t* b_tile = b + (int64_t)nb * Cfg::BN * ldk;
  SIM_STAMP(0);
  gemm_mainloop16_tall<Cfg>(a_tile, b_tile, ldk, kps, smem, acc);          // hi.hi: the prefix of every pair's chain
  SIM_STAMP(1);
  const int tid = fresh_tid();
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / Cfg::WGN, wn = wave % Cfg::WGN;
  const int row0 = mb * Cfg::BM + wm * (RT * 16) + 4 * (lane >> 4);
  const int col0 = nb * Cfg::BN + wn * (CT * 16) + (lane & 15);
  const int lrow0 = wm * (RT * 16) + 4 * (lane >> 4), lcol0 = wn * (CT * 16) + (lane & 15);
  // ---- phase 0: pad rows / columns and the ground-truth pairs leave the game
  {
    const int r_lo = mb * Cfg::BM, c_lo = nb * Cfg::BN;
    const bool edge = r_lo + Cfg::BM > n_img || c_lo + Cfg::BN > n_cap;
    const bool gtband = (int64_t)r_lo * ra.cpi < (int64_t)c_lo + Cfg::BN && (int64_t)(r_lo + Cfg::BM) * ra.cpi > c_lo;
    if (edge || gtband) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = row0 + rt * 16 + reg;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const int col = col0 + ct * 16;
            if (row >= n_img || col >= n_cap || (unsigned)(col - row * ra.cpi) < (unsigned)ra.cpi) acc[rt][ct][reg] = -INFINITY;
          }
        }
    }
  }
  if constexpr (MODE != 1) {
    // The analysis arrays live in the stage the LAST K step did not use: every wave left that stage before the last step's
    // barrier and nothing refills it any more, so no barrier is needed before writing them.
    char* ep = smem + ((kps & 1) ? Cfg::STAGE_BYTES : 0);
    float* l_thrRow = reinterpret_cast<float*>(ep);                  // [BM] s below this cannot reach the row's ground truth
    float* l_hiRow = l_thrRow + Cfg::BM;                             // [BM] s above this beats it whatever the dropped segments add
    float* l_argRow = l_hiRow + Cfg::BM;                             // [BM] s below this cannot be the row's arg-max (phase 1b)
    float* l_Lrow = l_argRow + Cfg::BM;                              // [BM] certified lower bound of the row's exact maximum (phase 1b)
    float* l_P = l_Lrow + Cfg::BM;
    float* l_R = l_P + Cfg::BM;
    float* l_Grow = l_R + Cfg::BM;
    float* l_bmaxRow = l_Grow + Cfg::BM;
    unsigned* l_rowmax = reinterpret_cast<unsigned*>(l_bmaxRow + Cfg::BM);     // key of the largest qualifying s of the row in this tile (0: none)
    int* l_rowcnt = reinterpret_cast<int*>(l_rowmax + Cfg::BM);
    float* l_thrCol = reinterpret_cast<float*>(l_rowcnt + Cfg::BM);  // [BN] ...
    float* l_hiCol = l_thrCol + Cfg::BN;
    float* l_argCol = l_hiCol + Cfg::BN;
    float* l_Lcol = l_argCol + Cfg::BN;
    float* l_Q = l_Lcol + Cfg::BN;
    float* l_T = l_Q + Cfg::BN;
    float* l_Gcol = l_T + Cfg::BN;
    float* l_bmaxCol = l_Gcol + Cfg::BN;
    unsigned* l_colmax = reinterpret_cast<unsigned*>(l_bmaxCol + Cfg::BN);
    int* l_colcnt = reinterpret_cast<int*>(l_colmax + Cfg::BN);
    SimEntry* l_list = reinterpret_cast<SimEntry*>(l_colcnt + Cfg::BN);        // 10 * (256 + 384) * 4 B = 25600 B: 16-B aligned
    int* l_listn = reinterpret_cast<int*>(l_list + SIM_LIST_CAP);
    float* l_wmax = reinterpret_cast<float*>(l_listn + 4);           // [8 waves][4]: per-wave maxima of P, R, Q, T over the tile
    int* l_rawn = reinterpret_cast<int*>(l_wmax + 4 * Cfg::NWAVES);  // [8 waves] raw candidates of each wave
    int* l_hits = l_rawn + Cfg::NWAVES;                              // [2] rows / columns of the tile with a score in reach of their ground truth
    SimRaw* l_raw = reinterpret_cast<SimRaw*>(l_hits + 2);            // [8 waves][SIM_RAW_WAVE]
    static_assert(Cfg::BM <= Cfg::THREADS && Cfg::BN <= Cfg::THREADS, "one row / column entry per thread");
    static_assert(SIM_LIST_CAP % 256 == 0, "sim_rescore_kernel compacts the list in passes of its 256 threads");
    static_assert(10 * (Cfg::BM + Cfg::BN) * 4 + SIM_LIST_CAP * 16 + 16 + 4 * Cfg::NWAVES * 4 + Cfg::NWAVES * 4 + 8 + Cfg::NWAVES * SIM_RAW_WAVE * 8 <= Cfg::STAGE_BYTES,
                  "the analysis arrays share one operand stage");
    // Hopeless data (ground truths deep in the bulk: every column of every tile nominates candidates and the lists overflow):
    // the analysis would be paid for nothing.  Tiles count themselves as analysed / overflowed; once at least 32 have
    // reported and 7 of 8 overflowed, a tile goes straight on to the exact path -- except the tiles of every EIGHTH round of 256
    // (by dispatch index), which keep probing (data may differ between regions of the grid; every fourth round until round 6:
    // at configs[2]'s six rounds that was a second analysed round for nothing, 0.717 vs 0.687 ms on hopeless data).  Probing by round, not by tile:
    // the workgroups of a round run in lockstep and share their operand panels through the L2 while they do; one tile in eight
    // taking longer than its neighbours (this round's first form) put every tile out of phase: 700 vs 580 us all-exact with
    // ground truths 2 sigma inside the bulk.  (A sample launch of 256 tiles followed by a launch-uniform decision for the rest
    // was measured too: no better on such data, + 10 us on clean data for the second launch.)  Both paths give the same integers.
    if (tid == 0) {
      const int n_an = __hip_atomic_load(&ra.stats[SIM_ST_ANALYSED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int n_ov = __hip_atomic_load(&ra.stats[SIM_ST_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *l_listn = (n_an >= 32 && 8 * n_ov >= 7 * n_an && ((blockIdx.x >> 8) & 7) != 0) ? -1 : 0;
      if constexpr (MODE == 2) *l_listn = -1;            // (diagnostic build) timing probe: every tile skips the analysis
    }
    // the tile's largest band factors bound every pair's band from above: the cheap test of phase 1
    const int e = tid;
    float2 pr = {0.f, 0.f}, qt = {0.f, 0.f};
    float g_row = INFINITY, g_col = INFINITY;                        // every global load of the analysis goes out here, in one latency
    if (e < Cfg::BM) {
      const int row = mb * Cfg::BM + e;
      pr = ra.na[row];                                               // padded rows exist and are zero
      if (row < n_img) {
        g_row = -INFINITY;
        for (int q = 0; q < ra.cpi; ++q) g_row = fmaxf(g_row, ra.gt[row * ra.cpi + q]);
      }
    }
    if (e < Cfg::BN) {
      const int col = nb * Cfg::BN + e;
      qt = ra.nb[col];
      if (col < n_cap) g_col = ra.gt[col];
    }
    {
      const float wP = wave_max(pr.x), wR = wave_max(pr.y), wQ = wave_max(qt.x), wT = wave_max(qt.y);
      if (lane == 0) { l_wmax[wave * 4 + 0] = wP; l_wmax[wave * 4 + 1] = wR; l_wmax[wave * 4 + 2] = wQ; l_wmax[wave * 4 + 3] = wT; }
    }
    __syncthreads();
    const bool skip_analysis = *l_listn < 0;                         // workgroup-uniform
    bool exact = true;
    if (!skip_analysis) {
    float Pg = 0.f, Rg = 0.f, Qg = 0.f, Tg = 0.f;
#pragma unroll
    for (int w = 0; w < Cfg::NWAVES; ++w) {
      Pg = fmaxf(Pg, l_wmax[w * 4 + 0]); Rg = fmaxf(Rg, l_wmax[w * 4 + 1]); Qg = fmaxf(Qg, l_wmax[w * 4 + 2]); Tg = fmaxf(Tg, l_wmax[w * 4 + 3]);
    }
    // thr: s < thr  =>  s + bm + 2^-14 |s| < g;   hi: s > hi  =>  s - bm - 2^-14 |s| > g   (roundings included: the slack is
    // 2^-13 against the band's 2^-14, plus 2^-20 of the band factor for the fp32 evaluation of g -+ bm itself)
    if (e < Cfg::BM) {
      const float g = g_row;
      float thr = INFINITY, hi = INFINITY;
      const float bm = fmaf(pr.x, Qg, pr.y * Tg);                    // >= fmaf(P, Q_j, R * T_j) for every j of the tile: the operations are monotone
      if (g < INFINITY) {
        const float t = g - bm, u = g + bm;
        thr = t - 0x1p-13f * fabsf(t) - 0x1p-20f * bm;
        hi = u + 0x1p-13f * fabsf(u) + 0x1p-20f * bm;
      }
      l_thrRow[e] = thr; l_hiRow[e] = hi; l_P[e] = pr.x; l_R[e] = pr.y; l_Grow[e] = g; l_bmaxRow[e] = bm; l_rowmax[e] = 0u; l_rowcnt[e] = 0;
    }
    if (e < Cfg::BN) {
      const float g = g_col;
      float thr = INFINITY, hi = INFINITY;
      const float bm = fmaf(Pg, qt.x, Rg * qt.y);
      if (g < INFINITY) {
        const float t = g - bm, u = g + bm;
        thr = t - 0x1p-13f * fabsf(t) - 0x1p-20f * bm;
        hi = u + 0x1p-13f * fabsf(u) + 0x1p-20f * bm;
      }
      l_thrCol[e] = thr; l_hiCol[e] = hi; l_Q[e] = qt.x; l_T[e] = qt.y; l_Gcol[e] = g; l_bmaxCol[e] = bm; l_colmax[e] = 0u; l_colcnt[e] = 0;
    }
    if (tid < Cfg::NWAVES + 2) l_rawn[tid] = 0;                      // and l_hits
    __syncthreads();
    SIM_STAMP(2);
    // ---- phase 1: which rows / columns of this wave hold a score within reach of their ground truth at all
    unsigned rowmask = 0u, colmask = 0u;
    {
      float cmax[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) cmax[ct] = -INFINITY;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const float4 thr4 = *reinterpret_cast<const float4*>(l_thrRow + lrow0 + rt * 16);
        const float thr[4] = {thr4.x, thr4.y, thr4.z, thr4.w};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          float m = fmax_nc(fmax_nc(fmax_nc(acc[rt][0][reg], acc[rt][1][reg]), fmax_nc(acc[rt][2][reg], acc[rt][3][reg])),
                            fmax_nc(acc[rt][4][reg], acc[rt][5][reg]));
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) cmax[ct] = fmax_nc(cmax[ct], acc[rt][ct][reg]);
          if (m >= thr[reg]) {
            rowmask |= 1u << (rt * 4 + reg);
            atomicMax(&l_rowmax[lrow0 + rt * 16 + reg], float_key(m));
          }
        }
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        if (cmax[ct] >= l_thrCol[lcol0 + ct * 16]) {
          colmask |= 1u << ct;
          atomicMax(&l_colmax[lcol0 + ct * 16], float_key(cmax[ct]));
        }
    }
    const unsigned rowAny = wave_or(rowmask), colAny = wave_or(colmask);      // wave-uniform
    __syncthreads();
    // ---- phase 1b: per row / column, L = max(G, lower bound of the largest s of the tile) <= the exact maximum, and the prefix
    // below which a score cannot be the arg-max (s + band < L).  A row without a score in reach keeps L = G: nothing qualifies.
    if (e < Cfg::BM) {
      const unsigned k = l_rowmax[e];
      const float g = l_Grow[e], bm = l_bmaxRow[e];
      float L = g;
      if (k) { const float m = key_float(k); L = fmaxf(g, (m - bm) - 0x1p-13f * fabsf(m)); }      // <= lo of that element <= the exact row maximum
      const float t = L - bm;
      l_Lrow[e] = L;
      l_argRow[e] = (g < INFINITY) ? t - 0x1p-13f * fabsf(t) - 0x1p-20f * bm : INFINITY;
    }
    if (e < Cfg::BN) {
      const unsigned k = l_colmax[e];
      const float g = l_Gcol[e], bm = l_bmaxCol[e];
      float L = g;
      if (k) { const float m = key_float(k); L = fmaxf(g, (m - bm) - 0x1p-13f * fabsf(m)); }
      const float t = L - bm;
      l_Lcol[e] = L;
      l_argCol[e] = (g < INFINITY) ? t - 0x1p-13f * fabsf(t) - 0x1p-20f * bm : INFINITY;
    }
    {
      // how many rows / columns of the tile hold a score in reach of their ground truth: each of them nominates at least the
      // largest such score as an arg-max candidate, one list entry per row (column) -- more of either than the list holds and
      // the tile cannot be listed: on to the exact path now, without paying for phase 2 (ground truths deep in the bulk)
      const unsigned long long hr = __ballot(e < Cfg::BM && l_rowmax[e] != 0u), hc = __ballot(e < Cfg::BN && l_colmax[e] != 0u);
      if (lane == 0) {
        if (hr) atomicAdd(&l_hits[0], __popcll(hr));
        if (hc) atomicAdd(&l_hits[1], __popcll(hc));
      }
    }
    if (tid == 0) *l_listn = 0;
    __syncthreads();
    SIM_STAMP(3);
    const bool hopeless = l_hits[0] + l_hits[1] > SIM_LIST_CAP;      // workgroup-uniform (a pair may serve a row AND a column: a heuristic, and both paths are exact)
    // ---- phase 2a: per accumulator register (rt, reg) = 4 rows x 96 columns of the wave and per column tile, against the rows'
    // and columns' thresholds -- only the SIDES phase 1 flagged (wave-uniform bits: with ground truths inside the bulk of one
    // direction's scores and clear of the other's, the usual case, half of the compares are never issued):
    //   * a score above its row's / column's `hi` beats that ground truth whatever the dropped segments add: COUNTED here, in a
    //     register per lane (rows: reduced over the 16 lanes of a row; columns: summed over the wave's 128 rows at the end) --
    //     round 4 sent these through the raw list too, and any data with ground truths inside the bulk of the scores (Recall@1
    //     below ~90 %: hundreds of such pairs per tile) overflowed it and paid for the exact path in every tile;
    //   * a score between `thr` and `hi` (undecided), or at / above `arg` (may be the arg-max), goes into the wave's segment of
    //     the RAW list (tile-local row, column, prefix s) for phase 2b -- nothing else is decided here.
    if ((rowAny | colAny) && !hopeless) {
      float thrC[CT], hiC[CT], argC[CT];
      int cntC[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        thrC[ct] = l_thrCol[lcol0 + ct * 16]; hiC[ct] = l_hiCol[lcol0 + ct * 16]; argC[ct] = l_argCol[lcol0 + ct * 16];
        cntC[ct] = 0;
      }
      // each wave fills its OWN segment of the raw list (SIM_RAW_WAVE slots, a running count in a scalar register): no LDS
      // atomic, no round trip per hit; a wave that runs out of slots sends the tile to the exact path
      int n_mine = 0;
      SimRaw* my_raw = l_raw + wave * SIM_RAW_WAVE;
#ifdef ALADIN_DIAG
      int n_full = 0;
#endif
      // ONE straight-line pass over the lane's 192 scores.  Per pair, column side: `up` = beats the column's ground truth for sure
      // (one compare, one add-with-carry into the lane's count of that column) and ONE more compare -- against `arg` if up,
      // `thr` if not -- says whether the pair must be looked at again (undecided, or a possible arg-max): 4 vector
      // instructions.  The row side runs only for the registers whose rows phase 1 flagged (a wave-uniform bit: with ground
      // truths inside the bulk of one direction's scores and clear of the other's, the usual case, it is rare).  The code is
      // executed ONCE per tile, so its SIZE is what it costs (three specialised copies of this pass, 100 KB of instructions,
      // ran three times slower than one: the instruction cache holds 64 KB): the rare paths are kept short, not fast.
      static_for<RT>([&](auto rt_) {
        constexpr int rt = decltype(rt_)::value;
        if (n_mine > SIM_RAW_WAVE) return;                     // wave-uniform
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          unsigned long long pm[CT];
          unsigned long long any = 0ull;
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const float s = acc[rt][ct][reg];
            const bool upC = s > hiC[ct];
            cntC[ct] += upC;
            pm[ct] = __ballot(s >= (upC ? argC[ct] : thrC[ct]));      // in reach of the column's ground truth and (undecided or an arg-max candidate)
            any |= pm[ct];
          }
          if ((rowAny >> (rt * 4 + reg)) & 1u) {               // wave-uniform
            const float thrR = l_thrRow[lrow0 + rt * 16 + reg], hiR = l_hiRow[lrow0 + rt * 16 + reg], argR = l_argRow[lrow0 + rt * 16 + reg];
            int cntR = 0;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              const float s = acc[rt][ct][reg];
              const bool upR = s > hiR;
              cntR += upR;
              const unsigned long long m = __ballot(s >= (upR ? argR : thrR));
              pm[ct] |= m;
              any |= m;
            }
            cntR = row16_isum(cntR);
            if ((lane & 15) == 0 && cntR) atomicAdd(&l_rowcnt[lrow0 + rt * 16 + reg], cntR);
          }
          if (any) {                                           // rare: a handful of such pairs per wave
#ifdef ALADIN_DIAG
            ++n_full;
#endif
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              if (!pm[ct]) continue;
              const int idx = n_mine + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(pm[ct] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)pm[ct], 0u));
              if (((pm[ct] >> lane) & 1ull) && idx < SIM_RAW_WAVE) my_raw[idx] = SimRaw{((lrow0 + rt * 16 + reg) << 16) | (lcol0 + ct * 16), acc[rt][ct][reg]};
              n_mine += __popcll(pm[ct]);
            }
          }
        }
      });
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        int c = cntC[ct];
        c += lane_xor16(c);
        c += lane_xor32(c);
        if (lane < 16 && c) atomicAdd(&l_colcnt[lcol0 + ct * 16], c);
      }
      if (lane == 0) l_rawn[wave] = n_mine;
#ifdef ALADIN_DIAG
      if (lane == 0 && (blockIdx.x & 63) == 0) { atomicAdd(&ra.stats[2], 32); atomicAdd(&ra.stats[3], n_full); atomicAdd(&ra.stats[4], 1); }     // a sample of the tiles
#endif
    }
    __syncthreads();
    SIM_STAMP(8);                                                    // (slots 8.. are the exact epilogue's: a listed tile never gets there)
    // ---- phase 2b: the raw candidates, one per thread: the per-pair decisions with the pair's own band
    {
      bool raw_over = hopeless;
#pragma unroll
      for (int w = 0; w < Cfg::NWAVES; ++w) raw_over |= l_rawn[w] > SIM_RAW_WAVE;
      if (!raw_over) {
        const int seg = tid >> 6, n_seg = l_rawn[seg];
        for (int slot = tid & 63; slot < n_seg; slot += 64) {
          const SimRaw rw = l_raw[seg * SIM_RAW_WAVE + slot];
          const int lr = rw.rc >> 16, lc = rw.rc & 0xffff;
          const float s = rw.s;
          const float P = l_P[lr], R = l_R[lr], Gr = l_Grow[lr], Lr = l_Lrow[lr];
          const float Gc = l_Gcol[lc], Qc = l_Q[lc], Tc = l_T[lc], Lc = l_Lcol[lc];
          const bool upR = s > l_hiRow[lr], upC = s > l_hiCol[lc];           // counted in phase 2a already
          const float band = fmaf(fabsf(s), 0x1p-14f, fmaf(P, Qc, R * Tc));
          const float hi = s + band, lo = s - band;
          int f = 0;
          const bool gr = upR | (lo > Gr), gc = upC | (lo > Gc);
          if (gr & !upR) atomicAdd(&l_rowcnt[lr], 1);
          if (gc & !upC) atomicAdd(&l_colcnt[lc], 1);
          if (hi >= Gr) { if (!gr) f |= SIM_F_ROWCNT; if (hi >= Lr) f |= SIM_F_ROWARG; }
          if (hi >= Gc) { if (!gc) f |= SIM_F_COLCNT; if (hi >= Lc) f |= SIM_F_COLARG; }
          if (f) {
            const int idx = atomicAdd(l_listn, 1);
            if (idx < SIM_LIST_CAP) l_list[idx] = SimEntry{mb * Cfg::BM + lr, nb * Cfg::BN + lc, s, f};
          }
        }
      } else if (tid == 0) {
        *l_listn = SIM_LIST_CAP + 1;                           // too many undecided scores / arg-max candidates: continue the chains in place
      }
    }
    __syncthreads();
    SIM_STAMP(4);
    const int n_list = *l_listn;
    exact = n_list > SIM_LIST_CAP;
    const int tile = mb * n_nblk + nb;
    if (threadIdx.x == 0) {
      ra.list_cnt[tile] = exact ? 0 : n_list;
      atomicAdd(&ra.stats[SIM_ST_ANALYSED], 1);
      if (exact) { atomicAdd(&ra.stats[SIM_ST_EXACT], 1); atomicAdd(&ra.stats[SIM_ST_OVERFLOW], 1); }
      else if (n_list) atomicAdd(&ra.stats[SIM_ST_LISTED], n_list);
    }
    if (!exact) {
      for (int q = threadIdx.x; q < Cfg::BM; q += Cfg::THREADS) {
        if (l_rowcnt[q]) atomicAdd(&ra.cnt_i2t[mb * Cfg::BM + q], l_rowcnt[q]);       // only valid rows ever count
        // the tile's certified lower bound of the row's exact maximum, for sim_rescore_kernel's filter
        if (l_rowmax[q]) atomicMax(&ra.lob_i2t[mb * Cfg::BM + q], float_key(l_Lrow[q]));
      }
      for (int q = threadIdx.x; q < Cfg::BN; q += Cfg::THREADS) {
        if (l_colcnt[q]) atomicAdd(&ra.cnt_t2i[nb * Cfg::BN + q], l_colcnt[q]);
        if (l_colmax[q]) atomicMax(&ra.lob_t2i[nb * Cfg::BN + q], float_key(l_Lcol[q]));
      }
      for (int q = threadIdx.x; q < n_list; q += Cfg::THREADS) ra.list[(int64_t)tile * SIM_LIST_CAP + q] = l_list[q];
      return;
    }
    } else if (threadIdx.x == 0) {
      ra.list_cnt[mb * n_nblk + nb] = 0;
      atomicAdd(&ra.stats[SIM_ST_EXACT], 1);
      atomicAdd(&ra.stats[SIM_ST_SKIPPED], 1);
    }
    __syncthreads();                                                 // the lists are dead: the stages may be refilled
  } else {
    if (threadIdx.x == 0) ra.list_cnt[mb * n_nblk + nb] = 0;
    __syncthreads();                                                 // the last K step's stage may be stage 0, which the continuation refills first
  }
  SIM_STAMP(5);
  gemm_mainloop16_tall<Cfg, true, KMapSplit>(a_tile, b_tile, ldk, 2 * kps, smem, acc, KMapSplit{kps, 1});     // lo.hi, hi.lo
  SIM_STAMP(6);
  sim_rank_epilogue_exact(acc, smem, mb, nb, n_img, n_cap, ra, n_nblk);
  SIM_STAMP(7);
}

// acc (+)= A[16 x K] . B[16 x K]^T over nblk ascending 32-deep K blocks, fragments straight from global memory (16 B per lane
// and block) with NB blocks of loads in flight: the chain of MFMAs is serial, the loads need not be.
// (sim_chain_lds of sim_pack.hip is the NB = 4 case with 32-bit offsets; kept apart: merging them changes sim_pack_gt_kernel's instruction text)
template <int NB = 8>
__device__ __forceinline__ void sim_chain_global(const half_t* __restrict__ ap, const half_t* __restrict__ bp, int nblk, f32x4& acc) {
  int k = 0;
  for (; k + NB <= nblk; k += NB) {
    half8 af[NB], bf[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      af[u] = *reinterpret_cast<const half8*>(ap + (int64_t)(k + u) * 32);
      bf[u] = *reinterpret_cast<const half8*>(bp + (int64_t)(k + u) * 32);
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u], bf[u], acc, 0, 0, 0);
  }
  if constexpr (NB > 8) {
    sim_chain_global<8>(ap + (int64_t)k * 32, bp + (int64_t)k * 32, nblk - k, acc);
    return;
  }
  for (; k < nblk; ++k) {
    const half8 af = *reinterpret_cast<const half8*>(ap + (int64_t)k * 32);
    const half8 bf = *reinterpret_cast<const half8*>(bp + (int64_t)k * 32);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc, 0, 0, 0);
  }
}

// Continue the chains of the listed pairs: 16 pairs per wave on the DIAGONAL of one 16 x 16 MFMA tile (row m of A = pair
// m's image, column m of B = pair m's caption, C[m][m] = its prefix s; the off-diagonal products are waste, the loads are
// what this costs: 4 x 2 Dp bytes per pair), then patch the counters / packed maxima with the exact value.
// Round 5: an entry listed ONLY as an arg-max candidate is first held against the certified bounds every tile left in
// lob_*: L* = the largest lower bound any tile proved for the row's (column's) exact maximum.  s + band < L* <= the maximum
// means the pair is strictly below it: no chain needed.  With ground truths inside the bulk every tile nominates the largest
// score of each column it holds (it cannot know the other tiles'), ~100 entries per tile, and all but ~one per column fall here.
// One workgroup per tile; its four waves take the tile's 16-entry groups in turn.
__global__ __launch_bounds__(256) void sim_rescore_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, int64_t ldk,
                                                          int kps, int n_tiles, SimRankArgs ra) {
  __shared__ SimEntry l_e[SIM_LIST_CAP];
  __shared__ int w_cnt[SIM_LIST_CAP / 256][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // SIM_RESCORE_SPLIT workgroups per tile.  Each filters and compacts the tile's WHOLE list -- in list order, so that all of them
  // build the same compacted list (ballot prefix sums, no atomics) -- and then takes the 16-pair groups whose index is its own modulo
  // the split: a tile that fills its 512 entries was a 32-group chain for ONE workgroup (80 us on the critical path of a launch
  // whose other tiles listed nothing), while splitting the list BEFORE compaction left every part with half-empty groups (a group
  // costs 98 KB of operand rows however few of its 16 pairs are live: sigma 8 went 0.385 -> 0.454 ms).
  // part-major block order: blocks [0, n_tiles) are part 0 of every tile.  (Tile-major -- part = blockIdx % 4 -- put the working
  // part-0 blocks on blockIdx = 0 mod 4, i.e. on TWO of the eight XCDs: the kernel ran 165 instead of 58 us.)
  const int tile = blockIdx.x % n_tiles, part = blockIdx.x / n_tiles;
  if (part >= SIM_RESCORE_SPLIT) return;
  const int n = ra.list_cnt[tile];
  // only a HEAVY list is shared out (more than a quarter of the capacity: the case the split exists for); below, part 0 takes everything
  // and the other parts leave at once -- every part filters the whole list, which is not free (sigma 6: + 19 us with every tile split)
  const int split = n > SIM_LIST_CAP / 4 ? SIM_RESCORE_SPLIT : 1;
  if (part >= split || n == 0) return;                                  // workgroup-uniform
  SimEntry mine[SIM_LIST_CAP / 256];
  int pre[SIM_LIST_CAP / 256];
#pragma unroll
  for (int pass = 0; pass < SIM_LIST_CAP / 256; ++pass) {
    const int q = pass * 256 + (int)threadIdx.x;
    SimEntry e = SimEntry{0, 0, 0.f, 0};
    if (q < n) {
      e = ra.list[(int64_t)tile * SIM_LIST_CAP + q];
      if (e.flags & (SIM_F_ROWARG | SIM_F_COLARG)) {
        const float2 pr = ra.na[e.row], qt = ra.nb[e.col];
        const float hi = e.s + fmaf(fabsf(e.s), 0x1p-14f, fmaf(pr.x, qt.x, pr.y * qt.y));
        if (e.flags & SIM_F_ROWARG) {
          const unsigned k = ra.lob_i2t[e.row];
          if (k && hi < key_float(k)) e.flags &= ~SIM_F_ROWARG;
        }
        if (e.flags & SIM_F_COLARG) {
          const unsigned k = ra.lob_t2i[e.col];
          if (k && hi < key_float(k)) e.flags &= ~SIM_F_COLARG;
        }
      }
    }
    mine[pass] = e;
    const unsigned long long live = __ballot(e.flags != 0);
    pre[pass] = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(live >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)live, 0u));
    if (lane == 0) w_cnt[pass][wave] = __popcll(live);
  }
  __syncthreads();
  int n_live = 0;
#pragma unroll
  for (int pass = 0; pass < SIM_LIST_CAP / 256; ++pass) {
    int base = n_live;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) base += w_cnt[pass][w];
      n_live += w_cnt[pass][w];
    }
    if (mine[pass].flags) l_e[base + pre[pass]] = mine[pass];
  }
  __syncthreads();
  if (threadIdx.x == 0 && part == 0 && n_live) atomicAdd(&ra.stats[SIM_ST_RESCORED], n_live);
  const int m = lane & 15;
  const int Dp = kps * 64;
  for (int grp = part + split * wave; grp * 16 < n_live; grp += 4 * split) {
    const bool need = grp * 16 + m < n_live;
    SimEntry e = SimEntry{0, 0, 0.f, 0};
    if (need) e = l_e[grp * 16 + m];
    const half_t* ap = a + (int64_t)e.row * ldk + 8 * (lane >> 4);
    const half_t* bp = b + (int64_t)e.col * ldk + 8 * (lane >> 4);
    const bool diag = (lane >> 4) == (m >> 2);                          // C[row][col]: col = lane & 15, row = 4 * (lane >> 4) + reg
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      if (diag && reg == (m & 3)) acc[reg] = e.s;
    sim_chain_global(ap + Dp, bp, 2 * kps, acc);                        // lo.hi
    sim_chain_global(ap, bp + Dp, 2 * kps, acc);                        // hi.lo
    if (!(need && diag)) continue;
    float v = acc[0];
#pragma unroll
    for (int reg = 1; reg < 4; ++reg)
      if (reg == (m & 3)) v = acc[reg];
    if (e.flags & (SIM_F_ROWCNT | SIM_F_ROWARG)) {
      if (e.flags & SIM_F_ROWCNT) {
        float g = -INFINITY;
        for (int q = 0; q < ra.cpi; ++q) g = fmaxf(g, ra.gt[e.row * ra.cpi + q]);
        if (v > g) atomicAdd(&ra.cnt_i2t[e.row], 1);
      }
      if (e.flags & SIM_F_ROWARG) atomicMax(&ra.best_i2t[e.row], pack_best(v, e.col));
    }
    if (e.flags & SIM_F_COLCNT) {
      if (v > ra.gt[e.col]) atomicAdd(&ra.cnt_t2i[e.col], 1);
    }
    if (e.flags & SIM_F_COLARG) atomicMax(&ra.best_t2i[e.col], pack_best(v, e.row));
  }
}

// Ground-truth scores gt[c] = chain(c / cpi, c) in the accumulators' scale, with the bits every other kernel that runs
// the chain produces for that pair (sim_common.hpp).  For 16 consecutive images the ground truths sit in the 16 x (16 * cpi) block
// starting at column 16 * cpi * t -- cpi aligned 16 x 16 tiles; one wave per tile, fragments straight from global memory
// (16 B per lane and K block).  The ground-truth pairs enter the arg-maxima here (the big kernel masks them out).
__global__ __launch_bounds__(256) void sim_gt_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, int n_img, int n_cap,
                                                     int cpi, int64_t ldk, int kps, float* __restrict__ gt,
                                                     unsigned long long* __restrict__ best_i2t, unsigned long long* __restrict__ best_t2i) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int t = tile / cpi, c = tile % cpi;
  if (t * 16 >= n_img) return;
  const int row_t = t * 16, col_t = t * 16 * cpi + c * 16;
  const half_t* ap = a + (int64_t)(row_t + (lane & 15)) * ldk + 8 * (lane >> 4);     // padded rows exist (Mp, Np)
  const half_t* bp = b + (int64_t)(col_t + (lane & 15)) * ldk + 8 * (lane >> 4);
  const int Dp = kps * 64;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // 1565 waves at configs[2] size, a wave and a half per SIMD: the kernel is a chain of load latencies, so a whole
  // segment's loads (24 blocks at D = 768) go out at once
  sim_chain_global<24>(ap, bp, 2 * kps, acc);                          // hi.hi   (the MFMA chain stays in K order)
  sim_chain_global<24>(ap + Dp, bp, 2 * kps, acc);                     // lo.hi
  sim_chain_global<24>(ap, bp + Dp, 2 * kps, acc);                     // hi.lo
  const int col = col_t + (lane & 15);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = row_t + 4 * (lane >> 4) + reg;
    if (row < n_img && col < n_cap && col / cpi == row) {
      gt[col] = acc[reg];
      if (best_i2t) {
        atomicMax(&best_i2t[row], pack_best(acc[reg], col));
        best_t2i[col] = pack_best(acc[reg], row);                      // one ground truth per column: a plain store, before the big kernel runs
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Fused retrieval, host side.
//   1. ground-truth scores (exact chain) on the band of 16 x 16 tiles that holds them
//   2. sim_screen_kernel: prefix + band per tile, lists or exact continuation
//   3. sim_rescore_kernel: the listed pairs, exactly
//   4. unpack_top1_kernel (recall.hip) unpacks the arg-maxima
// ------------------------------------------------------------------------------------------------
struct RetrWs {
  float* gt;
  unsigned long long *best_i2t, *best_t2i;
  int* stats;
  unsigned *lob_i2t, *lob_t2i;       // right behind the statistics: one zeroing range (stats_zero_words)
  int64_t stats_zero_words;
  int* list_cnt;
  SimEntry* list;
  size_t stats_off;                  // byte offset of `stats` in the workspace (aladin_retrieval_stats_offset)
};
static size_t retr_layout(int n_img, int n_cap, int D, char* base, RetrWs* w) {
  const int Mp = round_up(n_img, SimCfg::BM), Np = round_up(n_cap, SimCfg::BN), n_tiles = (Mp / SimCfg::BM) * (Np / SimCfg::BN);
  WsCursor c{base, (sim_ws_layout(n_img, n_cap, D, nullptr, nullptr) + 255) / 256 * 256};
  RetrWs r;
  r.gt = c.take<float>(n_cap, 256);
  r.best_i2t = c.take<unsigned long long>(n_img, 256);
  r.best_t2i = c.take<unsigned long long>(n_cap, 256);
  r.stats_off = c.off;
  r.stats = c.take<int>(SIM_STATS_WORDS, 256);
  r.lob_i2t = c.take<unsigned>(Mp, 256);
  r.lob_t2i = c.take<unsigned>(Np, 256);
  r.stats_zero_words = (int64_t)((c.off - r.stats_off) / 4);
  r.list_cnt = c.take<int>(n_tiles, 256);
  r.list = c.take<SimEntry>((size_t)n_tiles * SIM_LIST_CAP, 256);
  if (w) *w = r;
  return c.off;
}

extern "C" size_t aladin_retrieval_workspace_bytes(int n_img, int n_cap, int D) {
  if (n_img < 1 || n_cap < 1 || D < 1) return 0;
  return retr_layout(n_img, n_cap, D, nullptr, nullptr);
}

extern "C" size_t aladin_retrieval_stats_offset(int n_img, int n_cap, int D) {
  if (n_img < 1 || n_cap < 1 || D < 1) return 0;
  RetrWs rw;
  retr_layout(n_img, n_cap, D, nullptr, &rw);
  return rw.stats_off;
}

// reserve, launch, check: one MODE of sim_screen_kernel over the packed operands
template <int MODE>
static int sim_screen_launch(const SimPacked& p, int n_img, int n_cap, const SimRankArgs& ra, hipStream_t st) {
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)sim_screen_kernel<MODE>, SimCfg::LDS_BYTES, &lds_reserved, "sim_screen")) return rc;
  const int n_mblk = p.Mp / SimCfg::BM, n_nblk = p.Np / SimCfg::BN;
  hipLaunchKernelGGL(sim_screen_kernel<MODE>, dim3(n_mblk * n_nblk), dim3(SimCfg::THREADS), SimCfg::LDS_BYTES, st, p.ws.a, p.ws.b, p.ws.scale, n_img,
                     n_cap, (int64_t)2 * p.Dp, p.Dp / 64, n_nblk, n_mblk * n_nblk, ra);
  return aladin_check_launch("sim_screen_kernel");
}

static int retrieval_ranks_impl(const float* img, int64_t img_rs, const float* cap, int64_t cap_rs, int n_img, int n_cap,
                                int D, int caps_per_img, int32_t* rank_i2t, int32_t* top1_i2t, int32_t* rank_t2i,
                                int32_t* top1_t2i, void* workspace, void* stream, bool force_exact) {
  if (!img || !cap || !rank_i2t || !top1_i2t || !rank_t2i || !top1_t2i || !workspace || D < 1 || img_rs < D || cap_rs < D) {
    aladin_set_error("retrieval_ranks: bad argument");
    return ALADIN_ERR_ARG;
  }
  if (n_img < 1 || caps_per_img < 1 || n_cap != n_img * caps_per_img) {
    aladin_set_error("retrieval_ranks: need n_cap == n_img * caps_per_img (n_img=%d n_cap=%d cpi=%d)", n_img, n_cap, caps_per_img);
    return ALADIN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  RetrWs rw;
  retr_layout(n_img, n_cap, D, (char*)workspace, &rw);
  // the pack grid zeroes the statistics and the two rank (= counter) arrays.  The arg-max arrays: when the ground truths come out of
  // the packing pass (sim_pack_gt_kernel) every entry is first written, a plain store, with its ground-truth pair and nothing is
  // zeroed; when they need their own kernel (below), best_i2t is zeroed first (sim_gt_kernel's tiles meet there in an atomicMax)
  // and best_t2i is a plain store, one ground truth per column
  SimFusedPrep fused{caps_per_img, rw.gt, rw.best_i2t, rw.best_t2i, {rw.stats, rank_i2t, rank_t2i}, {rw.stats_zero_words, n_img, n_cap}, false};
  SimPacked p;
  int rc = sim_prepare(SimIn{img, img_rs, cap, cap_rs, n_img, n_cap, D}, workspace, st, &p, &fused);
  if (rc) return rc;
  const SimWs& ws = p.ws;
  // the band's 2^-14 |s| term allows for the fp32 rounding of at most ~2^10 more accumulator steps: wider rows take
  // the exact path on every tile
  if (p.Dp / 16 > 1024) force_exact = true;
  const int n_tiles = (p.Mp / SimCfg::BM) * (p.Np / SimCfg::BN);
  const int64_t ldk = (int64_t)2 * p.Dp;
  const int kps = p.Dp / 64;
  SimRankArgs ra{};
  ra.cpi = caps_per_img;
  ra.gt = rw.gt;
  ra.na = ws.na;
  ra.nb = ws.nb;
  ra.cnt_i2t = rank_i2t;                                 // the row counters ARE the i2t ranks
  ra.cnt_t2i = rank_t2i;                                 // the column counters ARE the t2i ranks
  ra.best_i2t = rw.best_i2t;
  ra.best_t2i = rw.best_t2i;
  ra.list = rw.list;
  ra.list_cnt = rw.list_cnt;
  ra.stats = rw.stats;
  ra.lob_i2t = rw.lob_i2t;
  ra.lob_t2i = rw.lob_t2i;
  if (!fused.gt_done) {
    if (hipMemsetAsync(rw.best_i2t, 0, (size_t)n_img * 8, st) != hipSuccess) { aladin_set_error("retrieval_ranks: memset failed"); return ALADIN_ERR_HIP; }
    const int tiles = cdiv(n_img, 16) * caps_per_img;
    hipLaunchKernelGGL(sim_gt_kernel, dim3(cdiv(tiles, 4)), dim3(256), 0, st, ws.a, ws.b, n_img, n_cap, caps_per_img, ldk, kps, rw.gt,
                       rw.best_i2t, rw.best_t2i);
  }
#ifdef ALADIN_DIAG
  static const char* probe_env = getenv("ALADIN_SIM_SKIP_PROBE");
  if (!force_exact && probe_env && probe_env[0] == '1') rc = sim_screen_launch<2>(p, n_img, n_cap, ra, st);
  else
#endif
  rc = force_exact ? sim_screen_launch<1>(p, n_img, n_cap, ra, st) : sim_screen_launch<0>(p, n_img, n_cap, ra, st);
  if (rc) return rc;
  if (!force_exact) {
    hipLaunchKernelGGL(sim_rescore_kernel, dim3(n_tiles * SIM_RESCORE_SPLIT), dim3(256), 0, st, ws.a, ws.b, ldk, kps, n_tiles, ra);
    rc = aladin_check_launch("sim_rescore_kernel");
    if (rc) return rc;
  }
  return sim_unpack_top1_launch(rw.best_i2t, n_img, top1_i2t, rw.best_t2i, n_cap, top1_t2i, st);
}

extern "C" int aladin_retrieval_ranks(const float* img, int64_t img_rs, const float* cap, int64_t cap_rs, int n_img, int n_cap,
                                      int D, int caps_per_img, int32_t* rank_i2t, int32_t* top1_i2t, int32_t* rank_t2i,
                                      int32_t* top1_t2i, void* workspace, void* stream) {
  return retrieval_ranks_impl(img, img_rs, cap, cap_rs, n_img, n_cap, D, caps_per_img, rank_i2t, top1_i2t, rank_t2i, top1_t2i, workspace,
                              stream, false);
}

extern "C" int aladin_retrieval_ranks_exact(const float* img, int64_t img_rs, const float* cap, int64_t cap_rs, int n_img, int n_cap,
                                            int D, int caps_per_img, int32_t* rank_i2t, int32_t* top1_i2t, int32_t* rank_t2i,
                                            int32_t* top1_t2i, void* workspace, void* stream) {
  return retrieval_ranks_impl(img, img_rs, cap, cap_rs, n_img, n_cap, D, caps_per_img, rank_i2t, top1_i2t, rank_t2i, top1_t2i, workspace,
                              stream, true);
}
