// Alignment scores S[i][j] = sum_w max_r <im^[i,r], s^[j,w]>  ('MrSw', reference
// alad/loss.py:79-125) for gfx950.  The operands are packed by pack.hip in the format of pack_rows.hpp, which folds every mask of
// the reference into the data (zero rows, tile-filling copies of region 0): the score kernel is mask-free.
//
// score kernel   one tile of whole images x whole captions per workgroup: LDS-staged fp16 MFMA GEMM (gemm_core.hpp) with regions
//                on the MFMA row axis and words on the lane axis, so max-over-regions is an in-lane max over the accumulator
//                registers plus one or two lane exchanges, and sum-over-words is a 16-lane reduction.  The B x B x R' x T'
//                tensor of the reference never exists.
//                Bodies (select_scores picks one from the class table of aladin_align_geometry and the grid size).  The
//                16x16x32 ones share one LDS image, one K order and one epilogue arithmetic (scores16_epilogue; the r48 body's own
//                scores16_epilogue_r48 does the same operations in the same order), so a score is bit-identical whichever computed it:
//                  align_scores16_tall_kernel   128 x 96 wave tiles, 2 x 4 waves = 256 x 384 (headline class: 14 LDS fragment
//                                               reads per 32-deep step); 128 x 80 for 40-word captions, 1 x 2 waves on their small grids
//                  align_scores16_kernel        64 x 192 wave tiles: 4 x 2 waves (16 reads; captions that do not tile 96 columns),
//                                               or 2 x 1 waves with a three-stage ring on grids of <= 64 big tiles (B <= 64)
//                  align_scores16_r48_kernel    the 48-row region class: 96 x 96 (96 x 80) wave tiles, 2 x 4 or 1 x 2 waves
//                  align_scores16_r48x3_kernel  48 rows x 40 words on large grids: 144 x 80 wave tiles, 288 x 320 per workgroup
//                  align_scores_kernel          v_mfma_f32_32x32x16_f16, the 96-row region class (an epilogue of its own)
//                align_argmax16_{tall,r48}_kernel: the same tiles and main loop, recording WHICH region won (argmax16_epilogue).
// side GEMM      R' = 33 = 32 + 1: the 33rd region of every image is gathered into one extra
//                operand (one row per image) whose plain GEMM against the captions (E) is folded
//                into the max by the score kernel -- 33/32 of the MFMA work instead of 64/32.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <tuple>
#include <type_traits>

#include "../../include/aladin_hip.h"
#include "gemm_core.hpp"
#include "pack_rows.hpp"

// ------------------------------------------------------------------------------------------------
// geometry
// ------------------------------------------------------------------------------------------------
extern "C" int aladin_align_geometry(int Bi, int Bc, int R, int T, int D, int x_tail, int y_tail, int precision, int layout,
                                     aladin_align_geom* g) {
  if (precision != ALADIN_PRECISION_FP16 && precision != ALADIN_PRECISION_SPLIT) { aladin_set_error("align_geometry: unknown precision %d", precision); return ALADIN_ERR_ARG; }
  if (layout < ALADIN_LAYOUT_AUTO || layout > ALADIN_LAYOUT_LONG) { aladin_set_error("align_geometry: unknown layout %d", layout); return ALADIN_ERR_ARG; }
  if (!g || Bi < 1 || Bc < 1 || D < 1) { aladin_set_error("align_geometry: bad sizes Bi=%d Bc=%d D=%d", Bi, Bc, D); return ALADIN_ERR_ARG; }
  if (x_tail < 0 || y_tail < 0 || x_tail > 8 || y_tail > 8) { aladin_set_error("align_geometry: bad tails %d %d", x_tail, y_tail); return ALADIN_ERR_ARG; }
  if (R < 2 + x_tail || T < 2 + y_tail) { aladin_set_error("align_geometry: sets too short (R=%d T=%d): position 0 and the last %d / %d positions are dropped", R, T, x_tail, y_tail); return ALADIN_ERR_ARG; }
  const bool past_tiles = R - 1 - x_tail > ALADIN_TILE_MAX_SCORED || T - 1 - y_tail > ALADIN_TILE_MAX_SCORED;
  if (layout == ALADIN_LAYOUT_AUTO) layout = past_tiles ? ALADIN_LAYOUT_LONG : ALADIN_LAYOUT_TILES;
  if (layout == ALADIN_LAYOUT_LONG) return aladin_internal_long_layout(Bi, Bc, R, T, D, x_tail, y_tail, precision, g);
  memset(g, 0, sizeof(*g));
  g->Bi = Bi; g->Bc = Bc; g->R = R; g->T = T; g->D = D;
  g->x_tail = x_tail; g->y_tail = y_tail;
  g->split = precision != ALADIN_PRECISION_FP16;
  g->layout = layout;
  g->Rq = R - 1 - x_tail; g->Tq = T - 1 - y_tail;
  if (past_tiles) { aladin_set_error("align_geometry: at most 97 regions / 99 tokens supported (got R=%d T=%d)", R, T); return ALADIN_ERR_UNSUPPORTED; }
  // R' = mrows + rem: `mrows` rows per image in the main operand (16-row MFMA tiles; rows past R' repeat region 0), `rem`
  // leftover regions per image go through the side GEMM instead of opening another tile (measured at B=256, T=50, D=768, forward
  // incl. packing: R'=34 0.183 vs 0.271 ms with a second region tile, R'=36 0.200 vs 0.273, R'=38 0.215 vs 0.277, R'=40 0.236 vs 0.276).
  //   33..40  : 32 rows + rem side rows (up to 8)
  //   41..56  : 48 rows (three 16-row tiles) + up to 8 side rows -- VinVL's 50 regions, the shape every shipped YAML trains
  //             on, pays for 48 + 2 rows instead of 64 (round 4; captions must tile a 96-column strip: tp16 in {1, 2, 3, 6})
  //   65      : 64 rows + one side row;   everything else: the next multiple of 32, no side rows
  g->tp16 = cdiv(g->Tq, 16);
  if (g->tp16 == 5) g->tp16 = 6;
  if (g->Rq > 32 && g->Rq <= 40) { g->mrows = 32; g->rem = g->Rq - 32; }
  else if (g->Rq > 40 && g->Rq <= 56 && 6 % g->tp16 == 0) { g->mrows = 48; g->rem = g->Rq > 48 ? g->Rq - 48 : 0; }
  else if (g->Rq == 65) { g->mrows = 64; g->rem = 1; }
  else { g->mrows = 32 * cdiv(g->Rq, 32); g->rem = 0; }
  // split precision: every packed row is three K segments of round_up(D, 64) halfs -- [hi | lo | hi] on the max
  // side, [hi | hi | lo] on the sum side -- so the unchanged main loops contract hi.hi + lo.hi + hi.lo
  g->Dp = round_up(D, 64) * (g->split ? 3 : 1);
  g->img_unit = (g->mrows == 32) ? 8 : 4;                     // images per workgroup tile: 256 rows (192 in the 48-row class, 384 at 96)
  // captions per unit: one 384-row score tile (the 16x16x32 kernels, up to 64 main rows); two 32-column tiles otherwise
  g->cap_unit = (g->mrows <= 64) ? 24 / g->tp16 : 2 * ((g->tp16 & 1) ? 2 : 1);
  // rows per caption in y: whole 16-word tiles, except the "half" classes -- T' <= 8 packs a caption into half a tile, T' 17..24
  // into 1.5, T' 33..40 (VinVL's 35-token captions: 35 words of 48 would be 27 % padding) into 2.5: two captions share 1 / 3 / 5
  // tiles and the epilogue splits the middle one between them by lane (caption_add).  Region classes of the 16x16x32 kernels (32,
  // 48 or 64 main rows); not under ALADIN_LAYOUT_TILES_WHOLE (the arg-max table kernel of the dense backward keeps
  // whole tiles).  Captions per unit: 384 / 640 rows = whole score tiles (384; 320 and 160 columns) and side GEMM tiles (64 / 128).
  g->trows = 16 * g->tp16;
  if (layout != ALADIN_LAYOUT_TILES_WHOLE && g->mrows <= 64) {
    if (g->Tq <= 8) { g->trows = 8; g->cap_unit = 48; }
    else if (g->Tq > 16 && g->Tq <= 24) { g->trows = 24; g->cap_unit = 16; }
    else if (g->Tq > 32 && g->Tq <= 40) { g->trows = 40; g->cap_unit = 16; }
  }
  g->Bi_pad = round_up(Bi, g->img_unit);
  g->Bc_pad = round_up(Bc, g->cap_unit);
  g->xm_rows = (int64_t)g->Bi_pad * g->mrows;
  g->xe_rows = g->rem ? round_up(g->Bi_pad * g->rem, 64) : 0;      // image i: rows [i*rem, i*rem + rem)
  g->y_rows = (int64_t)g->Bc_pad * g->trows;
  g->xm_bytes = g->xm_rows * g->Dp * 2;
  g->xe_bytes = g->xe_rows * g->Dp * 2;
  g->y_bytes = g->y_rows * g->Dp * 2;
  g->e_bytes = g->xe_rows * g->y_rows * 4;
  g->rnorm_bytes = (g->xm_rows + g->xe_rows + g->y_rows) * 4;
  return ALADIN_OK;
}

// ------------------------------------------------------------------------------------------------
// side GEMM: E[i][col] = <last region of image i, word col>   (fp32, xe_rows x y_rows)
// ------------------------------------------------------------------------------------------------
// one workgroup tile of E (tile index bid); shared by align_side_gemm_kernel and align_side_pack_kernel (below)
template <int NT, int SWM, int NS>
__device__ __forceinline__ void side_gemm_tile(const half_t* __restrict__ xe, const half_t* __restrict__ y, float* __restrict__ E,
                                               int64_t ldE, int64_t ldk, int ktiles, int n_nblk, unsigned bid) {
  using Cfg = GemmCfg<2, 2, SWM, NT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int mb = bid / n_nblk, nb = bid % n_nblk;
  f32x16 acc[SWM][NT];
#pragma unroll
  for (int m = 0; m < SWM; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
  gemm_mainloop<Cfg, NS>(xe + (int64_t)mb * Cfg::BM * ldk, y + (int64_t)nb * Cfg::BN * ldk, ldk, ktiles, smem, acc);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave / 2, wn = wave % 2;
  const int64_t row0 = (int64_t)mb * Cfg::BM + wm * SWM * 32 + 4 * (lane >> 5);
  const int64_t col0 = (int64_t)nb * Cfg::BN + wn * NT * 32 + (lane & 31);
#pragma unroll
  for (int m = 0; m < SWM; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        E[(row0 + m * 32 + (r & 3) + 8 * (r >> 2)) * ldE + col0 + n * 32] = acc[m][n][r];
}

template <int NT, int SWM, int NS>
__global__ __launch_bounds__(256) void align_side_gemm_kernel(const half_t* __restrict__ xe, const half_t* __restrict__ y,
                                                              float* __restrict__ E, int64_t ldE, int64_t ldk,
                                                              int ktiles, int n_nblk) {
  side_gemm_tile<NT, SWM, NS>(xe, y, E, ldE, ldk, ktiles, n_nblk, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// triplet forward prologue: [side GEMM tiles | blocks that pack the main image rows] in one launch (side_packs_main)
// ------------------------------------------------------------------------------------------------
static const int MAIN_PACK_ROWS = 8;        // rows a wave of a pack block has in flight
struct MainPack {
  const float* im; int64_t sb, sr; const int32_t* len;      // the raw image set
  int Bi, Rq, x_tail, D, Dp, mrows;
  int64_t xm_rows;
  half_t* xm; float* rnorm;                                 // rnorm may be nullptr
};

// Rows [0, xm_rows) of the main operand, MAIN_PACK_ROWS at a time per wave: wave w of n_waves takes the batches w, w + n_waves, ...
// The encoder's fp16 whole-row-in-registers form for each row (pack_rows.hpp: the bits pack_rows_kernel gives these rows), but the
// loads of all the batch's rows are issued before the first row is reduced.
__device__ __forceinline__ void pack_main_rows(const MainPack& m, int w, int n_waves) {
  constexpr int RB = MAIN_PACK_ROWS;
  const int lane = threadIdx.x & 63;
  for (int64_t d0 = (int64_t)w * RB; d0 < m.xm_rows; d0 += (int64_t)n_waves * RB) {
    const int i = (int)(d0 / m.mrows), k0 = (int)(d0 % m.mrows);        // mrows % RB == 0: one image per batch
    const int L = i < m.Bi ? scored_len(m.len[i], m.x_tail, m.Rq) : 0;  // regions of image i that count (alad/loss.py:89)
    float4 v[RB][4];
    int rho[RB];
    // a row of an image of the batch exists in memory whether its length masks it or not; an image that pads the batch has no columns
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      rho[j] = main_row_region(k0 + j, m.Rq);
      load_row_regs(v[j], m.im + i * m.sb + (int64_t)(rho[j] + 1) * m.sr, i < m.Bi ? m.D : 0, lane);      // region 0 dropped (alad/loss.py:87)
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      half_t* dst = m.xm + (d0 + j) * m.Dp;
      float* slot = m.rnorm ? m.rnorm + d0 + j : nullptr;
      if (rho[j] >= L) {                         // masked region, or an image that pads the batch: a zero row
        write_zero_row(dst, m.Dp, lane);
        write_rnorm(slot, 0.f, lane);
        continue;
      }
      const float inv = inv_norm_regs(v[j]);
      write_rnorm(slot, inv, lane);
      write_fp16_regs(dst, v[j], inv, m.Dp, lane);
    }
  }
}

// Grid [n_side side tiles | pack blocks].  No block reads what another block of the launch writes: the side tiles read xe and y
// (packed by the launch before) and write E; the pack blocks read the raw images and write xm and its rnorm entries.
// Whether the two overlap or merely run one after the other is decided by two things:
//   * few, fat pack blocks.  Dynamic LDS is per launch, so a pack block reserves the side tile's 64-120 KB as well and at most two
//     blocks share a CU; thousands of four-row blocks (pack_rows_kernel's shape) would leave HBM a handful of waves per CU.  So:
//     about one pack block per CU, each of its four waves with the loads of MAIN_PACK_ROWS rows in flight before it reduces any
//     (8 rows x 3 float4 a lane at D = 768: 96 VGPRs, ~96 KB in flight per CU), looping over batches when there are more rows;
//   * side tiles first in block order: they are dispatched first and set the length of the launch, and the pack blocks fill the
//     second slot of each CU (or the CUs a small grid of three-stage tiles leaves empty).
// Measured at B = 256, R = 34, T = 50, D = 768: the launch takes 15.2 us against the side GEMM's 11.8 alone, for
// 5.3 us of packing taken out of the launch before.  Half as many pack blocks with two batches each, pack blocks first in block
// order, four rows in flight, a raised wave priority for the side tiles, nontemporal loads and stores: none was faster.
template <int NT, int SWM, int NS>
__global__ __launch_bounds__(256) void align_side_pack_kernel(const half_t* __restrict__ xe, const half_t* __restrict__ y,
                                                              float* __restrict__ E, int64_t ldE, int64_t ldk, int ktiles,
                                                              int n_nblk, int n_side, MainPack mp) {
  if ((int)blockIdx.x < n_side) {
    side_gemm_tile<NT, SWM, NS>(xe, y, E, ldE, ldk, ktiles, n_nblk, blockIdx.x);
    return;
  }
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  pack_main_rows(mp, ((int)blockIdx.x - n_side) * 4 + wave, ((int)gridDim.x - n_side) * 4);
}

// Named first among the kernels of this file on purpose.  The score and arg-max kernels are sensitive to WHERE they lie in the code
// object (DESIGN_HISTORY.md, "Alignment backward: plain stages ..." and "Packed operands: one row map ..."): when the pack kernels
// left this file for pack.hip every kernel behind them moved up by 0x3900 bytes and the headline step lost 0.7 %.  This
// instantiation is 0x3900 bytes long; emitted here, ahead of the others, it puts each of them back at its old address.  It is one
// of the twelve that aladin_internal_side_with_main_pack (end of the file) launches anyway -- no kernel and no byte is added.
template __global__ void align_side_pack_kernel<3, 2, 2>(const half_t*, const half_t*, float*, int64_t, int64_t, int, int, int, MainPack);

// Diagnostic build only (the PROBE instantiation of align_scores16_kernel): per-workgroup shader-clock and 100 MHz real-time
// deltas around the main loop -> in-kernel clock = d(memtime)/d(memrealtime) * 100 MHz.
#ifdef ALADIN_DIAG
__device__ unsigned long long g_clock_probe[4 * 4096];
__device__ unsigned long long g_clock_cycles[2048];
#define ALADIN_DIAG_API extern "C" __attribute__((visibility("default")))

ALADIN_DIAG_API int aladin_debug_read_clock_cycles(unsigned long long* host_out, int n_blocks) {
  if (!host_out || n_blocks < 1 || n_blocks > 2048) { aladin_set_error("debug_read_clock_cycles: bad argument"); return ALADIN_ERR_ARG; }
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_clock_cycles), (size_t)n_blocks * 8) != hipSuccess) { aladin_set_error("debug_read_clock_cycles: copy failed"); return ALADIN_ERR_HIP; }
  return ALADIN_OK;
}

ALADIN_DIAG_API int aladin_debug_read_clock_probe(unsigned long long* host_out, int n_blocks) {
  if (!host_out || n_blocks < 1 || n_blocks > 4096) { aladin_set_error("debug_read_clock_probe: bad argument"); return ALADIN_ERR_ARG; }
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_clock_probe), (size_t)n_blocks * 32) != hipSuccess) { aladin_set_error("debug_read_clock_probe: copy failed"); return ALADIN_ERR_HIP; }
  return ALADIN_OK;
}
#endif  // ALADIN_DIAG

// ------------------------------------------------------------------------------------------------
// score kernel, v_mfma_f32_32x32x16_f16 body (the 96-row region class: R' 66..96, no side rows)
//   WM   M-tiles (32 rows) per wave = Q, the M-tiles per image: a wave's rows are ONE image
//   TP16 padded words per caption / 16;  a wave's column strip holds CPS = 1 or 2 whole captions
// ------------------------------------------------------------------------------------------------
template <int WM, int Q, int TP16, bool HAS_E>
__global__ __launch_bounds__(512) void align_scores_kernel(const half_t* __restrict__ xm, const half_t* __restrict__ y,
                                                           const float* __restrict__ E, int64_t ldE,
                                                           float* __restrict__ S, int64_t ldS, int Bi, int Bc,
                                                           int64_t ldk, int ktiles, int n_nblk, int n_blocks) {
  static_assert(WM == Q && !HAS_E, "one image per wave and no side rows: the one class this body serves (E and ldE are not read)");
  constexpr int WGM = 4;
  constexpr int NT = (TP16 & 1) ? TP16 : TP16 / 2;
  constexpr int CPS = (TP16 & 1) ? 2 : 1;
  using Cfg = GemmCfg<WGM, 2, WM, NT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 4, mb, nb);

  f32x16 acc[WM][NT];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][n][r] = 0.f;

  const half_t* a_rows = xm + (int64_t)mb * Cfg::BM * ldk;
  const half_t* b_rows = y + (int64_t)nb * Cfg::BN * ldk;
  gemm_mainloop<Cfg, 2, true>(a_rows, b_rows, ldk, ktiles, smem, acc);      // refill spread over the four MFMA groups

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave / 2, wn = wave % 2;
  const int l5 = lane & 31;

  // max over regions: 16 accumulator rows per lane and M-tile, then the other half-wave's
  float m[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    float p = acc[0][n][0];
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) p = fmaxf(p, acc[a][n][r]);
    m[n] = fmaxf(p, __shfl_xor(p, 32, 64));
  }
  const int img = mb * WGM + wm;

  // sum over words: 16-lane groups map to captions at compile time
  float v[CPS];
#pragma unroll
  for (int c = 0; c < CPS; ++c) v[c] = 0.f;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int c_lo = (2 * n) / TP16, c_hi = (2 * n + 1) / TP16;       // captions of the tile's two 16-column groups
    if (c_lo == c_hi) v[c_lo] += m[n];
    else { v[c_lo] += (l5 < 16) ? m[n] : 0.f; v[c_hi] += (l5 >= 16) ? m[n] : 0.f; }
  }
  const int cap = (nb * 2 + wn) * CPS;
#pragma unroll
  for (int c = 0; c < CPS; ++c) {
    const float t = half_wave_sum(v[c]);
    if (lane == 0 && img < Bi && cap + c < Bc) S[(int64_t)img * ldS + cap + c] = t;
  }
}

// IEEE-754-2019 maximum (v_maximum3_f32 on gfx950): unlike fmaxf / maxNum it needs no canonicalising v_max x, x, x of its
// inputs in IEEE mode (a third of the epilogue's VALU instructions), and like torch.max it propagates a NaN
__device__ __forceinline__ float vmax(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// max over lane i and lane i ^ 16 without the ds_bpermute round trip: v_permlane16_swap exchanges the odd 16-lane rows of its
// first operand with the even rows of its second; fed the same value twice it leaves [r0 r0 r2 r2] and [r1 r1 r3 r3]
__device__ __forceinline__ float max_xor16(float m) {
  auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return vmax(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}
__device__ __forceinline__ float max_xor32(float m) {
  auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return vmax(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}

// max of the values a lane holds of one image and one column -- TPI 16-row tiles from t0 on, four registers each -- written as
// one chain so that the compiler emits v_max3_f32 (4 instructions for 8 values instead of 7; max is exact in any order)
template <int TPI, int RT, int CT>
__device__ __forceinline__ float image_max(const f32x4 (&acc)[RT][CT], int t0, int ct) {
  float t = acc[t0][ct][0];
#pragma unroll
  for (int i = 1; i < 4 * TPI; ++i) t = vmax(t, acc[t0 + i / 4][ct][i % 4]);
  return t;
}

// Word sums of the "half" caption classes (8, 24 and 40 words: trows = 16 TP16 - 8): two captions share 2 TP16 - 1 column tiles,
// the middle one split between them by lane column (0-7 / 8-15).  ct is a compile-time constant in the unrolled callers.
template <int TP16, bool HALF, int NC>
__device__ __forceinline__ void caption_add(float (&v)[NC], int ct, int l4, float m) {
  if constexpr (!HALF) {
    v[ct / TP16] += m;
  } else {
    constexpr int G = 2 * TP16 - 1;
    const int p = ct / G, w = ct % G;
    if (w < TP16 - 1) v[2 * p] += m;
    else if (w > TP16 - 1) v[2 * p + 1] += m;
    else { v[2 * p] += l4 < 8 ? m : 0.f; v[2 * p + 1] += l4 < 8 ? 0.f : m; }
  }
}

// ------------------------------------------------------------------------------------------------
// score kernels, v_mfma_f32_16x16x32_f16 bodies: the epilogue of all of them.  A wave holds Cfg::RT16 x Cfg::CT16 accumulator
// tiles of 16 x 16: RT16 / TPI images of TPI row tiles each (TPI = 2: 32 main rows, 3: 48, 4: 64) x whole captions.
//   max over regions : in-lane over an image's TPI row tiles x 4 registers (image_max).  Images are finished in pairs:
//                      v_permlane32_swap gathers the first into lanes 0-31 and the second into lanes 32-63; an odd last image
//                      is finished by both half-waves.  One 16-lane exchange completes the rows; the side rows join from E.
//   sum over words   : a caption's column tiles in ascending order, in-lane (caption_add), then a 16-lane reduction
// Every body calls this one function, so a score gets the same operations in the same order -- and the same bits -- whichever
// computed it (the order of a max is free; that of the word sum is not).
//   REMC     side rows per image known at compile time (1, or 2 -- VinVL's 50 regions = 48 + 2; a run-time trip count costs
//            the headline kernel ~10 %, the 48-row one several per cent); 0: `rem` of them, up to 8, a run-time count
//   OVERHANG the workgroup's last row tile may hang over the operand's end: E is read at the last of the n_img images that exist
//            instead (such an image's scores are not stored); n_img is not looked at otherwise
// ------------------------------------------------------------------------------------------------
template <class Cfg, int TPI, bool HAS_E, int TP16, int REMC, bool HALF, bool OVERHANG = false>
__device__ __forceinline__ void scores16_epilogue(f32x4 (&acc)[Cfg::RT16][Cfg::CT16], int mb, int nb, const float* __restrict__ E,
                                                  int64_t ldE, int rem, float* __restrict__ S, int64_t ldS, int Bi, int Bc, int n_img = 0) {
  constexpr int CT = Cfg::CT16, NI = Cfg::RT16 / TPI;
  static_assert(Cfg::RT16 % TPI == 0, "whole images per wave");
  constexpr int NC = HALF ? 2 * CT / (2 * TP16 - 1) : CT / TP16;     // captions of the wave's column strip
  static_assert(HALF ? (CT % (2 * TP16 - 1) == 0) : (CT % TP16 == 0), "a caption must be a whole number of 16-word column tiles of the strip, or two captions 2 TP16 - 1 tiles");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave / Cfg::WGN, wn = wave % Cfg::WGN;
  const int half = lane >> 5, l4 = lane & 15;
  if constexpr (REMC >= 1) rem = REMC;
  const int cap = (nb * Cfg::WGN + wn) * NC;
#pragma unroll
  for (int i0 = 0; i0 < NI; i0 += 2) {
    const bool pair = i0 + 1 < NI;                                   // compile-time once unrolled
    const int img = (mb * Cfg::WGM + wm) * NI + i0 + (pair ? half : 0);
    int img_e = img;
    if constexpr (OVERHANG) img_e = img < n_img ? img : n_img - 1;
    const float* e = HAS_E ? E + (int64_t)img_e * rem * ldE + (int64_t)nb * Cfg::BN + wn * Cfg::WCOLS + l4 : nullptr;
    float v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = 0.f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      // rows are spread over the four 16-lane quarters
      float m = image_max<TPI>(acc, i0 * TPI, ct);
      if (pair) {
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(image_max<TPI>(acc, (i0 + 1) * TPI, ct)), false, false);
        m = vmax(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      } else {
        m = max_xor32(m);
      }
      m = max_xor16(m);
      if constexpr (HAS_E) {
        // REMC == 0 is branch-free: max is idempotent, so rows past the last side row re-read it (k clamped to rem - 1)
#pragma unroll
        for (int k = 0; k < (REMC ? REMC : 8); ++k) m = vmax(m, e[(int64_t)(REMC || k < rem ? k : rem - 1) * ldE + ct * 16]);
      }
      caption_add<TP16, HALF, NC>(v, ct, l4, m);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float t = row16_sum(v[c]);
      if ((lane & (pair ? 31 : 63)) == 0 && img < Bi && cap + c < Bc) S[(int64_t)img * ldS + cap + c] = t;
    }
  }
}

// The epilogue's side-row values were written by the side GEMM on OTHER XCDs: pull this wave's -- RT16 / TPI images x REMC rows x
// WCOLS columns, in lines of 32 floats -- into this XCD's L2 before the main loop, so that the epilogue's loads do not pay an HBM /
// fabric round trip 25 us from here.  An 80-column strip is not line aligned: up to four lines, touched at floats 0, 32, 64, 79.
// The data itself is dropped: one LDS-DMA dword per lane into the piece of stage 1 that this same wave overwrites with its own
// (later, in-order) refill.  OVERHANG / n_img: as in scores16_epilogue.
template <class Cfg, int TPI, int REMC, bool OVERHANG = false>
__device__ __forceinline__ void side_prefetch(const float* __restrict__ E, int64_t ldE, int mb, int nb, char* smem, int n_img = 0) {
  constexpr int NI = Cfg::RT16 / TPI;
  constexpr int LPR = Cfg::WCOLS % 32 ? Cfg::WCOLS / 32 + 2 : Cfg::WCOLS / 32;      // lines per row
  constexpr int LINES = NI * REMC * LPR;
  static_assert(REMC >= 1 && LINES <= 64, "one line per lane");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = (threadIdx.x & 63) % LINES;
  int img = (mb * Cfg::WGM + wave / Cfg::WGN) * NI + q / (LPR * REMC);
  if constexpr (OVERHANG) img = img < n_img ? img : n_img - 1;
  const int k = (q / LPR) % REMC;
  const int off = (q % LPR) * 32 < Cfg::WCOLS ? (q % LPR) * 32 : Cfg::WCOLS - 1;
  const float* src = E + ((int64_t)img * REMC + k) * ldE + (int64_t)nb * Cfg::BN + (wave % Cfg::WGN) * Cfg::WCOLS + off;
  __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(smem + Cfg::STAGE_BYTES + wave * 1024), 4, 0, 0);
}

// The TALL wave tile: 128 x 96 per wave = four images (two at Q = 2) x 96 / (16 TP16) captions; 2 x 4 waves per workgroup, 14 LDS
// fragment reads per 32-deep step against the WIDE tile's 16.
// HALF / CT: the 24- and 40-word caption classes (CT = 5: an 80-column strip = two captions of 40).  WGM x WGN = 1 x 2: the
// two-wave 128 x 160 tile the small grids of the 40-word class use (the other classes' small grids run align_scores16_kernel).
template <bool HAS_E, int TP16, int REMC, int Q = 1, bool HALF = false, int CT = 6, int WGM = 2, int WGN = 4>
__global__ __launch_bounds__(WGM * WGN * 64) void align_scores16_tall_kernel(const half_t* __restrict__ xm, const half_t* __restrict__ y,
                                                                  const float* __restrict__ E, int64_t ldE,
                                                                  float* __restrict__ S, int64_t ldS, int Bi, int Bc,
                                                                  int64_t ldk, int ktiles, int n_nblk, int n_blocks, int rem) {
  using Cfg = GemmCfg<WGM, WGN, 4, 3, CT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 8, mb, nb);
  f32x4 acc[8][CT];
#pragma unroll
  for (int rt = 0; rt < 8; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (HAS_E && REMC == 1 && Q == 1 && WGM == 2 && WGN == 4) side_prefetch<Cfg, 2, 1>(E, ldE, mb, nb, smem);
  gemm_mainloop16_tall<Cfg, true>(xm + (int64_t)mb * Cfg::BM * ldk, y + (int64_t)nb * Cfg::BN * ldk, ldk, ktiles, smem, acc);
  scores16_epilogue<Cfg, 2 * Q, HAS_E, TP16, REMC, HALF>(acc, mb, nb, E, ldE, rem, S, ldS, Bi, Bc);
}

// ------------------------------------------------------------------------------------------------
// The 48-row region class (R' 41..56: three 16-row tiles per image + up to 8 side rows; round 4).  VinVL's 50 regions -- the
// shape of every shipped YAML -- used to pay for two 32-row tiles (64 rows, 22 % of the MFMA rows padding).  Wave tile
// 96 x 96 = two images x 96 / (16 TP16) captions (6 x 6 accumulator tiles: 144 registers), workgroup 2 x 4 waves = 192 x 384
// (4 images x 8 captions at 48 padded words), same LDS image and main loop (gemm_mainloop16_tall with six row tiles: 12
// fragment reads per 36 MFMAs).  WGM x WGN = 1 x 2 (96 x 192, two waves) is the small-grid variant.
// HALF: the 24- / 40-word caption classes (caption_add); CT = 5: the wave's 80 columns are two captions of 40 words.
// ------------------------------------------------------------------------------------------------
// This body keeps an epilogue of its own: on scores16_epilogue<Cfg, 3, ...> -- the same operations in the same order per score, the same
// bits -- the shipped shape's 192 x 320 tile measured 0.16 % slower than before in all of five alternations.
__device__ __forceinline__ float max12(const f32x4& a, const f32x4& b, const f32x4& c) {
  float t = vmax(vmax(a[0], a[1]), a[2]);
  t = vmax(vmax(t, a[3]), b[0]);
  t = vmax(vmax(t, b[1]), b[2]);
  t = vmax(vmax(t, b[3]), c[0]);
  t = vmax(vmax(t, c[1]), c[2]);
  return vmax(t, c[3]);
}

// HALF: the 24- / 40-word caption classes (caption_add); CT = 5: the wave's 80 columns are two captions of 40 words.
template <bool HAS_E, int TP16, int REMC, int WGM, int WGN, int CT, bool HALF>
__device__ __forceinline__ void scores16_epilogue_r48(f32x4 (&acc)[6][CT], int mb, int nb, const float* __restrict__ E, int64_t ldE,
                                                      int rem, float* __restrict__ S, int64_t ldS, int Bi, int Bc) {
  using Cfg = GemmCfg<WGM, WGN, 3, 3, CT>;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave / WGN, wn = wave % WGN;
  const int half = lane >> 5, l4 = lane & 15;
  if constexpr (REMC >= 1) rem = REMC;
  constexpr int NC = HALF ? 2 * CT / (2 * TP16 - 1) : CT / TP16;
  static_assert(HALF ? (CT % (2 * TP16 - 1) == 0) : (CT % TP16 == 0), "a caption must be a whole number of 16-word column tiles of the strip, or two captions 2 TP16 - 1 tiles");
  const int cap = (nb * WGN + wn) * NC;
  const int img = (mb * WGM + wm) * 2 + half;                      // lanes 0-31 finish the wave's first image, 32-63 the second
  const float* e = HAS_E ? E + (int64_t)img * rem * ldE + (int64_t)nb * Cfg::BN + wn * Cfg::WCOLS + l4 : nullptr;
  float v[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) v[c] = 0.f;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const float p0 = max12(acc[0][ct], acc[1][ct], acc[2][ct]);
    const float p1 = max12(acc[3][ct], acc[4][ct], acc[5][ct]);
    auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(p0), __float_as_uint(p1), false, false);
    float m = vmax(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    m = max_xor16(m);
    if constexpr (HAS_E && REMC >= 1) {
      // REMC side rows, known at compile time (1 and 2 -- VinVL's 50 regions = 48 + 2 -- have their own instantiations: a
      // run-time trip count here costs the kernel several per cent)
#pragma unroll
      for (int k = 0; k < REMC; ++k) m = vmax(m, e[(int64_t)k * ldE + ct * 16]);
    }
    if constexpr (HAS_E && REMC == 0) {
      // branch-free: max is idempotent, so rows past the last side row re-read it (k clamped to rem - 1)
#pragma unroll
      for (int k = 0; k < 8; ++k) m = vmax(m, e[(int64_t)(k < rem ? k : rem - 1) * ldE + ct * 16]);
    }
    caption_add<TP16, HALF, NC>(v, ct, l4, m);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float t = row16_sum(v[c]);
    if ((lane & 31) == 0 && img < Bi && cap + c < Bc) S[(int64_t)img * ldS + cap + c] = t;
  }
}

template <bool HAS_E, int TP16, int REMC, int WGM, int WGN, int CT = 6, bool HALF = false>
__global__ __launch_bounds__(WGM * WGN * 64) void align_scores16_r48_kernel(const half_t* __restrict__ xm, const half_t* __restrict__ y,
                                                                            const float* __restrict__ E, int64_t ldE,
                                                                            float* __restrict__ S, int64_t ldS, int Bi, int Bc,
                                                                            int64_t ldk, int ktiles, int n_nblk, int n_blocks, int rem) {
  using Cfg = GemmCfg<WGM, WGN, 3, 3, CT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 8, mb, nb);
  f32x4 acc[6][CT];
#pragma unroll
  for (int rt = 0; rt < 6; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (HAS_E && REMC >= 1 && REMC <= 2 && WGM == 2 && WGN == 4) side_prefetch<Cfg, 3, REMC>(E, ldE, mb, nb, smem);
  gemm_mainloop16_tall<Cfg, true>(xm + (int64_t)mb * Cfg::BM * ldk, y + (int64_t)nb * Cfg::BN * ldk, ldk, ktiles, smem, acc);
  scores16_epilogue_r48<HAS_E, TP16, REMC, WGM, WGN, CT, HALF>(acc, mb, nb, E, ldE, rem, S, ldS, Bi, Bc);
}

// ------------------------------------------------------------------------------------------------
// 48-row region class x 40-word caption class on large grids: 288 x 320 workgroup tile, 144 x 80 wave tile (THREE images x two
// captions per wave, 45 accumulators).  The 192 x 320 tile above moves 0.0083 operand bytes through LDS per multiply-add and its
// loop's LDS time equals its matrix-pipe time (1920 cycles each per K step); this one moves 0.0066 (the headline tile's figure:
// 2400 LDS cycles under 2880 of matrix pipe).  Only the 80-column strip fits: two stages of 608 rows are 152 KB (96-column strips
// would need 168).  The packed operands keep the class's 4-image unit (xm_rows is a multiple of 192, so the sharded path's
// operands still concatenate): the last row tile may hang over the end and re-reads the operand's last 8-row piece for the rows
// that do not exist (gemm_stage_k a_avail); their scores are not stored, and E is read at the last image that exists (OVERHANG).
// ------------------------------------------------------------------------------------------------
using CfgR48x3 = GemmCfg<2, 4, 3, 3, 5, 9>;
template <bool HAS_E, int REMC>
__global__ __launch_bounds__(512) void align_scores16_r48x3_kernel(const half_t* __restrict__ xm, const half_t* __restrict__ y,
                                                                   const float* __restrict__ E, int64_t ldE,
                                                                   float* __restrict__ S, int64_t ldS, int Bi, int Bc,
                                                                   int64_t ldk, int ktiles, int n_nblk, int n_blocks, int rem, int xm_rows) {
  using Cfg = CfgR48x3;
  constexpr int CT = 5, RT = 9;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 8, mb, nb);
  f32x4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int n_img = xm_rows / 48;                                  // images that exist in the operands (>= Bi)
  if constexpr (HAS_E && REMC >= 1 && REMC <= 2) side_prefetch<Cfg, 3, REMC, true>(E, ldE, mb, nb, smem, n_img);
  gemm_mainloop16_tall<Cfg, true>(xm + (int64_t)mb * Cfg::BM * ldk, y + (int64_t)nb * Cfg::BN * ldk, ldk, ktiles, smem, acc, KMapLinear(),
                                  xm_rows - mb * Cfg::BM);
  scores16_epilogue<Cfg, 3, HAS_E, 3, REMC, true, true>(acc, mb, nb, E, ldE, rem, S, ldS, Bi, Bc, n_img);
}

// ------------------------------------------------------------------------------------------------
// Arg-max table for EVERY pair of a batch from the forward's own tile kernel (dense dS: max_violation = False, or a
// gradient arriving on the score matrix).  The one-workgroup-per-pair kernel of align_bwd.hip pays a ~22 us latency chain and
// 132 KB of operand traffic per pair: 1.88 ms for the 65 536 pairs of B = 256.  Here the split-precision operands
// ([hi | lo | hi] x [hi | hi | lo], K = 3 D: cosines good to ~1e-6) run through gemm_mainloop16_tall once, 64 pairs per
// workgroup sharing their panels, and the epilogue -- instead of max over regions / sum over words -- records for every
// (image, caption, word) WHICH region won:
//   * a lane packs the region index of each of its 8 accumulator values into the 6 low mantissa bits (values are
//     cos * 2^28: at most 3.8e-6 of a cosine), keeps the largest and the second largest DISTINCT value, and the same
//     permlane32-swap / 16-lane exchange network as the score epilogue merges (top1, top2) across the 32 rows of the image;
//     the side row (region 33) joins from E;
//   * masked regions (zero rows) all pack to the same value, so they count as ONE candidate (the zero fill of
//     alad/loss.py:116); a winner with index >= Li is NO_GRAD; tile-filling copies of region 0 are left out;
//   * a word whose top two candidates are closer than ARGMAX_TAU (1.6e-5 of a cosine: four times the packing + split error)
//     marks its PAIR in `flags`: those pairs (a few per cent) are re-decided exactly by the list-driven pair kernel.
// The table is the one bwd_rows_kernel reads (uint8, row stride tstride per pair).
// ------------------------------------------------------------------------------------------------
#define ARGMAX_TAU_ACC 4295.0f          // 1.6e-5 * 2^28
__device__ __forceinline__ void top2_merge(float& a1, float& a2, float b1, float b2) {
  const float hi = vmax(a1, b1), lo = fminf(a1, b1);
  // equal tops are the SAME candidate (the shared zero fill, or a value met twice through the exchange network)
  a2 = (a1 == b1) ? vmax(a2, b2) : vmax(lo, vmax(a2, b2));
  a1 = hi;
}
__device__ __forceinline__ float xchg16(float v) {          // the value of lane ^ 16
  auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float a = __uint_as_float(sw[0]), b = __uint_as_float(sw[1]);
  return (threadIdx.x & 16) ? a : b;
}

// The arg-max epilogue of both kernels below.  A wave's Cfg::RT16 row tiles are RT16 / TPI images of TPI tiles each (TPI = 2: 32
// main rows, 3: 48, both with up to 8 side rows from E -- regions 16 TPI .. 16 TPI + rem - 1; 4: 64 rows, none), finished in
// pairs as in scores16_epilogue: lanes 0-31 finish the pair's first image, lanes 32-63 the second.
template <class Cfg, int TPI, bool HAS_E, int TP16>
__device__ __forceinline__ void argmax16_epilogue(f32x4 (&acc)[Cfg::RT16][Cfg::CT16], int mb, int nb, const float* __restrict__ E, int64_t ldE, int rem,
                                                  const int32_t* __restrict__ im_len, int x_tail, int Rq,
                                                  const int32_t* __restrict__ s_len, int y_tail, int Tq,
                                                  uint8_t* __restrict__ table, int tstride, uint8_t* __restrict__ flags,
                                                  int Bi, int Bc) {
  constexpr int CT = Cfg::CT16, NC = CT / TP16, NI = Cfg::RT16 / TPI, R0 = 16 * TPI;
  static_assert(Cfg::RT16 % (2 * TPI) == 0, "whole pairs of images per wave");
  static_assert(!HAS_E || R0 + 8 <= 63, "the side rows' region indices must fit the 6 mantissa bits below the zero-fill candidate 63");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int wm = wave / Cfg::WGN, wn = wave % Cfg::WGN;
  const int half = lane >> 5, l4 = lane & 15, q4 = lane >> 4;
  const int cap0 = (nb * Cfg::WGN + wn) * NC;
  const float NEG = -3.0e38f;
  // words past the caption's length are zero columns: all their candidates tie at 0 -- they neither count nor flag
  int Lc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    Lc[c] = 0;
    if (cap0 + c < Bc) Lc[c] = scored_len(s_len[cap0 + c], y_tail, Tq);
  }
#pragma unroll
  for (int i0 = 0; i0 < NI; i0 += 2) {
    // regions that count of the pair's images A and B (wave-uniform), and of the one this lane finishes
    const int img_a = (mb * Cfg::WGM + wm) * NI + i0;
    int Li_a = 0, Li_b = 0;
    if (img_a < Bi) Li_a = scored_len(im_len[img_a], x_tail, Rq);
    if (img_a + 1 < Bi) Li_b = scored_len(im_len[img_a + 1], x_tail, Rq);
    const int img = img_a + half, Li = half ? Li_b : Li_a;
    const float* e = HAS_E ? E + (int64_t)img * rem * ldE + (int64_t)nb * Cfg::BN + wn * Cfg::WCOLS + l4 : nullptr;
    // region r with accumulator or side value v, of an image with L valid regions, as a candidate
    auto candidate = [&](float v, int r, int L) {
      unsigned bits = (__float_as_uint(v) & ~63u) | (unsigned)r;
      if (r >= L) bits = 63u;                                      // every masked region is the one zero-fill candidate
      return (r >= Rq) ? NEG : __uint_as_float(bits);              // rows past R' only fill the tile
    };
    bool pair_flag[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) pair_flag[c] = false;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      // this lane's 4 TPI values of image A (row tiles from i0 TPI on) and of image B (the next TPI): regions 16 t + 4 q4 + reg
      float a1 = NEG, a2 = NEG, b1 = NEG, b2 = NEG;
#pragma unroll
      for (int t = 0; t < TPI; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int r = 16 * t + 4 * q4 + reg;
          top2_merge(a1, a2, candidate(acc[i0 * TPI + t][ct][reg], r, Li_a), NEG);
          top2_merge(b1, b2, candidate(acc[(i0 + 1) * TPI + t][ct][reg], r, Li_b), NEG);
        }
      // lanes 0-31 take image A's partials of lane + 32, lanes 32-63 image B's of lane - 32
      auto s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(a1), __float_as_uint(b1), false, false);
      auto s2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(a2), __float_as_uint(b2), false, false);
      float t1 = __uint_as_float(s1[0]), t2 = __uint_as_float(s2[0]);
      top2_merge(t1, t2, __uint_as_float(s1[1]), __uint_as_float(s2[1]));
      { const float o1 = xchg16(t1), o2 = xchg16(t2); top2_merge(t1, t2, o1, o2); }
      if constexpr (HAS_E) {
        if (rem == 1) {                                                 // the headline class: one side row
          top2_merge(t1, t2, candidate(e[ct * 16], R0, Li), NEG);
        } else {
          // up to 8 side rows; rows past the last repeat it -- the same candidate, merged as one
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int kk = k < rem ? k : rem - 1;
            top2_merge(t1, t2, candidate(e[(int64_t)kk * ldE + ct * 16], R0 + kk, Li), NEG);
          }
        }
      }
      const unsigned idx = __float_as_uint(t1) & 63u;
      const int c = ct / TP16, w = (ct % TP16) * 16 + l4;
      // NO_GRAD: the zero fill won, or the word is padding (its raw row is not zero: bwd_rows_kernel must skip it)
      const uint8_t res = (idx >= (unsigned)Li || w >= Lc[c]) ? (uint8_t)255 : (uint8_t)idx;
      const bool close = (t1 - t2) < ARGMAX_TAU_ACC;                   // t2 == NEG when there is one candidate only
      if ((lane & 16) == 0 && img < Bi && cap0 + c < Bc && w < tstride) table[((int64_t)img * Bc + cap0 + c) * tstride + w] = res;
      pair_flag[c] = pair_flag[c] || (close && w < Lc[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const unsigned long long mask = half ? 0xffffffff00000000ull : 0x00000000ffffffffull;
      const bool any = (__ballot(pair_flag[c] && img < Bi && cap0 + c < Bc) & mask) != 0;
      if ((lane & 31) == 0 && any) flags[(int64_t)img * Bc + cap0 + c] = 1;
    }
  }
}

// 32 main rows per image (Q = 1: R' <= 40 with the side rows) or 64 (Q = 2: R' 57..64, none)
template <bool HAS_E, int TP16, int Q>
__global__ __launch_bounds__(512) void align_argmax16_tall_kernel(const half_t* __restrict__ xm, const half_t* __restrict__ y,
                                                                  const float* __restrict__ E, int64_t ldE, int rem,
                                                                  const int32_t* __restrict__ im_len, int x_tail, int Rq,
                                                                  const int32_t* __restrict__ s_len, int y_tail, int Tq,
                                                                  uint8_t* __restrict__ table, int tstride, uint8_t* __restrict__ flags,
                                                                  int Bi, int Bc, int64_t ldk, int ktiles, int n_nblk, int n_blocks) {
  using Cfg = GemmCfg<2, 4, 4, 3>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 8, mb, nb);
  f32x4 acc[8][6];
#pragma unroll
  for (int rt = 0; rt < 8; ++rt)
#pragma unroll
    for (int ct = 0; ct < 6; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_mainloop16_tall<Cfg, true>(xm + (int64_t)mb * Cfg::BM * ldk, y + (int64_t)nb * Cfg::BN * ldk, ldk, ktiles, smem, acc);
  argmax16_epilogue<Cfg, 2 * Q, HAS_E, TP16>(acc, mb, nb, E, ldE, rem, im_len, x_tail, Rq, s_len, y_tail, Tq, table, tstride, flags, Bi, Bc);
}

// The 48-row region class (see align_scores16_r48_kernel): a wave's 96 rows are two images of three row tiles each
template <bool HAS_E, int TP16>
__global__ __launch_bounds__(512) void align_argmax16_r48_kernel(const half_t* __restrict__ xm, const half_t* __restrict__ y,
                                                                 const float* __restrict__ E, int64_t ldE, int rem,
                                                                 const int32_t* __restrict__ im_len, int x_tail, int Rq,
                                                                 const int32_t* __restrict__ s_len, int y_tail, int Tq,
                                                                 uint8_t* __restrict__ table, int tstride, uint8_t* __restrict__ flags,
                                                                 int Bi, int Bc, int64_t ldk, int ktiles, int n_nblk, int n_blocks) {
  using Cfg = GemmCfg<2, 4, 3, 3>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 8, mb, nb);
  f32x4 acc[6][6];
#pragma unroll
  for (int rt = 0; rt < 6; ++rt)
#pragma unroll
    for (int ct = 0; ct < 6; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_mainloop16_tall<Cfg, true>(xm + (int64_t)mb * Cfg::BM * ldk, y + (int64_t)nb * Cfg::BN * ldk, ldk, ktiles, smem, acc);
  argmax16_epilogue<Cfg, 3, HAS_E, TP16>(acc, mb, nb, E, ldE, rem, im_len, x_tail, Rq, s_len, y_tail, Tq, table, tstride, flags, Bi, Bc);
}

// WGM x WGN waves of 64 x 192 each: 4 x 2 with a double buffer is the kernel above; 2 x 1 (128 x 192, two waves) with a
// three-stage ring is the SMALL-GRID variant: when the 256 x 384 tiling leaves most CUs idle (B <= 64: at most 64
// workgroups) a workgroup's 12 K steps are a chain of exposed memory latencies (24 us at B = 32, the same as B = 256's
// whole wave of tiles), and a second K step in flight on four times as many CUs halves it.  Same MFMA shape, same K
// order, same epilogue: a score is bit-identical whichever variant computed it.
template <bool HAS_E, int TP16 = 3, bool PROBE = false, int Q = 1, int REMC = 1, int WGM = 4, int WGN = 2, int NS = 2, bool HALF = false>
__global__ __launch_bounds__(WGM * WGN * 64) void align_scores16_kernel(const half_t* __restrict__ xm, const half_t* __restrict__ y,
                                                             const float* __restrict__ E, int64_t ldE,
                                                             float* __restrict__ S, int64_t ldS, int Bi, int Bc,
                                                             int64_t ldk, int ktiles, int n_nblk, int n_blocks, int rem) {
  using Cfg = GemmCfg<WGM, WGN, 2, 6>;
  constexpr int RT = 4, CT = 12;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 8, mb, nb);     // 8 x 16 patch per XCD: 121.7 / 126.8 us vs 125.4 / 128.1 with 4 x 32 (two boxes)

  f32x4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  if constexpr (HAS_E && REMC == 1 && Q == 1 && WGM == 4 && WGN == 2 && NS == 2) side_prefetch<Cfg, 2, 1>(E, ldE, mb, nb, smem);
  unsigned long long pt0 = 0, pr0 = 0, pt1 = 0, pr1 = 0;
  if constexpr (PROBE) { pt0 = __builtin_amdgcn_s_memtime(); pr0 = __builtin_amdgcn_s_memrealtime(); }
  gemm_mainloop16<Cfg, true, NS>(xm + (int64_t)mb * Cfg::BM * ldk, y + (int64_t)nb * Cfg::BN * ldk, ldk, ktiles, smem, acc);
  if constexpr (PROBE) { pt1 = __builtin_amdgcn_s_memtime(); pr1 = __builtin_amdgcn_s_memrealtime(); }

  scores16_epilogue<Cfg, 2 * Q, HAS_E, TP16, REMC, HALF>(acc, mb, nb, E, ldE, rem, S, ldS, Bi, Bc);
#ifdef ALADIN_DIAG
  if constexpr (PROBE) {
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < 4096) {
      g_clock_probe[4 * blockIdx.x + 1] = pr1 - pr0;
      g_clock_probe[4 * blockIdx.x + 2] = pr0;
      g_clock_probe[4 * blockIdx.x + 3] = pr1;
      g_clock_probe[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    }
    if (threadIdx.x == 64 && blockIdx.x < 2048) g_clock_cycles[blockIdx.x] = pt1 - pt0;
  }
#else
  (void)pt0; (void)pr0; (void)pt1; (void)pr1;
#endif
}

// split precision: the operands carry 2^14 each, so S comes out times 2^28 -- scale back (exact)
__global__ __launch_bounds__(256) void scores_unscale_kernel(float* __restrict__ S, int64_t ldS, int Bi, int Bc) {
  const int64_t n = (int64_t)Bi * Bc;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    S[(e / Bc) * ldS + (e % Bc)] *= ALADIN_SPLIT_UNSCALE;
}

// ------------------------------------------------------------------------------------------------
// kernel selection and launch
// ------------------------------------------------------------------------------------------------
// Score kernel bodies.  Scores are bit-identical across the 16x16x32 bodies wherever they overlap: same MFMA shape, K order and
// epilogue arithmetic.
enum ScoreBody {
  BODY_WIDE,      // align_scores16_kernel: 64 x 192 wave tiles
  BODY_TALL,      // align_scores16_tall_kernel: 128 x 96 wave tiles (128 x 80 for 40-word captions)
  BODY_R48,       // align_scores16_r48_kernel: the 48-row region class
  BODY_R48X3,     // align_scores16_r48x3_kernel: the 48-row region class x 40-word captions on large grids
  BODY_32X32,     // align_scores_kernel: v_mfma_f32_32x32x16_f16, 96 rows per image
};

struct ScoreCfg {
  ScoreBody body;
  int tp16;       // 16-word column tiles per caption (g->tp16)
  int half;       // 1: the 8- / 24- / 40-word caption classes (trows = 16 tp16 - 8)
  int q;          // 32-row region tiles per image
  int side;       // side rows the epilogue folds in: 0 none, 1 or 2 (a compile-time count), 8 (a run-time count up to 8)
  int small;      // 1: the small-grid variant of the workgroup tile
  int probe;      // diagnostic build: the clock-probe instantiation of the WIDE body
};

// The class table of aladin_align_geometry, with the grid-size rules.  One workgroup per CU: a grid of at most 64 big tiles (B <= 64
// at the headline shape) leaves most CUs idle, its 12 K steps a chain of exposed memory latencies (24 us at B = 32, the same as
// B = 256's whole wave of tiles); the small-grid variants (a quarter of the waves per workgroup, a deeper ring) halve it.
static ScoreCfg select_scores(const aladin_align_geom* g) {
  ScoreCfg c = {};
  c.tp16 = g->tp16;
  c.half = g->trows != 16 * g->tp16;
  c.q = g->mrows / 32;
  c.side = g->rem <= 1 ? g->rem : (g->rem == 2 && g->mrows == 48) ? 2 : 8;   // VinVL's 50 regions = 48 + 2: a count of its own
  const bool words40 = c.half && c.tp16 == 3;                                  // two captions per 80-column strip
  const int64_t M = g->xm_rows, N = g->y_rows;
  if (g->mrows == 96) { c.body = BODY_32X32; return c; }                      // R' 66..96
  if (g->mrows == 48) {                                                        // R' 41..56
    c.body = BODY_R48;
    c.small = (M / 192) * (N / (words40 ? 320 : 384)) <= 64;
    if (words40 && !c.small) {
      // the 288 x 320 tile where it wins: a grid takes ceil(tiles / 256) rounds; a 288-row tile takes 1.37x the time of a 192-row
      // one for 1.5x the work (measured at B = 256, D = 768: 29.0 vs 21.2 us), but B = 256 is 8.0 rounds of the small tile against
      // 5.4 -> 6 of the big one (170 vs 174 us): the big tile is taken when its rounds come out at least 3 % ahead
      const int64_t n_n = N / 320, r192 = ((M / 192) * n_n + 255) / 256, r288 = (((M + 287) / 288) * n_n + 255) / 256;
      if (1.37 * (double)r288 < 0.97 * (double)r192) c.body = BODY_R48X3;
    }
    return c;
  }
  // 32 or 64 main rows per image (R' <= 40, 57..65)
  if (words40) { c.body = BODY_TALL; c.small = (M / 256) * (N / 320) <= 64; return c; }
  c.small = (M / 256) * (N / 384) <= 64;
  // large grids of captions that tile a 96-column strip: the 128 x 96 wave tile (14 instead of 16 fragment reads per 32-deep step;
  // -2.4 % on the kernel, bit-identical scores)
  c.body = (c.small || 6 % c.tp16 != 0) ? BODY_WIDE : BODY_TALL;
#ifdef ALADIN_DIAG
  // ALADIN_CLOCK_PROBE=1 (diagnostic build): the headline class (32 main rows + at most one side row, 48-word captions) runs the
  // 4 x 2-wave WIDE body with the clock probe (tools/experiments/clock_probe.py)
  static const bool probe = getenv("ALADIN_CLOCK_PROBE") != nullptr;
  if (probe && !c.half && c.tp16 == 3 && c.q == 1 && c.side <= 1) { c.body = BODY_WIDE; c.small = 0; c.probe = 1; }
#endif
  return c;
}

struct SideCfg {
  int nt;         // 32-column tiles per wave (whole captions: y_rows is a multiple of the 64 nt-column workgroup tile)
  int big;        // 1: 128-row tiles
  int two;        // 1: a two-stage LDS ring, else three
};

// 128-row tiles halve the LDS-DMA traffic of this fill-bound kernel; they pay once there are enough rows for the grid to stay
// full: from two side rows per image on (measured at B=256: rem=1 0.187 vs 0.191 ms forward, rem=2 0.209 vs 0.205, rem=6 0.287
// vs 0.275).  LDS ring: two stages (two workgroups per CU) once the grid fills the chip, three (one workgroup, deeper prefetch) for
// the latency-bound small grids (profiles/r04_ab_side_gemm_stages.txt).  320-column tiles for the 40-word class measured slower.
static SideCfg select_side(const aladin_align_geom* g) {
  SideCfg c;
  const bool half = g->trows != 16 * g->tp16;
  c.nt = half ? (g->tp16 == 3 ? 2 : 1) : (g->tp16 & 1) ? g->tp16 : g->tp16 / 2;
  c.big = g->rem >= 2 && g->xe_rows % 128 == 0 && g->xe_rows >= 256;
  c.two = (g->xe_rows / (c.big ? 128 : 64)) * (g->y_rows / (64 * c.nt)) >= 128;
  return c;
}

// The triplet forward's prologue (aladin_align_triplet_fwd): pack [xe | y], then ONE launch of [side tiles | blocks that pack xm]
// (align_side_pack_kernel, beside the side GEMM above) instead of pack everything, then the side GEMM.  xm is first read by the score kernel,
// so nothing orders its packing before the side GEMM; the side tiles are bound by their L2 -> LDS fill, the packing by HBM.
// Every class with side rows takes it: 32 and 48 main rows (65 regions = 64 + 1 is not a class of the pair kernel), rem 1..8, all
// caption classes -- the side tile is select_side's, whatever it is.  Kept in the old order: problems without side rows (there
// is no launch to pack beside), split precision, and image views that float4 loads cannot address (the batched packer has only
// the encoder's whole-row-in-registers form: D % 4 == 0, D <= 1024, 16-byte aligned rows).
static bool side_packs_main(const aladin_set* im, const aladin_align_geom* g) {
  return g->rem > 0 && !g->split && g->D <= 1024 && is_vec4_ok(im->data, im->stride_b, im->stride_r, g->D) &&
         g->mrows % MAIN_PACK_ROWS == 0;      // a batch of rows never leaves its image
}

// f(std::integral_constant<int, v>...) for run-time values v, each drawn from its Set: every combination of the sets is compiled,
// so the callers instantiate kernels only under `if constexpr` rules (the configurations the selection above can return).
template <int... Vs> struct Set {};
template <class F> static int with_values(F&& f) { return f(); }
template <int... Vs, class... Rest, class F>
static int with_values(F&& f, Set<Vs...>, int v, Rest... rest) {
  int rc = ALADIN_ERR_UNSUPPORTED;
  const bool hit = ((v == Vs && ((rc = with_values([&](auto... cs) { return f(std::integral_constant<int, Vs>(), cs...); }, rest...)), true)) || ...);
  if (!hit) aladin_set_error("align: no kernel for tile parameter %d", v);
  return rc;
}

static int no_kernel(const char* what) {
  aladin_set_error("%s: no kernel for this tile class", what);
  return ALADIN_ERR_UNSUPPORTED;
}

// Workgroup tile of a launch: BM x BN over the packed rows; m_rows must be a multiple of m_unit (BM, or the image unit of a kernel
// whose last row tile may hang over the end).
struct Tiles { int bm, bn, m_unit, threads, lds; };
template <class Cfg> static constexpr Tiles tiles_of(int lds = Cfg::LDS_BYTES, int m_unit = Cfg::BM) {
  return Tiles{Cfg::BM, Cfg::BN, m_unit, Cfg::THREADS, lds};
}

// The one launch path of this file: tile check, dynamic LDS reserved once per device, launch, launch check.
// args(n_nblk, n_blocks) returns the kernel's arguments as a tuple.  extra_blocks: blocks behind the n_blocks tiles of the grid.
template <auto KERN, class Args>
static int launch_tiles(const char* what, Tiles t, int64_t m_rows, int64_t n_rows, hipStream_t stream, Args args, int extra_blocks = 0) {
  const int64_t n_mblk = (m_rows + t.bm - 1) / t.bm, n_nblk = n_rows / t.bn;
  if (m_rows % t.m_unit != 0 || n_nblk * t.bn != n_rows) {
    aladin_set_error("%s: packed rows (%lld, %lld) do not tile by (%d, %d)", what, (long long)m_rows, (long long)n_rows, t.bm, t.bn);
    return ALADIN_ERR_ARG;
  }
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)KERN, t.lds, &lds_reserved, what)) return rc;
  const int n_blocks = (int)(n_mblk * n_nblk);
  std::apply([&](auto... a) { hipLaunchKernelGGL(KERN, dim3(n_blocks + extra_blocks), dim3(t.threads), t.lds, stream, a...); }, args((int)n_nblk, n_blocks));
  return aladin_check_launch(what);
}

static int launch_side(const aladin_align_geom* g, const half_t* xe, const half_t* y, float* E, hipStream_t stream) {
  const SideCfg c = select_side(g);
  return with_values([&](auto nt, auto big, auto two) {
    constexpr int SWM = big ? 2 : 1, NS = two ? 2 : 3;
    using Cfg = GemmCfg<2, 2, SWM, nt>;
    return launch_tiles<align_side_gemm_kernel<nt, SWM, NS>>("align_side_gemm_kernel", tiles_of<Cfg>(NS * Cfg::STAGE_BYTES), g->xe_rows,
                                                            g->y_rows, stream, [&](int n_nblk, int) {
      return std::make_tuple(xe, y, E, (int64_t)g->y_rows, (int64_t)g->Dp, g->Dp / 64, n_nblk);
    });
  }, Set<1, 2, 3>(), c.nt, Set<0, 1>(), c.big, Set<0, 1>(), c.two);
}

static int launch_scores(const ScoreCfg& c, const aladin_align_geom* g, const half_t* xm, const half_t* y, const float* E, float* S,
                         int64_t ldS, hipStream_t stream) {
  const int64_t M = g->xm_rows, N = g->y_rows;
  auto args = [=](int n_nblk, int n_blocks) {
    return std::make_tuple(xm, y, E, N, S, ldS, g->Bi, g->Bc, (int64_t)g->Dp, g->Dp / 64, n_nblk, n_blocks, g->rem);
  };
  if (c.body == BODY_32X32)
    return with_values([&](auto tp16) {
      using Cfg = GemmCfg<4, 2, 3, (tp16 & 1) ? tp16 : tp16 / 2>;
      return launch_tiles<align_scores_kernel<3, 3, tp16, false>>("align_scores_kernel", tiles_of<Cfg>(), M, N, stream, [&](int n_nblk, int n_blocks) {
        return std::make_tuple(xm, y, E, N, S, ldS, g->Bi, g->Bc, (int64_t)g->Dp, g->Dp / 64, n_nblk, n_blocks);
      });
    }, Set<1, 2, 3, 4, 6>(), c.tp16);
  if (c.body == BODY_R48X3)
    return with_values([&](auto side) {
      return launch_tiles<align_scores16_r48x3_kernel<side != 0, side == 8 ? 0 : side == 0 ? 1 : side>>(
          "align_scores16_r48x3_kernel", tiles_of<CfgR48x3>(CfgR48x3::LDS_BYTES, 48), M, N, stream,
          [&](int n_nblk, int n_blocks) { return std::tuple_cat(args(n_nblk, n_blocks), std::make_tuple((int)M)); });
    }, Set<0, 1, 2, 8>(), c.side);
#ifdef ALADIN_DIAG
  if (c.probe)
    return with_values([&](auto side) {
      using Cfg = GemmCfg<4, 2, 2, 6>;
      return launch_tiles<align_scores16_kernel<side != 0, 3, true>>("align_scores16_kernel", tiles_of<Cfg>(), M, N, stream, args);
    }, Set<0, 1>(), c.side);
#endif
  return with_values([&](auto tp16, auto half, auto q, auto side, auto small) -> int {
    constexpr int TP16 = tp16, Q = q, SIDE = side;
    constexpr bool HALF = half, SMALL = small, HAS_E = SIDE != 0;
    constexpr int REMC = SIDE == 8 ? 0 : SIDE == 0 ? 1 : SIDE;     // compile-time side-row count (0: run-time; 1 when unused)
    constexpr bool cols = HALF ? TP16 <= 3 : true;                  // 8 / 24 / 40 words
    constexpr bool rows = Q == 1 ? SIDE != 2 : SIDE <= 1;            // WIDE / TALL: 64 main rows take R' 65's one side row only
    constexpr bool words40 = HALF && TP16 == 3;
    constexpr int CT = words40 ? 5 : 6;
    if (c.body == BODY_WIDE) {
      // small grids: 2 x 1 waves (128 x 192) with a three-stage ring; large grids: 4 x 2 waves with a double buffer (64-word
      // captions, which do not tile the tall body's 96-column strip)
      if constexpr (cols && rows && !words40 && (SMALL || (TP16 == 4 && !HALF))) {
        using Cfg = GemmCfg<SMALL ? 2 : 4, SMALL ? 1 : 2, 2, 6>;
        constexpr int NS = SMALL ? 3 : 2;
        return launch_tiles<align_scores16_kernel<HAS_E, TP16, false, Q, REMC, Cfg::WGM, Cfg::WGN, NS, HALF>>(
            "align_scores16_kernel", tiles_of<Cfg>(NS * Cfg::STAGE_BYTES), M, N, stream, args);
      }
    } else if (c.body == BODY_TALL) {
      // 2 x 4 waves; the 40-word class's small grids: 1 x 2 waves (128 x 160)
      if constexpr (cols && rows && 6 % TP16 == 0 && (!SMALL || words40)) {
        using Cfg = GemmCfg<SMALL ? 1 : 2, SMALL ? 2 : 4, 4, 3, CT>;
        return launch_tiles<align_scores16_tall_kernel<HAS_E, TP16, REMC, Q, HALF, CT, Cfg::WGM, Cfg::WGN>>(
            "align_scores16_tall_kernel", tiles_of<Cfg>(), M, N, stream, args);
      }
    } else if (c.body == BODY_R48) {
      // 2 x 4 waves (192 x 384, or 192 x 320 for 40-word captions); small grids: 1 x 2 waves
      if constexpr (cols && Q == 1 && 6 % TP16 == 0) {
        using Cfg = GemmCfg<SMALL ? 1 : 2, SMALL ? 2 : 4, 3, 3, CT>;
        return launch_tiles<align_scores16_r48_kernel<HAS_E, TP16, REMC, Cfg::WGM, Cfg::WGN, CT, HALF>>(
            "align_scores16_r48_kernel", tiles_of<Cfg>(), M, N, stream, args);
      }
    }
    return no_kernel("align_scores");
  }, Set<1, 2, 3, 4, 6>(), c.tp16, Set<0, 1>(), c.half, Set<1, 2>(), c.q, Set<0, 1, 2, 8>(), c.side, Set<0, 1>(), c.small);
}

// g: a SPLIT-precision geometry with 32 or 48 rows per image + up to 8 side rows (R' <= 40, 41..56) or 64 rows and no
// side rows (R' 57..64), captions tiling a 96-column strip;
// xm / xe / y: its packed operands; E: its side scratch (g->e_bytes); flags: Bi * Bc bytes, zeroed here.
int aladin_internal_align_argmax(const aladin_align_geom* g, const void* xm, const void* xe, const void* y, float* E,
                                 const int32_t* im_len, const int32_t* s_len, uint8_t* table, int tstride, uint8_t* flags,
                                 hipStream_t stream) {
  const bool ok_class = g && g->split && 6 % g->tp16 == 0 && g->trows == 16 * g->tp16 &&
                        ((g->mrows == 32 && g->rem <= 8) || (g->mrows == 48 && g->rem <= 8) || (g->mrows == 64 && g->rem == 0));
  if (!ok_class) { aladin_set_error("align_argmax: unsupported tile class (mrows=%d rem=%d tp16=%d split=%d)", g ? g->mrows : -1, g ? g->rem : -1, g ? g->tp16 : -1, g ? g->split : -1); return ALADIN_ERR_UNSUPPORTED; }
  if (hipMemsetAsync(flags, 0, (size_t)g->Bi * g->Bc, stream) != hipSuccess) { aladin_set_error("align_argmax: memset failed"); return ALADIN_ERR_HIP; }
  if (g->rem)
    if (int rc = launch_side(g, (const half_t*)xe, (const half_t*)y, E, stream)) return rc;
  auto args = [&](int n_nblk, int n_blocks) {
    return std::make_tuple((const half_t*)xm, (const half_t*)y, (const float*)E, (int64_t)g->y_rows, g->rem, im_len, g->x_tail, g->Rq, s_len,
                           g->y_tail, g->Tq, table, tstride, flags, g->Bi, g->Bc, (int64_t)g->Dp, g->Dp / 64, n_nblk, n_blocks);
  };
  // 48 rows: align_argmax16_r48_kernel; 32 rows (Q = 1, side rows from E) or 64 (Q = 2, none): align_argmax16_tall_kernel
  return with_values([&](auto tp16, auto has_e, auto q) -> int {
    if (g->mrows == 48) {
      if constexpr (q == 1) return launch_tiles<align_argmax16_r48_kernel<has_e, tp16>>("align_argmax16_r48_kernel", tiles_of<GemmCfg<2, 4, 3, 3>>(),
                                                                                      g->xm_rows, g->y_rows, stream, args);
    } else if constexpr (q == 1 || !has_e) {
      return launch_tiles<align_argmax16_tall_kernel<has_e, tp16, q>>("align_argmax16_tall_kernel", tiles_of<GemmCfg<2, 4, 4, 3>>(),
                                                                       g->xm_rows, g->y_rows, stream, args);
    }
    return no_kernel("align_argmax");
  }, Set<1, 2, 3, 6>(), g->tp16, Set<0, 1>(), g->rem != 0, Set<1, 2>(), g->mrows == 64 ? 2 : 1);
}

int aladin_internal_scores(const void* xm, const void* xe, const void* y, const aladin_align_geom* g, void* e_scratch, float* S,
                           int64_t ldS, int flags, void* stream) {
  if (!xm || !y || !g || !S || (g->rem && (!xe || !e_scratch))) { aladin_set_error("align_scores: null argument"); return ALADIN_ERR_ARG; }
  if (ldS < g->Bc) { aladin_set_error("align_scores: ldS %lld < Bc %d", (long long)ldS, g->Bc); return ALADIN_ERR_ARG; }
  if (g->trows != 16 * g->tp16 && !(g->trows == 16 * g->tp16 - 8 && g->tp16 <= 3)) { aladin_set_error("align_scores: bad geometry (trows=%d tp16=%d)", g->trows, g->tp16); return ALADIN_ERR_ARG; }
  if (g->tp16 < 1 || g->tp16 > 6 || g->tp16 == 5) { aladin_set_error("align_scores: unsupported padded caption length %d", 16 * g->tp16); return ALADIN_ERR_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  float* E = (float*)e_scratch;
  if (g->rem && !(flags & ALADIN_SCORES_REUSE_SIDE))
    if (int rc = launch_side(g, (const half_t*)xe, (const half_t*)y, E, st)) return rc;
  if (int rc = launch_scores(select_scores(g), g, (const half_t*)xm, (const half_t*)y, E, S, ldS, st)) return rc;
  if (!g->split) return ALADIN_OK;
  const int64_t n = (int64_t)g->Bi * g->Bc;
  int grid = (int)((n + 255) / 256); if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(scores_unscale_kernel, dim3(grid), dim3(256), 0, st, S, ldS, g->Bi, g->Bc);
  return aladin_check_launch("scores_unscale_kernel");
}

extern "C" int aladin_align_scores(const aladin_packed* p, const aladin_align_geom* g, void* e_scratch, float* S, int64_t ldS, int flags,
                                   void* stream) {
  if (!p) { aladin_set_error("align_scores: null argument"); return ALADIN_ERR_ARG; }
  if (flags & ~ALADIN_SCORES_REUSE_SIDE) { aladin_set_error("align_scores: unknown flags %d", flags); return ALADIN_ERR_ARG; }
  if (g && g->layout == ALADIN_LAYOUT_LONG) return aladin_internal_long_scores(p, g, S, ldS, stream);
  return aladin_internal_scores(p->xm, p->xe, p->y, g, e_scratch, S, ldS, flags, stream);
}

static const int MAIN_PACK_BLOCKS = 256;      // one per CU of the MI355X

int aladin_internal_check_prologue(const aladin_set* im, const aladin_set* s, const aladin_align_geom* g, const aladin_packed* out) {
  if (!g || !out || !set_ok(im) || !set_ok(s) || !out->xm || !out->xe || !out->y) { aladin_set_error("align_pack: null argument"); return ALADIN_ERR_ARG; }
  if (!side_packs_main(im, g)) { aladin_set_error("align_pack: not a problem whose side launch packs the main rows"); return ALADIN_ERR_UNSUPPORTED; }
  return ALADIN_OK;
}

bool aladin_internal_side_packs_main(const aladin_set* im, const aladin_align_geom* g) { return set_ok(im) && g && side_packs_main(im, g); }

// the side GEMM of packed xe and y into E, with the main rows of `im` packed by the blocks behind its tiles
int aladin_internal_side_with_main_pack(const aladin_set* im, const aladin_set* s, const aladin_align_geom* g, const aladin_packed* out,
                                        float* E, hipStream_t st) {
  if (int rc = aladin_internal_check_prologue(im, s, g, out)) return rc;
  if (!E) { aladin_set_error("align_side_pack: null side scratch"); return ALADIN_ERR_ARG; }
  const MainPack mp = {im->data, im->stride_b, im->stride_r, im->len, g->Bi, g->Rq, g->x_tail, g->D, g->Dp, g->mrows, g->xm_rows,
                       (half_t*)out->xm, out->rnorm};
  const int64_t wave_batches = (g->xm_rows / MAIN_PACK_ROWS + 3) / 4;
  const int n_pack = (int)(wave_batches < MAIN_PACK_BLOCKS ? wave_batches : MAIN_PACK_BLOCKS);
  const SideCfg c = select_side(g);
  return with_values([&](auto nt, auto big, auto two) {
    constexpr int SWM = big ? 2 : 1, NS = two ? 2 : 3;
    using Cfg = GemmCfg<2, 2, SWM, nt>;
    return launch_tiles<align_side_pack_kernel<nt, SWM, NS>>("align_side_pack_kernel", tiles_of<Cfg>(NS * Cfg::STAGE_BYTES), g->xe_rows,
                                                            g->y_rows, st, [&](int n_nblk, int n_blocks) {
      return std::make_tuple((const half_t*)out->xe, (const half_t*)out->y, E, (int64_t)g->y_rows, (int64_t)g->Dp, g->Dp / 64, n_nblk, n_blocks, mp);
    }, n_pack);
  }, Set<1, 2, 3>(), c.nt, Set<0, 1>(), c.big, Set<0, 1>(), c.two);
}
