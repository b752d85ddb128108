// Alignment scores and their backward for LONG sets: more than 96 scored positions on either side, up to 512 positions per set
// (R' <= 511 regions on the max side, T' <= 509 words on the sum side).  The tile classes of align_fwd.hip / align_bwd.hip
// (32 / 48 / 64 / 96 region rows, a caption inside one 96-column strip) are the limit of those kernels; this file holds the
// path beside them, and nothing the shorter shapes launch lives here.
//
// packing        the pack kernel of pack.hip (aladin_align_pack) on an ALADIN_LAYOUT_LONG geometry: mrows =
//                round_up(R', 32) rows per max-side sample (rows past R' repeat position 1: max is idempotent), no side rows,
//                trows = round_up(T', 16) rows per sum-side sample; the masking conventions of pack_rows.hpp carry over
//                (masked positions are zero rows, so the zero fill takes part in the max of a shorter sample).
// score kernel   one workgroup = one max-side sample x cap_unit whole sum-side samples (<= 512 columns, 32 column tiles of
//                16 words over 4 waves).  A wave walks ALL 32-row region tiles of its sample with v_mfma_f32_16x16x32_f16,
//                regions on the row axis, words on the lane axis, and keeps a running per-column max in registers: the max
//                over any number of row tiles is more in-lane max steps.  The per-tile word sums meet in LDS and every
//                score is the sum of its caption's tiles in a fixed order: no atomics, bitwise reproducible.  Split
//                precision is the same kernel over the three-segment K of the split packers.
// backward       1. compact the non-zero pairs of dS (the compaction of align_bwd.hip: aladin_internal_compact_pairs);
//                2. per pair the arg-max region of every word in fp32 (v_mfma_f32_32x32x2_f32 from the raw rows, as the
//                   fallback of align_bwd.hip) over 32-word windows and 32-region tiles with a running arg-max: the recorded
//                   winner is the fp32 winner for every word, with no fp16 screening to re-decide.  16-bit entries
//                   (LONG_NO_GRAD = 0xFFFF: padded word, or the zero fill won the max);
//                3. one wave per OUTPUT row gathers the partner rows the table points at (raw fp32 rows, or the forward's
//                   packed fp16 operands under ALADIN_BWD_PARTNERS_FP16 / ALADIN_BWD_OWN_ROW_FP16) and applies the
//                   normalise backward.  Every output row written exactly once, no atomics.
//                Dense dS (the sum-of-violations hinge, a gradient on S) takes the same pair-list path.
// Nothing is exported from here: aladin_align_geometry / aladin_align_scores (align_fwd.hip) and aladin_align_bwd with its workspace
// query (align_bwd.hip) hand a geometry whose layout is ALADIN_LAYOUT_LONG to the aladin_internal_long_* functions below.
#include <string.h>

#include "../../include/aladin_hip.h"
#include "bwd_common.hpp"

#define LONG_MAX_POS 512
#define LONG_NO_GRAD 0xFFFFu
#define LS_WAVES 4         // waves per score workgroup
#define LS_NT 8            // 16-column tiles per wave: a workgroup covers up to 512 columns
#define LS_COLS (16 * LS_WAVES * LS_NT)

// the ALADIN_LAYOUT_LONG branch of aladin_align_geometry, which has checked precision, sizes, tails and set lengths
int aladin_internal_long_layout(int Bi, int Bc, int R, int T, int D, int x_tail, int y_tail, int precision, aladin_align_geom* g) {
  if (R > LONG_MAX_POS || T > LONG_MAX_POS) { aladin_set_error("align_geometry: at most %d positions per set (got R=%d T=%d)", LONG_MAX_POS, R, T); return ALADIN_ERR_UNSUPPORTED; }
  memset(g, 0, sizeof(*g));
  g->Bi = Bi; g->Bc = Bc; g->R = R; g->T = T; g->D = D;
  g->x_tail = x_tail; g->y_tail = y_tail;
  g->split = precision == ALADIN_PRECISION_SPLIT;
  g->layout = ALADIN_LAYOUT_LONG;
  g->Rq = R - 1 - x_tail; g->Tq = T - 1 - y_tail;
  g->mrows = round_up(g->Rq, 32);
  g->rem = 0;
  g->trows = round_up(g->Tq, 16);
  g->tp16 = g->trows / 16;
  g->Dp = round_up(D, 64) * (g->split ? 3 : 1);
  g->img_unit = 1;
  g->cap_unit = LS_COLS / g->trows;                          // whole captions per score workgroup (>= 1: trows <= 512)
  g->Bi_pad = Bi;
  g->Bc_pad = round_up(Bc, g->cap_unit);
  g->xm_rows = (int64_t)Bi * g->mrows;
  g->xe_rows = 0;
  g->y_rows = (int64_t)g->Bc_pad * g->trows;
  g->xm_bytes = g->xm_rows * g->Dp * 2;
  g->xe_bytes = 0;
  g->y_bytes = g->y_rows * g->Dp * 2;
  g->e_bytes = 0;
  g->rnorm_bytes = (g->xm_rows + g->y_rows) * 4;
  return ALADIN_OK;
}

// the functions below take only what aladin_align_geometry makes for ALADIN_LAYOUT_LONG: recomputed and compared, layout included
// (a tile-class geometry relabelled by hand has other rows and units)
static bool long_geom_ok(const aladin_align_geom* g) {
  if (!g) return false;
  aladin_align_geom ref;
  if (aladin_align_geometry(g->Bi, g->Bc, g->R, g->T, g->D, g->x_tail, g->y_tail, g->split ? ALADIN_PRECISION_SPLIT : ALADIN_PRECISION_FP16,
                            ALADIN_LAYOUT_LONG, &ref) != ALADIN_OK) return false;
  return memcmp(&ref, g, sizeof(ref)) == 0;
}

// ------------------------------------------------------------------------------------------------
// score kernel
// ------------------------------------------------------------------------------------------------
// 16x16x32 fragments: lane l holds row (l & 15), k = 8 (l >> 4) + 0..7; C lane l holds column (l & 15), rows 4 (l >> 4) + 0..3.
// The fragments come straight from global memory (L2 / L1), not through LDS: why that limits its rate: DESIGN.md section 4.5.
__global__ __launch_bounds__(256) void long_scores_kernel(const half_t* __restrict__ xm, const half_t* __restrict__ y, int mrows,
                                                          int trows, int Dp, int Bc, int cap_unit, float* __restrict__ S,
                                                          int64_t ldS, float scale) {
  __shared__ float tile_sum[LS_WAVES * LS_NT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.y;
  const int j0 = blockIdx.x * cap_unit;
  const int ntiles = cap_unit * trows / 16;                  // column tiles of the workgroup (<= 32)
  const int per_wave = (ntiles + LS_WAVES - 1) / LS_WAVES;
  const int t0 = wave * per_wave;
  const int nt = ntiles - t0 < per_wave ? ntiles - t0 : per_wave;     // tiles this wave owns (may be <= 0)
  const half_t* xa = xm + ((int64_t)i * mrows + (lane & 15)) * Dp + 8 * (lane >> 4);
  const half_t* yb[LS_NT];
#pragma unroll
  for (int t = 0; t < LS_NT; ++t) {
    // a wave with fewer tiles repeats a tile it owns (or tile 0): the extra columns are computed and dropped
    const int tt = t < nt ? t0 + t : (nt > 0 ? t0 : 0);
    yb[t] = y + ((int64_t)j0 * trows + tt * 16 + (lane & 15)) * Dp + 8 * (lane >> 4);
  }
  float run[LS_NT];
#pragma unroll
  for (int t = 0; t < LS_NT; ++t) run[t] = -INFINITY;
  for (int r0 = 0; r0 < mrows; r0 += 32) {
    f32x4 acc[2][LS_NT];
#pragma unroll
    for (int t = 0; t < LS_NT; ++t) { acc[0][t] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const half_t* a0 = xa + (int64_t)r0 * Dp;
    const half_t* a1 = a0 + (int64_t)16 * Dp;
    for (int k = 0; k < Dp; k += 32) {
      const half8 fa0 = *reinterpret_cast<const half8*>(a0 + k);
      const half8 fa1 = *reinterpret_cast<const half8*>(a1 + k);
      half8 fb[LS_NT];
#pragma unroll
      for (int t = 0; t < LS_NT; ++t) fb[t] = *reinterpret_cast<const half8*>(yb[t] + k);
#pragma unroll
      for (int t = 0; t < LS_NT; ++t) {
        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa0, fb[t], acc[0][t], 0, 0, 0);
        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa1, fb[t], acc[1][t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < LS_NT; ++t) {
      float m = run[t];
#pragma unroll
      for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(acc[0][t][e], acc[1][t][e]));
      run[t] = m;
    }
  }
#pragma unroll
  for (int t = 0; t < LS_NT; ++t) {
    float m = run[t];
    m = fmaxf(m, lane_xor16(m));                             // the four row groups of the column
    m = fmaxf(m, lane_xor32(m));
    const float sum = row16_sum(m);                          // the tile's 16 words
    if (lane == 0 && t < nt) tile_sum[t0 + t] = sum;
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < cap_unit && j0 + c < Bc) {
    const int per_cap = trows / 16;
    float sc = 0.f;
    for (int q = 0; q < per_cap; ++q) sc += tile_sum[c * per_cap + q];
    S[(int64_t)i * ldS + j0 + c] = sc * scale;
  }
}

int aladin_internal_long_scores(const aladin_packed* p, const aladin_align_geom* g, float* S, int64_t ldS, void* stream) {
  if (!p || !p->xm || !p->y || !S) { aladin_set_error("align_scores: null argument"); return ALADIN_ERR_ARG; }
  if (!long_geom_ok(g)) { aladin_set_error("align_scores: not a long-set geometry of aladin_align_geometry"); return ALADIN_ERR_ARG; }
  if (ldS < g->Bc) { aladin_set_error("align_scores: ldS %lld < Bc %d", (long long)ldS, g->Bc); return ALADIN_ERR_ARG; }
  const float scale = g->split ? ALADIN_SPLIT_UNSCALE : 1.0f;       // split operands carry 2^14 each
  hipLaunchKernelGGL(long_scores_kernel, dim3((unsigned)(g->Bc_pad / g->cap_unit), (unsigned)g->Bi), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)p->xm, (const half_t*)p->y, g->mrows, g->trows, g->Dp, g->Bc, g->cap_unit, S, ldS, scale);
  return aladin_check_launch("long_scores_kernel");
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
using LongWs = PairWs<uint16_t>;     // the table: Bi*Bc rows of table_stride(Tq) 16-bit entries

size_t aladin_internal_long_bwd_bytes(const aladin_align_geom* g) {
  if (!long_geom_ok(g)) return 0;
  return pair_ws_layout<uint16_t>(g->Bi, g->Bc, g->Tq, nullptr, nullptr);
}

// (value, index) of the larger; the smaller index on a tie (the first maximum, as a scan in region order finds it)
__device__ __forceinline__ void argmax_take(float& best, int& arg, float v, int a) {
  if (v > best || (v == best && a < arg)) { best = v; arg = a; }
}

// One workgroup per listed pair: 32-word windows; in each, the four waves split the 32-region tiles and keep a running arg-max
// per word, merged across the wave's two row halves and then across the waves in LDS.
__global__ __launch_bounds__(256) void long_pair_argmax_kernel(
    const float* __restrict__ im, int64_t im_sb, int64_t im_sr, const int32_t* __restrict__ im_len,
    const float* __restrict__ s, int64_t s_sb, int64_t s_st, const int32_t* __restrict__ s_len, int Bc, int Rq, int Tq,
    int D, const int* __restrict__ counter, const int* __restrict__ pairs, uint16_t* __restrict__ table, int tstride,
    int x_tail, int y_tail) {
  __shared__ float w_best[4][32];
  __shared__ int w_arg[4][32];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int h = lane >> 5, l5 = lane & 31;
  const int count = *counter;
  const bool vec = (D % 8 == 0) && (im_sb % 4 == 0) && (im_sr % 4 == 0) && (s_sb % 4 == 0) && (s_st % 4 == 0) &&
                   (((uintptr_t)im & 15) == 0) && (((uintptr_t)s & 15) == 0);
  for (int p = blockIdx.x; p < count; p += gridDim.x) {
    const int i = pairs[p] / Bc, j = pairs[p] % Bc;
    int Li = im_len[i] - 1 - x_tail; Li = Li < 0 ? 0 : (Li > Rq ? Rq : Li);
    int Lj = s_len[j] - 1 - y_tail; Lj = Lj < 0 ? 0 : (Lj > Tq ? Tq : Lj);
    uint16_t* trow = table + ((int64_t)i * Bc + j) * tstride;
    for (int w = threadIdx.x; w < tstride; w += blockDim.x)
      if (w >= Lj || Li == 0) trow[w] = (uint16_t)LONG_NO_GRAD;
    if (Li == 0) continue;
    const int ntm = (Li + 31) / 32, ntn = (Lj + 31) / 32;
    for (int tn = 0; tn < ntn; ++tn) {
      float best = -INFINITY;
      int arg = 0x7fffffff;
      int w = tn * 32 + l5; if (w >= Lj) w = Lj - 1;              // clamp: value unused
      const float* yr = s + j * s_sb + (int64_t)(w + 1) * s_st;
      for (int tm = wave; tm < ntm; tm += 4) {
        int rho = tm * 32 + l5; if (rho >= Li) rho = Li - 1;
        const float* xr = im + i * im_sb + (int64_t)(rho + 1) * im_sr;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float ss = 0.f;                                           // this lane's half of ||x_rho||^2
        if (vec) {
          // lane (row, h) takes k = 8u + 4h .. 8u + 4h + 3: a fixed permutation of k shared by A and B
          for (int u = 0; u < D / 8; ++u) {
            const float4 a = *reinterpret_cast<const float4*>(xr + 8 * u + 4 * h);
            const float4 b = *reinterpret_cast<const float4*>(yr + 8 * u + 4 * h);
            ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
          }
        } else {
          for (int k = 0; k < D; k += 2) {
            const int kk = k + h;
            const float a = kk < D ? xr[kk] : 0.f;
            const float b = kk < D ? yr[kk] : 0.f;
            ss += a * a;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
          }
        }
        ss += __shfl_xor(ss, 32, 64);                             // lane l5 (both halves): ||x_{tm*32+l5}||^2
        // accumulator row = (r&3) + 8*(r>>2) + 4*h, column l5 = word; the caption norm is a positive column factor
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = cos_tile_row(r, h);
          const float v = acc[r] * cos_tile_inv_norm(ss, row);
          const int rg = tm * 32 + row;
          if (rg < Li) argmax_take(best, arg, v, rg);
        }
      }
      argmax_take(best, arg, lane_xor32(best), lane_xor32(arg));
      if (h == 0) { w_best[wave][l5] = best; w_arg[wave][l5] = arg; }
      __syncthreads();
      if (threadIdx.x < 32) {
        float b = w_best[0][threadIdx.x];
        int a = w_arg[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < 4; ++q) argmax_take(b, a, w_best[q][threadIdx.x], w_arg[q][threadIdx.x]);
        const int ww = tn * 32 + (int)threadIdx.x;
        // the zero fill of a shorter sample (alad/loss.py:116) competes: a non-positive best leaves the word without gradient
        if (ww < Lj) trow[ww] = (Li < Rq && b <= 0.f) ? (uint16_t)LONG_NO_GRAD : (uint16_t)a;
      }
      __syncthreads();
    }
  }
}

// partner row: a raw fp32 row normalised here, or (P16) the forward's packed unit vector
template <int NCH, bool P16>
__device__ __forceinline__ void long_gather(const float* __restrict__ raw, const half_t* __restrict__ packed, float g, int D, int lane,
                                            float4 (&acc)[NCH]) {
  float4 v[NCH];
  if constexpr (P16) {
    load_row_h<NCH, false>(packed, D, lane, v);
    axpy_row<NCH>(g, v, acc);
  } else {
    load_row<NCH, false>(raw, D, lane, v);
    const float ss = wave_sum(row_sumsq<NCH>(v));
    axpy_row<NCH>(g / fmaxf(sqrtf(ss), 1e-12f), v, acc);
  }
}

// where the packers put region r of max-side sample b / word w of sum-side sample b (ALADIN_LAYOUT_LONG), and the rows'
// inverse norms ([xm rows | y rows])
struct LongPacked { const half_t* xm; const half_t* y; const float* rnorm; int Dp, mrows, trows; int64_t y_row0; };

// One wave per output row (every (max-side sample, position) and (sum-side sample, position)): partners in increasing order,
// words in increasing order.  O16: the row's own unit vector and inverse norm from the packed operands too.
template <int NCH, bool P16, bool O16>
__global__ __launch_bounds__(256) void long_rows_kernel(
    const float* __restrict__ im, int64_t im_sb, int64_t im_sr, const int32_t* __restrict__ im_len,
    const float* __restrict__ s, int64_t s_sb, int64_t s_st, const int32_t* __restrict__ s_len, int Bi, int Bc, int R,
    int T, int D, const float* __restrict__ dS, int64_t ld, const float* __restrict__ gscale,
    const uint16_t* __restrict__ table, int tstride, float* __restrict__ d_im, float* __restrict__ d_s, int x_tail,
    int y_tail, int64_t dim_sb, int64_t dim_sr, int64_t ds_sb, int64_t ds_st, LongPacked pk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  const int64_t n_im_rows = (int64_t)Bi * R;
  if (row >= n_im_rows + (int64_t)Bc * T) return;
  const bool is_img = row < n_im_rows;
  const int Rq = R - 1 - x_tail, Tq = T - 1 - y_tail;
  int own_b, own_p;
  float* out;
  const float* xrow;
  if (is_img) { own_b = (int)(row / R); own_p = (int)(row % R); out = d_im + own_b * dim_sb + own_p * dim_sr; xrow = im + own_b * im_sb + (int64_t)own_p * im_sr; }
  else { const int64_t q = row - n_im_rows; own_b = (int)(q / T); own_p = (int)(q % T); out = d_s + own_b * ds_sb + own_p * ds_st; xrow = s + own_b * s_sb + (int64_t)own_p * s_st; }
  const int idx = own_p - 1;                                  // region / word index inside the alignment
  int L;
  if (is_img) { L = im_len[own_b] - 1 - x_tail; L = L < 0 ? 0 : (L > Rq ? Rq : L); }
  else { L = s_len[own_b] - 1 - y_tail; L = L < 0 ? 0 : (L > Tq ? Tq : L); }

  float4 acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  bool any = false;
  float4 xv[NCH];
  float own_inv = 0.f;
  if (idx >= 0 && idx < L) {
    if constexpr (O16) {
      if (is_img) { load_row_h<NCH, false>(pk.xm + ((int64_t)own_b * pk.mrows + idx) * pk.Dp, D, lane, xv); own_inv = pk.rnorm[(int64_t)own_b * pk.mrows + idx]; }
      else { load_row_h<NCH, false>(pk.y + ((int64_t)own_b * pk.trows + idx) * pk.Dp, D, lane, xv); own_inv = pk.rnorm[pk.y_row0 + (int64_t)own_b * pk.trows + idx]; }
    } else load_row<NCH, false>(xrow, D, lane, xv);
    const float gs = gscale ? *gscale : 1.f;
    const int nb = is_img ? Bc : Bi;
    for (int p0 = 0; p0 < nb; p0 += 64) {
      const int pl = p0 + lane;
      float g = 0.f;
      if (pl < nb) g = is_img ? dS[(int64_t)own_b * ld + pl] : dS[(int64_t)pl * ld + own_b];
      unsigned long long live = __ballot(g != 0.f);
      while (live) {
        const int k = __ffsll((long long)live) - 1; live &= live - 1;
        const int partner = p0 + k;
        const float gk = lane_bcast(g, k) * gs;
        if (!is_img) {
          // caption row (j, w): the winning region of image `partner`
          const unsigned rho = table[((int64_t)partner * Bc + own_b) * tstride + idx];
          if (rho != LONG_NO_GRAD) {
            long_gather<NCH, P16>(im + partner * im_sb + (int64_t)(rho + 1) * im_sr, pk.xm + ((int64_t)partner * pk.mrows + rho) * pk.Dp, gk,
                                  D, lane, acc);
            any = true;
          }
        } else {
          // image row (i, rho): every word of caption `partner` whose arg-max is rho (LONG_NO_GRAD never equals an index)
          const uint16_t* trow = table + ((int64_t)own_b * Bc + partner) * tstride;
          for (int w0 = 0; w0 < tstride; w0 += 64) {
            const int w = w0 + lane;
            unsigned long long hits = __ballot(w < tstride && trow[w < tstride ? w : 0] == (uint16_t)idx);
            while (hits) {
              const int wb = w0 + __ffsll((long long)hits) - 1; hits &= hits - 1;
              long_gather<NCH, P16>(s + partner * s_sb + (int64_t)(wb + 1) * s_st, pk.y + ((int64_t)partner * pk.trows + wb) * pk.Dp, gk,
                                    D, lane, acc);
              any = true;
            }
          }
        }
      }
    }
  }
  if (!any) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = lane * 4 + 256 * c;
      if (col < D) *reinterpret_cast<float4*>(out + col) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  // normalise backward: xh = x / n, dx = (dxh - xh <xh, dxh>) / n
  float ss = 0.f, dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    ss += xv[c].x * xv[c].x + xv[c].y * xv[c].y + xv[c].z * xv[c].z + xv[c].w * xv[c].w;
    dot += xv[c].x * acc[c].x + xv[c].y * acc[c].y + xv[c].z * acc[c].z + xv[c].w * acc[c].w;
  }
  ss = wave_sum(ss);
  dot = wave_sum(dot);
  const float inv = O16 ? own_inv : 1.0f / fmaxf(sqrtf(ss), 1e-12f);
  const float proj = O16 ? dot : dot * inv * inv;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = lane * 4 + 256 * c;
    if (col < D) {
      float4 o;
      o.x = (acc[c].x - xv[c].x * proj) * inv;
      o.y = (acc[c].y - xv[c].y * proj) * inv;
      o.z = (acc[c].z - xv[c].z * proj) * inv;
      o.w = (acc[c].w - xv[c].w * proj) * inv;
      *reinterpret_cast<float4*>(out + col) = o;
    }
  }
}

template <int NCH>
static int launch_long_rows(bool p16, bool o16, dim3 grid, hipStream_t st, const aladin_set* im, const aladin_set* s,
                            const aladin_align_geom* g, const float* dS, int64_t ld, const float* gscale, const uint16_t* table,
                            int tstride, const aladin_set_grad* d_im, const aladin_set_grad* d_s, LongPacked pk) {
#define LONG_ROWS_ARGS im->data, im->stride_b, im->stride_r, im->len, s->data, s->stride_b, s->stride_r, s->len, g->Bi, g->Bc, g->R, \
    g->T, g->D, dS, ld, gscale, table, tstride, d_im->data, d_s->data, g->x_tail, g->y_tail, d_im->stride_b, d_im->stride_r,       \
    d_s->stride_b, d_s->stride_r, pk
  if (o16) hipLaunchKernelGGL((long_rows_kernel<NCH, true, true>), grid, dim3(256), 0, st, LONG_ROWS_ARGS);
  else if (p16) hipLaunchKernelGGL((long_rows_kernel<NCH, true, false>), grid, dim3(256), 0, st, LONG_ROWS_ARGS);
  else hipLaunchKernelGGL((long_rows_kernel<NCH, false, false>), grid, dim3(256), 0, st, LONG_ROWS_ARGS);
#undef LONG_ROWS_ARGS
  return aladin_check_launch("long_rows_kernel");
}

// flags: the caller (aladin_align_bwd) has rejected unknown bits; the dense bits mean nothing here
int aladin_internal_long_bwd(const aladin_set* im, const aladin_set* s, const aladin_align_geom* g, const aladin_packed* p,
                             const float* dS, int64_t ld_dS, const float* gscale, const aladin_set_grad* d_im,
                             const aladin_set_grad* d_s, void* workspace, int flags, void* stream) {
  if (!set_ok(im) || !set_ok(s) || !dS || !workspace) { aladin_set_error("align_bwd: null argument"); return ALADIN_ERR_ARG; }
  if (!grad_ok(d_im) || !grad_ok(d_s)) { aladin_set_error("align_bwd: bad gradient views"); return ALADIN_ERR_ARG; }
  if (!long_geom_ok(g)) { aladin_set_error("align_bwd: not a long-set geometry of aladin_align_geometry"); return ALADIN_ERR_ARG; }
  if (g->split) { aladin_set_error("align_bwd: split-precision operands are forward-only (evaluation); pack with ALADIN_PRECISION_FP16"); return ALADIN_ERR_UNSUPPORTED; }
  if ((flags & ALADIN_BWD_OWN_ROW_FP16) && !(flags & ALADIN_BWD_PARTNERS_FP16)) { aladin_set_error("align_bwd: ALADIN_BWD_OWN_ROW_FP16 needs ALADIN_BWD_PARTNERS_FP16"); return ALADIN_ERR_ARG; }
  if ((flags & ALADIN_BWD_PARTNERS_FP16) && (!p || !p->xm || !p->y || !p->rnorm)) { aladin_set_error("align_bwd: ALADIN_BWD_PARTNERS_FP16 needs the packed operands with their inverse norms"); return ALADIN_ERR_ARG; }
  if (g->D % 4 != 0 || g->D > 1024) { aladin_set_error("align_bwd: D must be a multiple of 4 and <= 1024 (got %d)", g->D); return ALADIN_ERR_UNSUPPORTED; }
  if (ld_dS < g->Bc) { aladin_set_error("align_bwd: ld_dS %lld < Bc %d", (long long)ld_dS, g->Bc); return ALADIN_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  LongWs ws;
  pair_ws_layout(g->Bi, g->Bc, g->Tq, (char*)workspace, &ws);
  const int tstride = table_stride(g->Tq);
  if (int rc = aladin_internal_compact_pairs(dS, ld_dS, g->Bi, g->Bc, ws.counter, ws.pairs, "align_bwd", st)) return rc;     // list order is irrelevant: one workgroup per pair
  const int64_t n = (int64_t)g->Bi * g->Bc;
  const int pblocks = (int)(n < 2048 ? n : 2048);
  hipLaunchKernelGGL(long_pair_argmax_kernel, dim3(pblocks), dim3(256), 0, st, im->data, im->stride_b, im->stride_r, im->len, s->data,
                     s->stride_b, s->stride_r, s->len, g->Bc, g->Rq, g->Tq, g->D, ws.counter, ws.pairs, ws.table, tstride, g->x_tail,
                     g->y_tail);
  if (int rc = aladin_check_launch("long_pair_argmax_kernel")) return rc;
  const bool p16 = (flags & ALADIN_BWD_PARTNERS_FP16) != 0, o16 = (flags & ALADIN_BWD_OWN_ROW_FP16) != 0;
  LongPacked pk = {p16 ? (const half_t*)p->xm : nullptr, p16 ? (const half_t*)p->y : nullptr, p16 ? p->rnorm : nullptr, g->Dp, g->mrows,
                   g->trows, g->xm_rows};
  const int64_t rows = (int64_t)g->Bi * g->R + (int64_t)g->Bc * g->T;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const int nch = (g->D + 255) / 256;
  switch (nch) {
    case 1: return launch_long_rows<1>(p16, o16, grid, st, im, s, g, dS, ld_dS, gscale, ws.table, tstride, d_im, d_s, pk);
    case 2: return launch_long_rows<2>(p16, o16, grid, st, im, s, g, dS, ld_dS, gscale, ws.table, tstride, d_im, d_s, pk);
    case 3: return launch_long_rows<3>(p16, o16, grid, st, im, s, g, dS, ld_dS, gscale, ws.table, tstride, d_im, d_s, pk);
    default: return launch_long_rows<4>(p16, o16, grid, st, im, s, g, dS, ld_dS, gscale, ws.table, tstride, d_im, d_s, pk);
  }
}
