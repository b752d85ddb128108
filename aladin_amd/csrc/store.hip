// Device-resident embedding store for evaluation (replaces the
// (N, 71, D) fp32 host buffers of reference alad/evaluation.py:119-130).
//
// A store keeps, per sample, ONLY the positions the alignment head reads -- [1, len - tail) of its
// set (alad/loss.py:87-90) -- L2-normalised exactly as the pack kernels do (fp32 sum of squares, eps
// 1e-12, one rounding to fp16), contiguous by true length:
//     rows   : (total_rows, Dp) fp16, sample k at rows [offset[k], offset[k] + count[k])
// so a 25 000-caption set of ~12 scored words is 0.46 GB instead of 5.4 GB, and building the MFMA
// operands of any sub-grid is a pure 16-byte row copy (no normalisation, half the bytes read).
// Scores from a store are bit-identical to scores from the fp32 sets.
#include "pack_rows.hpp"

namespace {

// one wave per destination row; src fp32 row (or none -> nothing written).  The encoder of pack_rows.hpp: a row's bits are those
// pack_rows_kernel gives it
__global__ __launch_bounds__(256) void store_append_kernel(const float* __restrict__ src, int64_t sb, int64_t sr,
                                                           const int32_t* __restrict__ lens, int B, int L, int D, int Dp,
                                                           int tail, const int64_t* __restrict__ offsets,
                                                           half_t* __restrict__ rows, int vec4, int split) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);        // (sample, position) over B x (L - 1)
  if (d >= (int64_t)B * (L - 1)) return;
  const int k = (int)(d / (L - 1)), p = (int)(d % (L - 1));               // position p + 1 of the set
  if (p >= scored_len(lens[k], tail, L - 1)) return;
  const float* x = src + k * sb + (int64_t)(p + 1) * sr;
  half_t* dst = rows + (offsets[k] + p) * (split ? 2 * Dp : Dp);
  const float inv = inv_norm_mem(x, D, lane, vec4 != 0);
  if (split) write_split(dst, nullptr, dst + Dp, x, inv, D, Dp, lane);   // [hi | lo]
  else write_fp16_mem(dst, x, inv, D, Dp, lane, vec4 != 0);
}

__device__ __forceinline__ void copy_row(const half_t* __restrict__ src, half_t* __restrict__ dst, int Dp, int lane) {
  if (src == nullptr) {
    write_zero_row(dst, Dp, lane);
  } else {
    for (int c = lane * 8; c < Dp; c += 512) *reinterpret_cast<half8*>(dst + c) = *reinterpret_cast<const half8*>(src + c);
  }
}

// split rows: store [hi | lo] (2 * Dp0) -> operand [hi | lo | hi] (seg 1, max side) or [hi | hi | lo] (seg 2, sum side)
__device__ __forceinline__ void copy_row_split(const half_t* __restrict__ src, half_t* __restrict__ dst, int Dp0, int lane, int seg) {
  for (int c = lane * 8; c < Dp0; c += 512) {
    half8 hi = half8{0, 0, 0, 0, 0, 0, 0, 0}, lo = hi;
    if (src != nullptr) { hi = *reinterpret_cast<const half8*>(src + c); lo = *reinterpret_cast<const half8*>(src + Dp0 + c); }
    *reinterpret_cast<half8*>(dst + c) = hi;
    *reinterpret_cast<half8*>(dst + Dp0 + c) = seg == 1 ? lo : hi;
    *reinterpret_cast<half8*>(dst + 2 * Dp0 + c) = seg == 1 ? hi : lo;
  }
}

// a sample's scored row `pos` in the store (k = ids[sample], or the sample itself), or nullptr: a masked position
__device__ __forceinline__ const half_t* store_row(const half_t* __restrict__ rows, const int64_t* __restrict__ offsets,
                                                   const int32_t* __restrict__ counts, const int32_t* __restrict__ ids, int sample,
                                                   int pos, int cap, int Dp, int split) {
  const int k = ids ? ids[sample] : sample;
  const int n = counts[k] > cap ? cap : counts[k];
  return pos < n ? rows + (offsets[k] + pos) * (split ? 2 * (Dp / 3) : Dp) : nullptr;
}

// max-side operand (xm / xe) from a store: d over [xm rows | xe rows]
__global__ __launch_bounds__(256) void store_pack_x_kernel(const half_t* __restrict__ rows, const int64_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ ids, int Bi, int Dp, MaxSideMap map,
                                                           int64_t total_rows, half_t* __restrict__ xm,
                                                           half_t* __restrict__ xe, int split) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= total_rows) return;
  const MaxSideRow r = max_side_row(d, map);
  half_t* dst = (r.side ? xe : xm) + r.row * Dp;
  const half_t* src = r.i < Bi ? store_row(rows, offsets, counts, ids, r.i, r.rho, map.Rq, Dp, split) : nullptr;
  if (split) copy_row_split(src, dst, Dp / 3, lane, 1);
  else copy_row(src, dst, Dp, lane);
}

// sum-side operand (y): d over the y rows
__global__ __launch_bounds__(256) void store_pack_y_kernel(const half_t* __restrict__ rows, const int64_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ ids, int Bc, int Tq, int Dp, int tpad,
                                                           int64_t total_rows, half_t* __restrict__ y, int split) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= total_rows) return;
  const SumSideRow r = sum_side_row(d, tpad);
  const half_t* src = r.j < Bc ? store_row(rows, offsets, counts, ids, r.j, r.w, Tq, Dp, split) : nullptr;
  if (split) copy_row_split(src, y + d * Dp, Dp / 3, lane, 2);
  else copy_row(src, y + d * Dp, Dp, lane);
}

}  // namespace

static int store_row_width_fp16(int D) {
  aladin_align_geom g;
  if (aladin_align_geometry(1, 1, 2, 4, D, 0, 2, ALADIN_PRECISION_FP16, ALADIN_LAYOUT_TILES, &g) != ALADIN_OK) return -1;
  return g.Dp;
}

extern "C" int aladin_store_row_width(int D, int precision) {
  const int w = store_row_width_fp16(D);
  return (w > 0 && precision == ALADIN_PRECISION_SPLIT) ? 2 * w : w;
}

extern "C" int aladin_store_append(const float* sets, int64_t stride_b, int64_t stride_r, const int32_t* lens, int B, int L,
                                   int D, int tail, const int64_t* offsets, void* rows, int precision, void* stream) {
  if (precision != ALADIN_PRECISION_FP16 && precision != ALADIN_PRECISION_SPLIT) { aladin_set_error("store_append: unknown precision %d", precision); return ALADIN_ERR_ARG; }
  if (!sets || !lens || !offsets || !rows || B < 1 || L < 2 || D < 1 || tail < 0) {
    aladin_set_error("store_append: bad argument (B=%d L=%d D=%d tail=%d)", B, L, D, tail);
    return ALADIN_ERR_ARG;
  }
  const int Dp = store_row_width_fp16(D);
  if (Dp < D) return ALADIN_ERR_ARG;
  const int64_t total = (int64_t)B * (L - 1);
  hipLaunchKernelGGL(store_append_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, sets, stride_b,
                     stride_r, lens, B, L, D, Dp, tail, offsets, (half_t*)rows, is_vec4_ok(sets, stride_b, stride_r, D), precision == ALADIN_PRECISION_SPLIT);
  return aladin_check_launch("store_append_kernel");
}

extern "C" int aladin_align_pack_store_x(const void* rows, const int64_t* offsets, const int32_t* counts, const int32_t* ids,
                                         const aladin_align_geom* g, void* xm, void* xe, void* stream) {
  if (!rows || !offsets || !counts || !g || !xm || (g->rem && !xe)) { aladin_set_error("align_pack_store_x: null argument"); return ALADIN_ERR_ARG; }
  if (g->layout == ALADIN_LAYOUT_LONG) { aladin_set_error("align_pack_store_x: the store packers cover the tile classes, not a long-set geometry"); return ALADIN_ERR_ARG; }
  const int64_t total = g->xm_rows + g->xe_rows;
  hipLaunchKernelGGL(store_pack_x_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)rows, offsets, counts, ids, g->Bi, g->Dp, MaxSideMap{g->mrows, g->rem > 0 ? g->rem : 1, g->Rq, g->xm_rows}, total, (half_t*)xm,
                     (half_t*)xe, g->split);
  return aladin_check_launch("store_pack_x_kernel");
}

extern "C" int aladin_align_pack_store_y(const void* rows, const int64_t* offsets, const int32_t* counts, const int32_t* ids,
                                         const aladin_align_geom* g, void* y, void* stream) {
  if (!rows || !offsets || !counts || !g || !y) { aladin_set_error("align_pack_store_y: null argument"); return ALADIN_ERR_ARG; }
  if (g->layout == ALADIN_LAYOUT_LONG) { aladin_set_error("align_pack_store_y: the store packers cover the tile classes, not a long-set geometry"); return ALADIN_ERR_ARG; }
  hipLaunchKernelGGL(store_pack_y_kernel, dim3((unsigned)((g->y_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)rows, offsets, counts, ids, g->Bc, g->Tq, g->Dp, g->trows, g->y_rows, (half_t*)y, g->split);
  return aladin_check_launch("store_pack_y_kernel");
}
