// The packed fp16 operand format in one place: which raw row a packed row holds, which rows count, and how a row is
// normalised and rounded.  Everything that WRITES the format composes these helpers -- pack_rows_kernel (pack.hip), the batched
// main-row packer beside the side GEMM (pack_main_rows, align_fwd.hip), the evaluation store and its two packers (store.hip) --
// so a row's bits do not depend on which of them wrote it ("scores from a store are bit-identical to scores from the fp32 sets").
// Device and host inline helpers only; no kernels.
//
// Row space [xm | xe | y], one rnorm slot per row in the same order:
//   xm   image i at rows [i * mrows, (i + 1) * mrows): its scored regions 0 .. R' - 1 (raw positions 1 .. R'), rows past R' COPIES
//        of region 0 (max is idempotent; a zero would wrongly clamp the max of an image without padded regions);
//   xe   image i at rows [i * rem, (i + 1) * rem): regions mrows .. mrows + rem - 1, the side GEMM's operand;
//   y    caption j at rows [j * trows, (j + 1) * trows): its scored words 0 .. T' - 1 (raw positions 1 .. T').
// All masking of the reference (alad/loss.py:103-116) is folded into the packed data: a position at or past the sample's scored
// length, and every row of a sample that only pads a tile, is a ZERO row -- its dot products are exactly 0, which is what
// masked_fill_(.., 0) leaves in the reference before max / sum -- with rnorm 0 (such a row never carries a gradient).
#pragma once
#include "../../include/aladin_hip.h"
#include "common.hpp"

// Split precision: x^ * 2^14 = hi + lo, both fp16; a packed row is three K segments of Dp halfs, [hi | lo | hi] on the max side and
// [hi | hi | lo] on the sum side (the store keeps [hi | lo]).  The scale keeps lo out of the fp16 subnormals for every component
// above 2^-14 * 2^-3; what is lost below that is < 2^-39 absolute per component.  The scores come out scaled by 2^28 (a power of
// two: max and sum commute with it exactly) and are scaled back after the score kernel.
#define ALADIN_SPLIT_SCALE 16384.0f
#define ALADIN_SPLIT_UNSCALE (1.0f / (16384.0f * 16384.0f))

// positions of a set of length `len` that count: position 0 and the last `tail` are dropped (alad/loss.py:87-90), at most `cap`
__host__ __device__ __forceinline__ int scored_len(int len, int tail, int cap) {
  const int L = len - 1 - tail;
  return L < 0 ? 0 : (L > cap ? cap : L);
}

static inline bool set_ok(const aladin_set* v) { return v && v->data && v->len; }

// can rows of a (B, N, D) set be read as float4?
static inline int is_vec4_ok(const void* p, int64_t s0, int64_t s1, int D) {
  return (D % 4 == 0) && (s0 % 4 == 0) && (s1 % 4 == 0) && (((uintptr_t)p & 15) == 0);
}

// ------------------------------------------------------------------------------------------------
// row maps
// ------------------------------------------------------------------------------------------------
struct MaxSideMap { int mrows, rem, Rq; int64_t xm_rows; };      // rem >= 1 (a map without side rows never reaches the division)
struct MaxSideRow { int i, rho; bool side; int64_t row; };       // sample, region, and the row of xm (or of xe: side)

// region of the k-th row of an image's main tile: rows past R' are tile-filling copies of region 0
__device__ __forceinline__ int main_row_region(int k, int Rq) { return k >= Rq ? 0 : k; }

// d over [xm rows | xe rows]
__device__ __forceinline__ MaxSideRow max_side_row(int64_t d, const MaxSideMap& m) {
  MaxSideRow r;
  r.side = d >= m.xm_rows;
  if (!r.side) {
    r.i = (int)(d / m.mrows);
    r.rho = main_row_region((int)(d % m.mrows), m.Rq);
    r.row = d;
  } else {
    r.row = d - m.xm_rows;
    r.i = (int)(r.row / m.rem);
    r.rho = m.mrows + (int)(r.row % m.rem);                      // the leftover region(s)
  }
  return r;
}

struct SumSideRow { int j, w; };
// q over the y rows
__device__ __forceinline__ SumSideRow sum_side_row(int64_t q, int trows) { return SumSideRow{(int)(q / trows), (int)(q % trows)}; }

// ------------------------------------------------------------------------------------------------
// row encoder: fp32 sum of squares (the sumsq4 chain), wave_sum, 1 / max(sqrt, 1e-12), one rounding per element
// ------------------------------------------------------------------------------------------------
// The two inverse norms below are equal bit for bit: the register form adds fmaf(0, 0, ss) = ss for the float4 past D.
__device__ __forceinline__ float inv_norm_of(float ss_lane) {
  return 1.0f / fmaxf(sqrtf(wave_sum(ss_lane)), 1e-12f);         // F.normalize eps (alad/loss.py:80-81)
}

// a whole row in registers (D <= 1024, float4-addressable): <= 4 float4 per lane, all of the row's loads in flight at once.
// Columns past D read as zeros (D = 0: a row that does not exist, nothing is loaded)
__device__ __forceinline__ void load_row_regs(float4 (&v)[4], const float* __restrict__ src, int D, int lane) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane * 4 + 256 * k;
    v[k] = c < D ? *reinterpret_cast<const float4*>(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ float inv_norm_regs(const float4 (&v)[4]) {
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) ss = sumsq4(ss, v[k]);
  return inv_norm_of(ss);
}

__device__ __forceinline__ float inv_norm_mem(const float* __restrict__ src, int D, int lane, bool vec4) {
  float ss = 0.f;
  if (vec4) {
    for (int c = lane * 4; c < D; c += 256) ss = sumsq4(ss, *reinterpret_cast<const float4*>(src + c));
  } else {
    for (int c = lane; c < D; c += 64) ss = fmaf(src[c], src[c], ss);
  }
  return inv_norm_of(ss);
}

__device__ __forceinline__ half4 unit_half4(const float4& v, float inv) {
  return half4{(half_t)(v.x * inv), (half_t)(v.y * inv), (half_t)(v.z * inv), (half_t)(v.w * inv)};
}

// the fp16 row (Dp halfs, columns D .. Dp zero) from registers / from memory
__device__ __forceinline__ void write_fp16_regs(half_t* __restrict__ dst, const float4 (&v)[4], float inv, int Dp, int lane) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = lane * 4 + 256 * k;
    if (c < Dp) *reinterpret_cast<half4*>(dst + c) = unit_half4(v[k], inv);
  }
}

__device__ __forceinline__ void write_fp16_mem(half_t* __restrict__ dst, const float* __restrict__ src, float inv, int D, int Dp,
                                               int lane, bool vec4) {
  if (vec4) {
    for (int c = lane * 4; c < Dp; c += 256) {
      half4 h = {0, 0, 0, 0};
      if (c < D) h = unit_half4(*reinterpret_cast<const float4*>(src + c), inv);
      *reinterpret_cast<half4*>(dst + c) = h;
    }
  } else {
    for (int c = lane; c < Dp; c += 64) dst[c] = (c < D) ? (half_t)(src[c] * inv) : (half_t)0;
  }
}

// the split row: hi to d_hi and (unless nullptr) d_hi2, lo to d_lo, Dp halfs each.  [hi | lo | hi]: (dst, dst + 2 Dp, dst + Dp);
// [hi | hi | lo]: (dst, dst + Dp, dst + 2 Dp); the store's [hi | lo]: (dst, nullptr, dst + Dp)
__device__ __forceinline__ void write_split(half_t* __restrict__ d_hi, half_t* __restrict__ d_hi2, half_t* __restrict__ d_lo,
                                            const float* __restrict__ src, float inv, int D, int Dp, int lane) {
  for (int c = lane; c < Dp; c += 64) {
    half_t hi = (half_t)0, lo = (half_t)0;
    if (c < D) {
      const float v = src[c] * inv * ALADIN_SPLIT_SCALE;
      hi = (half_t)v;
      lo = (half_t)(v - (float)hi);
    }
    d_hi[c] = hi; d_lo[c] = lo;
    if (d_hi2 != nullptr) d_hi2[c] = hi;
  }
}

// width halfs of zeros (a multiple of 8: Dp is a multiple of 64)
__device__ __forceinline__ void write_zero_row(half_t* __restrict__ dst, int width, int lane) {
  for (int c = lane * 8; c < width; c += 64 * 8) *reinterpret_cast<half8*>(dst + c) = half8{0, 0, 0, 0, 0, 0, 0, 0};
}

// 1 / max(|x|, 1e-12) of the row -- what the backward's normalise step divides by, so that it need not read the raw fp32 row
// again (0 for a zero row).  slot may be nullptr.
__device__ __forceinline__ void write_rnorm(float* __restrict__ slot, float inv, int lane) {
  if (slot != nullptr && lane == 0) *slot = inv;
}
