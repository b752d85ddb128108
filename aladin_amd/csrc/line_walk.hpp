// One pass over the 2B lines of a B x B matrix S (line v in [0, 2B): row v, or column v - B) with an accumulator per line: the
// walk of xent_stats_kernel (xent.hip) and sem_stats_kernel (semantic.hip), and the frame of the finish pass behind it.
//   blocks [0, cdiv(B, 16))            rows, one wave each, lanes strided over the columns, met by Acc::wave_reduce
//   the following cdiv(B, 64) blocks   strips of 64 adjacent columns, lanes across columns (coalesced 256-byte reads); wave w walks
//                                      rows w, w + 16, .. four loads in flight; wave 0 merges the 16 partials from LDS, ascending
// Acc supplies clear(), wave_reduce() (result in every lane), merge(other) and its FIELDS 32-bit fields to and from LDS: put(p) /
// get(p), field f at p[64 * f].  Element order and merge order are fixed (the same bits every run); the walk does no arithmetic.
#pragma once
#include "common.hpp"

#define LINE_WALK_THREADS 1024
#define LINE_WALK_WAVES (LINE_WALK_THREADS / 64)

static inline int line_row_blocks(int B) { return cdiv(B, LINE_WALK_WAVES); }
static inline int line_walk_blocks(int B) { return line_row_blocks(B) + cdiv(B, 64); }

// the line this thread works on in line_walk, -1 if none: for what the caller keeps per line (an anchor)
__device__ __forceinline__ int line_walk_line(int B, int row_blocks) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int q = b < row_blocks ? b * LINE_WALK_WAVES + (t >> 6) : (b - row_blocks) * 64 + (t & 63);
  return q >= B ? -1 : b < row_blocks ? q : B + q;
}

// add(acc, s, i, j, t): element t of the line, S[i][j] = s;  store(acc, v): line v is complete (one lane calls it)
template <class Acc, class Add, class Store>
__device__ __forceinline__ void line_walk(const float* __restrict__ S, int64_t ld, int B, int row_blocks, Add add, Store store) {
  __shared__ float part[LINE_WALK_WAVES][Acc::FIELDS][64];   // lane-contiguous per field
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  Acc acc;
  acc.clear();
  if ((int)blockIdx.x < row_blocks) {
    const int i = blockIdx.x * LINE_WALK_WAVES + wave;
    if (i >= B) return;                                      // wave-uniform; no barrier on this side
    const float* __restrict__ row = S + (int64_t)i * ld;
    for (int j = lane; j < B; j += 64) add(acc, row[j], i, j, j);
    acc.wave_reduce();
    if (lane == 0) store(acc, i);
    return;
  }
  const int j = ((int)blockIdx.x - row_blocks) * 64 + lane;
  const bool live = j < B;
  const float* __restrict__ col = S + (live ? j : 0);
  // four rows in flight per wave: the loads do not depend on the running state
  int i = wave;
  for (; i + 3 * LINE_WALK_WAVES < B; i += 4 * LINE_WALK_WAVES) {
    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = live ? col[(int64_t)(i + q * LINE_WALK_WAVES) * ld] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (live) add(acc, x[q], i + q * LINE_WALK_WAVES, j, i + q * LINE_WALK_WAVES);
  }
  for (; i < B; i += LINE_WALK_WAVES)
    if (live) add(acc, col[(int64_t)i * ld], i, j, i);
  acc.put(&part[wave][0][lane]);
  __syncthreads();
  if (wave != 0 || !live) return;
  for (int w = 1; w < LINE_WALK_WAVES; ++w) {                // ascending waves: a fixed order
    Acc o;
    o.get(&part[w][0][lane]);
    acc.merge(o);
  }
  store(acc, B + j);
}

// The finish pass's grid: (cdiv(B, 256) column chunks, row groups: about 2048 workgroups at the most); no gradient: one block
static inline dim3 line_finish_grid(int B, bool want_grad) {
  const int gx = want_grad ? cdiv(B, 256) : 1;
  int gy = want_grad ? 2048 / gx : 1;
  if (gy > B) gy = B;
  if (gy < 1) gy = 1;
  return dim3(gx, gy);
}

// {sum of value(v) over the rows v in [0, B), over the columns v in [B, 2B)}: rows first, each a block_sum (`red`: its four entries)
template <class Value>
__device__ __forceinline__ float2 line_sums(int B, float* red, Value value) {
  float rs = 0.f, cs = 0.f;
  for (int t = threadIdx.x; t < B; t += blockDim.x) { rs += value(t); cs += value(B + t); }
  rs = block_sum(rs, red);
  cs = block_sum(cs, red);
  return make_float2(rs, cs);
}
