// What the two alignment backwards share (align_bwd.hip: the tile classes, 8-bit arg-max table; align_long.hip: long sets,
// 16-bit table; align_bwd_dense.hip: the GEMM row step): the problem description, the head of the workspace, and those device
// helpers of the fp32 pair kernels and of the row kernels that every kernel compiles to the same instructions with as with its own
// copy (which ones did not, and so stay where they were: DESIGN_HISTORY.md, "Alignment backward: plain stages ...").
#pragma once
#include "../../include/aladin_hip.h"
#include "common.hpp"
#include "pack_rows.hpp"      // set_ok

// One alignment-backward problem, as every host stage sees it.
struct BwdProblem {
  aladin_set im, s;                  // max-side / sum-side sets
  const aladin_align_geom* g;        // always present: sizes and tails
  const aladin_packed* pk;           // the forward's packed operands (xm and y at least); nullptr = none
  bool pair16;                       // pk is there and the fp16 pair kernel covers the class (pair16_covers)
  hipStream_t st;
};

static inline bool grad_ok(const aladin_set_grad* v) { return v && v->data && v->stride_b >= 1 && v->stride_r >= 1; }

// align_bwd.hip: zero the workspace's counter block and list the non-zero pairs of dS (bwd_compact_kernel); `entry` names the
// calling entry point in the error text
int aladin_internal_compact_pairs(const float* dS, int64_t ld, int Bi, int Bc, int* counter, int* pairs, const char* entry, hipStream_t st);
// align_long.hip: what aladin_align_bwd_workspace_bytes / aladin_align_bwd do for ALADIN_LAYOUT_LONG (0 bytes: not such a geometry)
size_t aladin_internal_long_bwd_bytes(const aladin_align_geom* g);
int aladin_internal_long_bwd(const aladin_set* im, const aladin_set* s, const aladin_align_geom* g, const aladin_packed* p, const float* dS,
                             int64_t ld_dS, const float* gscale, const aladin_set_grad* d_im, const aladin_set_grad* d_s, void* workspace,
                             int flags, void* stream);
// align_bwd_dense.hip: the row step of the dense-dS backward as two MFMA GEMMs over the arg-max table (see there)
size_t aladin_internal_dense_rows_bytes(const aladin_align_geom* g);
int aladin_internal_dense_rows(const BwdProblem& pr, const float* dS, int64_t ld_dS, const float* gscale, const uint8_t* table,
                               const unsigned* dsmax, const aladin_set_grad* d_im, const aladin_set_grad* d_s, int fp16_only, void* scratch);

// ---- head of the backward workspace: [counter | pairs | table], E = the table's entry type -------------------------------------
template <typename E>
struct PairWs {
  int* counter;      // [64] ints, [0] = number of listed pairs
  int* pairs;        // Bi*Bc
  E* table;          // Bi*Bc rows of table_stride(Tq) entries
};
static inline int table_stride(int Tq) { return (Tq + 15) / 16 * 16; }
template <typename E>
static size_t pair_ws_layout(int Bi, int Bc, int Tq, char* base, PairWs<E>* ws) {
  size_t off = 0;
  if (ws) ws->counter = (int*)(base + off);
  off += 256;
  if (ws) ws->pairs = (int*)(base + off);
  off += ((size_t)Bi * Bc * 4 + 255) / 256 * 256;
  if (ws) ws->table = (E*)(base + off);
  off += ((size_t)Bi * Bc * table_stride(Tq) * sizeof(E) + 255) / 256 * 256;
  return off;
}

// ---- fp32 cosine tile of the fp32 pair arg-max kernels (32 x 32 dot products of raw rows with v_mfma_f32_32x32x2_f32) -----------
// ss: ||x||^2 of region (lane & 31), on both half-waves; h = lane >> 5
// accumulator register r of a lane holds tile row cos_tile_row(r, h) (column lane & 31); its cosine needs the norm of THAT row,
// held by lane (row).  The caption norm is a positive column factor: irrelevant for arg-max / sign.
__device__ __forceinline__ int cos_tile_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ float cos_tile_inv_norm(float ss, int row) { return 1.0f / fmaxf(sqrtf(__shfl(ss, row, 64)), 1e-12f); }

// ---- row kernels: one wave per output row, lane owns float4 columns lane*4 + 256*c ----------------------------------------------
// FULL: D == 256 NCH (D = 768, 512, 256, 1024): every lane's columns exist and the loads need no per-chunk exec-mask branch
template <int NCH, bool FULL>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int D, int lane, float4 (&v)[NCH]) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = lane * 4 + 256 * c;
    v[c] = (FULL || col < D) ? *reinterpret_cast<const float4*>(p + col) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
// a row of the forward's PACKED operands: a unit vector already, rounded once to fp16
template <int NCH, bool FULL>
__device__ __forceinline__ void load_row_h(const half_t* __restrict__ p, int D, int lane, float4 (&v)[NCH]) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = lane * 4 + 256 * c;
    if (FULL || col < D) {
      const uint2 raw = *reinterpret_cast<const uint2*>(p + col);
      const half_t* h = reinterpret_cast<const half_t*>(&raw);
      v[c] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
    } else v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
template <int NCH>
__device__ __forceinline__ float row_sumsq(const float4 (&v)[NCH]) {
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) ss += v[c].x * v[c].x + v[c].y * v[c].y + v[c].z * v[c].z + v[c].w * v[c].w;
  return ss;
}
template <int NCH>
__device__ __forceinline__ void axpy_row(float f, const float4 (&v)[NCH], float4 (&acc)[NCH]) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) { acc[c].x += f * v[c].x; acc[c].y += f * v[c].y; acc[c].z += f * v[c].z; acc[c].w += f * v[c].w; }
}
