// What the evaluation similarity GEMM's users share: recall.hip (stored matrix, ranks, fused retrieval, top-k lists) and
// search.hip (top-k gallery search without the score matrix).  The operand layout, the chain order and the tile configuration
// live here once, so every kernel that runs the chain produces the same bits for the same pair.
#pragma once
#include "gemm_core.hpp"

using SimCfg = GemmCfg<2, 4, 4, 3>;       // 256 x 384 tile, 8 waves x (128 x 96), v_mfma_f32_16x16x32_f16 body (gemm_mainloop16_tall, gemm_core.hpp:
                                          // 14 instead of 16 LDS fragment reads per 32-deep step; an accumulator's bits do not depend on the wave tiling)
constexpr int SIM_RT = 2 * SimCfg::WM, SIM_CT = 2 * SimCfg::WN;      // 16 x 16 accumulator tiles per wave: 8 x 6

// K step -> K offsets inside [hi | lo] rows for the chain segments 0 = hi.hi, 1 = lo.hi, 2 = hi.lo
struct KMapSplit {
  int kps;        // 64-deep K steps per segment (Dp / 64)
  int seg0;       // segment of K step 0 of this call
  __device__ __forceinline__ int64_t a(int kt) const { const int q = kt / kps; return (int64_t)((seg0 + q == 1) ? kps : 0) * 64 + (int64_t)(kt - q * kps) * 64; }
  __device__ __forceinline__ int64_t b(int kt) const { const int q = kt / kps; return (int64_t)((seg0 + q == 2) ? kps : 0) * 64 + (int64_t)(kt - q * kps) * 64; }
};

struct SimWs {
  float* scale;      // [0] = 2^ea, [1] = 2^eb  (256 B block)
  float* partial;    // 2 x SIM_ABS_BLOCKS per-block absmax partials (images, captions)
  half_t* a;         // Mp x 2Dp  [hi | lo]
  half_t* b;         // Np x 2Dp
  float2* na;        // Mp: (P, R) = (|lo|, |hi|) of the image row, rounded up
  float2* nb;        // Np: (Q, T) = (|hi|, |lo|) of the caption row, rounded up
};

static size_t sim_ws_layout(int n_img, int n_cap, int D, char* base, SimWs* ws, int* Mp_, int* Np_, int* Dp_) {
  const int Mp = round_up(n_img, SimCfg::BM), Np = round_up(n_cap, SimCfg::BN), Dp = round_up(D, 64);
  if (Mp_) *Mp_ = Mp;
  if (Np_) *Np_ = Np;
  if (Dp_) *Dp_ = Dp;
  size_t off = 0;
  if (ws) ws->scale = (float*)(base + off);
  off += 256;
  if (ws) ws->partial = (float*)(base + off);
  off += 2 * 1024 * 4;                                     // SIM_ABS_BLOCKS
  if (ws) ws->a = (half_t*)(base + off);
  off += (size_t)Mp * 2 * Dp * 2;
  if (ws) ws->b = (half_t*)(base + off);
  off += (size_t)Np * 2 * Dp * 2;
  if (ws) ws->na = (float2*)(base + off);
  off += (size_t)Mp * 8;
  if (ws) ws->nb = (float2*)(base + off);
  off += (size_t)Np * 8;
  return off;
}

// scale search + split-fp16 packing shared by the GEMM modes (recall.hip; zero*: int32 words the pack grid clears on its way)
int sim_prepare(const float* img, int64_t img_rs, const float* cap, int64_t cap_rs, int n_img, int n_cap, int D,
                void* workspace, SimWs* ws, int* Mp, int* Np, int* Dp, hipStream_t st, int32_t* zero0 = nullptr, int64_t nz0 = 0,
                int32_t* zero1 = nullptr, int64_t nz1 = 0, int32_t* zero2 = nullptr, int64_t nz2 = 0, int cpi = 0,
                float* gt = nullptr, unsigned long long* best_i2t = nullptr, unsigned long long* best_t2i = nullptr,
                bool* gt_done = nullptr);

// the launch of topk_kernel (recall.hip) behind aladin_topk: arguments already checked, n_c <= TOPK_MAX_CAND
#define TOPK_MAX_CAND 36864          // 144 KiB of LDS
int sim_topk_launch(const float* M, int64_t q_stride, int64_t c_stride, int n_q, int n_c, int k, int32_t* out_idx, float* out_val,
                    hipStream_t st);

// order-preserving map float -> uint (NaN excluded by the callers) and back
__device__ __forceinline__ unsigned float_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ unsigned long long pack_best(float v, int idx) {
  return ((unsigned long long)float_key(v) << 32) | (unsigned)(0x7fffffff - idx);      // ties -> the smaller index wins
}

// threadIdx.x as a value the compiler cannot merge with the copy it computed before a main loop: what the epilogues derive from it
// is recomputed after the loop instead of living (or spilling) through it
__device__ __forceinline__ int fresh_tid() { int t = threadIdx.x; asm volatile("" : "+v"(t)); return t; }
__device__ __forceinline__ float fmax_nc(float a, float b) { return __builtin_elementwise_maximum(a, b); }    // IEEE maximum: no canonicalising v_max x, x, x
__device__ __forceinline__ float row16_max(float v) {
  v = fmax_nc(v, ALADIN_ROW_ROR(v, 8));
  v = fmax_nc(v, ALADIN_ROW_ROR(v, 4));
  v = fmax_nc(v, ALADIN_ROW_ROR(v, 2));
  v = fmax_nc(v, ALADIN_ROW_ROR(v, 1));
  return v;
}
