// What the users of the evaluation similarity GEMM share: sim_pack.hip (operand preparation), recall.hip (stored matrix, ranks, top-k
// lists), retrieval.hip (fused, prefix-screened retrieval) and search.hip (top-k gallery search without the score matrix).  The operand
// layout, the chain order and the tile configuration live here once, so every kernel that runs the chain produces the same bits for the
// same pair; so do the top-k selection rounds and the packed (score, index) key.
//
// Ranks must agree with the fp32 reference, so the 16-bit MFMA path uses a hi/lo split:
//   x * 2^e = hi + lo (both fp16),  <a,b> ~ (ah.bh + al.bh + ah.bl) * 2^-(ea+eb)
// i.e. three fp16 MFMA products accumulated in fp32 (~2^-21 relative operand error, the level of
// fp32 rounding in the reference's own sgemm).  An operand row is stored [hi | lo] (2 Dp halfs) and the
// EXACT score of a pair is ONE accumulator chain over the 32-deep K blocks of  hi.hi, then lo.hi, then
// hi.lo  (KMapSplit walks the LDS-staged main loop of gemm_core.hpp through the three segments).  An
// output element of v_mfma_f32_16x16x32_f16 depends only on its own row / column operands, its
// accumulator input and that block order, so every kernel that runs this chain -- the stored
// matrix, the ground-truth scores, the exact tiles of the fused kernel, the re-scored candidates, the gallery
// search -- produces the same bits for the same pair.  The power-of-two scale 2^e (from the operand's absmax)
// keeps lo in fp16's normal range; undoing it is exact.
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

constexpr int SIM_ABS_BLOCKS = 1024;      // blocks of sim_absmax_kernel = per-block partial maxima per operand

struct SimWs {
  float* scale;      // [0] = 2^ea, [1] = 2^eb  (256 B block)
  float* partial;    // 2 x SIM_ABS_BLOCKS per-block absmax partials (images, captions)
  half_t* a;         // Mp x 2Dp  [hi | lo]
  half_t* b;         // Np x 2Dp
  float2* na;        // Mp: (P, R) = (|lo|, |hi|) of the image row, rounded up
  float2* nb;        // Np: (Q, T) = (|hi|, |lo|) of the caption row, rounded up
};
struct SimIn {       // the two embedding matrices, row strides in floats
  const float* img;
  int64_t img_rs;
  const float* cap;
  int64_t cap_rs;
  int n_img, n_cap, D;
};
struct SimPacked {   // the padded sizes and where the packed operands live
  int Mp, Np, Dp;
  SimWs ws;
};

// Bump allocation over a workspace that may be absent (base == nullptr: offsets and sizes only).  take<T>(count, align) hands out
// count elements and pads the piece to a multiple of align bytes.
struct WsCursor {
  char* base;
  size_t off;
  template <class T>
  T* take(size_t count, size_t align = 1) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (count * sizeof(T) + align - 1) / align * align;
    return p;
  }
};

static size_t sim_ws_layout(int n_img, int n_cap, int D, char* base, SimPacked* out) {
  SimPacked p;
  p.Mp = round_up(n_img, SimCfg::BM), p.Np = round_up(n_cap, SimCfg::BN), p.Dp = round_up(D, 64);
  WsCursor c{base, 0};
  p.ws.scale = c.take<float>(64);
  p.ws.partial = c.take<float>(2 * SIM_ABS_BLOCKS);
  p.ws.a = c.take<half_t>((size_t)p.Mp * 2 * p.Dp);
  p.ws.b = c.take<half_t>((size_t)p.Np * 2 * p.Dp);
  p.ws.na = c.take<float2>(p.Mp);
  p.ws.nb = c.take<float2>(p.Np);
  if (out) *out = p;
  return c.off;
}

// What only the fused retrieval asks of the preparation (retrieval.hip constructs it): the pack grid clears three ranges of int32
// words on its way and, where a block's rows fit in LDS, the ground-truth scores gt[n_cap] (accumulators' scale) and their arg-max
// entries come out of the same pass.  gt_done (out): they did; false: the caller still has to run sim_gt_kernel.
struct SimFusedPrep {
  int cpi;
  float* gt;
  unsigned long long *best_i2t, *best_t2i;
  int32_t* zero[3];
  int64_t nz[3];
  bool gt_done;
};
// sim_pack.hip: scale search + split-fp16 packing of both operands into `workspace` (aladin_sim_workspace_bytes); fused: null except
// for the fused retrieval.  Returns ALADIN_OK or the error of a launch.
int sim_prepare(const SimIn& in, void* workspace, hipStream_t st, SimPacked* out, SimFusedPrep* fused);
// sim_pack.hip: ONE operand on its own (the gallery index of search.hip and the queries of a search against it).  The n rows of x are
// packed [hi | lo] into dst, rows [n, rows_p) zero; the power-of-two scale of x's absmax goes to scale[slot] and, where other_scale is
// not null, the scale another call left on the device is copied to scale[1 - slot], so a kernel finds the pair where sim_prepare puts
// it.  The same functions (row_absmax, sim_scale_of, sim_pack_row) as sim_prepare: the same bits for the same matrix.
struct SimOperand {
  const float* x;          // n x D, row stride rs floats
  int64_t rs;
  int n, rows_p, D;
  half_t* dst;             // rows_p x 2 Dp
  float* scale;
  int slot;                // 0: the operand is the images, 1: the captions
  const float* other_scale;
};
// any n: sim_absmax_kernel into partial (2 x SIM_ABS_BLOCKS floats), then a grid over the rows
int sim_pack_operand(const SimOperand& op, float* partial, hipStream_t st);
// n <= 32 (the queries of a small batch): one workgroup finds the absmax and packs -- one launch
int sim_pack_operand_small(const SimOperand& op, hipStream_t st);

// One segment of a pair's chain from [hi | lo] rows staged in LDS: nblk 32-deep K blocks in K order, fragment reads batched four blocks
// ahead of their MFMAs (32-bit offsets).
__device__ __forceinline__ void sim_chain_lds(const half_t* __restrict__ ap, const half_t* __restrict__ bp, int nblk, f32x4& acc) {
  int k = 0;
  for (; k + 4 <= nblk; k += 4) {
    half8 af[4], bf[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      af[u] = *reinterpret_cast<const half8*>(ap + (k + u) * 32);
      bf[u] = *reinterpret_cast<const half8*>(bp + (k + u) * 32);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u], bf[u], acc, 0, 0, 0);
  }
  for (; k < nblk; ++k) {
    const half8 af = *reinterpret_cast<const half8*>(ap + k * 32);
    const half8 bf = *reinterpret_cast<const half8*>(bp + k * 32);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc, 0, 0, 0);
  }
}

// recall.hip: for each of n_q queries the k best of its n_c <= TOPK_MAX_CAND scores M[q * q_stride + c * c_stride], as aladin_topk
// (arguments already checked)
#define TOPK_MAX_CAND 36864          // 144 KiB of LDS
int sim_topk_launch(const float* M, int64_t q_stride, int64_t c_stride, int n_q, int n_c, int k, int32_t* out_idx, float* out_val,
                    hipStream_t st);
// recall.hip: top-1 indices out of one or two arrays of packed arg-maxima (pack_best below; n1 = 0: one array)
int sim_unpack_top1_launch(const unsigned long long* p0, int n0, int32_t* top0, const unsigned long long* p1, int n1, int32_t* top1, hipStream_t st);

// order-preserving map float -> uint (NaN excluded by the callers) and back
__device__ __forceinline__ unsigned float_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ unsigned long long pack_best(float v, int idx) {
  return ((unsigned long long)float_key(v) << 32) | (unsigned)(0x7fffffff - idx);      // ties -> the smaller index wins
}
__device__ __forceinline__ int best_index(unsigned long long packed) { return 0x7fffffff - (int)(unsigned)(packed & 0xffffffffull); }

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
__device__ __forceinline__ unsigned wave_or(unsigned v) {
  auto s32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  v = s32[0] | s32[1];
  auto s16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = s16[0] | s16[1];
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false);
  return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ int row16_isum(int t) {
  t += __builtin_amdgcn_update_dpp(0, t, 0x128, 0xF, 0xF, false);
  t += __builtin_amdgcn_update_dpp(0, t, 0x124, 0xF, 0xF, false);
  t += __builtin_amdgcn_update_dpp(0, t, 0x122, 0xF, 0xF, false);
  t += __builtin_amdgcn_update_dpp(0, t, 0x121, 0xF, 0xF, false);
  return t;
}
__device__ __forceinline__ int row16_imin(int t) {
  int o;
  o = __builtin_amdgcn_update_dpp(0, t, 0x128, 0xF, 0xF, false); t = o < t ? o : t;
  o = __builtin_amdgcn_update_dpp(0, t, 0x124, 0xF, 0xF, false); t = o < t ? o : t;
  o = __builtin_amdgcn_update_dpp(0, t, 0x122, 0xF, 0xF, false); t = o < t ? o : t;
  o = __builtin_amdgcn_update_dpp(0, t, 0x121, 0xF, 0xF, false); t = o < t ? o : t;
  return t;
}

// The k selection rounds of a 256-thread workgroup over val[0, n_c) in LDS: larger score first, lower position on equal scores.  A NaN
// slot is RETIRED (live scores are never NaN: the callers map NaN to -inf when they fill the array).  Thread t owns the positions
// c = t mod 256 and touches no others: it keeps the best of them, every round is a workgroup-wide arg-max of those, and the winner's owner
// retires it and rescans its positions.  Thread 0 hands each round's (r, live, value, position) to emit; live = false once nothing is
// left (position = the 0x7fffffff sentinel), which is every round from r = the number of live slots on.
// the best live slot among the positions thread `tid` owns (ascending c: the first maximum is the lowest position); selects, not
// branches: the owner's rescan is the serial part of every round
__device__ __forceinline__ void topk_scan_owned(const float* val, int n_c, int tid, float& best, int& besti) {
  best = -INFINITY;
  besti = 0x7fffffff;
  for (int c = tid; c < n_c; c += 256) {
    const float v = val[c];
    const bool take = (v == v) & ((besti == 0x7fffffff) | (v > best));
    best = take ? v : best;
    besti = take ? c : besti;
  }
}
template <class Emit>
__device__ __forceinline__ void topk_rounds(float* val, int n_c, int k, float* redv, int* redi, Emit&& emit) {
  const int tid = threadIdx.x;
  float best;
  int besti;
  topk_scan_owned(val, n_c, tid, best, besti);
  for (int r = 0; r < k; ++r) {
    float bv = best;
    int bi = besti;
    block_argmax(bv, bi, redv, redi);
    const bool live = bi != 0x7fffffff;
    if (tid == 0) emit(r, live, bv, bi);
    if (live && (bi & 255) == tid) {
      val[bi] = __builtin_nanf("");
      topk_scan_owned(val, n_c, tid, best, besti);
    }
    __syncthreads();
  }
}
