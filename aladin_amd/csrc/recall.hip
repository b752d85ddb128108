// Matching-head retrieval at evaluation scale, the stored-matrix path: sim = img @ cap.T (aladin_sim_matrix), COCO-protocol ranks
// (aladin_recall_ranks) and top-k lists (aladin_topk) from it.
// Replaces ims.mm(caps.t()) + numpy argsort/where, reference alad/recall_auxiliary.py:30-56 and
// alad/evaluation.py:196,213-223,285,303-308.  The split-fp16 chain behind every score is described in sim_common.hpp, the operand
// preparation is sim_pack.hip's; retrieval.hip computes the same ranks without storing the matrix.
#include "../../include/aladin_hip.h"

#include "sim_common.hpp"

// ------------------------------------------------------------------------------------------------
// sim_gemm_store_kernel: the stored score matrix (aladin_sim_matrix), full chain.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void sim_gemm_store_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b,
                                                             const float* __restrict__ scale, float* __restrict__ sim,
                                                             int64_t ld, int n_img, int n_cap, int64_t ldk, int kps,
                                                             int n_nblk, int n_blocks) {
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
  gemm_mainloop16_tall<Cfg, true, KMapSplit>(a + (int64_t)mb * Cfg::BM * ldk, b + (int64_t)nb * Cfg::BN * ldk, ldk, 3 * kps, smem, acc,
                                             KMapSplit{kps, 0});
  const float unscale = 1.0f / (scale[0] * scale[1]);   // exact: powers of two
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave / Cfg::WGN, wn = wave % Cfg::WGN;
  // 16x16 C tile: col = lane & 15, row = 4 * (lane >> 4) + reg
  const int row0 = mb * Cfg::BM + wm * (RT * 16) + 4 * (lane >> 4);
  const int col0 = nb * Cfg::BN + wn * (CT * 16) + (lane & 15);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = row0 + rt * 16 + reg;
      if (row >= n_img) continue;
      float* out = sim + (int64_t)row * ld;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int col = col0 + ct * 16;
        if (col < n_cap) out[col] = acc[rt][ct][reg] * unscale;
      }
    }
}

extern "C" int aladin_sim_matrix(const float* img, int64_t img_rs, const float* cap, int64_t cap_rs, int n_img, int n_cap,
                                 int D, float* sim, int64_t ld_sim, void* workspace, void* stream) {
  if (!img || !cap || !sim || !workspace || n_img < 1 || n_cap < 1 || D < 1 || ld_sim < n_cap || img_rs < D || cap_rs < D) {
    aladin_set_error("sim_matrix: bad argument (n_img=%d n_cap=%d D=%d)", n_img, n_cap, D);
    return ALADIN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  SimPacked p;
  int rc = sim_prepare(SimIn{img, img_rs, cap, cap_rs, n_img, n_cap, D}, workspace, st, &p, nullptr);
  if (rc) return rc;
  const SimWs& ws = p.ws;
  const int Mp = p.Mp, Np = p.Np, Dp = p.Dp;
  static unsigned long long lds_reserved = 0;
  if ((rc = aladin_reserve_lds((const void*)sim_gemm_store_kernel, SimCfg::LDS_BYTES, &lds_reserved, "sim_gemm_store"))) return rc;
  const int n_mblk = Mp / SimCfg::BM, n_nblk = Np / SimCfg::BN;
  hipLaunchKernelGGL(sim_gemm_store_kernel, dim3(n_mblk * n_nblk), dim3(SimCfg::THREADS), SimCfg::LDS_BYTES, st, ws.a, ws.b,
                     ws.scale, sim, ld_sim, n_img, n_cap, (int64_t)2 * Dp, Dp / 64, n_nblk, n_mblk * n_nblk);
  return aladin_check_launch("sim_gemm_store_kernel");
}

// ------------------------------------------------------------------------------------------------
// ranks.  rank = number of strictly larger scores (argsort position unless scores tie exactly).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_i2t_kernel(const float* __restrict__ sim, int64_t ld, int n_cap, int cpi,
                                                       int32_t* __restrict__ rank, int32_t* __restrict__ top1) {
  __shared__ int red[4];
  __shared__ float redv[4];
  __shared__ int redi[4];
  const int i = blockIdx.x;
  const float* row = sim + (int64_t)i * ld;
  // best of the image's captions (recall_auxiliary.py:38-44): #(v > t) never grows with t, so the minimum
  // over the cpi ground truths is the count against the largest of them
  float gt = -INFINITY;
  for (int g = 0; g < cpi; ++g) gt = fmaxf(gt, row[(int64_t)i * cpi + g]);
  int cnt = 0;
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int c = threadIdx.x; c < n_cap; c += blockDim.x) {
    const float v = row[c];
    cnt += (v > gt);
    if (v > best) { best = v; besti = c; }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  cnt = row16_isum(cnt);
  cnt += lane_xor16(cnt);
  cnt += lane_xor32(cnt);
  if (lane == 0) red[wave] = cnt;
  block_argmax(best, besti, redv, redi);                 // its barrier publishes red[] too
  if (threadIdx.x == 0) {
    rank[i] = red[0] + red[1] + red[2] + red[3];
    top1[i] = besti;
  }
}

// columns: thread per caption, rows split over blockIdx.y; integer atomics (order independent)
__global__ __launch_bounds__(256) void rank_t2i_kernel(const float* __restrict__ sim, int64_t ld, int n_img, int n_cap,
                                                       int cpi, int rows_per_block, int32_t* __restrict__ rank,
                                                       unsigned long long* __restrict__ best_packed) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cap) return;
  const float gt = sim[(int64_t)(c / cpi) * ld + c];
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = (r0 + rows_per_block < n_img) ? r0 + rows_per_block : n_img;
  int cnt = 0;
  float best = -INFINITY;
  int besti = 0;
  for (int i = r0; i < r1; ++i) {
    const float v = sim[(int64_t)i * ld + c];
    cnt += (v > gt);
    if (v > best) { best = v; besti = i; }
  }
  if (r1 > r0) {
    atomicAdd(&rank[c], cnt);
    atomicMax(&best_packed[c], pack_best(best, besti));
  }
}

__global__ __launch_bounds__(256) void unpack_top1_kernel(const unsigned long long* __restrict__ p0, int n0, int32_t* __restrict__ top0,
                                                          const unsigned long long* __restrict__ p1, int n1, int32_t* __restrict__ top1) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n0) top0[t] = best_index(p0[t]);
  if (t < n1) top1[t] = best_index(p1[t]);
}
int sim_unpack_top1_launch(const unsigned long long* p0, int n0, int32_t* top0, const unsigned long long* p1, int n1, int32_t* top1, hipStream_t st) {
  hipLaunchKernelGGL(unpack_top1_kernel, dim3(cdiv(n0 > n1 ? n0 : n1, 256)), dim3(256), 0, st, p0, n0, top0, p1, n1, top1);
  return aladin_check_launch("unpack_top1_kernel");
}

extern "C" size_t aladin_recall_workspace_bytes(int n_cap) { return n_cap > 0 ? (size_t)n_cap * 8 : 0; }

extern "C" int aladin_recall_ranks(const float* sim, int64_t ld_sim, int n_img, int n_cap, int caps_per_img,
                                   int32_t* rank_i2t, int32_t* top1_i2t, int32_t* rank_t2i, int32_t* top1_t2i,
                                   void* workspace, void* stream) {
  if (!sim || !rank_i2t || !top1_i2t || !rank_t2i || !top1_t2i || !workspace) { aladin_set_error("recall_ranks: null argument"); return ALADIN_ERR_ARG; }
  if (n_img < 1 || caps_per_img < 1 || n_cap != n_img * caps_per_img || ld_sim < n_cap) {
    aladin_set_error("recall_ranks: need n_cap == n_img * caps_per_img (n_img=%d n_cap=%d cpi=%d)", n_img, n_cap, caps_per_img);
    return ALADIN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rank_i2t_kernel, dim3(n_img), dim3(256), 0, st, sim, ld_sim, n_cap, caps_per_img, rank_i2t, top1_i2t);
  int rc = aladin_check_launch("rank_i2t_kernel");
  if (rc) return rc;
  unsigned long long* packed = (unsigned long long*)workspace;
  if (hipMemsetAsync(packed, 0, (size_t)n_cap * 8, st) != hipSuccess || hipMemsetAsync(rank_t2i, 0, (size_t)n_cap * 4, st) != hipSuccess) {
    aladin_set_error("recall_ranks: hipMemsetAsync failed");
    return ALADIN_ERR_HIP;
  }
  const int ysplit = n_img >= 2048 ? 16 : (n_img >= 256 ? 4 : 1);
  const int rpb = cdiv(n_img, ysplit);
  hipLaunchKernelGGL(rank_t2i_kernel, dim3(cdiv(n_cap, 256), ysplit), dim3(256), 0, st, sim, ld_sim, n_img, n_cap,
                     caps_per_img, rpb, rank_t2i, packed);
  if ((rc = aladin_check_launch("rank_t2i_kernel"))) return rc;
  return sim_unpack_top1_launch(packed, n_cap, top1_t2i, nullptr, 0, nullptr, st);
}

// ------------------------------------------------------------------------------------------------
// Top-k lists (the `top50` table of t2i, reference alad/evaluation.py:262,309: inds[i][0:50] of the
// descending argsort of every query's score row).  One workgroup per query: its n_c scores are staged in
// LDS, and topk_rounds (sim_common.hpp) selects: every thread keeps the best of the elements it owns, and k
// rounds of a workgroup-wide arg-max (larger score first, lower index on ties) each retire one element.  Reads are strided
// (M[q * q_stride + c * c_stride]) so that the columns of a row-major (n_img x n_cap) matrix serve as
// queries without a transpose; workgroup ids are XCD-compact, so the queries that share cache lines of
// such a column sweep run on the same L2.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ M, int64_t q_stride, int64_t c_stride, int n_q,
                                                   int n_c, int k, int32_t* __restrict__ out_idx, float* __restrict__ out_val) {
  extern __shared__ __attribute__((aligned(16))) char topk_smem[];
  float* val = reinterpret_cast<float*>(topk_smem);
  __shared__ float redv[4];
  __shared__ int redi[4];
  const int q = xcd_remap(blockIdx.x, n_q);
  const float* row = M + (int64_t)q * q_stride;
  for (int c = threadIdx.x; c < n_c; c += 256) {         // the positions this thread owns in topk_rounds: no barrier needed
    const float v = row[(int64_t)c * c_stride];
    val[c] = (v == v) ? v : -INFINITY;                   // NaN sorts last
  }
  topk_rounds(val, n_c, k, redv, redi, [&](int r, bool live, float v, int pos) {
    out_idx[(int64_t)q * k + r] = live ? pos : -1;
    if (out_val) out_val[(int64_t)q * k + r] = live ? v : -INFINITY;
  });
}

int sim_topk_launch(const float* M, int64_t q_stride, int64_t c_stride, int n_q, int n_c, int k, int32_t* out_idx, float* out_val,
                    hipStream_t st) {
  const int lds = n_c * 4;
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)topk_kernel, TOPK_MAX_CAND * 4, &lds_reserved, "topk")) return rc;
  hipLaunchKernelGGL(topk_kernel, dim3(n_q), dim3(256), lds, st, M, q_stride, c_stride, n_q, n_c, k, out_idx, out_val);
  return aladin_check_launch("topk_kernel");
}

extern "C" int aladin_topk(const float* M, int64_t q_stride, int64_t c_stride, int n_q, int n_c, int k, int32_t* out_idx,
                           float* out_val, void* stream) {
  if (!M || !out_idx || n_q < 1 || n_c < 1 || k < 1) { aladin_set_error("topk: bad argument (n_q=%d n_c=%d k=%d)", n_q, n_c, k); return ALADIN_ERR_ARG; }
  if (n_c > TOPK_MAX_CAND) { aladin_set_error("topk: at most %d candidates per query (got %d)", TOPK_MAX_CAND, n_c); return ALADIN_ERR_UNSUPPORTED; }
  return sim_topk_launch(M, q_stride, c_stride, n_q, n_c, k, out_idx, out_val, (hipStream_t)stream);
}
