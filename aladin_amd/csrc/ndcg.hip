// nDCG of ranked lists against a relevance matrix (aladin_ndcg): per query the discounted cumulative gain of the listed gallery
// positions, the ideal DCG of its relevance row, and their ratio.  Replaces dcg_from_ranking / ndcg_from_ranking of reference
// alad/evaluate_utils/dcg.py:169-216 -- one numpy.argsort of the whole relevance row per query and method, on the host -- with one
// workgroup per query whose selection rounds are those of aladin_topk (topk_rounds, sim_common.hpp).
//   gain      exp2f(rel) - 1.0f in float32 (numpy's 2 ** rel - 1 on the float32 memmap stays float32)
//   discount  log2(r + 2) in double
//   sums      in double, in ascending r, every term added by the same instruction sequence in both kernels and for both sums
//             (wave_dcg_chunk): a ranking that lists the k largest relevances in descending order gives ndcg == 1.0 exactly, and
//             the IDEAL_GIVEN path gives the fused path's bits.
// NaN relevances are staged as -inf (as topk_kernel does); what they do to the result is unspecified.
#include "../../include/aladin_hip.h"

#include "sim_common.hpp"

__device__ __forceinline__ double ndcg_term(float rel, int r) {
  const float gain = exp2f(rel) - 1.0f;
  return (double)gain / log2((double)(r + 2));
}

// acc + the terms of positions [base, base + n), n <= 64, in ascending order; called by all 64 lanes of ONE wave, every lane returns
// the sum.  rel_at(r, v): the relevance at position r, false = no item there (adds nothing, the position keeps its discount).
template <class RelAt>
__device__ __forceinline__ double wave_dcg_chunk(double acc, int base, int n, RelAt&& rel_at) {
  const int lane = threadIdx.x & 63;
  double t = 0.0;
  if (lane < n) {
    float v;
    if (rel_at(base + lane, v)) t = ndcg_term(v, base + lane);
  }
  for (int j = 0; j < n; ++j) acc += __shfl(t, j);
  return acc;
}

// ------------------------------------------------------------------------------------------------
// ndcg_kernel: one workgroup per query.  The relevance row is staged in LDS with topk_kernel's strided read (the columns of a
// row-major matrix serve as queries without a transpose; XCD-compact ids keep the queries that share the cache lines of such a
// column sweep on one L2, recall.hip).  Wave 0 gathers the listed positions from LDS before the first round retires anything (the
// first retire follows a workgroup barrier that wave 0 has to reach); the ideal is k rounds of topk_rounds, 64 at a time, whose emit
// keeps the value -- the index is not needed and ties cannot matter.  Thread 0 writes the three doubles, each once.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ndcg_kernel(const float* __restrict__ rel, int64_t q_stride, int64_t c_stride, int n_q, int n_c,
                                                   const int32_t* __restrict__ ranking, int64_t ld_rank, int k,
                                                   double* __restrict__ ndcg, double* __restrict__ dcg, double* __restrict__ ideal) {
  extern __shared__ __attribute__((aligned(16))) char ndcg_smem[];
  float* val = reinterpret_cast<float*>(ndcg_smem);
  __shared__ float redv[4];
  __shared__ int redi[4];
  __shared__ float topv[64];
  const int q = xcd_remap(blockIdx.x, n_q);
  const float* row = rel + (int64_t)q * q_stride;
  for (int c = threadIdx.x; c < n_c; c += 256) {
    const float v = row[(int64_t)c * c_stride];
    val[c] = (v == v) ? v : -INFINITY;
  }
  __syncthreads();
  const bool wave0 = threadIdx.x < 64;
  double dsum = 0.0, isum = 0.0;
  if (wave0) {
    const int32_t* list = ranking + (int64_t)q * ld_rank;
    for (int base = 0; base < k; base += 64)
      dsum = wave_dcg_chunk(dsum, base, k - base < 64 ? k - base : 64, [&](int r, float& v) {
        const int idx = list[r];
        if ((unsigned)idx >= (unsigned)n_c) return false;
        v = val[idx];
        return true;
      });
  }
  for (int base = 0; base < k; base += 64) {
    const int n = k - base < 64 ? k - base : 64;
    topk_rounds(val, n_c, n, redv, redi, [&](int r, bool live, float v, int) { topv[r] = live ? v : __builtin_nanf(""); });
    if (wave0)                                           // the last round's barrier published topv; thread 0 refills it only after this
      isum = wave_dcg_chunk(isum, base, n, [&](int r, float& v) {
        v = topv[r - base];
        return v == v;
      });
  }
  if (threadIdx.x == 0) {
    ndcg[q] = isum == 0.0 ? 0.0 : dsum / isum;
    if (dcg) dcg[q] = dsum;
    if (ideal) ideal[q] = isum;
  }
}

// ------------------------------------------------------------------------------------------------
// ndcg_given_kernel (ALADIN_NDCG_IDEAL_GIVEN): the ideal DCG is the caller's, so nothing is staged or selected -- one wave per query,
// four queries per workgroup, the listed relevances read straight from global memory.  No barrier: a wave past n_q just leaves.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ndcg_given_kernel(const float* __restrict__ rel, int64_t q_stride, int64_t c_stride, int n_q,
                                                         int n_c, const int32_t* __restrict__ ranking, int64_t ld_rank, int k,
                                                         const double* __restrict__ ideal, double* __restrict__ ndcg,
                                                         double* __restrict__ dcg) {
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_q) return;
  const float* row = rel + q * q_stride;
  const int32_t* list = ranking + q * ld_rank;
  double dsum = 0.0;
  for (int base = 0; base < k; base += 64)
    dsum = wave_dcg_chunk(dsum, base, k - base < 64 ? k - base : 64, [&](int r, float& v) {
      const int idx = list[r];
      if ((unsigned)idx >= (unsigned)n_c) return false;
      const float x = row[(int64_t)idx * c_stride];
      v = (x == x) ? x : -INFINITY;
      return true;
    });
  if ((threadIdx.x & 63) == 0) {
    const double best = ideal[q];
    ndcg[q] = best == 0.0 ? 0.0 : dsum / best;
    if (dcg) dcg[q] = dsum;
  }
}

extern "C" int aladin_ndcg(const float* rel, int64_t q_stride, int64_t c_stride, int n_q, int n_c, const int32_t* ranking,
                           int64_t ld_rank, int rank, int flags, double* ndcg, double* dcg, double* ideal, void* stream) {
  const bool given = flags & ALADIN_NDCG_IDEAL_GIVEN;
  if (!rel || !ranking || !ndcg || n_q < 1 || n_c < 1 || rank < 1 || ld_rank < rank || (given && !ideal)) {
    aladin_set_error("ndcg: bad argument (n_q=%d n_c=%d rank=%d ld_rank=%lld%s)", n_q, n_c, rank, (long long)ld_rank,
                     given && !ideal ? ", IDEAL_GIVEN without ideal" : "");
    return ALADIN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const int k = rank < n_c ? rank : n_c;
  if (given) {
    hipLaunchKernelGGL(ndcg_given_kernel, dim3(cdiv(n_q, 4)), dim3(256), 0, st, rel, q_stride, c_stride, n_q, n_c, ranking, ld_rank, k,
                       ideal, ndcg, dcg);
    return aladin_check_launch("ndcg_given_kernel");
  }
  if (n_c > TOPK_MAX_CAND) {
    aladin_set_error("ndcg: the ideal DCG is selected among at most %d relevances per query (got %d); pass it with IDEAL_GIVEN",
                     TOPK_MAX_CAND, n_c);
    return ALADIN_ERR_UNSUPPORTED;
  }
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)ndcg_kernel, TOPK_MAX_CAND * 4, &lds_reserved, "ndcg")) return rc;
  hipLaunchKernelGGL(ndcg_kernel, dim3(n_q), dim3(256), n_c * 4, st, rel, q_stride, c_stride, n_q, n_c, ranking, ld_rank, k, ndcg, dcg,
                     ideal);
  return aladin_check_launch("ndcg_kernel");
}
