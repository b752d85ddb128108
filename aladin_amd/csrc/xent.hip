// The symmetric cross-entropy (InfoNCE) criterion on a B x B score matrix with a learnable temperature, reference
// alad/loss.py:190-201 (CrossEntropyCriterion).  With t = *log_temperature (a DEVICE scalar) and L = S * e^t:
//   loss = 1/(2B) [ sum_i (LSE_j L_ij - L_ii) + sum_j (LSE_i L_ij - L_jj) ]
//   dS   = e^t (P^r + P^c - 2 I) / (2B),   P^r = softmax_j L,  P^c = softmax_i L
//   dt   = 1/(2B) [ sum_i sum_j P^r_ij (L_ij - L_ii) + sum_j sum_i P^c_ij (L_ij - L_jj) ]       (= sum_ij dL_ij L_ij, separated)
// Two launches on the caller's stream:
//   xent_stats_kernel   per line (row i, or column j) ONE pass keeping (m, s, u) = (max, sum e^(x - m), sum e^(x - m) (x - m))
//                       of x = L over the line; partial triples meet by the log-sum-exp merge rule (lse_merge).  u carries the
//                       line's share of dt shifted by the maximum: sum_j P_ij (L_ij - L_ii) = u / s + (m - L_ii), which does not
//                       cancel where the softmax is one-hot (m == L_ii exactly, u / s tiny and relatively accurate) nor where L is
//                       of order 5000.  The pass runs over the line's OFF-DIAGONAL elements and the diagonal one joins last, so
//                       that the line's diagonal part of the gradient, P_dd - 1, is known as -(off-diagonal mass) / s: formed as
//                       e^(x - m) / s - 1 it is 0 as soon as the mass is below 2^-25, while the off-diagonal entries it balances
//                       are still exact -- the whole gradient of a well-trained batch.
//                       The lines are walked by line_walk (line_walk.hpp) with Lse as its accumulator: a wave per row, strips of
//                       64 columns under 16 waves; this file supplies the element (the logit, off the diagonal) and the store.
//                       line[b] = {m, s, P_dd - 1, 0} and piece[b] = {LSE - L_dd, the line's share of dt}, rows then columns.
//   xent_finish_kernel  block (0, 0) sums the lines' shares of loss and dt in a fixed order; every block writes dS for its
//                       256 columns (column statistics in registers) over the rows dealt to it.
// Nothing is accumulated with atomics and every sum runs in a fixed order: the same input gives the same bits.  A NaN score
// makes its row's and column's s NaN (fmaxf drops it from m, e^(NaN) keeps it in s) and with them the loss.
#include <float.h>
#include "../../include/aladin_hip.h"
#include "common.hpp"
#include "line_walk.hpp"

// No contraction: lse_merge must give both partners of a butterfly step the same bits (a * b + c * d contracted is not symmetric).
#pragma clang fp contract(off)

#define XENT_MAX_B ALADIN_XENT_MAX_B

// (m, s, u) of an empty set: m is the most negative FINITE float, so that m - M, 0 * (m - M) and e^(m - M) stay finite / zero
// without a guard (an infinite m would give inf - inf and 0 * inf)
struct Lse {
  float m, s, u;
  __device__ __forceinline__ void clear() { m = -FLT_MAX; s = 0.f; u = 0.f; }
  // one more element x
  __device__ __forceinline__ void add(float x) {
    const float dx = x - m;                      // a NaN x: the comparison below fails, t is NaN and the else branch puts it into s
    const float t = expf(-fabsf(dx));
    if (x > m) { u = t * (u - s * dx); s = s * t + 1.f; m = x; }      // a new maximum: the old terms shift by m - x = -dx
    else { u = u + t * dx; s = s + t; }
  }
  static constexpr int FIELDS = 3;                           // from here: what line_walk asks of an accumulator
  __device__ __forceinline__ void put(float* p) const { p[0] = m; p[64] = s; p[128] = u; }
  __device__ __forceinline__ void get(const float* p) { m = p[0]; s = p[64]; u = p[128]; }
  __device__ __forceinline__ void merge(const Lse& o);       // lse_merge
  __device__ __forceinline__ void wave_reduce();             // wave_lse
};

// the union of two sets; symmetric in its arguments bit for bit
__device__ __forceinline__ Lse lse_merge(const Lse& a, const Lse& b) {
  Lse r;
  r.m = fmaxf(a.m, b.m);
  const float da = a.m - r.m, db = b.m - r.m;
  const float ea = expf(da), eb = expf(db);
  const float sa = a.s * ea, sb = b.s * eb;
  r.s = sa + sb;
  r.u = (a.u * ea + sa * da) + (b.u * eb + sb * db);
  // a NaN s (a NaN element) survives: NaN * e is NaN whatever e
  return r;
}

#define XENT_LANE_STEP(EXPR_M, EXPR_S, EXPR_U) do { Lse o_; o_.m = (EXPR_M); o_.s = (EXPR_S); o_.u = (EXPR_U); v = lse_merge(v, o_); } while (0)
// over the 64 lanes of a wave, in every lane (the butterfly of wave_sum: xor 32, 16, then rotations inside a row of 16)
__device__ __forceinline__ Lse wave_lse(Lse v) {
  XENT_LANE_STEP(lane_xor32(v.m), lane_xor32(v.s), lane_xor32(v.u));
  XENT_LANE_STEP(lane_xor16(v.m), lane_xor16(v.s), lane_xor16(v.u));
  XENT_LANE_STEP(ALADIN_ROW_ROR(v.m, 8), ALADIN_ROW_ROR(v.s, 8), ALADIN_ROW_ROR(v.u, 8));
  XENT_LANE_STEP(ALADIN_ROW_ROR(v.m, 4), ALADIN_ROW_ROR(v.s, 4), ALADIN_ROW_ROR(v.u, 4));
  XENT_LANE_STEP(ALADIN_ROW_ROR(v.m, 2), ALADIN_ROW_ROR(v.s, 2), ALADIN_ROW_ROR(v.u, 2));
  XENT_LANE_STEP(ALADIN_ROW_ROR(v.m, 1), ALADIN_ROW_ROR(v.s, 1), ALADIN_ROW_ROR(v.u, 1));
  return v;
}
__device__ __forceinline__ void Lse::merge(const Lse& o) { *this = lse_merge(*this, o); }
__device__ __forceinline__ void Lse::wave_reduce() { *this = wave_lse(*this); }

// v: the line's off-diagonal elements; xd: its diagonal logit.  -> line = {m, s, P_dd - 1, 0}, piece = {LSE - L_dd, sum P (L - L_dd)}
__device__ __forceinline__ void xent_line_store(Lse v, float xd, float4* __restrict__ line, float2* __restrict__ piece) {
  const float m_off = v.m, s_off = v.s;
  v.add(xd);
  const float mass = s_off * expf(m_off - v.m);              // the off-diagonal terms at the line's maximum (0 for B = 1)
  const float off = v.m - xd;
  *line = make_float4(v.m, v.s, -(mass / v.s), 0.f);
  *piece = make_float2(off + logf(v.s), v.u / v.s + off);
}

// workspace: line[2B] (float4) | piece[2B] (float2)
static inline size_t xent_line_bytes(int B) { return (size_t)B * 2 * sizeof(float4); }

__global__ __launch_bounds__(LINE_WALK_THREADS) void xent_stats_kernel(const float* __restrict__ S, int64_t ld, int B,
                                                                       const float* __restrict__ log_t, int row_blocks,
                                                                       float4* __restrict__ line, float2* __restrict__ piece) {
  const float et = expf(*log_t);
  line_walk<Lse>(
      S, ld, B, row_blocks, [&](Lse& v, float s, int i, int j, int) { if (j != i) v.add(s * et); },
      [&](const Lse& v, int b) { const int d = b < B ? b : b - B; xent_line_store(v, S[(int64_t)d * ld + d] * et, line + b, piece + b); });
}

// grid line_finish_grid; dS == NULL: one block, the sums only
__global__ __launch_bounds__(256) void xent_finish_kernel(const float* __restrict__ S, int64_t ld, int B, const float* __restrict__ log_t,
                                                          const float4* __restrict__ line, const float2* __restrict__ piece,
                                                          float* __restrict__ loss, float* __restrict__ dS, float* __restrict__ d_log_t) {
  __shared__ float red[4];
  const float et = expf(*log_t);
  const float inv = 1.f / (2.f * (float)B);
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    float rl = 0.f, cl = 0.f, rt = 0.f, ct = 0.f;            // line_sums of both shares in one pass over piece: rows, then columns
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      const float2 r = piece[b], c = piece[B + b];
      rl += r.x; cl += c.x; rt += r.y; ct += c.y;
    }
    rl = block_sum(rl, red); cl = block_sum(cl, red); rt = block_sum(rt, red); ct = block_sum(ct, red);
    if (threadIdx.x == 0) {
      *loss = (rl + cl) * inv;
      if (d_log_t) *d_log_t = (rt + ct) * inv;
    }
  }
  if (dS == nullptr) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= B) return;
  const float4 c = line[B + j];
  const float k = et * inv;
  for (int i = blockIdx.y; i < B; i += gridDim.y) {
    const float4 r = line[i];                                // block-uniform
    const float x = S[(int64_t)i * ld + j] * et;
    // the diagonal: (P^r_ii - 1) + (P^c_ii - 1), each part on its own and from its line's off-diagonal mass (see the head of
    // this file); P^r + P^c - 2 would round away all there is to the gradient where both softmaxes are one-hot -- the trap
    // listnet_finish_kernel's comment describes
    const float g = i == j ? r.z + c.z : expf(x - r.x) / r.y + expf(x - c.x) / c.y;
    dS[(int64_t)i * B + j] = k * g;
  }
}

extern "C" size_t aladin_xent_workspace_bytes(int B) {
  if (B < 1 || B > XENT_MAX_B) return 0;
  return xent_line_bytes(B) + (size_t)B * 2 * sizeof(float2) + 256;
}

extern "C" int aladin_xent_fwd_bwd(const float* S, int64_t ldS, int B, const float* log_temperature, float* loss, float* dS,
                                   float* d_log_temperature, void* workspace, void* stream) {
  if (!S || !log_temperature || !loss || !workspace || B < 1 || ldS < B || ((uintptr_t)workspace & 15)) {
    aladin_set_error("xent_fwd_bwd: bad argument (B=%d ldS=%lld; S, log_temperature, loss and a 16-byte aligned workspace are required)",
                     B, (long long)ldS);
    return ALADIN_ERR_ARG;
  }
  if (B > XENT_MAX_B) {
    aladin_set_error("xent_fwd_bwd: B = %d, the limit is %d (the score matrix and dS hold B * B floats each)", B, XENT_MAX_B);
    return ALADIN_ERR_UNSUPPORTED;
  }
  float4* line = (float4*)workspace;
  float2* piece = (float2*)((char*)workspace + xent_line_bytes(B));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(xent_stats_kernel, dim3(line_walk_blocks(B)), dim3(LINE_WALK_THREADS), 0, st, S, ldS, B, log_temperature,
                     line_row_blocks(B), line, piece);
  if (int rc = aladin_check_launch("xent_stats_kernel")) return rc;
  hipLaunchKernelGGL(xent_finish_kernel, line_finish_grid(B, dS != nullptr), dim3(256), 0, st, S, ldS, B, log_temperature, line, piece,
                     loss, dS, d_log_temperature);
  return aladin_check_launch("xent_finish_kernel");
}

