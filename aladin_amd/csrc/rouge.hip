// ROUGE-L relevance of query captions against images (aladin_rouge_l): Rouge.score of reference alad/evaluate_utils/rouge.py:46-76
// for every (query caption, image) pair, as alad/evaluate_utils/compute_relevance.py fills its float32 matrix -- there one Python
// LCS table per (query, reference caption) on the host, here a bit-parallel LCS (Allison-Dix / Hyyro) per lane.
//   V        a bit vector over the QUERY's positions, m ones at the start of a reference caption; per reference token t with match
//            mask M_t (bit p set where query[p] == t):  u = V & M_t;  V = (V + u) | (V & ~M_t);  lcs = m - popcount(V, m bits).
//            W = 1, 2 or 4 64-bit words, the add's carry ripples across them.  A carry out of bit m - 1 lands above the query and
//            never comes back down (carries only climb), so the m-bit truncation happens once, in the popcount.
//   M_t      token ids are arbitrary int32, so the masks of a query live in an open-addressed LDS hash {id, mask[W]}, built by the
//            workgroup with LDS atomics (the table's layout may differ run to run, what a lookup returns cannot).
//   maxima   P = max lcs / m and R = max lcs_i / l_i, independently, found by integer cross-multiplication (correctly rounded
//            division is monotone), one double division each.
//   score    ((1 + b2) * P) * R / (R + b2 * P) in double with b2 = 1.2 * 1.2, NOT contracted (the pragma below), rounded to float
//            once on the store: the bits of the reference's float32 file.
// A 256-thread workgroup owns QB = 8 / W queries and a slab of images; a lane owns an image, walks its reference captions one
// after another and keeps both maxima of its QB queries in registers; every reference token is loaded once and serves the QB
// queries; consecutive lanes store consecutive floats of an output row.  Every output element is written once.
#include "../../include/aladin_hip.h"

#include "common.hpp"

#pragma clang fp contract(off)

#define ROUGE_MAX_LEN 256
#define ROUGE_EMPTY (-1)

template <int W>
struct rouge_cfg {
  static constexpr int QB = 8 / W;                   // queries per workgroup
  static constexpr int LOG_S = W == 1 ? 8 : 9;       // hash slots per query: 256 for <= 64 distinct tokens, 512 for <= 128 / <= 256
  static constexpr int S = 1 << LOG_S;               // LDS: 24 KB (W = 1), 40 KB (W = 2), 36 KB (W = 4)
};

template <int LOG_S>
__device__ __forceinline__ int rouge_slot(int id) {
  return (int)(((uint32_t)id * 0x9E3779B1u) >> (32 - LOG_S));
}

__device__ __forceinline__ int64_t rouge_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the F-measure of the reference, rouge.py:72-75, in its association
__device__ __forceinline__ double rouge_f(double P, double R) {
  const double b2 = 1.2 * 1.2;
  if (P == 0.0 || R == 0.0) return 0.0;
  const double num = ((1.0 + b2) * P) * R;
  const double den = R + (b2 * P);
  return num / den;
}

template <int W>
__global__ __launch_bounds__(256) void rouge_kernel(const int32_t* __restrict__ q_tok, const int64_t* __restrict__ q_off,
                                                    const int32_t* __restrict__ q_rows, int n_q, int q_max_len,
                                                    const int32_t* __restrict__ g_tok, const int64_t* __restrict__ g_off, int n_g,
                                                    int g_max_len, const int64_t* __restrict__ grp_off, int n_img, int slab,
                                                    float* __restrict__ out, int64_t ld_out, int want_lcs) {
  constexpr int QB = rouge_cfg<W>::QB, S = rouge_cfg<W>::S, LOG_S = rouge_cfg<W>::LOG_S;
  __shared__ int keys[QB][S];
  __shared__ unsigned long long masks[QB][S][W];
  __shared__ int q_len[QB];
  __shared__ int64_t q_beg[QB];
  const int tid = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * QB;

  for (int i = tid; i < QB * S; i += 256) (&keys[0][0])[i] = ROUGE_EMPTY;
  for (int i = tid; i < QB * S * W; i += 256) (&masks[0][0][0])[i] = 0ull;
  if (tid < QB) {
    int m = 0;
    int64_t b = 0;
    if (q0 + tid < n_q) {
      const int64_t total = q_off[n_q];
      b = rouge_clamp(q_off[q0 + tid], 0, total);
      const int64_t e = rouge_clamp(q_off[q0 + tid + 1], b, total);
      m = (int)(e - b < (int64_t)q_max_len ? e - b : (int64_t)q_max_len);
    }
    q_len[tid] = m;
    q_beg[tid] = b;
  }
  __syncthreads();
  // the hash of each query: position p of query qi claims (or finds) the slot of its id and sets bit p of the slot's mask
  for (int i = tid; i < QB * 64 * W; i += 256) {
    const int qi = i / (64 * W), p = i % (64 * W);
    if (p < q_len[qi]) {
      const int id = q_tok[q_beg[qi] + p];
      int h = rouge_slot<LOG_S>(id);
      for (;;) {                                     // at most 64 * W <= S / 2 ids per table: a free slot is always found
        const int prev = atomicCAS(&keys[qi][h], ROUGE_EMPTY, id);
        if (prev == ROUGE_EMPTY || prev == id) break;
        h = (h + 1) & (S - 1);
      }
      atomicOr(&masks[qi][h][p >> 6], 1ull << (p & 63));
    }
  }
  __syncthreads();

  int m_q[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) m_q[q] = q_len[q];
  const int64_t g_total = g_off[n_g];
  const int64_t img_lo = (int64_t)blockIdx.y * slab;
  const int64_t img_hi = img_lo + slab < (int64_t)n_img ? img_lo + slab : (int64_t)n_img;
  for (int64_t img = img_lo + tid; img < img_hi; img += 256) {
    const int64_t c0 = rouge_clamp(grp_off[img], 0, n_g), c1 = rouge_clamp(grp_off[img + 1], c0, n_g);
    int best[QB], rn[QB], rd[QB];                    // max lcs; the largest lcs / l as a fraction
#pragma unroll
    for (int q = 0; q < QB; ++q) best[q] = 0, rn[q] = 0, rd[q] = 1;
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t b = rouge_clamp(g_off[c], 0, g_total), e = rouge_clamp(g_off[c + 1], b, g_total);
      const int l = (int)(e - b < (int64_t)g_max_len ? e - b : (int64_t)g_max_len);
      if (l < 1) continue;                           // an empty reference holds no token (the tokenizer never makes one)
      unsigned long long V[QB][W];
#pragma unroll
      for (int q = 0; q < QB; ++q)
#pragma unroll
        for (int w = 0; w < W; ++w) V[q][w] = ~0ull;
      const int32_t* tok = g_tok + b;
      for (int j = 0; j < l; ++j) {
        const int t = tok[j];
        const int h0 = rouge_slot<LOG_S>(t);
#pragma unroll
        for (int q = 0; q < QB; ++q) {
          int h = h0;
          int k = keys[q][h];
          while (k != t && k != ROUGE_EMPTY) {       // an empty slot's mask is 0: a miss changes nothing
            h = (h + 1) & (S - 1);
            k = keys[q][h];
          }
          unsigned long long carry = 0;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            const unsigned long long M = masks[q][h][w], v = V[q][w];
            const unsigned long long s1 = v + (v & M);
            const unsigned long long s2 = s1 + carry;
            carry = (unsigned long long)(s1 < v) | (unsigned long long)(s2 < s1);
            V[q][w] = s2 | (v & ~M);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < QB; ++q) {
        int ones = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const int bits = m_q[q] - 64 * w;
          const unsigned long long keep = bits >= 64 ? ~0ull : (bits <= 0 ? 0ull : (1ull << bits) - 1ull);
          ones += __popcll(V[q][w] & keep);
        }
        const int lcs = m_q[q] - ones;
        best[q] = lcs > best[q] ? lcs : best[q];
        if (lcs * rd[q] > rn[q] * l) rn[q] = lcs, rd[q] = l;           // <= 256 * 256: no overflow
      }
    }
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      if (q0 + q >= n_q) continue;
      double v = 0.0;
      if (want_lcs)
        v = (double)best[q];
      else if (m_q[q] > 0)
        v = rouge_f((double)best[q] / (double)m_q[q], (double)rn[q] / (double)rd[q]);
      const int64_t row = q_rows ? (int64_t)q_rows[q0 + q] : q0 + q;
      out[row * ld_out + img] = (float)v;
    }
  }
}

template <int W>
static int rouge_launch(const int32_t* q_tok, const int64_t* q_off, const int32_t* q_rows, int n_q, int q_max_len, const int32_t* g_tok,
                        const int64_t* g_off, int n_g, int g_max_len, const int64_t* grp_off, int n_img, float* out, int64_t ld_out,
                        int flags, hipStream_t st) {
  // images per workgroup: 4 per lane where that still leaves thousands of workgroups (a query block's hash is built once per
  // workgroup), more only to keep the grid's y extent legal
  int64_t slab = n_img >= 4096 ? 1024 : 256;
  while (((int64_t)n_img + slab - 1) / slab > 65535) slab *= 2;
  const dim3 grid((unsigned)(((int64_t)n_q + rouge_cfg<W>::QB - 1) / rouge_cfg<W>::QB), (unsigned)(((int64_t)n_img + slab - 1) / slab));
  hipLaunchKernelGGL(rouge_kernel<W>, grid, dim3(256), 0, st, q_tok, q_off, q_rows, n_q, q_max_len, g_tok, g_off, n_g, g_max_len, grp_off,
                     n_img, (int)slab, out, ld_out, flags & ALADIN_ROUGE_LCS);
  return aladin_check_launch("rouge_kernel");
}

extern "C" int aladin_rouge_l(const int32_t* q_tok, const int64_t* q_off, const int32_t* q_rows, int n_q, int q_max_len,
                              const int32_t* g_tok, const int64_t* g_off, int n_g, int g_max_len, const int64_t* grp_off, int n_img,
                              float* out, int64_t ld_out, int flags, void* stream) {
  if (!q_tok || !q_off || !g_tok || !g_off || !grp_off || !out || n_q < 1 || n_g < 1 || n_img < 1 || ld_out < n_img ||
      (flags & ~ALADIN_ROUGE_LCS)) {
    aladin_set_error("rouge_l: bad argument (n_q=%d n_g=%d n_img=%d ld_out=%lld flags=%d%s)", n_q, n_g, n_img, (long long)ld_out, flags,
                     (!q_tok || !q_off || !g_tok || !g_off || !grp_off || !out) ? ", NULL pointer" : "");
    return ALADIN_ERR_ARG;
  }
  if (q_max_len < 1 || q_max_len > ROUGE_MAX_LEN || g_max_len < 1 || g_max_len > ROUGE_MAX_LEN) {
    aladin_set_error("rouge_l: captions of 1 to %d tokens are scored (got q_max_len=%d g_max_len=%d)", ROUGE_MAX_LEN, q_max_len,
                     g_max_len);
    return ALADIN_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  if (q_max_len <= 64)
    return rouge_launch<1>(q_tok, q_off, q_rows, n_q, q_max_len, g_tok, g_off, n_g, g_max_len, grp_off, n_img, out, ld_out, flags, st);
  if (q_max_len <= 128)
    return rouge_launch<2>(q_tok, q_off, q_rows, n_q, q_max_len, g_tok, g_off, n_g, g_max_len, grp_off, n_img, out, ld_out, flags, st);
  return rouge_launch<4>(q_tok, q_off, q_rows, n_q, q_max_len, g_tok, g_off, n_g, g_max_len, grp_off, n_img, out, ld_out, flags, st);
}
