// The formulas of the loss heads on the B x B score matrices, once: the VSE++ hinge (alad/loss.py:42-67), ListNet score
// distillation (alad/loss.py:369-370,427-445) and the weighted total (alad_model.py:450-453).  Two paths run them, chosen by
// batch size: losses.hip (any B; a workgroup per line) and small_batch.hip (B <= 64; a wave per line, three launches for the
// whole chain); the merged finish + pair-argmax kernel of align_bwd.hip runs either finish pass.  Each path keeps its own
// reductions and its own way of dealing elements to threads; what an element IS lives here, and so does what a thread keeps of
// the elements it has seen.  Who runs what:
//   hinge_x / hinge_cost / hinge_cost_is_nan   HingeAcc, hinge_vector_stats (small_batch.hip, a lane per element), sem_finish_kernel
//   HingeAcc                                   hinge_stats_kernel (losses.hip, a workgroup per line), sem_stats_kernel (semantic.hip,
//                                              line_walk against relevance-chosen anchors)
//   everything else                            both paths' statistics and finish passes
#pragma once
#include "common.hpp"
#include "line_walk.hpp"

// ---- the small-batch statistics: SB_ST floats per line v in [0, 2B), rows then columns ---------------------------------------
#define SB_MAX 64
#define SB_ST 12
#define SB_ST_MATCH 0                  // hinge on M: value, arg (an int's bit pattern)
#define SB_ST_LISTNET 2                // ListnetLine
#define SB_ST_ALIGN 8                  // hinge on S: value, arg

#define SB_MATCH_HINGE 1               // flags
#define SB_ALIGN_HINGE 2
#define SB_LISTNET 4

// ---- hinge ------------------------------------------------------------------------------------------------------------------
// (value, arg) of line v in [0, 2B): rows, then columns.
//   max_violation: value = max_j cost, arg = argmax          (alad/loss.py:63-65)
//   sum mode     : value = sum_j cost, arg = #(cost > 0)     (alad/loss.py:67)
// A line with a NaN cost has value NaN; its arg is unspecified.
struct HingeStats {
  const float* val; const int* arg; int step;
  __device__ __forceinline__ float value(int v) const { return val[(int64_t)v * step]; }
  __device__ __forceinline__ int index(int v) const { return arg[(int64_t)v * step]; }
};
// losses.hip's workspace: val[2B] | arg[2B]
__host__ __device__ __forceinline__ HingeStats hinge_stats_dense(const void* workspace, int B) {
  const float* val = (const float*)workspace;
  return {val, (const int*)(val + 2 * (size_t)B), 1};
}
// small_batch.hip's workspace: st[v * SB_ST + off], + 1 (off = SB_ST_MATCH or SB_ST_ALIGN)
__host__ __device__ __forceinline__ HingeStats hinge_stats_small(const float* st, int off) {
  return {st + off, (const int*)(st + off + 1), SB_ST};
}

// x of element (line q, position t) = margin + s - diag; its cost is max(x, 0), and 0 on the diagonal (:49 / :52, :55-60)
__device__ __forceinline__ float hinge_x(float margin, float s, float diag) { return margin + s - diag; }
__device__ __forceinline__ float hinge_cost(float x, bool on_diag) { return on_diag ? 0.f : fmaxf(x, 0.f); }
// fmaxf drops a NaN; the reference's clamp / max / sum keep it, so a NaN cost makes the line's statistic NaN
__device__ __forceinline__ bool hinge_cost_is_nan(float x, bool on_diag) { return (x != x) && !on_diag; }

// The running statistics of a line in a thread that sees many of its elements: the best cost with the lowest index on ties, the
// sum, the number of positive costs.  A NaN cost goes as itself into the sum and as (+inf, index -1) into the arg-max, which
// beats a true +inf.  As an accumulator of line_walk (line_walk.hpp) it brings its reductions along.
struct HingeAcc {
  float best, sum; int besti, cnt;
  __device__ __forceinline__ void clear() { best = 0.f; sum = 0.f; besti = 0x7fffffff; cnt = 0; }
  // element t of the line: score s against the line's anchor; `zero`: its cost is cleared (the diagonal, a masked positive)
  __device__ __forceinline__ void add(float margin, float s, float anchor, bool zero, int t) {
    const float x = hinge_x(margin, s, anchor);
    const bool nan = hinge_cost_is_nan(x, zero);
    const float c = nan ? INFINITY : hinge_cost(x, zero);
    const int ti = nan ? -1 : t;
    if (c > best || (c == best && ti < besti)) { best = c; besti = ti; }
    sum += nan ? x : c;
    cnt += (c > 0.f);
  }
  __device__ __forceinline__ void store(int max_violation, float* val, int* arg) const {       // reduced: the line's HingeStats
    if (max_violation) { *val = besti < 0 ? NAN : best; *arg = besti < 0 ? 0 : besti; }
    else { *val = sum; *arg = cnt; }
  }
  static constexpr int FIELDS = 4;
  __device__ __forceinline__ void put(float* p) const { p[0] = best; p[64] = __int_as_float(besti); p[128] = sum; p[192] = __int_as_float(cnt); }
  __device__ __forceinline__ void get(const float* p) { best = p[0]; besti = __float_as_int(p[64]); sum = p[128]; cnt = __float_as_int(p[192]); }
  __device__ __forceinline__ void merge(const HingeAcc& o) {
    float& v = best; int& idx = besti;
    ALADIN_ARGMAX_STEP(o.best, o.besti);
    sum += o.sum; cnt += o.cnt;
  }
  __device__ __forceinline__ void wave_reduce() {
    wave_argmax(best, besti);
    sum = wave_sum(sum);
    cnt = (int)wave_sum((float)cnt);                       // exact: cnt < 2^24
  }
};

// element (i, j) of dloss/dS
__device__ __forceinline__ float hinge_grad_at(const HingeStats& st, const float* S, int64_t ld, int B, int i, int j, float margin,
                                               int max_violation) {
  if (max_violation) {
    if (i == j) return -(float)((st.value(i) > 0.f) + (st.value(B + i) > 0.f));
    return (float)((st.value(i) > 0.f && st.index(i) == j) + (st.value(B + j) > 0.f && st.index(B + j) == i));
  }
  if (i == j) return -(float)(st.index(i) + st.index(B + i));
  const float s = S[(int64_t)i * ld + j];
  return (float)((hinge_x(margin, s, S[(int64_t)i * ld + i]) > 0.f) + (hinge_x(margin, s, S[(int64_t)j * ld + j]) > 0.f));
}

// The pairs of the hardest-negative mode without looking at dS: candidate p in [0, 3B) is one of sample q = p / 3's three --
// (q, q), (q, argmax of row q), (argmax of column q, q) -- and active if its term is, the third unless it is already listed as
// its image's row pair.  INVARIANT: the active pairs are exactly the non-zeros of hinge_grad_at(.., max_violation = 1), each once;
// change the two together.
__device__ __forceinline__ bool hinge_pair_at(const HingeStats& st, int B, int p, int* i, int* j) {
  const int q = p / 3, t = p - 3 * q;
  const float vr = st.value(q), vc = st.value(B + q);
  *i = q; *j = q;
  if (t == 0) return vr > 0.f || vc > 0.f;
  if (t == 1) { *j = st.index(q); return vr > 0.f; }
  if (!(vc > 0.f)) return false;
  *i = st.index(B + q);
  return !(st.value(*i) > 0.f && st.index(*i) == q);
}

// ---- ListNet ----------------------------------------------------------------------------------------------------------------
//   P = softmax(T), Q = softmax(tau * M), loss_term = -sum P log(Q + eps), W = P Q / (Q + eps)
//   dM = (tau / B) [ Q^r Wsum^r - W^r + Q^c Wsum^c - W^c ]           
// the six floats of a line's statistics, in the order both workspaces store them
struct ListnetLine { float t_max, t_sumexp, s_max, s_sumexp, w_sum, loss_term; };
__device__ __forceinline__ ListnetLine listnet_line(const float* p) { return {p[0], p[1], p[2], p[3], p[4], p[5]}; }
__device__ __forceinline__ void listnet_line_store(float* p, const ListnetLine& l) {
  p[0] = l.t_max; p[1] = l.t_sumexp; p[2] = l.s_max; p[3] = l.s_sumexp; p[4] = l.w_sum; p[5] = l.loss_term;
}
struct ListnetElem { float P, Q, W; };
// one element of a line: t = teacher score, m = tau * student score; of `l` the two maxima and sums only
__device__ __forceinline__ ListnetElem listnet_elem(float t, float m, const ListnetLine& l, float eps) {
  const float P = expf(t - l.t_max) / l.t_sumexp, Q = expf(m - l.s_max) / l.s_sumexp;
  return {P, Q, P * Q / (Q + eps)};
}
// the element's share of -loss_term
__device__ __forceinline__ float listnet_plogq(const ListnetElem& e, float eps) { return e.P * logf(e.Q + eps); }
// element of dloss/dM from its row's and its column's lines, k = tau / B
__device__ __forceinline__ float listnet_grad_at(float t, float m, const ListnetLine& r, const ListnetLine& c, float k, float eps) {
  const ListnetElem er = listnet_elem(t, m, r, eps), ec = listnet_elem(t, m, c, eps);
  // the row part and the column part each on its own: summed left to right, a part of size ~1 (P and Q saturated on the same
  // element) rounds the other one away at 2^-25, which is all there is to the gradient where both softmaxes are one-hot
  return k * (fmaf(er.Q, r.w_sum, -er.W) + fmaf(ec.Q, c.w_sum, -ec.W));
}
// rs, cs: the loss terms of the rows and of the columns, each summed; im_cost + s_cost (alad/loss.py:445)
__device__ __forceinline__ float listnet_loss(float rs, float cs, int B) { return cs / (float)B + rs / (float)B; }

// ---- the weighted total (alad_model.py:450-453, in the reference's key order) -------------------------------------------------
// total = 0, then this for each term present: separate multiply and add, as the eager sum rounds.  A zero weight means "computed
// for logging only" (the reference pops the distillation term before distill_epoch, alad_model.py:442-444): the term must not
// reach the total, or 0 * inf / 0 * NaN would poison it.
__device__ __forceinline__ float loss_total_add(float acc, float term, float w) {
  return w != 0.f ? __fadd_rn(acc, __fmul_rn(term, w)) : acc;
}

// ---- the finish pass of losses.hip --------------------------------------------------------------------------------------------
// The loss from the row / column statistics (virtual block 0), dloss/dS element by element and, optionally, the list of its
// non-zero pairs.  `vblock` of `nblocks` virtual workgroups: the rows are dealt to them.
__device__ __forceinline__ void hinge_finish_body(int vblock, int nblocks, const float* __restrict__ S, int64_t ld, int B,
                                                  float margin, int max_violation, const HingeStats st, float* __restrict__ loss,
                                                  float* __restrict__ dS, int* __restrict__ pairs,
                                                  int* __restrict__ pair_count, float* __restrict__ dST = nullptr) {
  __shared__ float red[4];
  if (vblock == 0) {
    const float2 t = line_sums(B, red, [&](int v) { return st.value(v); });
    if (threadIdx.x == 0) *loss = t.x + t.y;
  }
  if (dS == nullptr && pairs == nullptr) return;
  // rows are dealt to blocks, columns to threads: no integer division per element
  const int lane = threadIdx.x & 63;
  for (int i = vblock; i < B; i += nblocks) {
    for (int j0 = 0; j0 < B; j0 += blockDim.x) {
      const int j = j0 + threadIdx.x;
      float g = 0.f;
      if (j < B) {
        g = hinge_grad_at(st, S, ld, B, i, j, margin, max_violation);
        if (dS) dS[(int64_t)i * B + j] = g;
        if (dST) dST[(int64_t)j * B + i] = g;              // transposed copy: the row kernel's caption rows read it coalesced
      }
      if (pairs) {                                        // list of non-zero pairs for the alignment backward
        // ONE atomic per workgroup and 256 columns (the four waves' counts meet in LDS): every workgroup hits the
        // same counter, and a returning atomic per wave (~770 of them at B = 256) serialised there
        __shared__ int wcnt[4];
        __shared__ int wbase;
        const unsigned long long mask = __ballot(g != 0.f);
        const int wv = threadIdx.x >> 6;
        __syncthreads();                                   // previous iteration's readers are done with wcnt / wbase
        if (lane == 0) wcnt[wv] = __popcll(mask);
        __syncthreads();
        if (threadIdx.x == 0) {
          const int tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
          wbase = tot ? atomicAdd(pair_count, tot) : 0;
        }
        __syncthreads();
        if (g != 0.f) {
          int base = wbase;
          for (int q = 0; q < wv; ++q) base += wcnt[q];
          pairs[base + __popcll(mask & ((1ull << lane) - 1))] = i * B + j;
        }
      }
    }
  }
}
struct HingeFin {                      // its arguments, for the merged kernel (hardest-negative mode, no pair list)
  const float* S; int64_t ld; int B; float margin; HingeStats st; float* loss; float* dS; float* dST;
  __device__ __forceinline__ void run(int vblock, int nblocks) const {
    hinge_finish_body(vblock, nblocks, S, ld, B, margin, 1, st, loss, dS, nullptr, nullptr, dST);
  }
};

// ---- the finish pass of small_batch.hip -----------------------------------------------------------------------------------------
// dLoss/dM of the matching hinge and of ListNet, dLoss/dS of the alignment hinge (+ optional pair list), the three loss terms and
// their weighted sum; `vblock` of `nblocks` virtual workgroups: flat elements are dealt to them, the heads selected by flags.
struct SmallFin {
  const float* M; const float* S; int64_t ld_s; int B; float margin; int max_violation; int flags; float tau; float eps;
  float w_match, w_align, w_dist; const float* st; float* terms; float* total; float* dM_hinge; float* dM_listnet; float* dS;
  int* pairs; int* pair_count; float* dST;
  __device__ __forceinline__ void run(int vblock, int nblocks) const;
};
__device__ __forceinline__ void heads_small_finish_body(int vblock, int nblocks, const SmallFin& f) {
  const float* __restrict__ M = f.M; const float* __restrict__ S = f.S; const int64_t ld_s = f.ld_s; const int B = f.B;
  const float margin = f.margin; const int max_violation = f.max_violation, flags = f.flags; const float tau = f.tau, eps = f.eps;
  const float* __restrict__ st = f.st;
  float* __restrict__ terms = f.terms; float* __restrict__ total = f.total; float* __restrict__ dM_hinge = f.dM_hinge;
  float* __restrict__ dM_listnet = f.dM_listnet; float* __restrict__ dS = f.dS; int* __restrict__ pairs = f.pairs;
  int* __restrict__ pair_count = f.pair_count;
  const HingeStats st_match = hinge_stats_small(st, SB_ST_MATCH), st_align = hinge_stats_small(st, SB_ST_ALIGN);
  const int lane = threadIdx.x & 63;
  if (vblock == 0 && threadIdx.x < 64) {                           // the three terms: rows first, then columns
    float hm_r = 0.f, hm_c = 0.f, ha_r = 0.f, ha_c = 0.f, l_r = 0.f, l_c = 0.f;
    if (lane < B) {
      if (flags & SB_MATCH_HINGE) { hm_r = st_match.value(lane); hm_c = st_match.value(B + lane); }
      if (flags & SB_ALIGN_HINGE) { ha_r = st_align.value(lane); ha_c = st_align.value(B + lane); }
      if (flags & SB_LISTNET) {
        l_r = listnet_line(st + (int64_t)lane * SB_ST + SB_ST_LISTNET).loss_term;
        l_c = listnet_line(st + (int64_t)(B + lane) * SB_ST + SB_ST_LISTNET).loss_term;
      }
    }
    hm_r = wave_sum(hm_r); hm_c = wave_sum(hm_c); ha_r = wave_sum(ha_r); ha_c = wave_sum(ha_c);
    l_r = wave_sum(l_r); l_c = wave_sum(l_c);
    if (lane == 0) {
      const float t_m = hm_r + hm_c, t_a = ha_r + ha_c, t_d = listnet_loss(l_r, l_c, B);
      terms[0] = t_m; terms[1] = t_a; terms[2] = t_d;
      if (total) {
        float acc = 0.f;
        if (flags & SB_MATCH_HINGE) acc = loss_total_add(acc, t_m, f.w_match);
        if (flags & SB_ALIGN_HINGE) acc = loss_total_add(acc, t_a, f.w_align);
        if (flags & SB_LISTNET) acc = loss_total_add(acc, t_d, f.w_dist);
        *total = acc;
      }
    }
  }
  const float kk = tau / (float)B;
  for (int e0 = vblock * blockDim.x; e0 < B * B; e0 += nblocks * blockDim.x) {
    const int e = e0 + threadIdx.x;
    const bool in = e < B * B;
    const int i = in ? e / B : 0, j = in ? e % B : 0;
    if (in && (flags & SB_MATCH_HINGE) && dM_hinge) dM_hinge[e] = hinge_grad_at(st_match, M, B, B, i, j, margin, max_violation);
    if (in && (flags & SB_LISTNET) && dM_listnet)
      dM_listnet[e] = listnet_grad_at(S[(int64_t)i * ld_s + j], tau * M[e], listnet_line(st + (int64_t)i * SB_ST + SB_ST_LISTNET),
                                      listnet_line(st + (int64_t)(B + j) * SB_ST + SB_ST_LISTNET), kk, eps);
    if ((flags & SB_ALIGN_HINGE) && (dS || pairs)) {
      const float g = in ? hinge_grad_at(st_align, S, ld_s, B, i, j, margin, max_violation) : 0.f;
      if (in && dS) dS[e] = g;
      if (in && f.dST) f.dST[(int64_t)j * B + i] = g;
      if (pairs) {                                                    // the non-zero pairs, for the alignment backward
        const unsigned long long mask = __ballot(g != 0.f);
        if (mask) {
          int base = 0;
          if (lane == 0) base = atomicAdd(pair_count, __popcll(mask));
          base = __shfl(base, 0, 64);
          if (g != 0.f) pairs[base + __popcll(mask & ((1ull << lane) - 1))] = e;
        }
      }
    }
  }
}
__device__ __forceinline__ void SmallFin::run(int vblock, int nblocks) const { heads_small_finish_body(vblock, nblocks, *this); }

// launches hinge_stats_kernel (losses.hip): the statistics hinge_stats_dense reads, into `workspace` (aladin_hinge_workspace_bytes)
int aladin_internal_hinge_stats(const float* S, int64_t ldS, int B, float margin, int max_violation, void* workspace,
                                int* pair_count, hipStream_t st);
// launches heads_small_stats_kernel (small_batch.hip)
int aladin_internal_heads_small_stats(const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, const float* S,
                                      int64_t ld_S, int B, int D, float margin, int max_violation, int flags, float temperature,
                                      float eps, float* M, float* st, int* pair_count, hipStream_t stream);
