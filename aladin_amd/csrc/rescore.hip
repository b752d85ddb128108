// Alignment-head re-scoring of shortlists (aladin_align_rescore, aladin_rerank_order): the MrSw score (max over regions, sum
// over words; reference alad/loss.py:80-125) of LISTED (image, caption) pairs, straight from two embedding stores (store.hip).
// Work and memory are proportional to n_q * k: no operand is repacked, nothing of the size of the (n_q x gallery) grid exists.
//
// cand is an (n_q x k) table of gallery positions (the output of aladin_search_topk, -1 = no candidate).  dim = 1: query q is
// image q, its candidates are captions; dim = 0: query q is caption q, its candidates are images.  The image is always the max
// side and the MFMA's A operand (rows of the accumulator), the caption the sum side and the B operand (columns), so a pair's
// accumulators -- and every bit of its score -- are the same whichever side was the query.
//
// Workgroup = one query x a chunk of NW candidates (NW = 8 waves, 4 where the LDS does not hold 8 panels), one wave per pair.
// A sample's rows are contiguous in its store, so its operand panel is rows + offsets[id] * ldk: per 64-deep K step the query's
// panel (read ONCE per workgroup) and the NW candidate panels go global -> LDS by LDS-DMA in the 8-row pieces and with the
// XOR swizzle of gemm_core.hpp, double buffered, and come back as ds_read_b128 fragments (lds_frag16) of v_mfma_f32_16x16x32_f16.
// Split rows [hi | lo] walk the chain hi.hi, lo.hi, hi.lo in one fp32 accumulator (KMapSplit, a = image, b = caption).
//
// Rows past a sample's count belong to the NEXT sample -- or lie past the end of the allocation for the last one: a piece's
// per-lane source row is clamped to the sample's last row (gemm_stage_k's a_avail, per lane), pieces wholly past the count are
// not fetched at all, and the epilogue SELECTS by count (rows >= count are left out of the max, words >= count add 0.0): what
// an unfetched LDS row holds only reaches accumulator rows / columns that are never looked at.
//
// Epilogue, all in registers: word w of tile ct is column lane & 15; the max over the image's regions runs over the wave's row
// tiles, the 4 registers and the 4 lane groups (exact, any order), starts from 0 for an image shorter than the padded set (the
// zero fill of alad/loss.py:116,124) and from -inf for one that fills it; the sum over words is row16_sum per tile, tiles added
// in ascending order.  One lane writes the pair's score once: no atomics, and nothing depends on the slot, the chunk, k or n_q.
//
// aladin_align_pair_map is the kernel's second instance (rescore_kernel<true>): the same main loop, and an epilogue that keeps
// the arg-max the score throws away -- per word the best region, per region the best word (rescore_map_epilogue).
#include "../../include/aladin_hip.h"

#include "pack_rows.hpp"
#include "sim_common.hpp"

constexpr int RESCORE_MAX_K = 256;
constexpr int RESCORE_MAX_COUNT = 96;                     // the tile classes' limit: six 16-row tiles per side
constexpr int RESCORE_TILES = RESCORE_MAX_COUNT / 16;
constexpr int RESCORE_LDS_LIMIT = 160 * 1024;

struct RescoreSide {
  const half_t* rows;
  const int64_t* offsets;
  const int32_t* counts;
  const int32_t* ids;      // view position -> sample, or nullptr
  int n;                   // samples in the view
  int cmax;                // host-known bound of the counts (<= 96): counts are clamped to it
  int prows;               // LDS rows of one panel: round_up(cmax, 16)
};

// field by field: selecting whole kernel-argument structs by a run-time value would send them through scratch memory
__device__ __forceinline__ RescoreSide rescore_pick(bool first, const RescoreSide& a, const RescoreSide& b) {
  return RescoreSide{first ? a.rows : b.rows, first ? a.offsets : b.offsets, first ? a.counts : b.counts, first ? a.ids : b.ids,
                     first ? a.n : b.n, first ? a.cmax : b.cmax, first ? a.prows : b.prows};
}

// ------------------------------------------------------------------------------------------------
// aladin_align_pair_map: the alignment behind a pair's score.  The same accumulation (the body of rescore_kernel below), then
// per word the best region and per region the best word, (value, index) carried through the reductions rescore_kernel runs on the value
// alone, combined by ALADIN_ARGMAX_STEP: greater value, or equal value and lower index -- commutative and associative, so the
// order of a reduction does not matter.  The zero fill of a side shorter than its padded set takes part as (0.0, RESCORE_FILL),
// the largest index, so a real position wins a tie with it; it is written as -1 / 0.0.  Every output entry is written once,
// by one lane; no atomics; a pair's bits depend on the pair alone.
// ------------------------------------------------------------------------------------------------
constexpr int RESCORE_FILL = 0x7fffffff;

struct RescoreMapOut {
  float* score;            // (n_q x k), or nullptr
  int32_t* word_region;    // (n_q x k x word_ld) and its cosines, or both nullptr
  float* word_cos;
  int32_t* region_word;    // (n_q x k x region_ld) and its cosines, or both nullptr
  float* region_cos;
  int word_ld, region_ld;
  int y_full;              // the count at which a caption fills its padded set
};

__device__ __forceinline__ void rescore_map_epilogue(const f32x4 (&acc)[RESCORE_TILES][RESCORE_TILES], int q, int slot, int k, bool live,
                                                     int cnt_x, int cnt_y, int nrt, int nct, int x_full, int split, int lane,
                                                     const RescoreMapOut& o) {
  if (slot >= k) return;
  const int64_t pair = (int64_t)q * k + slot;
  const int row0 = 4 * (lane >> 4), col0 = lane & 15;
  const float unscale = split ? ALADIN_SPLIT_UNSCALE : 1.0f;                    // exact: a power of two
  int32_t* const w_idx = o.word_region ? o.word_region + pair * o.word_ld : nullptr;
  float* const w_cos = o.word_region ? o.word_cos + pair * o.word_ld : nullptr;
  int32_t* const r_idx = o.region_word ? o.region_word + pair * o.region_ld : nullptr;
  float* const r_cos = o.region_word ? o.region_cos + pair * o.region_ld : nullptr;

  // entries from the sample's count (0 where there is no candidate) up to the row stride: -1 / 0.0
  if (w_idx)
    for (int w = (live ? cnt_y : 0) + lane; w < o.word_ld; w += 64) { w_idx[w] = -1; w_cos[w] = 0.0f; }
  if (r_idx)
    for (int r = (live ? cnt_x : 0) + lane; r < o.region_ld; r += 64) { r_idx[r] = -1; r_cos[r] = 0.0f; }
  if (!live) {
    if (o.score && lane == 0) o.score[pair] = -INFINITY;
    return;
  }

  // word -> region, and the pair's score from the per-word maxima exactly as rescore_kernel sums them
  if (w_idx || o.score) {
    float total = 0.0f;
    const float floor_ = cnt_x < x_full ? 0.0f : -INFINITY;                    // the zero fill of an image shorter than the padded set
#pragma unroll
    for (int ct = 0; ct < RESCORE_TILES; ++ct) {
      if (ct >= nct) continue;
      float v = floor_;
      int idx = RESCORE_FILL;
#pragma unroll
      for (int rt = 0; rt < RESCORE_TILES; ++rt) {
        if (rt >= nrt) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = rt * 16 + row0 + reg;
          const bool in = row < cnt_x;                                         // selected, never multiplied
          ALADIN_ARGMAX_STEP(in ? acc[rt][ct][reg] : -INFINITY, in ? row : RESCORE_FILL);
        }
      }
      ALADIN_ARGMAX_STEP(lane_xor16(v), lane_xor16(idx));
      ALADIN_ARGMAX_STEP(lane_xor32(v), lane_xor32(idx));
      const int w = ct * 16 + col0;
      total += row16_sum(w < cnt_y ? v : 0.0f);
      if (w_idx && lane < 16 && w < cnt_y) {
        w_idx[w] = idx == RESCORE_FILL ? -1 : idx;
        w_cos[w] = v * unscale;
      }
    }
    if (split) total *= ALADIN_SPLIT_UNSCALE;
    if (o.score && lane == 0) o.score[pair] = total;
  }

  // region -> word, one row tile at a time: in-lane over the word tiles, then the 16 lanes of the row (row_ror 8, 4, 2, 1)
  if (r_idx) {
    const float floor_ = cnt_y < o.y_full ? 0.0f : -INFINITY;                    // ... of a caption shorter than the padded set
#pragma unroll
    for (int rt = 0; rt < RESCORE_TILES; ++rt) {
      if (rt >= nrt) continue;
      float bv = 0.0f;
      int bi = -1;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float v = floor_;
        int idx = RESCORE_FILL;
#pragma unroll
        for (int ct = 0; ct < RESCORE_TILES; ++ct) {
          if (ct >= nct) continue;
          const int w = ct * 16 + col0;
          const bool in = w < cnt_y;
          ALADIN_ARGMAX_STEP(in ? acc[rt][ct][reg] : -INFINITY, in ? w : RESCORE_FILL);
        }
        row16_argmax(v, idx);
        if (col0 == reg) { bv = v; bi = idx; }                                 // every lane of the row holds the result: lane `reg` keeps it
      }
      const int r = rt * 16 + row0 + col0;                                     // lanes 0..3 of each row: 16 consecutive regions a tile
      if (col0 < 4 && r < cnt_x) {
        r_idx[r] = bi == RESCORE_FILL ? -1 : bi;
        r_cos[r] = bv * unscale;
      }
    }
  }
}

// rescore_kernel<false> writes the pair's score (aladin_align_rescore), rescore_kernel<true> the alignment behind it
// (aladin_align_pair_map): one body -- side selection, the double-buffered LDS-DMA loop, the accumulation -- and the instance's
// epilogue.  acc[rt][ct][reg] = <region rt * 16 + 4 * (lane >> 4) + reg, word ct * 16 + (lane & 15)>, scaled by 2^28 for split rows.
template <bool MAP> struct RescoreOut { typedef float* __restrict__ type; };
template <> struct RescoreOut<true> { typedef RescoreMapOut type; };

template <bool MAP>
__global__ __launch_bounds__(512) void rescore_kernel(RescoreSide x, RescoreSide y, const int32_t* __restrict__ cand, int k, int dim,
                                                      int x_full, int64_t ldk, int kps, int split, typename RescoreOut<MAP>::type out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nw = blockDim.x >> 6;
  const int nchunk = (k + nw - 1) / nw;
  const int q = blockIdx.x / nchunk;
  const int slot = (blockIdx.x - q * nchunk) * nw + wave;
  const RescoreSide sh = rescore_pick(dim == 1, x, y);     // the query's side, shared by the workgroup
  const RescoreSide ga = rescore_pick(dim == 1, y, x);     // the candidates' side, one panel per wave
  const int stage_bytes = (sh.prows + nw * ga.prows) * 128;
  const int g_row0 = sh.prows + wave * ga.prows;

  const int sq = sh.ids ? sh.ids[q] : q;
  const int cnt_s = min(max(sh.counts[sq], 0), sh.cmax);
  const half_t* pan_s = sh.rows + sh.offsets[sq] * ldk;
  const int c = __builtin_amdgcn_readfirstlane(slot < k ? cand[(int64_t)q * k + slot] : -1);      // one pair per wave: uniform
  const bool live = c >= 0 && c < ga.n;
  int cnt_g = 0;
  const half_t* pan_g = ga.rows;
  if (live) {
    const int sg = ga.ids ? ga.ids[c] : c;
    cnt_g = min(max(ga.counts[sg], 0), ga.cmax);
    pan_g = ga.rows + ga.offsets[sg] * ldk;
  }
  cnt_g = __builtin_amdgcn_readfirstlane(cnt_g);
  const int cnt_x = dim == 1 ? cnt_s : cnt_g, cnt_y = dim == 1 ? cnt_g : cnt_s;
  const int nrt = live ? (cnt_x + 15) >> 4 : 0, nct = live ? (cnt_y + 15) >> 4 : 0;      // 16-row tiles of this pair
  const int a_row0 = (dim == 1 ? 0 : g_row0) + (lane & 15), b_row0 = (dim == 1 ? g_row0 : 0) + (lane & 15);

  f32x4 acc[RESCORE_TILES][RESCORE_TILES];
#pragma unroll
  for (int rt = 0; rt < RESCORE_TILES; ++rt)
#pragma unroll
    for (int ct = 0; ct < RESCORE_TILES; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  const KMapSplit km{kps, 0};
  const int ktiles = split ? 3 * kps : kps;
  // K offsets of the image (a) and caption (b) rows; the shared / gathered panels take the one of their side
  auto k_sh = [&](int kt) { return split ? (dim == 1 ? km.a(kt) : km.b(kt)) : (int64_t)kt * 64; };
  auto k_ga = [&](int kt) { return split ? (dim == 1 ? km.b(kt) : km.a(kt)) : (int64_t)kt * 64; };
  sample_panel_stage(pan_s, cnt_s, ldk, k_sh(0), smem, 0, wave, nw, lane);
  sample_panel_stage(pan_g, cnt_g, ldk, k_ga(0), smem, g_row0, 0, 1, lane);
  for (int kt = 0; kt < ktiles; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                          // step kt is in LDS for every wave; every wave is done with step kt - 1
    const char* cur = smem + (kt & 1) * stage_bytes;
    if (kt + 1 < ktiles) {
      char* nxt = smem + ((kt + 1) & 1) * stage_bytes;
      sample_panel_stage(pan_s, cnt_s, ldk, k_sh(kt + 1), nxt, 0, wave, nw, lane);
      sample_panel_stage(pan_g, cnt_g, ldk, k_ga(kt + 1), nxt, g_row0, 0, 1, lane);
    }
#pragma unroll
    for (int k32 = 0; k32 < 2; ++k32) {
      half8 a[RESCORE_TILES], b[RESCORE_TILES];
#pragma unroll
      for (int t = 0; t < RESCORE_TILES; ++t) {
        a[t] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        b[t] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        if (t < nrt) a[t] = lds_frag16(cur, a_row0 + t * 16, k32, lane);
        if (t < nct) b[t] = lds_frag16(cur, b_row0 + t * 16, k32, lane);
      }
#pragma unroll
      for (int rt = 0; rt < RESCORE_TILES; ++rt) {
        if (rt >= nrt) continue;
#pragma unroll
        for (int ct = 0; ct < RESCORE_TILES; ++ct)
          if (ct < nct) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
      }
    }
  }

  if constexpr (MAP) {
    rescore_map_epilogue(acc, q, slot, k, live, cnt_x, cnt_y, nrt, nct, x_full, split, lane, out);
  } else {
    if (slot >= k) return;
    float total = -INFINITY;
    if (live) {
      total = 0.0f;
      const float floor_ = cnt_x < x_full ? 0.0f : -INFINITY;                    // the zero fill of an image shorter than the padded set
      const int row0 = 4 * (lane >> 4);
  #pragma unroll
      for (int ct = 0; ct < RESCORE_TILES; ++ct) {
        if (ct >= nct) continue;
        float m = floor_;
  #pragma unroll
        for (int rt = 0; rt < RESCORE_TILES; ++rt) {
          if (rt >= nrt) continue;
  #pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const float v = rt * 16 + row0 + reg < cnt_x ? acc[rt][ct][reg] : -INFINITY;      // selected, never multiplied
            m = fmax_nc(m, v);
          }
        }
        m = fmax_nc(m, lane_xor16(m));
        m = fmax_nc(m, lane_xor32(m));
        const float wv = ct * 16 + (lane & 15) < cnt_y ? m : 0.0f;
        total += row16_sum(wv);
      }
      if (split) total *= ALADIN_SPLIT_UNSCALE;                                 // exact: a power of two
    }
    if (lane == 0) out[(int64_t)q * k + slot] = total;
  }
}

// ------------------------------------------------------------------------------------------------
// One workgroup per query: the stable descending order of its re-scored shortlist.  Entry t goes to position
// #{j : j precedes t}, j precedes t when it is a candidate and t is none, or both are alike and score_j > score_t, or the
// scores are equal and j < t (the earlier shortlist slot: the matching head breaks ties).  NaN counts as -inf.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rerank_order_kernel(const int32_t* __restrict__ cand, const float* __restrict__ scores, int k,
                                                           int32_t* __restrict__ out_idx, float* __restrict__ out_val) {
  __shared__ float val[RESCORE_MAX_K];
  __shared__ int idx[RESCORE_MAX_K];
  const int q = blockIdx.x, t = threadIdx.x;
  if (t < k) {
    const int c = cand[(int64_t)q * k + t];
    float v = scores[(int64_t)q * k + t];
    if (!(v == v) || c < 0) v = -INFINITY;
    val[t] = v;
    idx[t] = c < 0 ? -1 : c;
  }
  __syncthreads();
  if (t < k) {
    const float v = val[t];
    const bool none = idx[t] < 0;
    int rank = 0;
    for (int j = 0; j < k; ++j) {
      const bool jnone = idx[j] < 0;
      const bool before = jnone != none ? none : (val[j] > v || (val[j] == v && j < t));
      rank += before;
    }
    out_idx[(int64_t)q * k + rank] = idx[t];
    out_val[(int64_t)q * k + rank] = v;
  }
}

static int rescore_waves(int sh_rows, int ga_rows) {
  for (int nw = 8; nw >= 4; nw >>= 1)
    if (2 * (sh_rows + nw * ga_rows) * 128 <= RESCORE_LDS_LIMIT) return nw;
  return 0;
}

// The checks and the launch geometry aladin_align_rescore and aladin_align_pair_map share; `who` names the caller in messages.
struct RescorePlan {
  RescoreSide x, y;
  int width, kps, split, nw, lds_bytes;
  unsigned blocks;
};

static int rescore_plan(const char* who, const void* x_rows, const int64_t* x_offsets, const int32_t* x_counts, const int32_t* x_ids, int n_x,
                        int x_max_count, const void* y_rows, const int64_t* y_offsets, const int32_t* y_counts, const int32_t* y_ids, int n_y,
                        int y_max_count, int D, int precision, int dim, int x_full, const int32_t* cand, int k, bool outputs_ok,
                        RescorePlan* p) {
  if (!x_rows || !x_offsets || !x_counts || !y_rows || !y_offsets || !y_counts || !cand || !outputs_ok || n_x < 1 || n_y < 1 || D < 1 ||
      (dim != 0 && dim != 1) || (precision != ALADIN_PRECISION_FP16 && precision != ALADIN_PRECISION_SPLIT) || x_full < 1 ||
      x_max_count < 0 || y_max_count < 0) {
    aladin_set_error("%s: bad argument (n_x=%d n_y=%d D=%d precision=%d dim=%d x_full=%d; null table or output, dim 0 or 1)", who, n_x,
                     n_y, D, precision, dim, x_full);
    return ALADIN_ERR_ARG;
  }
  if (k < 1 || k > RESCORE_MAX_K) {
    aladin_set_error("%s: 1 <= k <= %d candidates per query, got %d", who, RESCORE_MAX_K, k);
    return ALADIN_ERR_UNSUPPORTED;
  }
  if (x_max_count > RESCORE_MAX_COUNT || y_max_count > RESCORE_MAX_COUNT) {
    aladin_set_error("%s: at most %d scored positions per set, got %d regions / %d words", who, RESCORE_MAX_COUNT, x_max_count,
                     y_max_count);
    return ALADIN_ERR_UNSUPPORTED;
  }
  p->width = aladin_store_row_width(D, precision);
  if (p->width < D) {
    aladin_set_error("%s: feature size %d is not one a store holds", who, D);
    return ALADIN_ERR_UNSUPPORTED;
  }
  p->split = precision == ALADIN_PRECISION_SPLIT;
  const int Dp = p->split ? p->width / 2 : p->width;
  if (Dp % 64) {
    aladin_set_error("%s: store rows of %d halfs are not whole 64-deep K steps", who, Dp);
    return ALADIN_ERR_UNSUPPORTED;
  }
  p->kps = Dp / 64;
  p->x = RescoreSide{(const half_t*)x_rows, x_offsets, x_counts, x_ids, n_x, x_max_count, round_up(x_max_count > 0 ? x_max_count : 1, 16)};
  p->y = RescoreSide{(const half_t*)y_rows, y_offsets, y_counts, y_ids, n_y, y_max_count, round_up(y_max_count > 0 ? y_max_count : 1, 16)};
  const int sh_rows = dim == 1 ? p->x.prows : p->y.prows, ga_rows = dim == 1 ? p->y.prows : p->x.prows;
  p->nw = rescore_waves(sh_rows, ga_rows);
  if (!p->nw) {
    aladin_set_error("%s: no chunk of %d + n x %d rows fits the LDS", who, sh_rows, ga_rows);
    return ALADIN_ERR_UNSUPPORTED;
  }
  p->lds_bytes = 2 * (sh_rows + p->nw * ga_rows) * 128;
  const int n_q = dim == 1 ? n_x : n_y;
  const int64_t blocks = (int64_t)n_q * cdiv(k, p->nw);
  if (blocks > 0x7fffffff) {
    aladin_set_error("%s: %d queries x %d candidates are more workgroups than one launch takes", who, n_q, k);
    return ALADIN_ERR_UNSUPPORTED;
  }
  p->blocks = (unsigned)blocks;
  return ALADIN_OK;
}

extern "C" int aladin_align_rescore(const void* x_rows, const int64_t* x_offsets, const int32_t* x_counts, const int32_t* x_ids, int n_x,
                                    int x_max_count, const void* y_rows, const int64_t* y_offsets, const int32_t* y_counts,
                                    const int32_t* y_ids, int n_y, int y_max_count, int D, int precision, int dim, int x_full,
                                    const int32_t* cand, int k, float* out, void* stream) {
  RescorePlan p;
  if (int rc = rescore_plan("align_rescore", x_rows, x_offsets, x_counts, x_ids, n_x, x_max_count, y_rows, y_offsets, y_counts, y_ids, n_y,
                            y_max_count, D, precision, dim, x_full, cand, k, out != nullptr, &p))
    return rc;
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)rescore_kernel<false>, RESCORE_LDS_LIMIT, &lds_reserved, "rescore_kernel")) return rc;
  hipLaunchKernelGGL(rescore_kernel<false>, dim3(p.blocks), dim3(p.nw * 64), p.lds_bytes, (hipStream_t)stream, p.x, p.y, cand, k, dim, x_full,
                     (int64_t)p.width, p.kps, p.split, out);
  return aladin_check_launch("rescore_kernel");
}

extern "C" int aladin_align_pair_map(const void* x_rows, const int64_t* x_offsets, const int32_t* x_counts, const int32_t* x_ids, int n_x,
                                     int x_max_count, const void* y_rows, const int64_t* y_offsets, const int32_t* y_counts,
                                     const int32_t* y_ids, int n_y, int y_max_count, int D, int precision, int dim, int x_full, int y_full,
                                     const int32_t* cand, int k, float* out_score, int32_t* word_region, float* word_cos, int64_t word_ld,
                                     int32_t* region_word, float* region_cos, int64_t region_ld, void* stream) {
  const bool words = word_region || word_cos, regions = region_word || region_cos;
  if ((!out_score && !words && !regions) || !word_region != !word_cos || !region_word != !region_cos) {
    aladin_set_error("align_pair_map: no output, or one of an (index, cosine) pair of outputs without the other");
    return ALADIN_ERR_ARG;
  }
  if (y_full < 1 || (words && (word_ld < y_max_count || word_ld > 0x7fffffff)) ||
      (regions && (region_ld < x_max_count || region_ld > 0x7fffffff))) {
    aladin_set_error("align_pair_map: bad argument (y_full=%d word_ld=%lld for %d words, region_ld=%lld for %d regions)", y_full,
                     (long long)word_ld, y_max_count, (long long)region_ld, x_max_count);
    return ALADIN_ERR_ARG;
  }
  RescorePlan p;
  if (int rc = rescore_plan("align_pair_map", x_rows, x_offsets, x_counts, x_ids, n_x, x_max_count, y_rows, y_offsets, y_counts, y_ids, n_y,
                            y_max_count, D, precision, dim, x_full, cand, k, true, &p))
    return rc;
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)rescore_kernel<true>, RESCORE_LDS_LIMIT, &lds_reserved, "rescore_kernel<true>")) return rc;
  const RescoreMapOut o{out_score, word_region, word_cos, region_word, region_cos, words ? (int)word_ld : 0, regions ? (int)region_ld : 0,
                        y_full};
  hipLaunchKernelGGL(rescore_kernel<true>, dim3(p.blocks), dim3(p.nw * 64), p.lds_bytes, (hipStream_t)stream, p.x, p.y, cand, k, dim,
                     x_full, (int64_t)p.width, p.kps, p.split, o);
  return aladin_check_launch("rescore_kernel<true>");
}

extern "C" int aladin_rerank_order(const int32_t* cand, const float* scores, int n_q, int k, int32_t* out_idx, float* out_val,
                                   void* stream) {
  if (!cand || !scores || !out_idx || !out_val || n_q < 1) {
    aladin_set_error("rerank_order: bad argument (n_q=%d; null table or output)", n_q);
    return ALADIN_ERR_ARG;
  }
  if (k < 1 || k > RESCORE_MAX_K) {
    aladin_set_error("rerank_order: 1 <= k <= %d candidates per query, got %d", RESCORE_MAX_K, k);
    return ALADIN_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(rerank_order_kernel, dim3(n_q), dim3(256), 0, (hipStream_t)stream, cand, scores, k, out_idx, out_val);
  return aladin_check_launch("rerank_order_kernel");
}
