// Top-k gallery search straight from the embeddings (aladin_search_topk): for every query the k best gallery items and,
// optionally, their scores -- the result of aladin_sim_matrix + aladin_topk without the (n_img x n_cap) score matrix, and
// without aladin_topk's limit of 36864 candidates per query.
//
// The gallery axis is cut into GROUPS of 16 consecutive items: the 16 columns (dim = 1) or the 16 rows (dim = 0) of one
// 16 x 16 accumulator tile.  A query's k best scores, in the output order (score descending, index ascending), all lie in
// its k best groups by (group maximum descending, group index ascending): if a score s sits in a group that was not
// selected, each of the k selected groups holds its own maximum, which precedes s -- it is larger, or equal with a lower
// index (an equal maximum in a LATER group would mean s's group had the better (maximum, index) key and was selected).
// Four passes, no data-dependent lists, no overflow path, no atomics:
//   1. search_gemm_kernel<DIM, false>: the full chain hi.hi, lo.hi, hi.lo (the main loop of sim_gemm_store_kernel), epilogue
//      gmax[query][group] = the group's maximum.  Gallery positions past the gallery (the partial last group, tile padding)
//      and NaN count as -inf -- never as the 0 a zero-padded operand row produces, or an all-negative query would select padding;
//   2. topk_kernel on gmax (sim_topk_launch): the min(k, n_groups) best groups of every query, by exactly that key;
//      search_slots_kernel: the selected groups sorted by INDEX are the query's slots; table[query][group] = slot, 0xFFFF = none;
//   3. search_gemm_kernel<DIM, true>: the same GEMM again, epilogue cand[query][slot][16] = the scores of the selected
//      (query, group) pairs, each written once by one lane;
//   4. search_final_kernel: top-k over the query's 16 * min(k, n_groups) candidates.  Slots ascend with the group index, so a
//      candidate's position ascends with its gallery index and "lower position first" IS the output's tie rule.
// Every score is the one-chain exact score times the same power-of-two unscale as in sim_gemm_store_kernel: the same bits.
#include "../../include/aladin_hip.h"

#include "sim_common.hpp"

constexpr int SEARCH_MAX_K = 256;
constexpr int SEARCH_GROUP = 16;
constexpr unsigned SEARCH_NO_SLOT = 0xFFFFu;

struct SearchGeom {
  int n_q, n_g;          // queries, gallery items
  int n_groups;          // ceil(n_g / 16)
  int kk;                // groups selected per query = slots: min(k, n_groups)
  int G_ld;              // groups per row of gmax / table: the padded gallery axis / 16 (a multiple of 24 or 16)
};
struct SearchWs {
  SimPacked sim;         // the packed operands and their padded sizes
  float* gmax;           // n_q x G_ld           (passes 1, 2)
  float* cand;           // n_q x kk x 16        (passes 3, 4: the same bytes as gmax, which is dead by then)
  uint16_t* table;       // n_q x G_ld
  int32_t* sel;          // n_q x kk: selected groups, best maximum first
  int32_t* sorted;       // n_q x kk: the same groups, ascending = slot -> group
};

static size_t search_layout(int n_img, int n_cap, int D, int k, int dim, char* base, SearchWs* ws, SearchGeom* geo) {
  SimPacked p;
  WsCursor c{base, (sim_ws_layout(n_img, n_cap, D, base, &p) + 255) / 256 * 256};
  SearchGeom g;
  g.n_q = dim == 1 ? n_img : n_cap;
  g.n_g = dim == 1 ? n_cap : n_img;
  g.n_groups = cdiv(g.n_g, SEARCH_GROUP);
  g.kk = k < g.n_groups ? k : g.n_groups;
  g.G_ld = (dim == 1 ? p.Np : p.Mp) / SEARCH_GROUP;
  if (geo) *geo = g;
  SearchWs w;
  w.sim = p;
  const size_t gmax_n = (size_t)g.n_q * g.G_ld, cand_n = (size_t)g.n_q * g.kk * SEARCH_GROUP;
  w.gmax = w.cand = c.take<float>(gmax_n > cand_n ? gmax_n : cand_n, 256);
  w.table = c.take<uint16_t>((size_t)g.n_q * g.G_ld, 256);
  w.sel = c.take<int32_t>((size_t)g.n_q * g.kk, 256);
  w.sorted = c.take<int32_t>((size_t)g.n_q * g.kk, 256);
  if (ws) *ws = w;
  return c.off;
}

static bool search_shape_ok(int n_img, int n_cap, int D, int k, int dim) {
  return n_img >= 1 && n_cap >= 1 && D >= 1 && k >= 1 && k <= SEARCH_MAX_K && (dim == 0 || dim == 1);
}
static bool search_gallery_ok(int n_img, int n_cap, int dim) { return cdiv(dim == 1 ? n_cap : n_img, SEARCH_GROUP) <= TOPK_MAX_CAND; }

extern "C" size_t aladin_search_workspace_bytes(int n_img, int n_cap, int D, int k, int dim) {
  if (!search_shape_ok(n_img, n_cap, D, k, dim) || !search_gallery_ok(n_img, n_cap, dim)) return 0;
  return search_layout(n_img, n_cap, D, k, dim, nullptr, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------
// The GEMM of passes 1 and 3.  DIM = 1: queries are the rows (images), a group is the 16 columns of an accumulator tile;
// DIM = 0: queries are the columns (captions), a group is the tile's 16 rows.  16 x 16 C tile: col = lane & 15,
// row = 4 * (lane >> 4) + reg.
// ------------------------------------------------------------------------------------------------
template <int DIM, bool COLLECT>
__global__ __launch_bounds__(512) void search_gemm_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b,
                                                          const float* __restrict__ scale, int n_img, int n_cap, int64_t ldk, int kps,
                                                          int n_nblk, int n_blocks, float* __restrict__ gmax,
                                                          const uint16_t* __restrict__ table, float* __restrict__ cand, int G_ld, int kk) {
  using Cfg = SimCfg;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int mb, nb;
  tile_coords(blockIdx.x, n_blocks / n_nblk, n_nblk, 4, mb, nb);
  constexpr int RT = SIM_RT, CT = SIM_CT;
  static_assert(RT == 8 && CT == 6, "the epilogues spell out the 128 x 96 wave tile");
  f32x4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  gemm_mainloop16_tall<Cfg, true, KMapSplit>(a + (int64_t)mb * Cfg::BM * ldk, b + (int64_t)nb * Cfg::BN * ldk, ldk, 3 * kps, smem, acc,
                                             KMapSplit{kps, 0});
  const float unscale = 1.0f / (scale[0] * scale[1]);   // exact: powers of two; the products below are sim_gemm_store_kernel's
  const int tid = fresh_tid();
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / Cfg::WGN, wn = wave % Cfg::WGN;
  const int row0 = mb * Cfg::BM + wm * (RT * 16) + 4 * (lane >> 4);
  const int col0 = nb * Cfg::BN + wn * (CT * 16) + (lane & 15);
  if constexpr (!COLLECT && DIM == 1) {
    // a row's six group maxima of this wave sit in six neighbouring lanes: one 24-byte run per row and store instruction
    const int g0 = nb * (Cfg::BN / 16) + wn * CT;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = row0 + rt * 16 + reg;
        float out = -INFINITY;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          float v = acc[rt][ct][reg] * unscale;
          if (!(v == v) || col0 + ct * 16 >= n_cap) v = -INFINITY;
          v = row16_max(v);
          if ((lane & 15) == ct) out = v;
        }
        if (row < n_img && (lane & 15) < CT) gmax[(int64_t)row * G_ld + g0 + (lane & 15)] = out;
      }
  } else if constexpr (!COLLECT && DIM == 0) {
    // a column's eight group maxima of this wave: lane group (lane >> 4) = j writes groups 2j, 2j + 1 -- 32 bytes per column
    const int g0 = mb * (Cfg::BM / 16) + wm * RT;
    const int quad = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int col = col0 + ct * 16;
      float m[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        float mm = -INFINITY;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          float v = acc[rt][ct][reg] * unscale;
          if (!(v == v) || row0 + rt * 16 + reg >= n_img) v = -INFINITY;
          mm = fmax_nc(mm, v);
        }
        mm = fmax_nc(mm, lane_xor16(mm));
        m[rt] = fmax_nc(mm, lane_xor32(mm));
      }
      float2 o;
      o.x = quad == 0 ? m[0] : quad == 1 ? m[2] : quad == 2 ? m[4] : m[6];
      o.y = quad == 0 ? m[1] : quad == 1 ? m[3] : quad == 2 ? m[5] : m[7];
      if (col < n_cap) *reinterpret_cast<float2*>(gmax + (int64_t)col * G_ld + g0 + 2 * quad) = o;
    }
  } else if constexpr (DIM == 1) {
    // the tile's slice of the slot table, 256 rows x 24 groups, through LDS (free after the main loop): 12 words per row
    constexpr int TG = Cfg::BN / 16, TW = TG / 2;
    __syncthreads();                                                   // every wave is done with the operand stages
    uint32_t* l_tab = reinterpret_cast<uint32_t*>(smem);
    for (int e = tid; e < Cfg::BM * TW; e += Cfg::THREADS) {
      const int r = e / TW, w = e - r * TW, row = mb * Cfg::BM + r;
      l_tab[e] = row < n_img ? reinterpret_cast<const uint32_t*>(table + (int64_t)row * G_ld + nb * TG)[w] : 0xFFFFFFFFu;
    }
    __syncthreads();
    const int lrow0 = wm * (RT * 16) + 4 * (lane >> 4);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = row0 + rt * 16 + reg;
        const uint32_t* t = l_tab + (lrow0 + rt * 16 + reg) * TW + wn * (CT / 2);
        const uint32_t w[3] = {t[0], t[1], t[2]};
        if ((w[0] & w[1] & w[2]) == 0xFFFFFFFFu) continue;             // pad rows too: their entries are all "none"
        float* out = cand + (int64_t)row * kk * SEARCH_GROUP + (lane & 15);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const unsigned slot = (w[ct >> 1] >> (16 * (ct & 1))) & 0xFFFFu;
          if (slot != SEARCH_NO_SLOT) out[slot * SEARCH_GROUP] = acc[rt][ct][reg] * unscale;
        }
      }
  } else {
    // 384 columns x 16 groups: 32 bytes per column
    constexpr int TG = Cfg::BM / 16;
    static_assert(TG == 16, "two 16-byte words per column");
    __syncthreads();
    uint4* l_tab = reinterpret_cast<uint4*>(smem);
    for (int e = tid; e < Cfg::BN * 2; e += Cfg::THREADS) {
      const int c = e >> 1, col = nb * Cfg::BN + c;
      l_tab[e] = col < n_cap ? reinterpret_cast<const uint4*>(table + (int64_t)col * G_ld + mb * TG)[e & 1]
                             : uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    }
    __syncthreads();
    const int lcol0 = wn * (CT * 16) + (lane & 15);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int col = col0 + ct * 16;
      const uint4 t = l_tab[(lcol0 + ct * 16) * 2 + wm];               // the eight groups of this wave's rows
      const uint32_t w[4] = {t.x, t.y, t.z, t.w};
      if ((w[0] & w[1] & w[2] & w[3]) == 0xFFFFFFFFu) continue;
      float* out = cand + (int64_t)col * kk * SEARCH_GROUP + 4 * (lane >> 4);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const unsigned slot = (w[rt >> 1] >> (16 * (rt & 1))) & 0xFFFFu;
        if (slot != SEARCH_NO_SLOT)
          *reinterpret_cast<float4*>(out + slot * SEARCH_GROUP) =
              float4{acc[rt][ct][0] * unscale, acc[rt][ct][1] * unscale, acc[rt][ct][2] * unscale, acc[rt][ct][3] * unscale};
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// One workgroup per query: its row of the slot table is set to "none", its kk selected groups are ranked by index (kk <= 256:
// every thread counts the smaller ones), sorted[rank] = group and table[group] = rank.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void search_slots_kernel(const int32_t* __restrict__ sel, int n_groups, int kk, int G_ld,
                                                           int32_t* __restrict__ sorted, uint16_t* __restrict__ table) {
  __shared__ int g[SEARCH_MAX_K];
  const int q = blockIdx.x, tid = threadIdx.x;
  uint16_t* trow = table + (int64_t)q * G_ld;
  for (int e = tid; e < G_ld / 2; e += 256) reinterpret_cast<uint32_t*>(trow)[e] = 0xFFFFFFFFu;        // G_ld is even
  if (tid < kk) g[tid] = sel[(int64_t)q * kk + tid];
  __syncthreads();                                                     // the fill has landed before a slot overwrites it
  if (tid < kk) {
    const int mine = g[tid];
    int rank = 0;
    for (int j = 0; j < kk; ++j) rank += g[j] < mine;                  // the selected groups are distinct
    sorted[(int64_t)q * kk + rank] = mine;
    if ((unsigned)mine < (unsigned)n_groups) trow[mine] = (uint16_t)rank;
  }
}

// ------------------------------------------------------------------------------------------------
// Pass 4, one workgroup per query: the selection rounds of aladin_topk (topk_rounds, sim_common.hpp) over cand[q][kk * 16].  Candidate c
// is gallery item sorted[q][c >> 4] * 16 + (c & 15), ascending in c; positions past the gallery are retired before the first round.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void search_final_kernel(const float* __restrict__ cand, const int32_t* __restrict__ sorted, int n_g, int kk,
                                                           int k, int32_t* __restrict__ out_idx, float* __restrict__ out_val) {
  __shared__ float val[SEARCH_MAX_K * SEARCH_GROUP];
  __shared__ int grp[SEARCH_MAX_K];
  __shared__ float redv[4];
  __shared__ int redi[4];
  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  const int n_c = kk * SEARCH_GROUP;
  const float* row = cand + (int64_t)q * n_c;
  if (tid < kk) grp[tid] = sorted[(int64_t)q * kk + tid];
  __syncthreads();
  for (int c = tid; c < n_c; c += 256) {                 // the positions this thread owns in topk_rounds: no barrier needed
    const int gi = grp[c >> 4];
    float v = row[c];
    if (!(v == v)) v = -INFINITY;                        // NaN sorts last
    if (gi < 0 || gi * SEARCH_GROUP + (c & 15) >= n_g) v = __builtin_nanf("");      // not a gallery item: retired
    val[c] = v;
  }
  topk_rounds(val, n_c, k, redv, redi, [&](int r, bool live, float v, int pos) {
    out_idx[(int64_t)q * k + r] = live ? grp[pos >> 4] * SEARCH_GROUP + (pos & 15) : -1;
    if (out_val) out_val[(int64_t)q * k + r] = live ? v : -INFINITY;
  });
}

template <int DIM, bool COLLECT>
static int search_gemm_launch(const SearchWs& ws, const SearchGeom& g, int n_img, int n_cap, hipStream_t st) {
  const int Mp = ws.sim.Mp, Np = ws.sim.Np, Dp = ws.sim.Dp;
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)search_gemm_kernel<DIM, COLLECT>, SimCfg::LDS_BYTES, &lds_reserved, "search_gemm")) return rc;
  const int n_mblk = Mp / SimCfg::BM, n_nblk = Np / SimCfg::BN;
  hipLaunchKernelGGL((search_gemm_kernel<DIM, COLLECT>), dim3(n_mblk * n_nblk), dim3(SimCfg::THREADS), SimCfg::LDS_BYTES, st, ws.sim.ws.a, ws.sim.ws.b,
                     ws.sim.ws.scale, n_img, n_cap, (int64_t)2 * Dp, Dp / 64, n_nblk, n_mblk * n_nblk, ws.gmax, ws.table, ws.cand, g.G_ld, g.kk);
  return aladin_check_launch(COLLECT ? "search_gemm_kernel (collect)" : "search_gemm_kernel (group maxima)");
}

extern "C" int aladin_search_topk(const float* img, int64_t img_rs, const float* cap, int64_t cap_rs, int n_img, int n_cap, int D, int k,
                                  int dim, int32_t* out_idx, float* out_val, void* workspace, void* stream) {
  if (!img || !cap || !out_idx || !workspace || !search_shape_ok(n_img, n_cap, D, k, dim) || img_rs < D || cap_rs < D) {
    aladin_set_error("search_topk: bad argument (n_img=%d n_cap=%d D=%d k=%d dim=%d; 1 <= k <= %d, dim 0 or 1)", n_img, n_cap, D, k, dim,
                     SEARCH_MAX_K);
    return ALADIN_ERR_ARG;
  }
  if (!search_gallery_ok(n_img, n_cap, dim)) {
    aladin_set_error("search_topk: at most %d gallery items (%d groups of %d), got %d", TOPK_MAX_CAND * SEARCH_GROUP, TOPK_MAX_CAND,
                     SEARCH_GROUP, dim == 1 ? n_cap : n_img);
    return ALADIN_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  SearchWs ws;
  SearchGeom g;
  search_layout(n_img, n_cap, D, k, dim, (char*)workspace, &ws, &g);
  int rc = sim_prepare(SimIn{img, img_rs, cap, cap_rs, n_img, n_cap, D}, workspace, st, &ws.sim, nullptr);
  if (rc) return rc;
  if ((rc = dim == 1 ? search_gemm_launch<1, false>(ws, g, n_img, n_cap, st)
                     : search_gemm_launch<0, false>(ws, g, n_img, n_cap, st)))
    return rc;
  if ((rc = sim_topk_launch(ws.gmax, g.G_ld, 1, g.n_q, g.n_groups, g.kk, ws.sel, nullptr, st))) return rc;
  hipLaunchKernelGGL(search_slots_kernel, dim3(g.n_q), dim3(256), 0, st, ws.sel, g.n_groups, g.kk, g.G_ld, ws.sorted, ws.table);
  if ((rc = aladin_check_launch("search_slots_kernel"))) return rc;
  if ((rc = dim == 1 ? search_gemm_launch<1, true>(ws, g, n_img, n_cap, st)
                     : search_gemm_launch<0, true>(ws, g, n_img, n_cap, st)))
    return rc;
  hipLaunchKernelGGL(search_final_kernel, dim3(g.n_q), dim3(256), 0, st, ws.cand, ws.sorted, g.n_g, g.kk, k, out_idx, out_val);
  return aladin_check_launch("search_final_kernel");
}
