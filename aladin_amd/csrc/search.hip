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
// GATHER (the small-batch route of an index search, below): cand is the query's row of the score strip, ld floats long, and candidate c
// lies at grp * 16 + (c & 15) of it.
template <bool GATHER>
__global__ __launch_bounds__(256) void search_final_kernel(const float* __restrict__ cand, const int32_t* __restrict__ sorted, int n_g, int kk,
                                                           int k, int64_t ld, int32_t* __restrict__ out_idx, float* __restrict__ out_val) {
  __shared__ float val[SEARCH_MAX_K * SEARCH_GROUP];
  __shared__ int grp[SEARCH_MAX_K];
  __shared__ float redv[4];
  __shared__ int redi[4];
  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  const int n_c = kk * SEARCH_GROUP;
  const float* row = cand + (int64_t)q * (GATHER ? ld : (int64_t)n_c);
  if (tid < kk) grp[tid] = sorted[(int64_t)q * kk + tid];
  __syncthreads();
  for (int c = tid; c < n_c; c += 256) {                 // the positions this thread owns in topk_rounds: no barrier needed
    const int gi = grp[c >> 4];
    float v;
    if constexpr (GATHER) v = gi < 0 ? 0.f : row[(int64_t)gi * SEARCH_GROUP + (c & 15)];
    else v = row[c];
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

// passes 1 - 4 over packed operands: ws.sim names them and their scale pair (the workspace of aladin_search_topk, or a gallery
// index and the queries packed beside it)
static int search_passes(const SearchWs& ws, const SearchGeom& g, int n_img, int n_cap, int k, int dim, int32_t* out_idx, float* out_val,
                         hipStream_t st) {
  int rc;
  if ((rc = dim == 1 ? search_gemm_launch<1, false>(ws, g, n_img, n_cap, st)
                     : search_gemm_launch<0, false>(ws, g, n_img, n_cap, st)))
    return rc;
  if ((rc = sim_topk_launch(ws.gmax, g.G_ld, 1, g.n_q, g.n_groups, g.kk, ws.sel, nullptr, st))) return rc;
  hipLaunchKernelGGL(search_slots_kernel, dim3(g.n_q), dim3(256), 0, st, ws.sel, g.n_groups, g.kk, g.G_ld, ws.sorted, ws.table);
  if ((rc = aladin_check_launch("search_slots_kernel"))) return rc;
  if ((rc = dim == 1 ? search_gemm_launch<1, true>(ws, g, n_img, n_cap, st)
                     : search_gemm_launch<0, true>(ws, g, n_img, n_cap, st)))
    return rc;
  hipLaunchKernelGGL(search_final_kernel<false>, dim3(g.n_q), dim3(256), 0, st, ws.cand, ws.sorted, g.n_g, g.kk, k, (int64_t)0, out_idx, out_val);
  return aladin_check_launch("search_final_kernel");
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
  if (int rc = sim_prepare(SimIn{img, img_rs, cap, cap_rs, n_img, n_cap, D}, workspace, st, &ws.sim, nullptr)) return rc;
  return search_passes(ws, g, n_img, n_cap, k, dim, out_idx, out_val, st);
}

// ================================================================================================
// Gallery index (aladin_search_index_*): the gallery packed ONCE, queried many times.
//
// The index is the gallery in the operand format of sim_common.hpp behind a header:
//   [0, 256)               scale: float [0] = 2^e of the gallery's absmax
//   [256, INDEX_HEADER)    the absmax partials of the build (scratch; dead after it)
//   [INDEX_HEADER, ...)    index_rows(n) rows [hi | lo] of 2 Dp halfs; rows past n are zero.  index_rows(n) covers the padding of
//                          BOTH operand roles (a multiple of 256 as images, of 384 as captions), so the tile kernels read it as either.
// A search packs only its queries (their scale from the absmax of the whole query matrix of the call) and copies the gallery's scale
// beside theirs.  Two routes, index_plan() decides:
//   stream (n_q <= 32, Dp <= 768): search_stream_kernel reads the gallery ONCE and leaves the n_q x 16 n_groups score strip and the
//     group maxima; sim_topk_launch + search_slots_kernel select and sort the groups as in passes 2; search_final_kernel<true>
//     gathers the selected groups' scores from the strip.  No second pass over the gallery.
//   tile: passes 1 - 4 above, the gallery operand pointing into the index.
// Both run the chain of search_gemm_kernel on the same packed bits: images the A operand, captions the B operand, hi.hi, lo.hi, hi.lo.
// ================================================================================================
constexpr size_t INDEX_HEADER = 256 + 2 * SIM_ABS_BLOCKS * sizeof(float);
constexpr int STREAM_MAX_Q = 32;               // two 16-row accumulator tiles of queries
constexpr int STREAM_PF = 12;                  // 16-byte pieces a thread keeps in flight: 256 threads x 12 x 16 B = 48 KiB, one group at Dp = 768
constexpr int STREAM_MAX_DP = STREAM_PF * 256 * 16 / (SEARCH_GROUP * 4);      // 768: a group of 16 rows x 4 Dp bytes fits the pieces in flight
constexpr int STREAM_MAX_GROUPS = 8;           // groups per slab at small Dp
constexpr int STREAM_WGS = 256;                // one workgroup per CU of the MI355X: each takes the LDS of its CU
constexpr int STREAM_ROW_PAD = 16;             // bytes between LDS rows: the 16 rows of a fragment read land on 16 different bank groups
// the most LDS any plan asks for (reserved once per device): 32 query rows at Dp = 768, a slab's pieces in flight, its rows' padding
constexpr int STREAM_LDS_MAX = STREAM_MAX_Q * (4 * STREAM_MAX_DP + STREAM_ROW_PAD) + STREAM_PF * 256 * 16 +
                               STREAM_MAX_GROUPS * SEARCH_GROUP * STREAM_ROW_PAD;
static_assert(STREAM_LDS_MAX <= 160 * 1024, "a workgroup takes the LDS of one CU");

static int index_rows(int n) {
  const int a = round_up(n, SimCfg::BM), b = round_up(n, SimCfg::BN);
  return a > b ? a : b;
}
static bool index_shape_ok(int n, int D) { return n >= 1 && D >= 1; }
static bool index_size_ok(int n) { return cdiv(n, SEARCH_GROUP) <= TOPK_MAX_CAND; }

extern "C" size_t aladin_search_index_bytes(int n, int D) {
  if (!index_shape_ok(n, D) || !index_size_ok(n)) return 0;
  return INDEX_HEADER + (size_t)index_rows(n) * 2 * round_up(D, 64) * sizeof(half_t);
}

extern "C" int aladin_search_index_build(const float* x, int64_t row_stride, int n, int D, void* index, void* stream) {
  if (!x || !index || !index_shape_ok(n, D) || row_stride < D) {
    aladin_set_error("search_index_build: bad argument (n=%d D=%d row_stride=%lld)", n, D, (long long)row_stride);
    return ALADIN_ERR_ARG;
  }
  if (!index_size_ok(n)) {
    aladin_set_error("search_index_build: at most %d gallery items (%d groups of %d), got %d", TOPK_MAX_CAND * SEARCH_GROUP, TOPK_MAX_CAND,
                     SEARCH_GROUP, n);
    return ALADIN_ERR_UNSUPPORTED;
  }
  char* base = (char*)index;
  return sim_pack_operand(SimOperand{x, row_stride, n, index_rows(n), D, (half_t*)(base + INDEX_HEADER), (float*)base, 0, nullptr},
                          (float*)(base + 256), (hipStream_t)stream);
}

struct IndexPlan {
  bool stream;           // the small-batch route
  int n_qt, S;           // stream: 16-row query tiles, groups per slab
  int n_slabs;
  size_t lds;
  int q_rows;            // rows of the packed query operand
  SearchGeom g;
  SearchWs ws;           // ws.sim.ws.a / b / scale: the operands in their roles (one of them inside the index)
  float* strip;          // stream: n_q x 16 n_groups scores
};

// THE routing rule, and the workspace either route needs
static size_t index_plan(const void* index, int n, int D, int n_q, int k, int dim, char* base, IndexPlan* out) {
  IndexPlan p{};
  const int Dp = round_up(D, 64);
  p.stream = n_q <= STREAM_MAX_Q && Dp <= STREAM_MAX_DP;
  SearchGeom& g = p.g;
  g.n_q = n_q, g.n_g = n;
  g.n_groups = cdiv(n, SEARCH_GROUP);
  g.kk = k < g.n_groups ? k : g.n_groups;
  SimPacked& sp = p.ws.sim;
  sp.Dp = Dp;
  if (p.stream) {
    p.n_qt = cdiv(n_q, 16);
    p.S = 1;
    while (p.S * 2 <= STREAM_MAX_GROUPS && p.S * 2 * SEARCH_GROUP * 4 * Dp <= STREAM_PF * 256 * 16) p.S *= 2;
    p.n_slabs = cdiv(g.n_groups, p.S);
    p.lds = (size_t)(p.n_qt * 16 + p.S * SEARCH_GROUP) * (4 * Dp + STREAM_ROW_PAD);
    p.q_rows = p.n_qt * 16;
    g.G_ld = round_up(g.n_groups, 2);
  } else {
    sp.Mp = round_up(dim == 1 ? n_q : n, SimCfg::BM), sp.Np = round_up(dim == 1 ? n : n_q, SimCfg::BN);
    p.q_rows = dim == 1 ? sp.Mp : sp.Np;
    g.G_ld = (dim == 1 ? sp.Np : sp.Mp) / SEARCH_GROUP;
  }
  WsCursor c{base, 0};
  sp.ws.scale = c.take<float>(64);
  sp.ws.partial = c.take<float>(2 * SIM_ABS_BLOCKS);
  half_t* q = c.take<half_t>((size_t)p.q_rows * 2 * Dp, 256);
  half_t* gal = index ? (half_t*)((char*)index + INDEX_HEADER) : nullptr;
  sp.ws.a = dim == 1 ? q : gal;
  sp.ws.b = dim == 1 ? gal : q;
  const size_t gmax_n = (size_t)n_q * g.G_ld, cand_n = (size_t)n_q * g.kk * SEARCH_GROUP;
  if (p.stream) {
    p.strip = c.take<float>((size_t)n_q * g.n_groups * SEARCH_GROUP, 256);
    p.ws.gmax = c.take<float>(gmax_n, 256);
  } else {
    p.ws.gmax = p.ws.cand = c.take<float>(gmax_n > cand_n ? gmax_n : cand_n, 256);
  }
  p.ws.table = c.take<uint16_t>((size_t)n_q * g.G_ld, 256);
  p.ws.sel = c.take<int32_t>((size_t)n_q * g.kk, 256);
  p.ws.sorted = c.take<int32_t>((size_t)n_q * g.kk, 256);
  if (out) *out = p;
  return c.off;
}

static bool index_search_ok(int n_q, int n, int D, int k, int dim) {
  return n_q >= 1 && index_shape_ok(n, D) && k >= 1 && k <= SEARCH_MAX_K && (dim == 0 || dim == 1);
}

extern "C" size_t aladin_search_index_workspace_bytes(int n_q, int n, int D, int k, int dim) {
  if (!index_search_ok(n_q, n, D, k, dim) || !index_size_ok(n)) return 0;
  return index_plan(nullptr, n, D, n_q, k, dim, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------
// The small-batch route's one pass over the gallery.  A workgroup (4 waves, the LDS of a CU) keeps the packed queries in LDS and walks
// the slabs blockIdx.x, blockIdx.x + gridDim.x, ...: a slab is S consecutive groups = 16 S whole rows, contiguous in the index.
// Every thread fetches 16-byte pieces of the slab in address order (whole lines, each byte once) into registers; while they are in
// flight the waves multiply the slab that is in LDS, then the registers are written to LDS and the next slab is requested.  A wave
// owns the (group, query tile) pairs wave, wave + 4, ... of the slab and runs each pair's chain from LDS fragment reads (sim_chain_lds):
// images are the A operand in both directions.  16 x 16 C tile: col = lane & 15, row = 4 * (lane >> 4) + reg.
// ------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void search_stream_kernel(const half_t* __restrict__ gal, int64_t gal_bytes, const half_t* __restrict__ qpk,
                                                            const float* __restrict__ scale, int n_q, int n_g, int n_groups, int Dp, int n_qt,
                                                            int S, int n_slabs, float* __restrict__ strip, float* __restrict__ gmax, int G_ld) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row_b = 4 * Dp, ldl_b = row_b + STREAM_ROW_PAD;            // bytes of a packed row in memory / in LDS
  char* lq = smem;
  char* lg = smem + n_qt * 16 * ldl_b;
  const int slab_b = S * SEARCH_GROUP * row_b;                         // <= STREAM_PF * 4096
  int loff[STREAM_PF];                                                 // where this thread's pieces go in LDS: the same for every slab
#pragma unroll
  for (int u = 0; u < STREAM_PF; ++u) {
    const int o = (u * 256 + tid) * 16;
    loff[u] = o < slab_b ? (o / row_b) * ldl_b + o % row_b : -1;
  }
  uint4 pf[STREAM_PF];
  auto fetch = [&](int slab) {
    const int64_t base = (int64_t)slab * slab_b;
#pragma unroll
    for (int u = 0; u < STREAM_PF; ++u) {
      const int64_t o = base + (u * 256 + tid) * 16;
      pf[u] = uint4{0u, 0u, 0u, 0u};
      if (loff[u] >= 0 && o < gal_bytes) pf[u] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(gal) + o);
    }
  };
  int slab = blockIdx.x;                                               // the grid never exceeds n_slabs
  fetch(slab);
  for (int o = tid * 16; o < n_qt * 16 * row_b; o += 256 * 16)
    *reinterpret_cast<uint4*>(lq + (o / row_b) * ldl_b + o % row_b) = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(qpk) + o);
  const float unscale = 1.0f / (scale[0] * scale[1]);                  // exact: powers of two; the products below are search_gemm_kernel's
  const int nblk = Dp / 32;
  const int64_t ld_strip = (int64_t)n_groups * SEARCH_GROUP;
  for (; slab < n_slabs; slab += gridDim.x) {
    __syncthreads();                                                   // the waves are done with the slab in LDS (first trip: nothing)
#pragma unroll
    for (int u = 0; u < STREAM_PF; ++u)
      if (loff[u] >= 0) *reinterpret_cast<uint4*>(lg + loff[u]) = pf[u];
    __syncthreads();                                                   // the slab (first trip: and the queries) is in LDS
    if (slab + (int)gridDim.x < n_slabs) fetch(slab + gridDim.x);      // in flight under the chains below
    for (int p = wave; p < S * n_qt; p += 4) {
      const int gs = p / n_qt, qt = p - gs * n_qt, grp = slab * S + gs;
      if (grp >= n_groups) continue;
      const half_t* qp = reinterpret_cast<const half_t*>(lq + (qt * 16 + (lane & 15)) * ldl_b) + 8 * (lane >> 4);
      const half_t* gp = reinterpret_cast<const half_t*>(lg + (gs * SEARCH_GROUP + (lane & 15)) * ldl_b) + 8 * (lane >> 4);
      const half_t* ap = DIM == 1 ? qp : gp;                           // images
      const half_t* bp = DIM == 1 ? gp : qp;                           // captions
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      sim_chain_lds(ap, bp, nblk, acc);                                // hi.hi
      sim_chain_lds(ap + Dp, bp, nblk, acc);                           // lo.hi
      sim_chain_lds(ap, bp + Dp, nblk, acc);                           // hi.lo
      if constexpr (DIM == 1) {
        // rows = queries, columns = the group's items: a query's 16 scores sit in 16 neighbouring lanes
        const int item = grp * SEARCH_GROUP + (lane & 15);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int q = qt * 16 + 4 * (lane >> 4) + reg;
          const float v = acc[reg] * unscale;
          float m = v;
          if (!(m == m) || item >= n_g) m = -INFINITY;                 // past the gallery and NaN: never the 0 of a zero row
          m = row16_max(m);
          if (q < n_q) {
            strip[q * ld_strip + item] = v;
            if ((lane & 15) == 0) gmax[(int64_t)q * G_ld + grp] = m;
          }
        }
      } else {
        // rows = the group's items, columns = queries: a lane holds four neighbouring scores of its query
        const int q = qt * 16 + (lane & 15), item0 = grp * SEARCH_GROUP + 4 * (lane >> 4);
        float4 o;
        float mm = -INFINITY;
        float* ov = &o.x;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float v = acc[reg] * unscale;
          ov[reg] = v;
          float m = v;
          if (!(m == m) || item0 + reg >= n_g) m = -INFINITY;
          mm = fmax_nc(mm, m);
        }
        mm = fmax_nc(mm, lane_xor16(mm));
        mm = fmax_nc(mm, lane_xor32(mm));
        if (q < n_q) {
          *reinterpret_cast<float4*>(strip + q * ld_strip + item0) = o;
          if (lane < 16) gmax[(int64_t)q * G_ld + grp] = mm;
        }
      }
    }
  }
}

template <int DIM>
static int search_stream_launch(const IndexPlan& p, int n, hipStream_t st) {
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)search_stream_kernel<DIM>, STREAM_LDS_MAX, &lds_reserved, "search_stream")) return rc;
  const SimWs& w = p.ws.sim.ws;
  const half_t* gal = DIM == 1 ? w.b : w.a;
  const half_t* q = DIM == 1 ? w.a : w.b;
  const int Dp = p.ws.sim.Dp;
  hipLaunchKernelGGL(search_stream_kernel<DIM>, dim3(p.n_slabs < STREAM_WGS ? p.n_slabs : STREAM_WGS), dim3(256), p.lds, st, gal,
                     (int64_t)index_rows(n) * 4 * Dp, q, w.scale, p.g.n_q, n, p.g.n_groups, Dp, p.n_qt, p.S, p.n_slabs, p.strip, p.ws.gmax,
                     p.g.G_ld);
  return aladin_check_launch("search_stream_kernel");
}

extern "C" int aladin_search_index_topk(const void* index, int n, int D, const float* q, int64_t q_rs, int n_q, int k, int dim,
                                        int32_t* out_idx, float* out_val, void* workspace, void* stream) {
  if (!index || !q || !out_idx || !workspace || !index_search_ok(n_q, n, D, k, dim) || q_rs < D) {
    aladin_set_error("search_index_topk: bad argument (n=%d D=%d n_q=%d k=%d dim=%d q_row_stride=%lld; 1 <= k <= %d, dim 0 or 1)", n, D, n_q, k,
                     dim, (long long)q_rs, SEARCH_MAX_K);
    return ALADIN_ERR_ARG;
  }
  if (!index_size_ok(n)) {
    aladin_set_error("search_index_topk: at most %d gallery items (%d groups of %d), got %d", TOPK_MAX_CAND * SEARCH_GROUP, TOPK_MAX_CAND,
                     SEARCH_GROUP, n);
    return ALADIN_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  IndexPlan p;
  index_plan(index, n, D, n_q, k, dim, (char*)workspace, &p);
  const SimWs& w = p.ws.sim.ws;
  const int q_slot = dim == 1 ? 0 : 1;                                 // the queries are the images (scale[0]) or the captions (scale[1])
  const SimOperand qop{q, q_rs, n_q, p.q_rows, D, dim == 1 ? w.a : w.b, w.scale, q_slot, (const float*)index};
  int rc = p.stream ? sim_pack_operand_small(qop, st) : sim_pack_operand(qop, w.partial, st);
  if (rc) return rc;
  if (!p.stream) return search_passes(p.ws, p.g, dim == 1 ? n_q : n, dim == 1 ? n : n_q, k, dim, out_idx, out_val, st);
  if ((rc = dim == 1 ? search_stream_launch<1>(p, n, st) : search_stream_launch<0>(p, n, st))) return rc;
  if ((rc = sim_topk_launch(p.ws.gmax, p.g.G_ld, 1, n_q, p.g.n_groups, p.g.kk, p.ws.sel, nullptr, st))) return rc;
  // search_slots_kernel is taken as it is: it also fills the slot table (2 bytes per (query, group)), which nothing reads on this route --
  // search_final_kernel<true> gathers by `sorted` alone.  At most 2.4 MB written per call (32 x 36864), beside the 75 MB strip.
  hipLaunchKernelGGL(search_slots_kernel, dim3(n_q), dim3(256), 0, st, p.ws.sel, p.g.n_groups, p.g.kk, p.g.G_ld, p.ws.sorted, p.ws.table);
  if ((rc = aladin_check_launch("search_slots_kernel"))) return rc;
  hipLaunchKernelGGL(search_final_kernel<true>, dim3(n_q), dim3(256), 0, st, p.strip, p.ws.sorted, n, p.g.kk, k,
                     (int64_t)p.g.n_groups * SEARCH_GROUP, out_idx, out_val);
  return aladin_check_launch("search_final_kernel (gather)");
}
