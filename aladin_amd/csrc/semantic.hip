// The semantic contrastive loss on a B x B score matrix S with a B x B relevance matrix Rel, reference alad/loss.py:203-270
// (SemanticContrastiveLoss): the VSE++ hinge anchored not at the diagonal but, per row and per column, at ONE pair chosen among
// those whose relevance exceeds a threshold.  Line v in [0, 2B) is row v, or column v - B.
//   candidates   of row i: the columns j with Rel[i,j] > threshold, ascending; of column j: the rows, likewise (NaN: no candidate)
//   pos[v]       the (draws[v] mod n)-th of the line's n candidates; n = 0: the diagonal cell (the reference raises there)
//   a1[i]        S[i, pos[i]]
//   a2[m]        'aligned' order: S[pos[B+m], m].  'reference' order (what scores[cols_mask].view(B, 1).t() does): the score at
//                the m-th of the B chosen cells (pos[B+j], j) sorted by (row, column); rank[j] is column j's cell's place there
//   cs[i,j]      hinge_cost(margin + S[i,j] - a1[i]),  ci[i,j] = hinge_cost(margin + S[i,j] - a2[j]);  both 0 on the diagonal and,
//                with ALADIN_SEM_MASK_POSITIVES, wherever Rel[i,j] > threshold
//   loss         sum cs + sum ci, or sum_i max_j cs + sum_j max_i ci (ties: the lowest index)
//   dS[i,j]      [cs active] + [ci active] - [pos[i] == j] nrow[i] - [pos[B+j] == i] ncol[rank[j]]
// FOUR launches on the caller's stream in 'reference' order, THREE in 'aligned' order (the ranking needs every column's pick, the
// anchors need the ranking, the gradient needs every line's count):
//   sem_select_kernel  a line's candidates are counted, then the wanted one is found in a second walk.  Rel is read through its
//                      strides, so each of the two line sets takes the shape its memory asks for: lines whose elements lie closer
//                      together than the lines do get one wave each, lanes along the line; the others go in strips of 64 adjacent
//                      lines, lanes across lines, 16 waves sharing the line's length in ascending pieces -- coalesced either way,
//                      for a row-major Rel and for a transposed view of one.  Writes pos, a1 and, in 'aligned' order, a2 / rank.
//   sem_rank_kernel    ('reference' order) one wave per column j counts the chosen cells before (pos[B+j], j); rank[j] = k,
//                      a2[k] = S[pos[B+j], j].
//   sem_stats_kernel   HingeStats of every line: line_walk (line_walk.hpp) with HingeAcc (matrix_losses.hpp), the VSE++ hinge's own
//                      running statistics, against the line's anchor; the masks are this file's.
//   sem_finish_kernel  block (0, 0) sums the lines' values, rows then columns; every block writes dS for its 256 columns over the
//                      rows dealt to it (owner-computes: a cell receives at most one row anchor and one column anchor).
// Nothing is accumulated with atomics and every sum runs in a fixed order: the same input gives the same bits.  draws and the
// threshold comparison are read on the device: no host synchronisation, a replayed graph follows the current draws.
#include "../../include/aladin_hip.h"
#include "common.hpp"
#include "matrix_losses.hpp"

#define SEM_MAX_B ALADIN_SEM_MAX_B
#define SEM_THREADS 1024                 // 16 waves: 16 wave-lines, or one strip of 64 lines shared by 16 waves
#define SEM_WAVES (SEM_THREADS / 64)

// workspace: val[2B] | arg[2B] (hinge_stats_dense) | pos[2B] | a1[B] | a2[B] | rank[B]
struct SemWs { float* val; int* arg; int* pos; float* a1; float* a2; int* rank; };
static inline SemWs sem_ws(void* workspace, int B) {
  float* val = (float*)workspace;
  SemWs w;
  w.val = val; w.arg = (int*)(val + 2 * (size_t)B); w.pos = w.arg + 2 * (size_t)B;
  w.a1 = (float*)(w.pos + 2 * (size_t)B); w.a2 = w.a1 + B; w.rank = (int*)(w.a2 + B);
  return w;
}

struct SemRel {
  const float* p; int64_t rs, cs; float thr;
  __device__ __forceinline__ bool above(int i, int j) const { return p[(int64_t)i * rs + (int64_t)j * cs] > thr; }
};

static inline bool sem_wave_lines(int64_t along, int64_t across) { return along <= across; }
static inline int sem_line_blocks(int B, bool wave_lines) { return cdiv(B, wave_lines ? SEM_WAVES : 64); }

// One line per wave, lanes along it: element t of the line at p[t * along].  -> the chosen position (wave-uniform)
__device__ __forceinline__ int sem_pick_wave_line(const float* __restrict__ p, int64_t along, int B, float thr, unsigned draw, int diag) {
  const int lane = threadIdx.x & 63;
  int n = 0;
  for (int t0 = 0; t0 < B; t0 += 64) {
    const int t = t0 + lane;
    n += __popcll(__ballot(t < B && p[(int64_t)t * along] > thr));
  }
  if (n == 0) return diag;
  const int k = (int)(draw % (unsigned)n);
  int c = 0;
  for (int t0 = 0; t0 < B; t0 += 64) {
    const int t = t0 + lane;
    const bool pred = t < B && p[(int64_t)t * along] > thr;
    const unsigned long long mask = __ballot(pred);
    const int m = __popcll(mask);
    if (c + m > k) {
      const unsigned long long hit = __ballot(pred && __popcll(mask & ((1ull << lane) - 1)) == k - c);
      return t0 + __ffsll((long long)hit) - 1;
    }
    c += m;
  }
  return diag;                                               // not reached: k < n
}

// blocks [0, row_blocks): the rows of Rel;  blocks [row_blocks, ..): its columns
__global__ __launch_bounds__(SEM_THREADS) void sem_select_kernel(const float* __restrict__ S, int64_t ld, SemRel rel, int B,
                                                                 const int* __restrict__ draws, int row_blocks, int rows_by_wave,
                                                                 int cols_by_wave, int aligned, int* __restrict__ pos,
                                                                 float* __restrict__ a1, float* __restrict__ a2,
                                                                 int* __restrict__ rank, int* __restrict__ positives) {
  __shared__ int cnt[SEM_WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool is_row = (int)blockIdx.x < row_blocks;
  const int blk = is_row ? (int)blockIdx.x : (int)blockIdx.x - row_blocks;
  // a line's elements are `along` apart, neighbouring lines `across`
  const int64_t along = is_row ? rel.cs : rel.rs, across = is_row ? rel.rs : rel.cs;
  int line, p = 0;
  bool writer;
  if (is_row ? rows_by_wave : cols_by_wave) {
    line = blk * SEM_WAVES + wave;
    if (line >= B) return;                                   // wave-uniform; no barrier on this side
    p = sem_pick_wave_line(rel.p + (int64_t)line * across, along, B, rel.thr, (unsigned)draws[(is_row ? 0 : B) + line], line);
    writer = lane == 0;
  } else {
    line = blk * 64 + lane;
    const bool live = line < B;
    const float* __restrict__ q = rel.p + (int64_t)(live ? line : 0) * across;
    const int piece = (B + SEM_WAVES - 1) / SEM_WAVES;
    const int t0 = wave * piece, t1 = min(B, t0 + piece);
    int c = 0;
    for (int t = t0; t < t1; ++t) c += (live && q[(int64_t)t * along] > rel.thr) ? 1 : 0;
    cnt[wave][lane] = c;
    __syncthreads();
    if (!live) return;
    int n = 0, before = 0;
    for (int w = 0; w < SEM_WAVES; ++w) {
      const int x = cnt[w][lane];
      before += w < wave ? x : 0;
      n += x;
    }
    writer = false;
    if (n == 0) {
      p = line;
      writer = wave == 0;
    } else {
      const int k = (int)((unsigned)draws[(is_row ? 0 : B) + line] % (unsigned)n);
      if (before <= k && k < before + c) {                   // the wanted candidate lies in this wave's piece
        int cc = before;
        p = line;
        for (int t = t0; t < t1; ++t)
          if (q[(int64_t)t * along] > rel.thr) {
            if (cc == k) { p = t; break; }
            ++cc;
          }
        writer = true;
      }
    }
  }
  if (!writer) return;
  const int v = (is_row ? 0 : B) + line;
  pos[v] = p;
  if (positives) positives[v] = p;
  if (is_row) a1[line] = S[(int64_t)line * ld + p];
  else if (aligned) { a2[line] = S[(int64_t)p * ld + line]; rank[line] = line; }
}

// one wave per column j: the number of chosen cells (pos[B+j'], j') before (pos[B+j], j) in (row, column) order
__global__ __launch_bounds__(256) void sem_rank_kernel(const float* __restrict__ S, int64_t ld, int B, const int* __restrict__ pos,
                                                       float* __restrict__ a2, int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= B) return;
  const int* __restrict__ prow = pos + B;
  const int r = prow[j];
  int k = 0;
  for (int t = lane; t < B; t += 64) {
    const int rt = prow[t];
    k += (rt < r || (rt == r && t < j)) ? 1 : 0;
  }
  k = (int)wave_sum((float)k);                               // exact: k < 2^24
  if (lane == 0) { rank[j] = k; a2[k] = S[(int64_t)r * ld + j]; }
}

// HingeStats of every line: line_walk with HingeAcc, each line against its own anchor
__global__ __launch_bounds__(LINE_WALK_THREADS) void sem_stats_kernel(const float* __restrict__ S, int64_t ld, SemRel rel, int B,
                                                                      float margin, int max_violation, int mask_positives, int row_blocks,
                                                                      const float* __restrict__ a1, const float* __restrict__ a2,
                                                                      float* __restrict__ val, int* __restrict__ arg) {
  const int line = line_walk_line(B, row_blocks);
  const float anchor = line < 0 ? 0.f : line < B ? a1[line] : a2[line - B];
  line_walk<HingeAcc>(
      S, ld, B, row_blocks,
      [&](HingeAcc& acc, float s, int i, int j, int t) { acc.add(margin, s, anchor, i == j || (mask_positives && rel.above(i, j)), t); },
      [&](const HingeAcc& acc, int v) { acc.store(max_violation, val + v, arg + v); });
}

// grid line_finish_grid; dS == NULL: one block, the sum only
__global__ __launch_bounds__(256) void sem_finish_kernel(const float* __restrict__ S, int64_t ld, SemRel rel, int B, float margin,
                                                         int max_violation, int mask_positives, const float* __restrict__ val,
                                                         const int* __restrict__ arg, const int* __restrict__ pos,
                                                         const float* __restrict__ a1, const float* __restrict__ a2,
                                                         const int* __restrict__ rank, float* __restrict__ loss,
                                                         float* __restrict__ dS) {
  __shared__ float red[4];
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    const float2 t = line_sums(B, red, [&](int v) { return val[v]; });
    if (threadIdx.x == 0) *loss = t.x + t.y;
  }
  if (dS == nullptr) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= B) return;
  // the column's part, in registers: its anchor, its statistics, and the cell its anchor's gradient lands in
  const float anchor_c = a2[j];
  const float val_c = val[B + j];
  const int arg_c = arg[B + j];
  const int prow = pos[B + j];
  const int k = rank[j];
  const int ncol = max_violation ? (val[B + k] > 0.f) : arg[B + k];
  for (int i = blockIdx.y; i < B; i += gridDim.y) {
    const float anchor_r = a1[i];                            // block-uniform
    const float val_r = val[i];
    const int arg_r = arg[i];
    int g;
    if (max_violation) {
      g = (val_r > 0.f && arg_r == j) + (val_c > 0.f && arg_c == i);
      if (pos[i] == j) g -= (val_r > 0.f);
    } else {
      const float s = S[(int64_t)i * ld + j];
      const bool zero = i == j || (mask_positives && rel.above(i, j));
      g = (hinge_cost(hinge_x(margin, s, anchor_r), zero) > 0.f) + (hinge_cost(hinge_x(margin, s, anchor_c), zero) > 0.f);
      if (pos[i] == j) g -= arg_r;
    }
    if (prow == i) g -= ncol;
    dS[(int64_t)i * B + j] = (float)g;
  }
}

extern "C" size_t aladin_semantic_hinge_workspace_bytes(int B) {
  if (B < 1 || B > SEM_MAX_B) return 0;
  return (size_t)B * 9 * 4 + 256;
}

extern "C" int aladin_semantic_hinge_fwd_bwd(const float* S, int64_t ldS, const float* rel, int64_t rel_row_stride,
                                             int64_t rel_col_stride, int B, float margin, float threshold, int flags,
                                             const int32_t* draws, float* loss, float* dS, int32_t* positives, void* workspace,
                                             void* stream) {
  const int known = ALADIN_SEM_MAX_VIOLATION | ALADIN_SEM_COLUMNS_ALIGNED | ALADIN_SEM_MASK_POSITIVES;
  if (!S || !rel || !draws || !loss || !workspace || B < 1 || ldS < B || rel_row_stride < 0 || rel_col_stride < 0 || (flags & ~known) ||
      ((uintptr_t)workspace & 15)) {
    aladin_set_error("semantic_hinge_fwd_bwd: bad argument (B=%d ldS=%lld relevance strides %lld, %lld flags=%d; S, rel, draws, loss and "
                     "a 16-byte aligned workspace are required, the strides are not negative)",
                     B, (long long)ldS, (long long)rel_row_stride, (long long)rel_col_stride, flags);
    return ALADIN_ERR_ARG;
  }
  if (B > SEM_MAX_B) {
    aladin_set_error("semantic_hinge_fwd_bwd: B = %d, the limit is %d (the ranking of the column positives compares every pair of "
                     "columns)", B, SEM_MAX_B);
    return ALADIN_ERR_UNSUPPORTED;
  }
  const SemWs w = sem_ws(workspace, B);
  const SemRel r = {rel, rel_row_stride, rel_col_stride, threshold};
  const int max_violation = (flags & ALADIN_SEM_MAX_VIOLATION) != 0, aligned = (flags & ALADIN_SEM_COLUMNS_ALIGNED) != 0;
  const int mask_positives = (flags & ALADIN_SEM_MASK_POSITIVES) != 0;
  hipStream_t st = (hipStream_t)stream;
  const bool rows_by_wave = sem_wave_lines(rel_col_stride, rel_row_stride), cols_by_wave = sem_wave_lines(rel_row_stride, rel_col_stride);
  const int sel_rows = sem_line_blocks(B, rows_by_wave);
  hipLaunchKernelGGL(sem_select_kernel, dim3(sel_rows + sem_line_blocks(B, cols_by_wave)), dim3(SEM_THREADS), 0, st, S, ldS, r, B,
                     (const int*)draws, sel_rows, (int)rows_by_wave, (int)cols_by_wave, aligned, w.pos, w.a1, w.a2, w.rank,
                     (int*)positives);
  if (int rc = aladin_check_launch("sem_select_kernel")) return rc;
  if (!aligned) {
    hipLaunchKernelGGL(sem_rank_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, S, ldS, B, (const int*)w.pos, w.a2, w.rank);
    if (int rc = aladin_check_launch("sem_rank_kernel")) return rc;
  }
  hipLaunchKernelGGL(sem_stats_kernel, dim3(line_walk_blocks(B)), dim3(LINE_WALK_THREADS), 0, st, S, ldS, r, B, margin, max_violation,
                     mask_positives, line_row_blocks(B), (const float*)w.a1, (const float*)w.a2, w.val, w.arg);
  if (int rc = aladin_check_launch("sem_stats_kernel")) return rc;
  hipLaunchKernelGGL(sem_finish_kernel, line_finish_grid(B, dS != nullptr), dim3(256), 0, st, S, ldS, r, B, margin, max_violation,
                     mask_positives, (const float*)w.val, (const int*)w.arg, (const int*)w.pos, (const float*)w.a1, (const float*)w.a2,
                     (const int*)w.rank, loss, dS);
  return aladin_check_launch("sem_finish_kernel");
}
