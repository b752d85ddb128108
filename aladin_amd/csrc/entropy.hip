// The 'entropy' loss term: nearest-neighbour uniformity of the matching head's embeddings, reference
// alad/alad_model.py:17-27 (pairwise_NNs_inner) and :410-421.  Row r of the virtual N x D matrix all_emb is img[r] for
// r < Bi and cap[r - Bi] otherwise (cap == NULL: N = Bi, one source); no concatenated copy exists.
//   forward, three launches on the caller's stream:
//     nn_gram_kernel    one workgroup per 64 x 64 tile of all_emb @ all_emb.T, in exact fp32 (sgemm_tile_64).  The grid walks
//                       the tiles of each source separately, so a tile never straddles img and cap; its epilogue sets the
//                       diagonal to -1.0f and reduces every row over the tile's columns to (max, index): one partial per
//                       (row, column tile).  The Gram matrix itself is never stored.
//     nn_rows_kernel    one wave per row: merges the row's partials, stores nn[i], recomputes u = x_i - x_nn + 1e-6f and
//                       dist_i = sqrt(sum u^2), stores dist_i and the row's term log(N * dist_i).
//     nn_loss_kernel    one workgroup: loss = -(sum of the terms) / N.
//   backward, one launch: nn_bwd_kernel, one wave per OUTPUT row j (a gather): its own c_j * u_j, minus c_i * u_i of every
//     row i with nn[i] == j in ascending i; c_i = -g / (N * dist_i^2), g read from a device scalar.
// Ties go to the lowest index at every level (lanes, waves, column tiles): ALADIN_ARGMAX_STEP is commutative and associative,
// so the merge order does not matter and the result is the lowest index attaining the row's maximum.  Duplicate rows give
// bit-equal products wherever their columns lie: a product's fma chain depends on K alone (sgemm_tile.hpp).
// Every sum runs in a fixed order and nothing is accumulated with atomics: the same input gives the same bits.
#include "../../include/aladin_hip.h"
#include "common.hpp"
#include "sgemm_tile.hpp"

// No contraction below this line: the backward adds c * u to a row and subtracts c * u from its neighbour's row as separately rounded
// products, so that a self-neighbour row comes out exactly 0 (a fused multiply-subtract would leave the product's rounding error);
// the fma chains that are wanted are written as fmaf.  (The __fmul_rn / __fsub_rn intrinsics are plain operators to the compiler
// and contract like them.)
#pragma clang fp contract(off)

#define NN_MAX_N ALADIN_NN_ENTROPY_MAX_N     // the partial buffer is N * tiles * 8 B = 128 MiB there
#define NN_EPS 1e-6f                   // nn.PairwiseDistance's eps, added to the difference inside the norm

struct NNPartial { float v; int idx; };

struct NNSources {
  const float* img; int64_t ld_img; int Bi;
  const float* cap; int64_t ld_cap; int Bc;
  __device__ __forceinline__ const float* row(int r) const { return r < Bi ? img + (int64_t)r * ld_img : cap + (int64_t)(r - Bi) * ld_cap; }
};

static inline int nn_tiles(int Bi, int Bc) { return cdiv(Bi, 64) + cdiv(Bc, 64); }

__global__ __launch_bounds__(1024) void nn_gram_kernel(NNSources s, int D, NNPartial* __restrict__ partial, int n_tiles) {
  extern __shared__ __attribute__((aligned(16))) char sg_smem[];
  const int ti = (s.Bi + 63) / 64;
  const int rsrc = (int)blockIdx.y >= ti, csrc = (int)blockIdx.x >= ti;
  const int m0 = ((int)blockIdx.y - (rsrc ? ti : 0)) * 64, n0 = ((int)blockIdx.x - (csrc ? ti : 0)) * 64;
  const int M = rsrc ? s.Bc : s.Bi, Nc = csrc ? s.Bc : s.Bi;
  const int rbase = rsrc ? s.Bi : 0, cbase = csrc ? s.Bi : 0;          // global index of the sources' first rows
  f32x16 acc;
  const bool own = sgemm_tile_64(M, Nc, D, rsrc ? s.cap : s.img, rsrc ? s.ld_cap : s.ld_img, 1, csrc ? s.cap : s.img, 1,
                                 csrc ? s.ld_cap : s.ld_img, m0, n0, sg_smem, acc);
  const int wave = (threadIdx.x & 255) >> 6, lane = threadIdx.x & 63;
  const int wm = wave >> 1, wn = wave & 1;
  NNPartial* right = reinterpret_cast<NNPartial*>(sg_smem);            // [64 tile rows]: the best of columns 32..63
  float mv = -INFINITY;
  int mi = 0x7fffffff;
  if (own) {
    const int col = n0 + wn * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      float v = acc[r];
      int idx = cbase + col;
      if (rbase + row == idx) v = -1.0f;                               // the reference's diagonal fill: -1, not -inf
      if (col >= Nc) { v = -INFINITY; idx = 0x7fffffff; }
      half_wave_argmax(v, idx);                                        // this half-wave holds one row of the accumulator
      if ((lane & 31) == r) { mv = v; mi = idx; }                      // lane r of each half keeps register r's row
    }
  }
  const int r = lane & 31;
  const int lrow = wm * 32 + (r & 3) + 8 * ((r & 15) >> 2) + 4 * (lane >> 5);
  if (own && wn == 1 && r < 16) { right[lrow].v = mv; right[lrow].idx = mi; }
  __syncthreads();
  if (own && wn == 0 && r < 16 && m0 + lrow < M) {
    float v = mv;
    int idx = mi;
    ALADIN_ARGMAX_STEP(right[lrow].v, right[lrow].idx);
    NNPartial p; p.v = v; p.idx = idx;
    partial[(size_t)(rbase + m0 + lrow) * n_tiles + blockIdx.x] = p;
  }
}

// 256 threads = 4 rows
__global__ __launch_bounds__(256) void nn_rows_kernel(NNSources s, int D, const NNPartial* __restrict__ partial, int n_tiles,
                                                      int32_t* __restrict__ nn, float* __restrict__ dist, float* __restrict__ term) {
  const int N = s.Bi + s.Bc, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  float v = -INFINITY;
  int idx = 0x7fffffff;
  for (int t = lane; t < n_tiles; t += 64) {
    const NNPartial p = partial[(size_t)i * n_tiles + t];
    ALADIN_ARGMAX_STEP(p.v, p.idx);
  }
  wave_argmax(v, idx);
  if ((unsigned)idx >= (unsigned)N) idx = i;          // a row of NaN products compares with nothing: it reports itself, in bounds
  const float* xi = s.row(i);
  const float* xn = s.row(idx);
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float u = xi[d] - xn[d] + NN_EPS;
    ss = fmaf(u, u, ss);
  }
  ss = wave_sum(ss);
  if (lane == 0) {
    const float ds = sqrtf(ss);
    nn[i] = idx;
    dist[i] = ds;
    term[i] = logf((float)N * ds);
  }
}

__global__ __launch_bounds__(256) void nn_loss_kernel(const float* __restrict__ term, int N, float* __restrict__ loss) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int t = threadIdx.x; t < N; t += 256) acc += term[t];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *loss = -(acc / (float)N);
}

// 256 threads = 4 output rows; a wave keeps 256 columns of its row in registers at a time and scans nn[] once per such chunk.
__global__ __launch_bounds__(256) void nn_bwd_kernel(NNSources s, int D, const int32_t* __restrict__ nn, const float* __restrict__ dist,
                                                     const float* __restrict__ gscale, float* __restrict__ d_img, float* __restrict__ d_cap) {
  const int N = s.Bi + s.Bc, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= N) return;
  float* out = j < s.Bi ? d_img + (int64_t)j * D : d_cap + (int64_t)(j - s.Bi) * D;
  const float* xj = s.row(j);
  const float k = -(*gscale) / (float)N;
  const int nj = nn[j];
  const bool own = (unsigned)nj < (unsigned)N;
  const float* xnj = s.row(own ? nj : j);
  const float dj = dist[j];
  const float cj = k / (dj * dj);
  for (int d0 = 0; d0 < D; d0 += 256) {
    float x[4], acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = d0 + lane + 64 * q;
      x[q] = d < D ? xj[d] : 0.f;
      acc[q] = (own && d < D) ? cj * (x[q] - xnj[d] + NN_EPS) : 0.f;
    }
    for (int i0 = 0; i0 < N; i0 += 64) {
      const int i = i0 + lane;
      unsigned long long m = __ballot(i < N && nn[i] == j);
      while (m) {                                                      // ascending i
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int src = i0 + b;
        const float* xs = s.row(src);
        const float dsrc = dist[src];
        const float cs = k / (dsrc * dsrc);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int d = d0 + lane + 64 * q;
          if (d < D) acc[q] = acc[q] - cs * (xs[d] - x[q] + NN_EPS);          // not contracted: see the pragma
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = d0 + lane + 64 * q;
      if (d < D) out[d] = acc[q];
    }
  }
}

static size_t nn_partial_bytes(int N, int n_tiles) { return ((size_t)N * n_tiles * sizeof(NNPartial) + 255) / 256 * 256; }

extern "C" size_t aladin_nn_entropy_workspace_bytes(int N) {
  if (N < 1 || N > NN_MAX_N) return 0;
  const int half = (N + 1) / 2;
  return nn_partial_bytes(N, nn_tiles(half, half)) + (size_t)N * sizeof(float);      // two sources need the most tiles
}

static int nn_check(const char* what, const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, int B, int D) {
  if (!img || B < 1 || D < 1 || (B > 1 && ld_img < D) || (cap && B > 1 && ld_cap < D)) {
    aladin_set_error("%s: bad argument (B=%d D=%d ld_img=%lld ld_cap=%lld)", what, B, D, (long long)ld_img, (long long)ld_cap);
    return ALADIN_ERR_ARG;
  }
  const int64_t N = (int64_t)B * (cap ? 2 : 1);
  if (N > NN_MAX_N) {
    aladin_set_error("%s: N = %lld rows, the limit is %d (the per-tile partial maxima of the neighbour search)", what, (long long)N, NN_MAX_N);
    return ALADIN_ERR_UNSUPPORTED;
  }
  return ALADIN_OK;
}

extern "C" int aladin_nn_entropy_fwd(const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, int B, int D, float* loss,
                                     int32_t* nn, float* dist, void* workspace, void* stream) {
  if (int rc = nn_check("nn_entropy_fwd", img, ld_img, cap, ld_cap, B, D)) return rc;
  if (!nn || !dist || !workspace) { aladin_set_error("nn_entropy_fwd: null nn / dist / workspace"); return ALADIN_ERR_ARG; }
  const NNSources s = {img, ld_img, B, cap, ld_cap, cap ? B : 0};
  const int N = s.Bi + s.Bc, T = nn_tiles(s.Bi, s.Bc);
  NNPartial* partial = (NNPartial*)workspace;
  float* term = (float*)((char*)workspace + nn_partial_bytes(N, T));
  hipStream_t st = (hipStream_t)stream;
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)nn_gram_kernel, SG_LDS_BYTES, &lds_reserved, "nn_entropy_fwd")) return rc;
  hipLaunchKernelGGL(nn_gram_kernel, dim3(T, T), dim3(1024), SG_LDS_BYTES, st, s, D, partial, T);
  if (int rc = aladin_check_launch("nn_gram_kernel")) return rc;
  hipLaunchKernelGGL(nn_rows_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, s, D, partial, T, nn, dist, term);
  if (int rc = aladin_check_launch("nn_rows_kernel")) return rc;
  if (!loss) return ALADIN_OK;
  hipLaunchKernelGGL(nn_loss_kernel, dim3(1), dim3(256), 0, st, term, N, loss);
  return aladin_check_launch("nn_loss_kernel");
}

extern "C" int aladin_nn_entropy_bwd(const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, int B, int D, const int32_t* nn,
                                     const float* dist, const float* gscale, float* d_img, float* d_cap, void* stream) {
  if (int rc = nn_check("nn_entropy_bwd", img, ld_img, cap, ld_cap, B, D)) return rc;
  if (!nn || !dist || !gscale || !d_img || (cap && !d_cap)) { aladin_set_error("nn_entropy_bwd: null nn / dist / gscale / output"); return ALADIN_ERR_ARG; }
  const NNSources s = {img, ld_img, B, cap, ld_cap, cap ? B : 0};
  hipLaunchKernelGGL(nn_bwd_kernel, dim3(cdiv(s.Bi + s.Bc, 4)), dim3(256), 0, (hipStream_t)stream, s, D, nn, dist, gscale, d_img, d_cap);
  return aladin_check_launch("nn_bwd_kernel");
}
