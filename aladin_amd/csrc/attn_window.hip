// Head-mean attention window (aladin_attn_window_mean): from one BERT layer's query(x) / key(x) outputs, the mean over heads of
// softmax_j(<q_i, k_j> / sqrt(dh) + (1 - mask_j) * -10000) for the rows [row0, row0 + W) and the columns [col0, col0 + Rw) -- what the
// cross-encoder teacher (reference alad/train.py:340-384) cuts out of `attention[-1].mean(dim=1)` after asking every layer for its
// (N, H, L, L) probabilities (oscar/modeling/modeling_bert.py:47-53).  The probabilities never exist here: a 16-row tile's logit
// strip over ALL L columns lives in one wave's accumulators, the head sum of the window's columns in another register set.
// include/aladin_hip.h states the formula.
//
// attn_window_kernel<NT>: workgroup = one sequence, one wave per 16-row query tile that meets the row window (at most AW_MAX_WAVES
// at a time: a taller window takes several passes).  Per head the workgroup stages the head's K panel (L x dh fp32, pitch dh + 1
// floats: the 64 lanes of a B-operand read fall into 64 banks) in LDS once for all of its row tiles; a wave keeps its tile's q rows
// of the head in registers.  Logits: v_mfma_f32_16x16x4_f32 on the raw fp32 values, as attdistill.hip's backward uses it
// (A: lane -> (row lane & 15, k-slot lane >> 4), B: lane -> (k-slot lane >> 4, column lane & 15)).  The contraction index is
// PERMUTED: the lane of k-slot s holds the dh / 4 CONSECUTIVE features [s * dh / 4, (s + 1) * dh / 4) of its row, so a q row is
// read as contiguous (16-byte where the address allows) loads; A and B use the same permutation, the sum runs over the same
// products in a fixed order.
// acc[ct][reg] = S[row tile * 16 + 4 * (lane >> 4) + reg][column ct * 16 + (lane & 15)]: a row's columns sit in one lane's
// registers across ct and in the 16 lanes of its DPP row, so the row maximum and the row sum are in-lane loops plus row16_max /
// row16_sum (no serial lane walks through LDS).  The additive mask is ADDED (a sequence whose mask is all zero keeps a finite
// softmax over its raw scores, as the reference's); columns at or past L do not exist and are selected away.  Heads are summed in
// the order 0 .. H - 1 and divided by H once; every output element is written exactly once by the lane that owns it: no atomics,
// no workspace, bit-reproducible.
#include "../../include/aladin_hip.h"

#include "common.hpp"
#include "sim_common.hpp"

// No contraction: s - max must subtract the ROUNDED logit (the value the maximum was taken over), or the row's largest
// exponential is exp(rounding residual) instead of exactly 1.
#pragma clang fp contract(off)

constexpr int AW_MAX_WAVES = 8;
constexpr int AW_LDS_LIMIT = 160 * 1024;

struct AwArgs {
  const float* q; int64_t q_sn, q_sr;       // strides in floats
  const float* k; int64_t k_sn, k_sr;
  const void* mask; int64_t m_sn;           // (N, L), unit inner stride; int64 or fp32
  float* out; int64_t o_sn, o_sr;
  int L, H, dh, row0, W, col0, Rw;
  int mask_i64, vec_q, vec_k;               // vec_*: every row of the tensor starts 16-byte aligned and dh % 16 == 0 / dh % 4 == 0
  float sqrt_dh, heads;
};

// features [s0, s0 + 4) of a lane's dq (zeros at and past dq); vec: one 16-byte load (dq % 4 == 0 and aligned rows)
__device__ __forceinline__ void aw_load_q4(float (&v)[4], const float* __restrict__ src, int s0, int dq, bool vec) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(src + s0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = s0 + e < dq ? src[s0 + e] : 0.f;
  }
}

template <int NT>
__global__ __launch_bounds__(AW_MAX_WAVES * 64) void attn_window_kernel(AwArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kp[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nw = blockDim.x >> 6;
  const int n = blockIdx.x;
  const int L = a.L, dh = a.dh, dq = dh >> 2, pitch = dh + 1;
  const int nct = (L + 15) >> 4;                                  // column tiles in use, <= NT
  const int rt_lo = a.row0 >> 4, rt_hi = (a.row0 + a.W - 1) >> 4;
  const int ct_lo = a.col0 >> 4, ct_hi = (a.col0 + a.Rw - 1) >> 4;
  const int col = lane & 15, slot = lane >> 4;

  // the additive mask of this lane's columns, once per sequence: (1 - m) * -10000, exactly as the reference forms it
  float madd[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const int j = ct * 16 + col;
    madd[ct] = 0.f;
    if (ct < nct && j < L) {
      const float m = a.mask_i64 ? (float)(reinterpret_cast<const long long*>(a.mask)[n * a.m_sn + j])
                                 : reinterpret_cast<const float*>(a.mask)[n * a.m_sn + j];
      madd[ct] = (1.0f - m) * -10000.0f;
    }
  }

  const float* const qn = a.q + n * a.q_sn;
  const float* const kn = a.k + n * a.k_sn;
  for (int rt0 = rt_lo; rt0 <= rt_hi; rt0 += nw) {
    const int rt = rt0 + wave;
    const bool active = rt <= rt_hi;                              // wave-uniform
    const int qrow = min(rt * 16 + col, L - 1);                   // rows past L are computed on row L - 1 and never stored
    f32x4 osum[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) osum[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int h = 0; h < a.H; ++h) {
      __syncthreads();                                            // every wave is done with the previous panel
      // ---- the head's K panel: rows [0, L) x dh, rows up to nct * 16 zero
      {
        const int chunks = nct * 16 * dq;                         // 4 floats each
        for (int c = threadIdx.x; c < chunks; c += blockDim.x) {
          const int r = c / dq, c4 = (c - r * dq) * 4;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (r < L) {
            const float* src = kn + (int64_t)r * a.k_sr + h * dh + c4;
            if (a.vec_k) v = *reinterpret_cast<const float4*>(src);
            else { v.x = src[0]; v.y = src[1]; v.z = src[2]; v.w = src[3]; }
          }
          float* dst = kp + r * pitch + c4;
          dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
      }
      __syncthreads();
      if (!active) continue;                                      // wave-uniform; the barriers above are reached by every wave

      // ---- logits of the 16 rows against all columns: the lane's k-slot walks its dq consecutive features four at a time (a
      // group past dq multiplies zeros), the next group of the q row in flight under the current group's MFMAs
      f32x4 acc[NT];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* const qsrc = qn + (int64_t)qrow * a.q_sr + h * dh + slot * dq;
      const float* const kb = kp + col * pitch + slot * dq;
      float qnext[4];
      aw_load_q4(qnext, qsrc, 0, dq, a.vec_q);
      for (int s0 = 0; s0 < dq; s0 += 4) {
        float qv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) qv[e] = qnext[e];
        if (s0 + 4 < dq) aw_load_q4(qnext, qsrc, s0 + 4, dq, a.vec_q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool kv = s0 + e < dq;
#pragma unroll
          for (int ct = 0; ct < NT; ++ct) {
            if (ct >= nct) continue;
            const float b = kb[ct * 16 * pitch + (kv ? s0 + e : 0)];
            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(qv[e], kv ? b : 0.f, acc[ct], 0, 0, 0);
          }
        }
      }

      // ---- softmax over the L columns, per register row; the window's column tiles join the head sum
      float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if (ct >= nct) continue;
        const bool in = ct * 16 + col < L;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          acc[ct][reg] = acc[ct][reg] / a.sqrt_dh + madd[ct];
          mx[reg] = fmax_nc(mx[reg], in ? acc[ct][reg] : -INFINITY);
        }
      }
      float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) mx[reg] = row16_max(mx[reg]);
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if (ct >= nct) continue;
        const bool in = ct * 16 + col < L;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          acc[ct][reg] = in ? expf(acc[ct][reg] - mx[reg]) : 0.f;
          sum[reg] += acc[ct][reg];
        }
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sum[reg] = row16_sum(sum[reg]);
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if (ct < ct_lo || ct > ct_hi) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) osum[ct][reg] += acc[ct][reg] / sum[reg];
      }
    }

    // ---- the window's elements of this row tile, each by the lane that holds it
    if (!active) continue;
    float* const on = a.out + n * a.o_sn;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      if (ct < ct_lo || ct > ct_hi) continue;
      const int j = ct * 16 + col - a.col0;
      if (j < 0 || j >= a.Rw) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = rt * 16 + 4 * slot + reg - a.row0;
        if (i >= 0 && i < a.W) on[(int64_t)i * a.o_sr + j] = osum[ct][reg] / a.heads;
      }
    }
  }
}

static bool aw_rows_aligned(const float* p, int64_t sn, int64_t sr) { return ((uintptr_t)p & 15) == 0 && sn % 4 == 0 && sr % 4 == 0; }

template <int NT>
static int aw_launch(const AwArgs& a, int N, int nw, int lds, hipStream_t st) {
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)attn_window_kernel<NT>, AW_LDS_LIMIT, &lds_reserved, "attn_window_kernel")) return rc;
  hipLaunchKernelGGL(attn_window_kernel<NT>, dim3((unsigned)N), dim3(nw * 64), lds, st, a);
  return aladin_check_launch("attn_window_kernel");
}

extern "C" int aladin_attn_window_mean(const float* q, int64_t q_sn, int64_t q_sr, const float* k, int64_t k_sn, int64_t k_sr,
                                       const void* mask, int mask_ndim, int mask_is_int64, int64_t mask_sn, int N, int L, int H, int dh,
                                       int row0, int W, int col0, int Rw, float* out, int64_t o_sn, int64_t o_sr, void* stream) {
  if (!q || !k || !mask || !out || N < 1 || L < 1 || H < 1 || dh < 1 || mask_ndim != 2) {
    aladin_set_error("attn_window_mean: bad argument (N=%d L=%d H=%d dh=%d, a %d-D mask; q, k, out and a 2-D (N, L) mask are required)",
                     N, L, H, dh, mask_ndim);
    return ALADIN_ERR_ARG;
  }
  if (L > ALADIN_ATTN_WINDOW_MAX_L || H > ALADIN_ATTN_WINDOW_MAX_HEADS || dh > ALADIN_ATTN_WINDOW_MAX_DH || dh % 4) {
    aladin_set_error("attn_window_mean: L <= %d, H <= %d, dh a multiple of 4 up to %d expected, got L=%d H=%d dh=%d",
                     ALADIN_ATTN_WINDOW_MAX_L, ALADIN_ATTN_WINDOW_MAX_HEADS, ALADIN_ATTN_WINDOW_MAX_DH, L, H, dh);
    return ALADIN_ERR_ARG;
  }
  if (row0 < 0 || W < 1 || row0 > L - W || col0 < 0 || Rw < 1 || col0 > L - Rw) {
    aladin_set_error("attn_window_mean: the window rows [%d, %d + %d) x columns [%d, %d + %d) must be non-empty and lie inside L=%d",
                     row0, row0, W, col0, col0, Rw, L);
    return ALADIN_ERR_ARG;
  }
  const int64_t row_w = (int64_t)H * dh;
  if (q_sr < row_w || k_sr < row_w || q_sn < 0 || k_sn < 0 || mask_sn < 0 || o_sr < Rw || o_sn < 0 || (N > 1 && (o_sn < (int64_t)W * o_sr)) ||
      ((uintptr_t)q & 3) || ((uintptr_t)k & 3) || ((uintptr_t)out & 3)) {
    aladin_set_error("attn_window_mean: q / k rows hold H * dh = %lld floats (row strides %lld / %lld), out rows %d (strides %lld, %lld); "
                     "4-byte aligned pointers and non-overlapping output rows are required",
                     (long long)row_w, (long long)q_sr, (long long)k_sr, Rw, (long long)o_sn, (long long)o_sr);
    return ALADIN_ERR_ARG;
  }
  AwArgs a{q, q_sn, q_sr, k, k_sn, k_sr, mask, mask_sn, out, o_sn, o_sr, L, H, dh, row0, W, col0, Rw, mask_is_int64 != 0,
           aw_rows_aligned(q, q_sn, q_sr) && dh % 16 == 0, aw_rows_aligned(k, k_sn, k_sr), (float)sqrt((double)dh), (float)H};
  const int nct = cdiv(L, 16);
  const int nrt = ((row0 + W - 1) >> 4) - (row0 >> 4) + 1;
  const int nw = nrt < AW_MAX_WAVES ? nrt : AW_MAX_WAVES;
  const int lds = nct * 16 * (dh + 1) * 4;
  hipStream_t st = (hipStream_t)stream;
  if (nct <= 4) return aw_launch<4>(a, N, nw, lds, st);
  if (nct <= 9) return aw_launch<9>(a, N, nw, lds, st);
  return aw_launch<16>(a, N, nw, lds, st);
}
