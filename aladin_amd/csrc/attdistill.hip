// Attention distillation (aladin_attdistill_fwd / _bwd): the KL divergence between a teacher's word-by-region attention and the
// softmax over regions of the scaled dot products <s_seq[j, w + 1], im_set[i, r + 1]> / sqrt(D), for EVERY (image, caption) pair;
// reference alad/loss.py:273-334 (AttentionDistillationLoss).  The (Bi, Bc, R', T') logits tensor of the reference never exists:
// a pair's block lives in one wave's accumulators, forward and backward.  include/aladin_hip.h states the formulas.
//
// Operands (attdistill_pack_kernel, the row encoders of pack_rows.hpp): every scored row as a UNIT row in split precision,
// [hi | lo] fp16 halves of x^ * 2^14 (2 Dp halfs, the evaluation store's row), plus its fp32 norm; a sample's rows are contiguous
// ([i * Rq, (i + 1) * Rq) / [j * Tq, (j + 1) * Tq)); masked positions are zero rows with norm 0.  A raw row is never rounded to
// fp16: its norm stays in fp32 and joins the dot product in the epilogue.  Plain fp16 unit rows are not enough for THIS loss:
// the softmax turns a logit's absolute error into a relative one of the gradient, and at logits of +-50 the gradients moved by
// 1.0e-3 of their largest entry against the project's 5e-4 (tests/test_attdistill_cpu.py measures both); the split chain
// hi.hi, lo.hi, hi.lo leaves ~2^-22.
//
// Forward (attdistill_fwd_kernel): workgroup = one image x a chunk of NW captions, one wave per pair.  attdistill_pair_dots is
// rescore_kernel's main loop: LDS-DMA panels with the gemm_core.hpp swizzle, double buffered, rows past a count clamped and
// SELECTED, v_mfma_f32_16x16x32_f16, KMapSplit's chain in one fp32 accumulator.
// acc[rt][ct][reg] = <region rt * 16 + 4 * (lane >> 4) + reg, word ct * 16 + (lane & 15)>: a word's regions sit in one lane's
// registers and in the lanes ^ 16, ^ 32, so the log-sum-exp over regions, the teacher's L1 norm and the KL sum are in-lane loops
// plus lane_xor16 / lane_xor32, and a lane's four consecutive regions of the teacher are one 16-byte load where the address
// allows.  Per (i, j, w) the kernel leaves (LSE, 1 / L1, sigma) in the workspace, per pair one double partial;
// attdistill_finish_kernel sums the partials in a fixed order, counts N = Bi * sum_j m_j on the device and writes the loss.
//
// Backward (attdistill_bwd_kernel, ONE launch): two passes, each OWNING its output -- blockIdx.z = 0 walks the images for
// d im_set, 1 the captions for d s_seq (attdistill_bwd_body<IMG>) -- times chunks of 128 feature columns.  A workgroup of four
// waves walks the partners four at a time: each wave recomputes one pair's logits (the forward's code, the same bits) and forms
// g = softmax * sigma - P in its registers from the saved LSE; then the four pairs take turns in ONE fp32 tile G[r][w] in LDS
// and all four waves run the second product on it, each on its own 32 feature columns:
//   out[r][d] += sum_w G[r][w] * s_seq[j, w + 1, d] (IMG)   or   out[w][d] += sum_r G[r][w] * im_set[i, r + 1, d],
// v_mfma_f32_16x16x4_f32 with the partner's RAW fp32 rows as the B operand.  g is never rounded to 16 bits and the second
// operand is exact, so the gradient carries the rounding of the unit rows in the logits and nothing else (DESIGN.md 4.3.1 says
// why this departs from a 16-bit second product, and what it costs: the logits are recomputed once per column chunk).
// 1 / (N sqrt(D)) and the upstream gradient (a device scalar) are applied once, in fp32, on the way out.  Every output row is
// written exactly once -- slot 0 and masked positions as zeros -- no atomics, a fixed order everywhere.
#include "../../include/aladin_hip.h"

#include "pack_rows.hpp"
#include "sim_common.hpp"

// No contraction: the backward must see the forward's ROUNDED logit.  Contracted, x * |y| - LSE becomes an fma on the unrounded
// product, and a word whose softmax equals its teacher row (an image with one region: both are 1) gets
// exp(rounding residual) * sigma - P = -2^-24 for a gradient that is exactly 0; the same holds for x - max in the forward.
#pragma clang fp contract(off)

constexpr int AD_MAX_COUNT = ALADIN_TILE_MAX_SCORED;      // six 16-row tiles per side
constexpr int AD_TILES = AD_MAX_COUNT / 16;
constexpr int AD_LDS_LIMIT = 160 * 1024;
constexpr int AD_BWD_WAVES = 4;
constexpr int AD_BWD_CT = 3;                              // 16-column tiles of the output per wave
constexpr int AD_BWD_COLS = AD_BWD_WAVES * AD_BWD_CT * 16;

struct AdSide {
  const float* data;       // the fp32 set and its strides in floats
  int64_t sb, sr;
  const int32_t* len;
  const half_t* rows;      // packed unit rows [hi | lo], Q per sample, and their norms
  const float* norm;
  int B, Q;                // samples; scored positions per sample (R - 1 / T - 1)
  int prows;               // LDS rows of one panel: round_up(Q, 16)
};

struct AdTeacher {
  const float* data;
  int64_t si, sj, sw;      // strides in floats; the regions are contiguous
};

__device__ __forceinline__ int ad_count(const AdSide& s, int k) { return scored_len(s.len[k], 0, s.Q); }

// field by field: selecting whole kernel-argument structs by a run-time value would send them through scratch memory
__device__ __forceinline__ AdSide ad_pick(bool first, const AdSide& a, const AdSide& b) {
  return AdSide{first ? a.data : b.data, first ? a.sb : b.sb, first ? a.sr : b.sr, first ? a.len : b.len, first ? a.rows : b.rows,
                first ? a.norm : b.norm, first ? a.B : b.B, first ? a.Q : b.Q, first ? a.prows : b.prows};
}

// ------------------------------------------------------------------------------------------------
// operands
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attdistill_pack_kernel(AdSide x, AdSide y, int D, int Dp, half_t* __restrict__ xh,
                                                              float* __restrict__ xn, half_t* __restrict__ yh, float* __restrict__ yn,
                                                              int vec_x, int vec_y) {
  const int lane = threadIdx.x & 63;
  int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);                // over [Bi * Rq | Bc * Tq]
  const int64_t nx = (int64_t)x.B * x.Q;
  const bool cap = d >= nx;
  if (cap) d -= nx;
  const AdSide s = ad_pick(!cap, x, y);
  if (d >= (int64_t)s.B * s.Q) return;
  const int k = (int)(d / s.Q), p = (int)(d % s.Q);                        // position p + 1 of the set
  half_t* dst = (cap ? yh : xh) + d * 2 * Dp;
  float* nslot = (cap ? yn : xn) + d;
  if (p >= ad_count(s, k)) {
    write_zero_row(dst, 2 * Dp, lane);
    if (lane == 0) *nslot = 0.f;
    return;
  }
  const float* src = s.data + k * s.sb + (int64_t)(p + 1) * s.sr;
  const bool vec4 = (cap ? vec_y : vec_x) != 0;
  const float inv = inv_norm_mem(src, D, lane, vec4);
  write_split(dst, nullptr, dst + Dp, src, inv, D, Dp, lane);                // [hi | lo]
  if (lane == 0) *nslot = 1.0f / inv;
}

// ------------------------------------------------------------------------------------------------
// one wave, one pair: the unit dot products (rescore_kernel's loop; the image is the A operand, the caption the B operand)
// sh / ga: the panel the workgroup shares and the one this wave brings; img_shared says which of them is the image.
// Every wave of the workgroup calls this together (one barrier per K step).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void attdistill_pair_dots(f32x4 (&acc)[AD_TILES][AD_TILES], const half_t* pan_s, int cnt_s, int sh_prows,
                                                     const half_t* pan_g, int cnt_g, int ga_prows, bool img_shared, int nrt, int nct,
                                                     int64_t ldk, int kps, char* smem, int wave, int nw, int lane) {
  const int stage_bytes = (sh_prows + nw * ga_prows) * 128;
  const int g_row0 = sh_prows + wave * ga_prows;
  const int a_row0 = (img_shared ? 0 : g_row0) + (lane & 15), b_row0 = (img_shared ? g_row0 : 0) + (lane & 15);
#pragma unroll
  for (int rt = 0; rt < AD_TILES; ++rt)
#pragma unroll
    for (int ct = 0; ct < AD_TILES; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the split chain hi.hi, lo.hi, hi.lo (a = image, b = caption); the shared / gathered panels take the K offset of their side
  const KMapSplit km{kps, 0};
  const int ktiles = 3 * kps;
  auto k_sh = [&](int kt) { return img_shared ? km.a(kt) : km.b(kt); };
  auto k_ga = [&](int kt) { return img_shared ? km.b(kt) : km.a(kt); };
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
      half8 a[AD_TILES], b[AD_TILES];
#pragma unroll
      for (int t = 0; t < AD_TILES; ++t) {
        a[t] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        b[t] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        if (t < nrt) a[t] = lds_frag16(cur, a_row0 + t * 16, k32, lane);
        if (t < nct) b[t] = lds_frag16(cur, b_row0 + t * 16, k32, lane);
      }
#pragma unroll
      for (int rt = 0; rt < AD_TILES; ++rt) {
        if (rt >= nrt) continue;
#pragma unroll
        for (int ct = 0; ct < AD_TILES; ++ct)
          if (ct < nct) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
      }
    }
  }
}

// unit dot products (scaled by 2^28: split rows) -> logits without the word's norm: rows times
// |im_set[i, r + 1]| / sqrt(D) / 2^28.  (The word's norm joins per
// column tile: ad_word_norm.)  Forward and backward run the same two multiplications in the same order.
__device__ __forceinline__ void ad_scale_rows(f32x4 (&acc)[AD_TILES][AD_TILES], const float* __restrict__ xnorm, int Rq, int nrt,
                                              float inv_sqrt_d, int lane) {
#pragma unroll
  for (int rt = 0; rt < AD_TILES; ++rt) {
    if (rt >= nrt) continue;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = rt * 16 + 4 * (lane >> 4) + reg;
      const float f = xnorm[min(r, Rq - 1)] * inv_sqrt_d * ALADIN_SPLIT_UNSCALE;
#pragma unroll
      for (int ct = 0; ct < AD_TILES; ++ct) acc[rt][ct][reg] *= f;
    }
  }
}

// a lane's four consecutive regions r0 .. r0 + 3 of one teacher row (regions at or past Rq: 0); on == false: nothing is read
__device__ __forceinline__ void ad_teacher4(float (&a)[4], const float* __restrict__ row, int r0, int Rq, bool on) {
  a[0] = a[1] = a[2] = a[3] = 0.f;
  if (!on || r0 >= Rq) return;
  const float* p = row + r0;
  if (r0 + 3 < Rq && ((uintptr_t)p & 15) == 0) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
  } else {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      if (r0 + reg < Rq) a[reg] = p[reg];
  }
}

// sum over a word's regions: the lanes ^ 16 and ^ 32 hold the other twelve rows of each tile (a + b == b + a: the four agree)
__device__ __forceinline__ float ad_region_sum(float v) {
  v += lane_xor16(v);
  v += lane_xor32(v);
  return v;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void attdistill_fwd_kernel(AdSide x, AdSide y, AdTeacher t, int64_t ldk, int kps, float inv_sqrt_d,
                                                             float4* __restrict__ stats, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nw = blockDim.x >> 6;
  const int nchunk = (y.B + nw - 1) / nw;
  const int i = blockIdx.x / nchunk;
  const int j = (blockIdx.x - i * nchunk) * nw + wave;
  const bool live = j < y.B;
  const int n_i = __builtin_amdgcn_readfirstlane(ad_count(x, i));
  const int m_j = __builtin_amdgcn_readfirstlane(live ? ad_count(y, j) : 0);
  const bool work = n_i > 0 && m_j > 0;                                          // wave-uniform
  const int nrt = work ? (n_i + 15) >> 4 : 0, nct = work ? (m_j + 15) >> 4 : 0;
  const int Rq = x.Q, Tq = y.Q;

  f32x4 acc[AD_TILES][AD_TILES];
  attdistill_pair_dots(acc, x.rows + (int64_t)i * Rq * ldk, n_i, x.prows, y.rows + (int64_t)(live ? j : 0) * Tq * ldk, work ? m_j : 0,
                       y.prows, true, nrt, nct, ldk, kps, smem, wave, nw, lane);
  if (!live) return;
  ad_scale_rows(acc, x.norm + (int64_t)i * Rq, Rq, nrt, inv_sqrt_d, lane);

  const int64_t pair = (int64_t)i * y.B + j;
  const int row0 = 4 * (lane >> 4);
  const int n_tiles_all = (Rq + 15) >> 4;                                        // the teacher's L1 norm runs over all Rq regions
  double total = 0.0;
#pragma unroll
  for (int ct = 0; ct < AD_TILES; ++ct) {
    if (ct >= nct) continue;
    const int w = ct * 16 + (lane & 15);
    const bool wv = w < m_j;
    const float ny = y.norm[(int64_t)j * Tq + min(w, Tq - 1)];
    // log-sum-exp over the valid regions, selected by count and never multiplied
    float m = -INFINITY;
#pragma unroll
    for (int rt = 0; rt < AD_TILES; ++rt) {
      if (rt >= nrt) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        acc[rt][ct][reg] *= ny;
        m = fmax_nc(m, rt * 16 + row0 + reg < n_i ? acc[rt][ct][reg] : -INFINITY);
      }
    }
    m = fmax_nc(m, lane_xor16(m));
    m = fmax_nc(m, lane_xor32(m));
    float s = 0.f;
#pragma unroll
    for (int rt = 0; rt < AD_TILES; ++rt) {
      if (rt >= nrt) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) s += rt * 16 + row0 + reg < n_i ? expf(acc[rt][ct][reg] - m) : 0.f;
    }
    s = ad_region_sum(s);
    const float lse = m + logf(s);
    // the teacher's row: L1 norm over ALL Rq sliced regions (F.normalize, alad/loss.py:325), sigma over the valid ones
    const float* trow = t.data + i * t.si + j * t.sj + (int64_t)(wv ? w : 0) * t.sw;
    float a[AD_TILES][4];
    float l1 = 0.f, sig = 0.f;
#pragma unroll
    for (int rt = 0; rt < AD_TILES; ++rt) {
      if (rt >= n_tiles_all) { a[rt][0] = a[rt][1] = a[rt][2] = a[rt][3] = 0.f; continue; }
      ad_teacher4(a[rt], trow, rt * 16 + row0, Rq, wv);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        l1 += fabsf(a[rt][reg]);
        sig += rt * 16 + row0 + reg < n_i ? a[rt][reg] : 0.f;
      }
    }
    l1 = ad_region_sum(l1);
    sig = ad_region_sum(sig);
    const float inv = 1.0f / fmaxf(l1, 1e-12f);
    float kl = 0.f;
#pragma unroll
    for (int rt = 0; rt < AD_TILES; ++rt) {
      if (rt >= nrt) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float p = a[rt][reg] * inv;
        const bool in = rt * 16 + row0 + reg < n_i && p > 0.f;                   // xlogy(0, 0) = 0, and 0 * logp = 0
        kl += in ? p * (logf(p) - (acc[rt][ct][reg] - lse)) : 0.f;
      }
    }
    kl = ad_region_sum(kl);
    if (lane < 16 && wv) {
      total += (double)kl;
      stats[pair * Tq + w] = make_float4(lse, inv, sig * inv, 0.f);
    }
  }
  total = wave_sum_f64(total);
  if (lane == 0) partial[pair] = total;
}

// one workgroup: N = Bi * sum_j m_j, the pairs' partials in a fixed order, loss = sum / N (0 for N = 0).  head[0] = N for the backward.
__global__ __launch_bounds__(256) void attdistill_finish_kernel(AdSide y, int Bi, const double* __restrict__ partial,
                                                                double* __restrict__ head, float* __restrict__ loss) {
  __shared__ double red[4];
  double words = 0.0, sum = 0.0;
  for (int j = threadIdx.x; j < y.B; j += 256) words += (double)ad_count(y, j);
  const int64_t pairs = (int64_t)Bi * y.B;
  for (int64_t k = threadIdx.x; k < pairs; k += 256) sum += partial[k];
  words = block_sum_f64(words, red);
  sum = block_sum_f64(sum, red);
  if (threadIdx.x == 0) {
    const double N = words * (double)Bi;
    head[0] = N;
    *loss = N > 0.0 ? (float)(sum / N) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// backward: IMG = true owns d im_set[blockIdx.x], IMG = false owns d s_seq[blockIdx.x]; blockIdx.y = the chunk of AD_BWD_COLS columns
// ------------------------------------------------------------------------------------------------
struct AdGrad {
  float* data;             // the caller's gradient tensor and its strides in floats, or nullptr
  int64_t sb, sr;
};

template <bool IMG>
__device__ __forceinline__ void attdistill_bwd_body(const AdSide& x, const AdSide& y, const AdTeacher& t, int64_t ldk, int kps, int D,
                                                    float inv_sqrt_d, const float4* __restrict__ stats, const double* __restrict__ head,
                                                    const float* __restrict__ gscale, float* __restrict__ dst, int64_t dst_sb,
                                                    int64_t dst_sr, char* smem) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const AdSide& own = IMG ? x : y;
  const AdSide& par = IMG ? y : x;
  const int o = blockIdx.x;
  const int n_own = __builtin_amdgcn_readfirstlane(ad_count(own, o));
  const int nt_own = (n_own + 15) >> 4;
  const int Rq = x.Q, Tq = y.Q;
  const int gp = y.prows + 1;                                                    // pitch of G[r][w] in floats
  float* const G = reinterpret_cast<float*>(smem + 2 * (own.prows + AD_BWD_WAVES * par.prows) * 128);
  const int col0 = blockIdx.y * AD_BWD_COLS + wave * (AD_BWD_CT * 16) + (lane & 15);
  const int row0 = 4 * (lane >> 4);
  const half_t* pan_own = own.rows + (int64_t)o * own.Q * ldk;

  f32x4 out[AD_TILES][AD_BWD_CT];
#pragma unroll
  for (int tt = 0; tt < AD_TILES; ++tt)
#pragma unroll
    for (int c = 0; c < AD_BWD_CT; ++c) out[tt][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int p0 = 0; p0 < par.B; p0 += AD_BWD_WAVES) {
    // ---- this wave's pair: logits as the forward formed them, then g = softmax * sigma - P (times N: in [-1, 1])
    const int p = p0 + wave;
    const bool live = p < par.B;
    const int n_par = __builtin_amdgcn_readfirstlane(live ? ad_count(par, p) : 0);
    const bool work = n_own > 0 && n_par > 0;
    const int i = IMG ? o : (live ? p : 0), j = IMG ? (live ? p : 0) : o;
    const int n_i = IMG ? n_own : n_par, m_j = IMG ? n_par : n_own;
    const int nrt = work ? (n_i + 15) >> 4 : 0, nct = work ? (m_j + 15) >> 4 : 0;
    f32x4 acc[AD_TILES][AD_TILES];
    attdistill_pair_dots(acc, pan_own, n_own, own.prows, par.rows + (int64_t)(live ? p : 0) * par.Q * ldk, work ? n_par : 0,
                         par.prows, IMG, nrt, nct, ldk, kps, smem, wave, AD_BWD_WAVES, lane);
    ad_scale_rows(acc, x.norm + (int64_t)i * Rq, Rq, nrt, inv_sqrt_d, lane);
    const int64_t pair = (int64_t)i * y.B + j;
#pragma unroll
    for (int ct = 0; ct < AD_TILES; ++ct) {
      if (ct >= nct) continue;
      const int w = ct * 16 + (lane & 15);
      const bool wv = w < m_j;
      const float ny = y.norm[(int64_t)j * Tq + min(w, Tq - 1)];
      const float4 st = wv ? stats[pair * Tq + w] : make_float4(0.f, 0.f, 0.f, 0.f);      // (LSE, 1 / L1, sigma)
      const float* trow = t.data + i * t.si + j * t.sj + (int64_t)(wv ? w : 0) * t.sw;
#pragma unroll
      for (int rt = 0; rt < AD_TILES; ++rt) {
        if (rt >= nrt) continue;
        float a[4];
        ad_teacher4(a, trow, rt * 16 + row0, Rq, wv);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float l = acc[rt][ct][reg] * ny;
          const bool in = wv && rt * 16 + row0 + reg < n_i;
          acc[rt][ct][reg] = in ? expf(l - st.x) * st.z - a[reg] * st.y : 0.f;
        }
      }
    }

    // ---- the four pairs take turns in G; every wave adds the pair's second product on its own columns
    for (int u = 0; u < AD_BWD_WAVES; ++u) {
      const int pu = p0 + u;
      if (pu >= par.B) break;                                                    // workgroup-uniform
      const int n_pu = __builtin_amdgcn_readfirstlane(ad_count(par, pu));
      __syncthreads();                                                           // the panels / the previous G have been read
      if (wave == u) {
#pragma unroll
        for (int rt = 0; rt < AD_TILES; ++rt) {
          if (rt >= nrt) continue;
#pragma unroll
          for (int ct = 0; ct < AD_TILES; ++ct) {
            if (ct >= nct) continue;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) G[(rt * 16 + row0 + reg) * gp + ct * 16 + (lane & 15)] = acc[rt][ct][reg];
          }
        }
      }
      __syncthreads();
      if (n_own == 0 || n_pu == 0) continue;
      // the contraction runs over the partner's positions k < n_pu; its raw fp32 row k + 1 is the B operand:
      // lane -> (k = lane >> 4, column lane & 15)
      const float* prow = par.data + pu * par.sb;
      for (int k0 = 0; k0 < n_pu; k0 += 4) {
        const int k = k0 + (lane >> 4);
        const bool kv = k < n_pu;
        const float* src = prow + (int64_t)(min(k, n_pu - 1) + 1) * par.sr;
        float b[AD_BWD_CT];
#pragma unroll
        for (int c = 0; c < AD_BWD_CT; ++c) {
          const int d = col0 + c * 16;
          const float v = src[min(d, D - 1)];
          b[c] = kv && d < D ? v : 0.f;                                          // selected: a masked row may hold anything
        }
#pragma unroll
        for (int tt = 0; tt < AD_TILES; ++tt) {
          if (tt >= nt_own) continue;
          const int q = tt * 16 + (lane & 15);                                   // the A operand: lane -> (own position q, k = lane >> 4)
          const float a = IMG ? G[q * gp + k] : G[k * gp + q];
#pragma unroll
          for (int c = 0; c < AD_BWD_CT; ++c) out[tt][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[c], out[tt][c], 0, 0, 0);
        }
      }
    }
    __syncthreads();                                                             // G has been read before the next round stages panels
  }

  // ---- every row of the sample's gradient, this workgroup's columns: positions 1 .. n_own scaled, the rest (slot 0 too) zeros
  const double N = head[0];
  const float scale = N > 0.0 ? (float)((double)*gscale * (double)inv_sqrt_d / N) : 0.f;
  float* const base = dst + o * dst_sb;
#pragma unroll
  for (int c = 0; c < AD_BWD_CT; ++c) {
    const int d = col0 + c * 16;
    if (d >= D) continue;
    if (lane < 16) base[d] = 0.f;
#pragma unroll
    for (int tt = 0; tt < AD_TILES; ++tt) {
      if (tt * 16 >= own.Q) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int q = tt * 16 + row0 + reg;
        if (q < own.Q) base[(int64_t)(q + 1) * dst_sr + d] = (tt < nt_own && q < n_own) ? out[tt][c][reg] * scale : 0.f;
      }
    }
  }
}

// One launch for both passes, so that they share the chip: blockIdx.z = 0 images, 1 captions where both gradients are wanted.
// blockIdx.x runs to the larger batch; a workgroup past its side's batch leaves before any barrier.
__global__ __launch_bounds__(AD_BWD_WAVES * 64) void attdistill_bwd_kernel(AdSide x, AdSide y, AdTeacher t, int64_t ldk, int kps, int D,
                                                                           float inv_sqrt_d, const float4* __restrict__ stats,
                                                                           const double* __restrict__ head,
                                                                           const float* __restrict__ gscale, AdGrad gx, AdGrad gy) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool img = gx.data != nullptr && (gy.data == nullptr || blockIdx.z == 0);      // workgroup-uniform
  if (img) {
    if ((int)blockIdx.x < x.B) attdistill_bwd_body<true>(x, y, t, ldk, kps, D, inv_sqrt_d, stats, head, gscale, gx.data, gx.sb, gx.sr, smem);
  } else {
    if ((int)blockIdx.x < y.B) attdistill_bwd_body<false>(x, y, t, ldk, kps, D, inv_sqrt_d, stats, head, gscale, gy.data, gy.sb, gy.sr, smem);
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct AdWs {
  double* head;            // [0] = N
  half_t *xh, *yh;
  float *xn, *yn;
  float4* stats;           // (Bi, Bc, Tq): LSE, 1 / L1, sigma
  double* partial;         // (Bi, Bc)
};

static size_t ad_ws_layout(int Bi, int Bc, int Rq, int Tq, int Dp, char* base, AdWs* out) {
  WsCursor c{base, 0};
  AdWs w;
  w.head = c.take<double>(32, 256);
  w.xh = c.take<half_t>((size_t)Bi * Rq * 2 * Dp, 256);
  w.yh = c.take<half_t>((size_t)Bc * Tq * 2 * Dp, 256);
  w.xn = c.take<float>((size_t)Bi * Rq, 256);
  w.yn = c.take<float>((size_t)Bc * Tq, 256);
  w.stats = c.take<float4>((size_t)Bi * Bc * Tq, 256);
  w.partial = c.take<double>((size_t)Bi * Bc, 256);
  if (out) *out = w;
  return c.off;
}

static int ad_fwd_waves(int x_prows, int y_prows) {
  for (int nw = 8; nw >= 1; nw >>= 1)
    if (2 * (x_prows + nw * y_prows) * 128 <= AD_LDS_LIMIT) return nw;
  return 0;
}

struct AdPlan {
  AdSide x, y;
  AdTeacher t;
  AdWs ws;
  int Dp, kps;             // Dp: halfs of one half of a split row; kps: 64-deep K steps per chain segment
  float inv_sqrt_d;
};

// the checks the three entry points share, before any launch; `who` names the caller in messages
static int ad_plan(const char* who, const aladin_set* im, const aladin_set* s, int Bi, int Bc, int R, int T, int D, const float* teacher,
                   int64_t t_si, int64_t t_sj, int64_t t_sw, int Wt, int Rt, void* workspace, AdPlan* p) {
  if (!set_ok(im) || !set_ok(s) || !teacher || !workspace || Bi < 1 || Bc < 1 || R < 2 || T < 2 || D < 1 || ((uintptr_t)workspace & 15)) {
    aladin_set_error("%s: bad argument (Bi=%d Bc=%d R=%d T=%d D=%d; both sets with lengths, the teacher and a 16-byte aligned workspace "
                     "are required, R and T at least 2)", who, Bi, Bc, R, T, D);
    return ALADIN_ERR_ARG;
  }
  const int Rq = R - 1, Tq = T - 1;
  if (Rq > AD_MAX_COUNT || Tq > AD_MAX_COUNT) {
    aladin_set_error("%s: at most %d scored positions per set, got %d regions / %d words", who, AD_MAX_COUNT, Rq, Tq);
    return ALADIN_ERR_UNSUPPORTED;
  }
  if (Wt < Tq || Rt < Rq || t_si < 0 || t_sj < 0 || t_sw < Rt) {
    aladin_set_error("%s: the teacher holds %d x %d (words x regions, row stride %lld) per pair, the sets need %d x %d", who, Wt, Rt,
                     (long long)t_sw, Tq, Rq);
    return ALADIN_ERR_ARG;
  }
  if ((int64_t)Bi * Bc > 0x7fffffff) {
    aladin_set_error("%s: %d x %d pairs are more workgroups than one launch takes", who, Bi, Bc);
    return ALADIN_ERR_UNSUPPORTED;
  }
  p->Dp = round_up(D, 64);
  p->kps = p->Dp / 64;
  p->inv_sqrt_d = (float)(1.0 / sqrt((double)D));
  ad_ws_layout(Bi, Bc, Rq, Tq, p->Dp, (char*)workspace, &p->ws);
  p->x = AdSide{im->data, im->stride_b, im->stride_r, im->len, p->ws.xh, p->ws.xn, Bi, Rq, round_up(Rq, 16)};
  p->y = AdSide{s->data, s->stride_b, s->stride_r, s->len, p->ws.yh, p->ws.yn, Bc, Tq, round_up(Tq, 16)};
  p->t = AdTeacher{teacher, t_si, t_sj, t_sw};
  return ALADIN_OK;
}

extern "C" size_t aladin_attdistill_workspace_bytes(int Bi, int Bc, int R, int T, int D) {
  if (Bi < 1 || Bc < 1 || R < 2 || T < 2 || D < 1 || R - 1 > AD_MAX_COUNT || T - 1 > AD_MAX_COUNT) return 0;
  return ad_ws_layout(Bi, Bc, R - 1, T - 1, round_up(D, 64), nullptr, nullptr);
}

extern "C" int aladin_attdistill_fwd(const aladin_set* im, const aladin_set* s, int Bi, int Bc, int R, int T, int D, const float* teacher,
                                     int64_t t_si, int64_t t_sj, int64_t t_sw, int Wt, int Rt, float* loss, void* workspace, void* stream) {
  AdPlan p;
  if (!loss) { aladin_set_error("attdistill_fwd: null loss"); return ALADIN_ERR_ARG; }
  if (int rc = ad_plan("attdistill_fwd", im, s, Bi, Bc, R, T, D, teacher, t_si, t_sj, t_sw, Wt, Rt, workspace, &p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)Bi * p.x.Q + (int64_t)Bc * p.y.Q;
  hipLaunchKernelGGL(attdistill_pack_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, p.x, p.y, D, p.Dp, p.ws.xh, p.ws.xn,
                     p.ws.yh, p.ws.yn, is_vec4_ok(im->data, im->stride_b, im->stride_r, D), is_vec4_ok(s->data, s->stride_b, s->stride_r, D));
  if (int rc = aladin_check_launch("attdistill_pack_kernel")) return rc;
  const int nw = ad_fwd_waves(p.x.prows, p.y.prows);
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)attdistill_fwd_kernel, AD_LDS_LIMIT, &lds_reserved, "attdistill_fwd_kernel")) return rc;
  hipLaunchKernelGGL(attdistill_fwd_kernel, dim3((unsigned)(Bi * cdiv(Bc, nw))), dim3(nw * 64), 2 * (p.x.prows + nw * p.y.prows) * 128, st,
                     p.x, p.y, p.t, (int64_t)2 * p.Dp, p.kps, p.inv_sqrt_d, p.ws.stats, p.ws.partial);
  if (int rc = aladin_check_launch("attdistill_fwd_kernel")) return rc;
  hipLaunchKernelGGL(attdistill_finish_kernel, dim3(1), dim3(256), 0, st, p.y, Bi, p.ws.partial, p.ws.head, loss);
  return aladin_check_launch("attdistill_finish_kernel");
}

extern "C" int aladin_attdistill_bwd(const aladin_set* im, const aladin_set* s, int Bi, int Bc, int R, int T, int D, const float* teacher,
                                     int64_t t_si, int64_t t_sj, int64_t t_sw, int Wt, int Rt, const float* gscale,
                                     const aladin_set_grad* d_im, const aladin_set_grad* d_s, void* workspace, void* stream) {
  AdPlan p;
  if (!gscale || (!d_im && !d_s) || (d_im && !d_im->data) || (d_s && !d_s->data)) {
    aladin_set_error("attdistill_bwd: the upstream gradient (a device scalar) and at least one output are required");
    return ALADIN_ERR_ARG;
  }
  if (int rc = ad_plan("attdistill_bwd", im, s, Bi, Bc, R, T, D, teacher, t_si, t_sj, t_sw, Wt, Rt, workspace, &p)) return rc;
  // panels of the owner and of four partners, double buffered, and the fp32 tile G[r][w]: the larger of the two passes
  const int rows_img = p.x.prows + AD_BWD_WAVES * p.y.prows, rows_cap = p.y.prows + AD_BWD_WAVES * p.x.prows;
  const int rows = d_im && d_s ? (rows_img > rows_cap ? rows_img : rows_cap) : (d_im ? rows_img : rows_cap);
  const int lds = 2 * rows * 128 + p.x.prows * (p.y.prows + 1) * 4;
  static unsigned long long lds_reserved = 0;
  if (int rc = aladin_reserve_lds((const void*)attdistill_bwd_kernel, AD_LDS_LIMIT, &lds_reserved, "attdistill_bwd_kernel")) return rc;
  const AdGrad gx{d_im ? d_im->data : nullptr, d_im ? d_im->stride_b : 0, d_im ? d_im->stride_r : 0};
  const AdGrad gy{d_s ? d_s->data : nullptr, d_s ? d_s->stride_b : 0, d_s ? d_s->stride_r : 0};
  const int owners = d_im && d_s ? (Bi > Bc ? Bi : Bc) : (d_im ? Bi : Bc);
  hipLaunchKernelGGL(attdistill_bwd_kernel, dim3(owners, cdiv(D, AD_BWD_COLS), d_im && d_s ? 2 : 1), dim3(AD_BWD_WAVES * 64), lds,
                     (hipStream_t)stream, p.x, p.y, p.t, (int64_t)2 * p.Dp, p.kps, D, p.inv_sqrt_d, p.ws.stats, p.ws.head, gscale, gx, gy);
  return aladin_check_launch("attdistill_bwd_kernel");
}
