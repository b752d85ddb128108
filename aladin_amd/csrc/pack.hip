// fp32 sets -> the packed fp16 MFMA operands (aladin_align_pack): one kernel, one wave per destination row of the [xm | xe | y] row
// space.  The format -- row maps, masks, the normalise-and-round arithmetic -- is pack_rows.hpp's; this file holds the kernel that
// walks a row range with it and the two range choices of its launcher:
//   aladin_internal_pack                 every row of the sets given: [xm | xe | y], [xm | xe] (images alone) or [y] (captions alone)
//   aladin_internal_pack_side_operands   [xe | y]: the triplet forward's prologue, whose side launch packs xm itself
//                                        (align_side_pack_kernel, align_fwd.hip)
// It is a translation unit of its own so that an edit to packing does not move the score kernels inside their code object
// (DESIGN_HISTORY.md, "Alignment backward: plain stages over one problem struct": that alone cost the headline step 0.9 %).
#include "pack_rows.hpp"

namespace {

struct PackJob {
  aladin_set im, s;                      // an absent set's rows are never in the launch's range
  int vec_i, vec_s;                      // is_vec4_ok of each
  int Bi, Bc, Rq, Tq, x_tail, y_tail, D, Dp, trows, split;
  MaxSideMap xmap;
  int64_t img_rows;                      // xm_rows + xe_rows: where the y rows begin
  half_t *xm, *xe, *y;
  float* rnorm;                          // [xm rows | xe rows | y rows], or nullptr
  // When is a row's length looked at?  0: after the row's loads are issued (the row exists in memory either way), so that the
  // length and the row arrive together instead of one memory latency after the other; 1: first, so that a masked row is never
  // loaded.  Wave-uniform, set by the launcher from the kind of launch: both sets -> 0, a single set -> 1, as the three kernels
  // this one replaces did.  Only the whole-row-in-registers path (fp16, float4 rows, D <= 1024) has a choice; the measured
  // times that keep the flag are in DESIGN_HISTORY.md ("Packed operands: one row map, one normaliser, one pack kernel").
  int len_first;
};

// rows [row0, row0 + n) of the row space
__global__ __launch_bounds__(256) void pack_rows_kernel(PackJob p, int64_t row0, int64_t n) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // the wave's row: uniform, so in scalar registers
  if (k >= n) return;
  const int64_t d = row0 + k;
  const float* src = nullptr;            // the raw row, if the sample exists
  int len = 0, pos, tail, cap, seg;
  half_t* dst;
  bool vec4;
  if (d < p.img_rows) {
    const MaxSideRow r = max_side_row(d, p.xmap);
    if (r.i < p.Bi) { src = p.im.data + r.i * p.im.stride_b + (int64_t)(r.rho + 1) * p.im.stride_r; len = p.im.len[r.i]; }   // region 0 dropped (alad/loss.py:87)
    pos = r.rho; tail = p.x_tail; cap = p.Rq;
    dst = (r.side ? p.xe : p.xm) + r.row * p.Dp;
    vec4 = p.vec_i != 0;
    seg = 1;
  } else {
    const SumSideRow r = sum_side_row(d - p.img_rows, p.trows);
    if (r.j < p.Bc && r.w < p.Tq) { src = p.s.data + r.j * p.s.stride_b + (int64_t)(r.w + 1) * p.s.stride_r; len = p.s.len[r.j]; }   // token 0 dropped (alad/loss.py:88)
    pos = r.w; tail = p.y_tail; cap = p.Tq;
    dst = p.y + (d - p.img_rows) * p.Dp;
    vec4 = p.vec_s != 0;
    seg = 2;
  }
  float* slot = p.rnorm ? p.rnorm + d : nullptr;
  const int Dp = p.split ? p.Dp / 3 : p.Dp;
  const bool regs = vec4 && !p.split && p.D <= 1024;
  bool counts = src != nullptr;
  if (counts && !(regs && !p.len_first)) counts = pos < scored_len(len, tail, cap);
  if (!counts) {
    write_zero_row(dst, p.Dp, lane);
    write_rnorm(slot, 0.f, lane);
    return;
  }
  if (regs) {
    float4 v[4];
    load_row_regs(v, src, p.D, lane);
    if (!p.len_first && pos >= scored_len(len, tail, cap)) {      // masked after all: a zero row
      write_zero_row(dst, p.Dp, lane);
      write_rnorm(slot, 0.f, lane);
      return;
    }
    const float inv = inv_norm_regs(v);
    write_rnorm(slot, inv, lane);
    write_fp16_regs(dst, v, inv, Dp, lane);
    return;
  }
  const float inv = inv_norm_mem(src, p.D, lane, vec4);
  write_rnorm(slot, inv, lane);
  if (!p.split) write_fp16_mem(dst, src, inv, p.D, Dp, lane, vec4);
  else if (seg == 1) write_split(dst, dst + 2 * Dp, dst + Dp, src, inv, p.D, Dp, lane);      // [hi | lo | hi]
  else write_split(dst, dst + Dp, dst + 2 * Dp, src, inv, p.D, Dp, lane);                    // [hi | hi | lo]
}

// rows [row0, row0 + n) from the sets given; a set that is nullptr must have no row in the range
int launch_pack(const aladin_set* im, const aladin_set* s, const aladin_align_geom* g, const aladin_packed* out, int64_t row0,
                int64_t n, hipStream_t st) {
  PackJob p = {};
  if (im) { p.im = *im; p.vec_i = is_vec4_ok(im->data, im->stride_b, im->stride_r, g->D); }
  if (s) { p.s = *s; p.vec_s = is_vec4_ok(s->data, s->stride_b, s->stride_r, g->D); }
  p.Bi = g->Bi; p.Bc = g->Bc; p.Rq = g->Rq; p.Tq = g->Tq; p.x_tail = g->x_tail; p.y_tail = g->y_tail;
  p.D = g->D; p.Dp = g->Dp; p.trows = g->trows; p.split = g->split;
  p.xmap = MaxSideMap{g->mrows, g->rem > 0 ? g->rem : 1, g->Rq, g->xm_rows};
  p.img_rows = g->xm_rows + g->xe_rows;
  p.xm = (half_t*)out->xm; p.xe = (half_t*)out->xe; p.y = (half_t*)out->y; p.rnorm = out->rnorm;
  p.len_first = !(im && s);
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, p, row0, n);
  return aladin_check_launch("pack_rows_kernel");
}

}  // namespace

int aladin_internal_pack(const aladin_set* im, const aladin_set* s, const aladin_align_geom* g, const aladin_packed* out, hipStream_t st) {
  if (!g || !out || (!im && !s)) { aladin_set_error("align_pack: null argument"); return ALADIN_ERR_ARG; }
  if ((im && (!set_ok(im) || !out->xm || (g->rem && !out->xe))) || (s && (!set_ok(s) || !out->y))) { aladin_set_error("align_pack: null argument"); return ALADIN_ERR_ARG; }
  const int64_t img_rows = g->xm_rows + g->xe_rows;
  return launch_pack(im, s, g, out, im ? 0 : img_rows, (im ? img_rows : 0) + (s ? g->y_rows : 0), st);
}

// [xe | y] and their rnorm entries: the bits aladin_internal_pack gives them
int aladin_internal_pack_side_operands(const aladin_set* im, const aladin_set* s, const aladin_align_geom* g, const aladin_packed* out,
                                       hipStream_t st) {
  if (int rc = aladin_internal_check_prologue(im, s, g, out)) return rc;
  return launch_pack(im, s, g, out, g->xm_rows, g->xe_rows + g->y_rows, st);
}

extern "C" int aladin_align_pack(const aladin_set* im, const aladin_set* s, const aladin_align_geom* g, const aladin_packed* out,
                                 void* stream) {
  return aladin_internal_pack(im, s, g, out, (hipStream_t)stream);
}
