/*
 * aladin_hip.h -- C ABI of libaladin_hip.so: ALADIN's fine-grained alignment-scoring and
 * matching-retrieval hot path as hand-written HIP kernels for gfx950 (MI355X, CDNA4).
 *
 * The reference (mesnico/ALADIN) is pure Python/PyTorch and has no FFI of its own; the boundary
 * this library slots under is the Python call surface of alad/loss.py, alad/recall_auxiliary.py
 * and alad/evaluation.py.  Each entry point below names the reference
 * lines it replaces.  INTEGRATION.md shows the ctypes binding a maintainer would add there;
 * aladin_amd/_lib.py is that binding as shipped.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless a parameter says "host";
 *   - `stream` is a hipStream_t (PyTorch: torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued asynchronously on it, nothing synchronises, nothing is allocated: outputs and
 *     workspaces are caller-owned, and no pointer is retained after return;
 *   - output buffers and workspaces may hold ANYTHING on entry (fresh, recycled from another call,
 *     never zeroed): a call writes exactly the documented extent of each output -- every element of
 *     it, masked and padded positions included -- zeroes whatever it accumulates into, reads no
 *     workspace word it has not written in the same call, and stays inside *_workspace_bytes /
 *     *_index_bytes.  What a workspace holds afterwards is unspecified except where an entry point
 *     documents it (the arg-max table and dS^T for the backward, the statistics behind
 *     aladin_retrieval_stats_offset);
 *   - return value: 0 = ok, 1 = bad argument, 2 = unsupported shape, 3 = HIP launch error;
 *     aladin_last_error() gives the message (thread-local).  Never aborts.
 *   - float = IEEE binary32.  16-bit packed operands are IEEE binary16 (fp16): the MFMA path
 *     multiplies fp16 operands and accumulates in fp32 (see DESIGN.md for why not bf16).
 */
#ifndef ALADIN_HIP_H
#define ALADIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALADIN_ABI_VERSION 13

/* The library is built with -fvisibility=hidden: the entry points declared here are its ONLY exports. */
#if defined(__GNUC__)
#define ALADIN_API __attribute__((visibility("default")))
#else
#define ALADIN_API
#endif

ALADIN_API int aladin_version(void);
ALADIN_API const char* aladin_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Alignment scores  S[i][j] = sum_w max_r <im^[i,r], s^[j,w]>      (aggregation 'MrSw')
 * replaces AlignmentContrastiveLoss.forward, reference alad/loss.py:79-125 (normalise :80-81,
 * drop region 0 / token 0 / last two tokens :87-90, B*B batched matmul :97-99, length masks
 * :103-116, max over regions + sum over words :124-125).
 *
 * Three steps so that the packed image operand can be all-gathered between GPUs (RCCL) before
 * scoring:  pack(images) -> [all-gather] -> scores  <- pack(captions).  The training step of one
 * GPU is ONE call per direction: aladin_align_triplet_fwd / _bwd below.
 *
 * One entry point per operation; the alignment family takes its arguments in three small structs
 * (aladin_set, aladin_set_grad, aladin_packed).
 * ------------------------------------------------------------------------------------------- */

/* A batch of sets (B, N, D) fp32 in HBM: element [b][n][d] at data[b * stride_b + n * stride_r + d] (strides in floats,
 * unit inner stride, rows 16-byte aligned when D % 4 == 0: the reference hands permuted (S,B,D)->(B,S,D) views,
 * alad/alad_model.py:377-378).  len: B int32 on the device, the reference's length lists. */
typedef struct aladin_set {
  const float* data;
  int64_t stride_b, stride_r;
  const int32_t* len;
} aladin_set;

/* Where a gradient of such a batch goes: the CALLER'S layout (the same permuted views), every row written exactly once. */
typedef struct aladin_set_grad {
  float* data;
  int64_t stride_b, stride_r;
} aladin_set_grad;

typedef struct aladin_align_geom {
  int32_t Bi, Bc, R, T, D;      /* inputs: im (Bi,R,D), s (Bc,T,D)                              */
  int32_t Rq, Tq;               /* R-1 regions and T-3 words take part (alad/loss.py:87-88)     */
  int32_t mrows;                /* rows per image in the main operand xm: 32, 48, 64 or 96 (rows past R' repeat region 0);
                                   ALADIN_LAYOUT_LONG: round_up(R', 32) up to 512 */
  int32_t rem;                  /* leftover regions per image (R' - mrows when positive) that go through the side GEMM: <= 8 */
  int32_t tp16;                 /* 16-word column tiles a caption needs: ceil(trows / 16)       */
  int32_t trows;                /* rows per caption in y: 16 * tp16, or 16 * tp16 - 8 = 8 / 24 / 40 (T' <= 8 / 17..24 / 33..40
                                   with 32, 48 or 64 main rows: two captions share one / three / five 16-word tiles) */
  int32_t Dp;                   /* halfs per packed row: D rounded up to 64 (zero filled), x3 when split */
  int32_t img_unit, cap_unit;   /* images / captions per workgroup tile                         */
  int32_t Bi_pad, Bc_pad;       /* batch sizes rounded up to the units (zero rows)              */
  int32_t x_tail, y_tail;       /* positions dropped at the END of the max-side / sum-side sets: the
                                   set uses positions 1 .. N-1-tail and length len-1-tail.  Images 0
                                   (alad/loss.py:87,89), captions 2 (:88,90)                      */
  int32_t split;                /* 1: split-fp16 operands (ALADIN_PRECISION_SPLIT), Dp = 3 * round_up(D, 64) */
  int32_t layout;               /* ALADIN_LAYOUT_TILES, _TILES_WHOLE or _LONG (below): which kernel family reads the operands */
  int64_t xm_rows, xe_rows, y_rows;            /* rows of the packed fp16 operands              */
  int64_t xm_bytes, xe_bytes, y_bytes;         /* their sizes                                   */
  int64_t e_bytes;              /* fp32 scratch for the side GEMM, xe_rows x y_rows (0 if !rem) */
  int64_t rnorm_bytes;          /* fp32, one per packed row in the order [xm rows | xe rows | y rows]: 1 / max(|x|, 1e-12) of the
                                   raw vector a row holds (0 for a zero row) -- what the backward's normalise step divides by */
} aladin_align_geom;

/* The packed fp16 MFMA operands of one problem (caller-owned buffers of geom->xm_bytes, xe_bytes, y_bytes, rnorm_bytes).
 * xe may be NULL when !geom->rem; rnorm may be NULL (then the backward reads the raw fp32 rows instead). */
typedef struct aladin_packed {
  void* xm;
  void* xe;
  void* y;
  float* rnorm;
} aladin_packed;

/* Operand precision of the packed sets.
 *   ALADIN_PRECISION_FP16   one rounding of every unit vector to fp16: scores within ~1e-4 of the fp32
 *                           reference (the training path: north_star's 1e-3 tolerance, full MFMA rate).
 *   ALADIN_PRECISION_SPLIT  x^ * 2^14 = hi + lo (fp16 each); a packed row is three K segments
 *                           [hi | lo | hi] (max side) / [hi | hi | lo] (sum side), so the SAME pack / score entry
 *                           points contract hi.hi + lo.hi + hi.lo with fp32 accumulation: ~2^-22 relative operand
 *                           error, i.e. the rounding level of the reference's own fp32 bmm, at 3x the MFMA work.
 *                           This is what evaluation uses: Recall needs rank-exact scores (near-ties between
 *                           thousands of candidates flip at the 1e-4 level; alad/evaluation.py:213-223,303-308).
 *                           Forward only: the backward entry points reject split operands. */
#define ALADIN_PRECISION_FP16 0
#define ALADIN_PRECISION_SPLIT 1

/* Packed layout of a geometry: the field `layout` of aladin_align_geom, which every entry point dispatches on.
 *   ALADIN_LAYOUT_TILES        the tile classes: at most 96 scored positions on either side (R' = R - 1 - x_tail, T' = T - 1 -
 *                              y_tail); 32 / 48 / 64 / 96 main rows + side rows, captions in 16-word tiles or the 8- / 24- /
 *                              40-row classes (the fields of aladin_align_geom above).  0: a zero-initialised struct reads as tiles.
 *   ALADIN_LAYOUT_TILES_WHOLE  the same with whole 16-word caption tiles only (no 8- / 24- / 40-row classes): what the dense
 *                              backward's arg-max table kernel reads.
 *   ALADIN_LAYOUT_LONG         long sets (csrc/align_long.hip): up to 512 positions per set -- R <= 512 and T <= 512, i.e. up to
 *                              511 scored regions on the max side and 509 scored words on the sum side.  mrows = round_up(R', 32)
 *                              rows per max-side sample (rows past R' repeat its first scored position), no side rows (rem 0,
 *                              xe_bytes 0, e_bytes 0), trows = round_up(T', 16) rows per sum-side sample, cap_unit = 512 / trows
 *                              samples per score workgroup, Bc_pad rounded to it; rnorm is [xm rows | y rows].
 * aladin_align_pack, aladin_align_scores and aladin_align_bwd (with its workspace query) take every layout they are given a
 * geometry of; the entry points that exist only for the tile classes (aladin_align_triplet_*, aladin_heads_small_fwd_argmax,
 * aladin_align_pack_store_x / _y) refuse a LONG geometry before launching anything.  The score and backward entry points
 * validate a LONG geometry by recomputation (one that aladin_align_geometry did not make: ALADIN_ERR_ARG, workspace 0); tile
 * geometries are trusted.
 * ALADIN_LAYOUT_AUTO is a REQUEST only: TILES when R' <= ALADIN_TILE_MAX_SCORED and T' <= ALADIN_TILE_MAX_SCORED, else LONG. */
#define ALADIN_LAYOUT_AUTO (-1)
#define ALADIN_LAYOUT_TILES 0
#define ALADIN_LAYOUT_TILES_WHOLE 1
#define ALADIN_LAYOUT_LONG 2
#define ALADIN_TILE_MAX_SCORED 96

/* Host-only: derive the packed layout.  The set on the MAX side (Bi x R) and the set on the SUM side (Bc x T) each state
 * how many trailing positions they drop: 'MrSw' = (images, x_tail 0) x (captions, y_tail 2); 'MwSr' (alad/loss.py:134-135,
 * max over words, sum over regions) = (captions, tail 2) x (images, tail 0), result transposed.  Every "image" / "caption"
 * argument below means max-side / sum-side set.  precision: ALADIN_PRECISION_FP16 or _SPLIT; layout: a request, ALADIN_LAYOUT_*
 * above.  TILES / TILES_WHOLE past 96 scored positions and LONG past 512 positions per set: ALADIN_ERR_UNSUPPORTED. */
ALADIN_API int aladin_align_geometry(int Bi, int Bc, int R, int T, int D, int x_tail, int y_tail, int precision, int layout,
                                     aladin_align_geom* out);

/* L2-normalise (eps 1e-12, F.normalize), slice, length-mask and convert sets to the packed fp16 MFMA operands: the image
 * sets into out->xm / xe, the caption sets into out->y, in ONE launch when both are given; either may be NULL (the members
 * of `out` it would fill are then not touched).  out->rnorm, when not NULL, receives the rows' inverse norms. */
ALADIN_API int aladin_align_pack(const aladin_set* im, const aladin_set* s, const aladin_align_geom* geom,
                                 const aladin_packed* out, void* stream);

/* S (Bi x Bc, row stride ldS floats) from packed operands, any layout and both precisions; bitwise reproducible.
 * e_scratch: geom->e_bytes (may be NULL when !geom->rem, so for every LONG geometry).
 * ALADIN_SCORES_REUSE_SIDE: e_scratch already holds the side-GEMM result of a previous call on the same operands, launch
 * the score kernel alone (used by bench.py to time the dominant kernel in isolation); ignored without side rows. */
#define ALADIN_SCORES_REUSE_SIDE 1
ALADIN_API int aladin_align_scores(const aladin_packed* packed, const aladin_align_geom* geom, void* e_scratch, float* S,
                                   int64_t ldS, int flags, void* stream);

/* Backward of S w.r.t. the raw sets (autograd of alad/loss.py:80-125).
 * dS (Bi x Bc, stride ld_dS) is multiplied by *gscale (device float, may be NULL = 1).  Pairs with dS == 0 are skipped, so
 * the max_violation=True hinge (<= 3B non-zeros) costs O(B) pair blocks.  Three steps: (1) the non-zero pairs (compacted
 * here, or given: pairs / pair_count as aladin_hinge_fused emits them; both or neither), (2) per pair the arg-max region of
 * every word -- recomputed on the fp16 MFMA from `packed` when given (xm, y and, with side rows, xe), with every word whose
 * top candidates are closer than the fp16 error bound re-decided by exact fp32 dot products, or entirely in fp32 when
 * packed is NULL -- the recorded arg-max is the fp32 arg-max, as autograd's; (3) one wave per OUTPUT row gathers the partner
 * rows the table points at and applies the normalise backward.  d_im / d_s: fully written, no atomics.
 * workspace: aladin_align_bwd_workspace_bytes(geom, flags).  Split operands are rejected (forward only).
 *   ALADIN_BWD_PARTNERS_FP16  step 3 gathers the PARTNER rows (the unit vectors an output row's gradient is a weighted sum of)
 *       from the forward's packed fp16 operands instead of normalising the raw fp32 rows again: half the bytes per partner, no norm
 *       reduction.  One fp16 rounding of those vectors (<= 2^-11 relative per component) leaves the gradients within 5e-4 of their
 *       LARGEST entry of the reference's autograd for D >= 128 (3e-7 without the flag; element by element the error reaches
 *       ~3e-3 of an entry a tenth of the largest -- a max-normalised bound).  Needs packed->xm, y, rnorm
 *       (and xe with side rows) of THIS problem.  The Python layer sets it by default (ops.set_backward_precision('exact') clears
 *       it).  The arg-maxima are the exact fp32 ones either way.
 *   ALADIN_BWD_OWN_ROW_FP16  (with ALADIN_BWD_PARTNERS_FP16) the output row's OWN unit vector and inverse norm come from the packed
 *       operands and packed->rnorm too: the raw sets are not read by step 3 at all.  Up to ~7e-4 of the largest entry when the
 *       partners are aligned with the row (cosines near 1): an opt-in ('fp16-own').
 *   ALADIN_BWD_DENSE  the caller states that (almost) every pair carries a gradient -- the sum-of-violations hinge
 *       (max_violation = False, alad/loss.py:60-67), or a gradient arriving on the score matrix itself.  The arg-max table of
 *       ALL pairs then comes from the forward's own tile kernel run in split precision (64 pairs per workgroup sharing their
 *       operand panels) instead of one workgroup per pair; only the pairs with a word whose two best regions it cannot
 *       separate (a few per cent) go through the exact per-pair kernel.  Same table, same gradients.  Classes the tile kernel
 *       does not cover (R' > 64, small batches) silently take the list path.  `pairs` / `pair_count` are ignored.
 *       With the table of all pairs in hand step 3 runs as two MFMA GEMMs, dXh = P Yh and dYh = P^T Xh with
 *       P[(i,r),(c,w)] = dS[i,c] [argmax == r] generated in registers from the table (csrc/align_bwd_dense.hip), exact to
 *       ~2^-22 by hi + lo splitting (one product under ALADIN_BWD_PARTNERS_FP16) -- sums in a different order than the
 *       gather, so equal to it to rounding, not bit for bit.
 *   ALADIN_BWD_DENSE_GATHER  (with ALADIN_BWD_DENSE) keep the per-row gather as step 3: bit-identical to the list path.
 * A LONG geometry takes the pair-list path for any dS, a dense one included: the non-zero pairs of dS are compacted here
 * (`pairs` / `pair_count` are ignored, as are ALADIN_BWD_DENSE and ALADIN_BWD_DENSE_GATHER), every word's arg-max region of
 * every listed pair is decided in fp32 from the raw rows (16-bit table entries), and one wave per output row gathers the partner
 * rows.  ALADIN_BWD_PARTNERS_FP16 (`packed` then needs xm, y and rnorm) and ALADIN_BWD_OWN_ROW_FP16 mean what they mean above;
 * `packed` may be NULL otherwise.  D % 4 == 0, D <= 1024. */
#define ALADIN_BWD_PARTNERS_FP16 1
#define ALADIN_BWD_DENSE 2
#define ALADIN_BWD_DENSE_GATHER 4
#define ALADIN_BWD_OWN_ROW_FP16 16
ALADIN_API size_t aladin_align_bwd_workspace_bytes(const aladin_align_geom* geom, int flags);
ALADIN_API int aladin_align_bwd(const aladin_set* im, const aladin_set* s, const aladin_align_geom* geom,
                                const aladin_packed* packed, const float* dS, int64_t ld_dS, const float* gscale,
                                const int32_t* pairs, const int32_t* pair_count, const aladin_set_grad* d_im,
                                const aladin_set_grad* d_s, void* workspace, int flags, void* stream);

/* The training step of AlignmentContrastiveLoss(max_violation=True, aggregation='MrSw') -- every shipped YAML,
 * alad/loss.py:79-159 through alad/alad_model.py:386 -- as ONE call per direction, so that an eager drop-in module costs one
 * FFI crossing per direction.
 *   fwd: pack both sets (-> packed, kept by the caller for the backward), side GEMM + score kernel (-> S, Bi x Bi), the
 *        hinge's row / column statistics, then ONE kernel whose workgroups either recompute a non-zero pair of dloss/dS --
 *        the pairs follow from the statistics: (q, q), (q, hardest caption of image q), (hardest image of caption q, q) --
 *        into the backward's arg-max table, or run the hinge's element-wise pass (-> *loss, dS: (B, B) contiguous, fully
 *        written).  Square problems (Bi == Bc) of the classes the fp16 pair kernel covers (geom->mrows 32 / 48 with side rows
 *        or 64 without, <= 64 padded words; D % 4 == 0, D <= 1024), fp16 operands; anything else: ALADIN_ERR_UNSUPPORTED,
 *        and the caller composes pack + scores + aladin_hinge_fused + aladin_align_bwd.
 *   bwd: step 3 of aladin_align_bwd alone (the table is in the workspace), dS scaled by *gscale (the upstream gradient of
 *        the loss: a device scalar, may be NULL = 1).  flags: ALADIN_BWD_PARTNERS_FP16 and / or
 *        ALADIN_TRIPLET_BWD_BASE_WORKSPACE (`workspace` is the bwd_workspace aladin_heads_small_fwd_argmax filled, not the
 *        triplet workspace).
 * workspace: aladin_align_triplet_workspace_bytes(geom) -- side-GEMM scratch, hinge statistics, arg-max table, dS^T;
 * written by fwd, read by bwd: the caller keeps it (and packed, dS) untouched in between.  Both calls are asynchronous,
 * allocation-free and capturable in a HIP graph. */
#define ALADIN_TRIPLET_BWD_BASE_WORKSPACE 8
ALADIN_API size_t aladin_align_triplet_workspace_bytes(const aladin_align_geom* geom);
ALADIN_API int aladin_align_triplet_fwd(const aladin_set* im, const aladin_set* s, const aladin_align_geom* geom, float margin,
                                        const aladin_packed* packed, float* S, int64_t ldS, float* loss, float* dS,
                                        void* workspace, void* stream);
ALADIN_API int aladin_align_triplet_bwd(const aladin_set* im, const aladin_set* s, const aladin_align_geom* geom,
                                        const aladin_packed* packed, const float* dS, const float* gscale,
                                        const aladin_set_grad* d_im, const aladin_set_grad* d_s, void* workspace, int flags,
                                        void* stream);

/* The same forward for the small-batch loss heads (B <= 64; aladin_heads_small_fwd below): S is given (aladin_align_scores on
 * `packed`), one statistics launch + ONE kernel running the element-wise pass of all heads next to the pair recompute.
 * Hardest-negative hinge only; flags must include ALADIN_HEAD_ALIGN_HINGE.  Arguments as aladin_heads_small_fwd (no pair
 * list) followed by the alignment problem; D_emb is the width of the matching embeddings.  bwd_workspace:
 * aladin_align_bwd_workspace_bytes(geom, 0) -- it receives the arg-max table and dS^T; the backward is
 * aladin_align_triplet_bwd on that workspace. */
ALADIN_API int aladin_heads_small_fwd_argmax(const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, const float* S,
                                             int64_t ld_S, int D_emb, float margin, int flags, float temperature, float eps,
                                             float w_match, float w_align, float w_dist, float* M, float* terms, float* total,
                                             float* dM_hinge, float* dM_listnet, float* dS, void* heads_workspace,
                                             const aladin_set* im, const aladin_set* s, const aladin_align_geom* geom,
                                             const aladin_packed* packed, void* bwd_workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 'sum' / 'mean' pooling (alad/loss.py:120-123): sum_r sum_w <im^,s^> = <sum_r im^, sum_w s^>.
 * normsum: out[b][:] = sum over positions 1 .. len[b]-1-tail of the L2-normalised rows of x (B,N,D);
 * the scores are then aladin_sgemm_strided(out_img, out_cap^T).  bwd: d_x (B,N,D contiguous, fully
 * written) from d_out (B,D).
 * ------------------------------------------------------------------------------------------- */
ALADIN_API int aladin_normsum_fwd(const float* x, int64_t stride_b, int64_t stride_r, const int32_t* len, int B, int N, int D,
                       int tail, float* out, void* stream);
ALADIN_API int aladin_normsum_bwd(const float* x, int64_t stride_b, int64_t stride_r, const int32_t* len, int B, int N, int D,
                       int tail, const float* d_out, float* d_x, void* stream);

/* ---------------------------------------------------------------------------------------------
 * VSE++ hinge loss on a square score matrix -- Contrastive.compute_contrastive_loss,
 * reference alad/loss.py:42-67.  loss: 1 float.  dS (B x B, contiguous) may be NULL; it receives
 * dloss/dS (max_violation: +-1 at the hardest negatives and the diagonal, <= 3B non-zeros).
 * A NaN score makes the loss NaN, as the reference's clamp / max / sum do (dS is then unspecified on
 * the rows and columns holding a NaN cost).  workspace: aladin_hinge_workspace_bytes(B).
 * ------------------------------------------------------------------------------------------- */
ALADIN_API size_t aladin_hinge_workspace_bytes(int B);
ALADIN_API int aladin_hinge_fwd_bwd(const float* S, int64_t ldS, int B, float margin, int max_violation,
                         float* loss, float* dS, void* workspace, void* stream);

/* Same, additionally emitting the list of non-zero pairs of dS (pairs: B*B int32 holding i*B + j in
 * arbitrary order, pair_count: 1 int32) that aladin_align_bwd can consume directly. */
ALADIN_API int aladin_hinge_fused(const float* S, int64_t ldS, int B, float margin, int max_violation, float* loss,
                       float* dS, int32_t* pairs, int32_t* pair_count, void* workspace, void* stream);

/* ListNet score distillation -- DistillationLoss(mode='listnet'), reference alad/loss.py:427-445
 * (teacher detached :370; temperature 6 on the student only; eps 1e-10 inside the log).
 * d_student (B x B contiguous) may be NULL. */
ALADIN_API size_t aladin_listnet_workspace_bytes(int B);
ALADIN_API int aladin_listnet_fwd_bwd(const float* teacher, int64_t ld_t, const float* student, int64_t ld_s, int B,
                           float temperature, float eps, float* loss, float* d_student,
                           void* workspace, void* stream);

/* The fixed-weight sum of the loss terms (alad_model.py:450-453) and its backward without element-wise glue launches
 * (any batch size; the B <= 64 heads below do this inside their own kernels).
 *   aladin_loss_total    *total = wa * *a + wb * *b + wc * *c over up to three DEVICE scalars (NULL = absent)
 *   aladin_grad_combine  out[e] = *g * (wa * A[e] + wb * B[e]), e < n (A / B may be NULL; out may be NULL), and
 *                        *scale_out = *g * w_scale (may be NULL): the upstream gradient of the total applied to the
 *                        dLoss/dM matrices of the matching hinge and of ListNet, and turned into the alignment
 *                        backward's gscale, in one launch. */
ALADIN_API int aladin_loss_total(const float* a, float wa, const float* b, float wb, const float* c, float wc, float* total,
                                 void* stream);
ALADIN_API int aladin_grad_combine(int64_t n, const float* g, float wa, const float* A, float wb, const float* B, float* out,
                                   float w_scale, float* scale_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loss heads at the shipped batch size (B <= 64; every YAML trains with bs 32): three launches instead of the
 * ~15 few-microsecond kernels of the general path (csrc/small_batch.hip).  `flags` selects the heads:
 *   ALADIN_HEAD_MATCH_HINGE  M = img . cap^T (dot_sim, alad/loss.py:8-11) and the VSE++ hinge on it (:42-67)
 *   ALADIN_HEAD_ALIGN_HINGE  the same hinge on the alignment scores S (B x B, from aladin_align_scores)
 *   ALADIN_HEAD_LISTNET      ListNet distillation of M from the teacher S (:427-445; also computes M)
 * fwd (2 launches) writes M (B x B contiguous; needed by MATCH_HINGE / LISTNET), terms[3] = {matching hinge,
 * alignment hinge, listnet} (0 for a head that is off), *total = sum of the selected terms times w_* (the
 * fixed-weight sum of alad_model.py:450-453; may be NULL), and -- each optional -- dM_hinge, dM_listnet (B x B),
 * dS (B x B) with the non-zero pair list pairs / pair_count of the alignment hinge, in the form
 * aladin_align_bwd takes.  workspace: aladin_heads_small_workspace_bytes(B).
 * bwd (1 launch): d_img = C . cap, d_cap = C^T . img, C = *g_hinge * w_hinge * dM_hinge + *g_listnet * w_listnet *
 * dM_listnet + g_M (every term optional: NULL = absent; g_* are DEVICE scalars, g_M a (B x B) upstream gradient of M);
 * align_scale_out (may be NULL) receives *g_align * w_align, the `gscale` of the alignment backward.
 * d_img / d_cap: (B x D) contiguous, either may be NULL.
 * ------------------------------------------------------------------------------------------- */
#define ALADIN_HEAD_MATCH_HINGE 1
#define ALADIN_HEAD_ALIGN_HINGE 2
#define ALADIN_HEAD_LISTNET 4
ALADIN_API size_t aladin_heads_small_workspace_bytes(int B);
ALADIN_API int aladin_heads_small_fwd(const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, const float* S,
                                      int64_t ld_S, int B, int D, float margin, int max_violation, int flags, float temperature,
                                      float eps, float w_match, float w_align, float w_dist, float* M, float* terms, float* total,
                                      float* dM_hinge, float* dM_listnet, float* dS, int32_t* pairs, int32_t* pair_count,
                                      void* workspace, void* stream);
ALADIN_API int aladin_heads_small_bwd(const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, int B, int D,
                                      const float* dM_hinge, const float* g_hinge, float w_hinge, const float* dM_listnet,
                                      const float* g_listnet, float w_listnet, const float* g_M, int64_t ld_gM,
                                      const float* g_align, float w_align, float* align_scale_out, float* d_img, float* d_cap,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device-resident evaluation store (replaces the (N, 71, D) fp32 host buffers that encode_data fills,
 * reference alad/evaluation.py:119-130, and the per-query H2D copies of i2t / t2i :179,202,267,291).
 * A store holds, per sample, only positions [1, len - tail) of its set, L2-normalised like the pack
 * kernels and rounded once to fp16, contiguous by true length:
 *   rows (total_rows x aladin_store_row_width(D)) fp16; sample k = rows [offsets[k], offsets[k]+counts[k]).
 * aladin_store_append normalises one encoder batch (B, L, D; strides in elements) into rows at the
 * given per-sample offsets (int64, device); counts are max(0, lens[k] - 1 - tail) clipped to L - 1.
 * aladin_align_pack_store_x / _y build the max-side (xm, xe) / sum-side (y) operands of
 * aladin_align_scores for the samples ids[0..Bi) / ids[0..Bc) (ids NULL = 0, 1, 2, ...) under a
 * geometry whose Rq / Tq bound the counts; the operands -- hence the scores -- are bit-identical to
 * aladin_align_pack on the fp32 sets (no inverse norms: the store is forward-only).
 * Split stores (precision ALADIN_PRECISION_SPLIT): a row is [hi | lo], 2 * round_up(D, 64) halfs;
 * aladin_align_pack_store_x / _y take such rows when (and only when) geom->split.
 * ------------------------------------------------------------------------------------------- */
ALADIN_API int aladin_store_row_width(int D, int precision);      /* halfs per store row */
ALADIN_API int aladin_store_append(const float* sets, int64_t stride_b, int64_t stride_r, const int32_t* lens, int B, int L,
                                   int D, int tail, const int64_t* offsets, void* rows, int precision, void* stream);
ALADIN_API int aladin_align_pack_store_x(const void* rows, const int64_t* offsets, const int32_t* counts, const int32_t* ids,
                              const aladin_align_geom* g, void* xm, void* xe, void* stream);
ALADIN_API int aladin_align_pack_store_y(const void* rows, const int64_t* offsets, const int32_t* counts, const int32_t* ids,
                              const aladin_align_geom* g, void* y, void* stream);

/* l2norm -- reference alad/utils.py:134-139: out = X / sqrt(sum_dim1 X^2) on (rows, D), NO eps (a zero row
 * gives NaN, as the reference; F.normalize would give 0), and its backward.  out / d_x are contiguous. */
ALADIN_API int aladin_l2norm_fwd(const float* x, int64_t row_stride, int rows, int D, float* out, void* stream);
ALADIN_API int aladin_l2norm_bwd(const float* x, int64_t row_stride, const float* d_out, int64_t d_out_stride, int rows, int D,
                      float* d_x, void* stream);

/* ---------------------------------------------------------------------------------------------
 * aggregation = 'scan-sentences' -- reference alad/loss.py:136-149 (no shipped config uses it).
 * Per pair: relu(cosines) L2-normalised over regions, softmax over the caption's valid words for each
 * valid region, attended sentence vector, S = sum over regions of cos(region, attended vector).
 * Everything in fp32 (exact-fp32 MFMA GEMMs).  Same set / length / stride conventions as
 * aladin_align_bwd; R - 1 <= 96, T - 3 <= 96.  A caption without scored words gives NaN like the
 * reference.  aladin_scan_bwd recomputes the forward state itself and returns the gradient of the
 * length-masked expression (the reference's autograd is NaN on ragged batches and equal to this on
 * full-length ones); gscale (device scalar, may be NULL) multiplies dS.
 * ------------------------------------------------------------------------------------------- */
ALADIN_API size_t aladin_scan_workspace_bytes(int Bi, int Bc, int R, int T, int D, int backward);
ALADIN_API int aladin_scan_fwd(const float* im, int64_t im_stride_b, int64_t im_stride_r, const int32_t* im_len, const float* s,
                    int64_t s_stride_b, int64_t s_stride_t, const int32_t* s_len, int Bi, int Bc, int R, int T, int D,
                    float* S, int64_t ldS, void* workspace, void* stream);
ALADIN_API int aladin_scan_bwd(const float* im, int64_t im_stride_b, int64_t im_stride_r, const int32_t* im_len, const float* s,
                    int64_t s_stride_b, int64_t s_stride_t, const int32_t* s_len, int Bi, int Bc, int R, int T, int D,
                    const float* dS, int64_t ld_dS, const float* gscale, float* d_im, float* d_s, void* workspace,
                    void* stream);

/* The other modes of DistillationLoss, reference alad/loss.py:359-425 (teacher detached :370).
 * One workspace query covers the three of them.  d_student (B x B contiguous) may be NULL.
 *   mse          :371-373  mean((student*wb[0] + wb[1] - teacher)^2); wb = the module's learnable
 *                          pair (:366), a DEVICE pointer; d_wb (2 floats, may be NULL) receives its gradient
 *   contrastive  :401-425  as written: teacher diagonal zeroed, its row argmax selects whole columns
 *                          of cost_s and its column argmax whole rows of cost_im, diagonals kept
 *   ordinal      :374-399  per-row and per-column teacher sort, strided hinge on the student in that
 *                          order where teacher_sorted[p + stride] >= threshold; a side with no selected
 *                          position makes the loss NaN and contributes a zero gradient (as torch). B <= 8192 */
ALADIN_API size_t aladin_distill_workspace_bytes(int B);
ALADIN_API int aladin_distill_mse_fwd_bwd(const float* teacher, int64_t ld_t, const float* student, int64_t ld_s, int B,
                               const float* wb, float* loss, float* d_student, float* d_wb, void* workspace,
                               void* stream);
ALADIN_API int aladin_distill_contrastive_fwd_bwd(const float* teacher, int64_t ld_t, const float* student, int64_t ld_s, int B,
                                       float margin, float* loss, float* d_student, void* workspace, void* stream);
ALADIN_API int aladin_distill_ordinal_fwd_bwd(const float* teacher, int64_t ld_t, const float* student, int64_t ld_s, int B,
                                   float margin, float threshold, int stride, float* loss, float* d_student,
                                   void* workspace, void* stream);

/* Order-embedding similarity -- order_sim, reference alad/loss.py:20-26 (measure='order'):
 * scores[i][j] = -|| max(s_j - im_i, 0) ||_2, and its backward given d_scores and the forward's scores
 * (a pair without any violation has 0/0 = NaN gradient, as autograd).  d_im / d_s may be NULL. */
ALADIN_API int aladin_order_sim_fwd(const float* im, int64_t ld_im, const float* s, int64_t ld_s, int Bi, int Bc, int D,
                         float* scores, int64_t ld_scores, void* stream);
ALADIN_API int aladin_order_sim_bwd(const float* im, int64_t ld_im, const float* s, int64_t ld_s, int Bi, int Bc, int D,
                         const float* d_scores, int64_t ld_g, const float* scores, int64_t ld_scores,
                         float* d_im, int64_t ld_dim, float* d_s, int64_t ld_ds, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dot-product scores  C[m][n] = sum_k A[m*a_rs + k*a_cs] * B[k*b_rs + n*b_cs]   (fp32 in/out,
 * exact-fp32 MFMA).  With a_cs = 1, b_rs = 1 it is dot_sim  im.mm(s.t()), reference
 * alad/loss.py:8-11; the strides also give the two backward products.
 * ------------------------------------------------------------------------------------------- */
ALADIN_API int aladin_sgemm_strided(int M, int N, int K, const float* A, int64_t a_rs, int64_t a_cs,
                         const float* B, int64_t b_rs, int64_t b_cs, float* C, int64_t ldc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The 'entropy' loss term (csrc/entropy.hip): nearest-neighbour uniformity of the matching head's embeddings, reference
 * alad/alad_model.py:17-27 (pairwise_NNs_inner) and :410-421.  Row r of the virtual N x D matrix all_emb is img[r * ld_img + d]
 * for r < B and cap[(r - B) * ld_cap + d] otherwise, N = 2 B; cap == NULL: img alone, N = B (pairwise_NNs_inner of one matrix).
 *   nn[i]   = argmax_j (all_emb @ all_emb.T)[i][j] with the diagonal set to -1.0f (not -inf, as the reference: a row whose other
 *             products are all below -1 is its own neighbour), products in exact fp32 (fma chains in k order).
 *             TIES GO TO THE LOWEST INDEX, at every level of the reduction (the reference's torch.max leaves them open).
 *   dist[i] = || all_emb_i - all_emb_nn[i] + 1e-6f ||_2   (nn.PairwiseDistance(2): eps inside the norm)
 *   loss    = -(1 / N) * sum_i log(N * dist[i])
 * fwd: loss (1 float, may be NULL: neighbours and distances only), nn (N int32), dist (N floats).
 * bwd: d_img (B x D) and d_cap (B x D, unused when cap == NULL), contiguous, WRITTEN not accumulated, from fwd's nn and dist:
 *   with c_i = -*gscale / (N * dist[i]^2) and u_i = all_emb_i - all_emb_nn[i] + 1e-6f, row j receives c_j * u_j minus c_i * u_i of
 *   every i with nn[i] == j in ascending i (a gather; a self-neighbour row comes out exactly 0, as autograd's).
 *   gscale: a DEVICE scalar, the upstream gradient -- no host synchronisation.
 * Limits: B >= 1, D >= 1 (no alignment requirement), N <= ALADIN_NN_ENTROPY_MAX_N -- the workspace holds one (max, index) per row
 * and 64-column tile, 128 MiB there; beyond it ALADIN_ERR_UNSUPPORTED, checked before any launch.
 * workspace: aladin_nn_entropy_workspace_bytes(N) (0 outside the limits), the caller's.  Three launches forward, one backward, all
 * on `stream`; no allocation, no synchronisation, no atomics: deterministic and graph-capturable.
 * ------------------------------------------------------------------------------------------- */
#define ALADIN_NN_ENTROPY_MAX_N 32768
ALADIN_API size_t aladin_nn_entropy_workspace_bytes(int N);
ALADIN_API int aladin_nn_entropy_fwd(const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, int B, int D, float* loss,
                          int32_t* nn, float* dist, void* workspace, void* stream);
ALADIN_API int aladin_nn_entropy_bwd(const float* img, int64_t ld_img, const float* cap, int64_t ld_cap, int B, int D,
                          const int32_t* nn, const float* dist, const float* gscale, float* d_img, float* d_cap, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Symmetric cross-entropy (InfoNCE) with a learnable temperature on a B x B score matrix -- CrossEntropyCriterion, reference
 * alad/loss.py:190-201 (csrc/xent.hip).  With t = *log_temperature and L = S * e^t:
 *   loss = 1/(2B) [ sum_i (LSE_j L_ij - L_ii) + sum_j (LSE_i L_ij - L_jj) ]
 *   dS   = e^t (softmax_j L + softmax_i L - 2 I) / (2B)                 (B x B contiguous, WRITTEN; may be NULL)
 *   d_log_temperature = sum_ij dL_ij L_ij, dL = dS / e^t               (1 float; may be NULL)
 * Both gradients are those of an upstream gradient of 1.  log_temperature is a DEVICE scalar, read by the kernels: no host
 * synchronisation, and a replayed graph follows its current value.  The log-sum-exps are max-subtracted in fp32 (L of order
 * +-5000 is handled like L of order 1); the diagonal of dS is formed from each softmax's off-diagonal mass, so it is not rounded
 * away where both softmaxes are one-hot.  A NaN score makes the loss NaN (dS is then unspecified on its row and column); a
 * non-finite e^t propagates.  B = 1: loss, dS and d_log_temperature are exactly 0.
 * Limits: 1 <= B <= ALADIN_XENT_MAX_B (beyond it ALADIN_ERR_UNSUPPORTED), ldS >= B; checked before any launch.
 * workspace: aladin_xent_workspace_bytes(B) bytes (0 outside the limits), 16-byte aligned, the caller's.  Two launches on
 * `stream`; no allocation, no atomics, every sum in a fixed order: deterministic and graph-capturable.
 * ------------------------------------------------------------------------------------------- */
#define ALADIN_XENT_MAX_B 32768
ALADIN_API size_t aladin_xent_workspace_bytes(int B);
ALADIN_API int aladin_xent_fwd_bwd(const float* S, int64_t ldS, int B, const float* log_temperature, float* loss, float* dS,
                        float* d_log_temperature, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Semantic contrastive loss on a B x B score matrix with relevance-chosen positives -- SemanticContrastiveLoss, reference
 * alad/loss.py:203-270 (csrc/semantic.hip).  S: images x captions, row stride ldS, unit column stride.  rel: B x B relevances
 * aligned with S, element [i][j] at rel[i * rel_row_stride + j * rel_col_stride] (strides in floats, >= 0: a transposed or sliced
 * view is read in place).  draws: 2B int32 values in [0, 2^31 - 1) on the DEVICE.  Line v < B is row v, line B + j is column j:
 *   candidates of row i: the columns j with rel[i][j] > threshold, ascending; of column j: the rows, likewise.  NaN compares false.
 *   pos[v] = the (draws[v] mod n)-th of line v's n candidates.  n = 0: the line's DIAGONAL cell (the reference raises inside
 *            torch.randint(0, ..); a kernel cannot raise without a synchronisation).
 *   a1[i]  = S[i][pos[i]].
 *   a2[m]  = ALADIN_SEM_COLUMNS_ALIGNED: S[pos[B+m]][m].  Otherwise the reference's order (scores[cols_mask].view(B, 1).t() reads
 *            the chosen cells back row-major): the score at the m-th of the B cells (pos[B+j], j) sorted by (row, column); rank[j]
 *            is the place of column j's cell.  With diagonal-only positives both orders are the VSE++ hinge.
 *   cs[i][j] = max(margin + S[i][j] - a1[i], 0),  ci[i][j] = max(margin + S[i][j] - a2[j], 0); both 0 on the DIAGONAL (not at the
 *            chosen positive, as alad/loss.py:249-254) and, with ALADIN_SEM_MASK_POSITIVES (not in the reference: its TODO at :239),
 *            wherever rel[i][j] > threshold.
 *   loss   = sum cs + sum ci;  ALADIN_SEM_MAX_VIOLATION: sum_i max_j cs + sum_j max_i ci, TIES GO TO THE LOWEST INDEX.
 *   dS[i][j] = [cs active] + [ci active] - [pos[i] == j] nrow[i] - [pos[B+j] == i] ncol[rank[j]]   (B x B contiguous, WRITTEN; may
 *            be NULL), the gradient of an upstream gradient of 1: nrow / ncol count a line's active terms; under MAX_VIOLATION a
 *            line counts 1 if its maximum is > 0 and its active element is the arg-max.  Integer valued; no atomics.
 *   positives (2B int32; may be NULL) receives pos: every row's column, then every column's row.
 * A NaN cost makes the loss NaN (dS is then unspecified on its row and column).
 * Limits: 1 <= B <= ALADIN_SEM_MAX_B (beyond it ALADIN_ERR_UNSUPPORTED: the ranking of the column positives compares every pair
 * of columns), ldS >= B; checked before any launch.
 * workspace: aladin_semantic_hinge_workspace_bytes(B) bytes (0 outside the limits), 16-byte aligned, the caller's.  Four launches
 * on `stream` (select, rank, line statistics, finish), three with ALADIN_SEM_COLUMNS_ALIGNED (no ranking); draws and the threshold
 * comparison are read by the kernels: no host synchronisation, and a replayed graph follows the current draws.  No allocation, no
 * atomics, every sum in a fixed order: deterministic and graph-capturable.
 * ------------------------------------------------------------------------------------------- */
#define ALADIN_SEM_MAX_B 8192
#define ALADIN_SEM_MAX_VIOLATION 1
#define ALADIN_SEM_COLUMNS_ALIGNED 2
#define ALADIN_SEM_MASK_POSITIVES 4
ALADIN_API size_t aladin_semantic_hinge_workspace_bytes(int B);
ALADIN_API int aladin_semantic_hinge_fwd_bwd(const float* S, int64_t ldS, const float* rel, int64_t rel_row_stride,
                                  int64_t rel_col_stride, int B, float margin, float threshold, int flags, const int32_t* draws,
                                  float* loss, float* dS, int32_t* positives, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention distillation -- AttentionDistillationLoss, reference alad/loss.py:273-334 (csrc/attdistill.hip): the fine-grained head's
 * word-by-region attention against a teacher's, for every (image, caption) pair, without the (Bi, Bc, R - 1, T - 1) logits tensor.
 * With Rq = R - 1, Tq = T - 1, n_i = clamp(im.len[i] - 1, 0, Rq), m_j = clamp(s.len[j] - 1, 0, Tq) (no tail is dropped here) and
 *   L[i,j,w,r] = <s[j, w + 1], im[i, r + 1]> / sqrt(D)   (raw dot products),   logp = L - logsumexp_{r < n_i} L,
 *   P[i,j,w,r] = A[i,j,w,r] / max(sum_{r' < Rq} |A[i,j,w,r']|, 1e-12)          (A = teacher; the norm runs over ALL Rq regions),
 *   loss = (1 / N) sum_i sum_j sum_{w < m_j} sum_{r < n_i} [ xlogy(P, P) - P logp ],   N = Bi * sum_j m_j  (N = 0: loss 0),
 *   g    = (softmax_r L * sigma - P) / N,  sigma = sum_{r < n_i} P,
 *   d im[i, r + 1] = sum_j sum_w g s[j, w + 1] / sqrt(D),   d s[j, w + 1] = sum_i sum_r g im[i, r + 1] / sqrt(D);
 * slot 0 and positions past a length get exactly 0, the teacher gets no gradient.  Masked regions drop out of the loss (the
 * reference evaluates 0 * -inf there); an image without a valid region contributes nothing.
 * teacher: (Bi, Bc, Wt, Rt) fp32, element [i][j][w][r] at teacher[i * t_si + j * t_sj + w * t_sw + r] (strides in floats), read in
 * place; Wt >= Tq, Rt >= Rq, t_sw >= Rt.  The logits run on unit rows in split precision ([hi | lo] fp16, ~2^-22) times fp32 norms,
 * fp32 accumulation; the backward's second products run in fp32 on the raw rows.
 * fwd: three launches (pack, pairs, finish) -> *loss; leaves the operands, (LSE, 1 / L1, sigma) per (i, j, w) and N in `workspace`.
 * bwd: after fwd on the SAME arguments and workspace; one launch per output (d_im, d_s: either may be NULL), every row written
 *      exactly once; gscale: a DEVICE scalar, the upstream gradient.
 * Limits: Bi, Bc >= 1, R, T >= 2, Rq and Tq <= ALADIN_TILE_MAX_SCORED (beyond it ALADIN_ERR_UNSUPPORTED), D >= 1; checked before
 * any launch.  workspace: aladin_attdistill_workspace_bytes(...) bytes (0 outside the limits), 16-byte aligned, the caller's.  All
 * on `stream`; no allocation, no synchronisation, no atomics, every sum in a fixed order: deterministic and graph-capturable.
 * ------------------------------------------------------------------------------------------- */
ALADIN_API size_t aladin_attdistill_workspace_bytes(int Bi, int Bc, int R, int T, int D);
ALADIN_API int aladin_attdistill_fwd(const aladin_set* im, const aladin_set* s, int Bi, int Bc, int R, int T, int D, const float* teacher,
                          int64_t t_si, int64_t t_sj, int64_t t_sw, int Wt, int Rt, float* loss, void* workspace, void* stream);
ALADIN_API int aladin_attdistill_bwd(const aladin_set* im, const aladin_set* s, int Bi, int Bc, int R, int T, int D, const float* teacher,
                          int64_t t_si, int64_t t_sj, int64_t t_sw, int Wt, int Rt, const float* gscale, const aladin_set_grad* d_im,
                          const aladin_set_grad* d_s, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Head-mean attention window -- what the cross-encoder teacher reads of its last layer, reference alad/train.py:373-376 over
 * oscar/modeling/modeling_bert.py:47-53 (csrc/attn_window.hip), without any (N, H, L, L) probability tensor.  For every
 * sequence n and head h, with q, k that layer's query(x) / key(x) outputs (N, L, H * dh):
 *   S[n,h,i,j] = <q[n,i,h*dh:(h+1)*dh], k[n,j,h*dh:(h+1)*dh]> / sqrt(dh) + (1 - mask[n,j]) * (-10000)      j over ALL L columns
 *   P[n,h,i,:] = softmax_j S[n,h,i,:]
 *   out[n, i - row0, j - col0] = (1 / H) * sum_h P[n,h,i,j]       row0 <= i < row0 + W,  col0 <= j < col0 + Rw
 * The mask is ADDED, not selected: a masked column's exponential underflows to exactly 0 wherever the row attends one column,
 * and a sequence whose mask is all zero keeps a finite softmax over its raw scores, as the reference does.
 * q, k: fp32, element [n][i][c] at q[n * q_sn + i * q_sr + c] (strides in floats, unit inner stride, 4-byte aligned; 16-byte
 * loads are taken where pointer and strides allow), read in place.  mask: (N, L) of 0 / 1, row n at element n * mask_sn, unit
 * inner stride, int64 (mask_is_int64 != 0) or fp32; mask_ndim is the caller's mask rank and must be 2 (the (N, L, L) form of
 * the reference's model is not covered).  out: fp32, element [n][i][j] at out[n * o_sn + i * o_sr + j]; o_sr >= Rw and
 * o_sn >= W * o_sr, so a chunk of sequences can land in its slice of a larger tensor; every element written exactly once.
 * The logits run on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), the softmax in fp32, the heads are summed
 * in the order 0 .. H - 1.
 * Limits: N >= 1, 1 <= L <= ALADIN_ATTN_WINDOW_MAX_L, 1 <= H <= ALADIN_ATTN_WINDOW_MAX_HEADS, dh a multiple of 4 up to
 * ALADIN_ATTN_WINDOW_MAX_DH, 0 <= row0, W >= 1, row0 + W <= L and the same for the columns; outside them ALADIN_ERR_ARG, checked
 * before any launch.  One launch on `stream`; no workspace, no allocation, no atomics: deterministic and graph-capturable.
 * ------------------------------------------------------------------------------------------- */
#define ALADIN_ATTN_WINDOW_MAX_L 256
#define ALADIN_ATTN_WINDOW_MAX_DH 128
#define ALADIN_ATTN_WINDOW_MAX_HEADS 32
ALADIN_API int aladin_attn_window_mean(const float* q, int64_t q_sn, int64_t q_sr, const float* k, int64_t k_sn, int64_t k_sr,
                            const void* mask, int mask_ndim, int mask_is_int64, int64_t mask_sn, int N, int L, int H, int dh,
                            int row0, int W, int col0, int Rw, float* out, int64_t o_sn, int64_t o_sr, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Retrieval similarity matrix  sim = img @ cap.T  at evaluation scale (5000 x 25000 x 768) on the
 * 16-bit MFMA path with a hi/lo fp16 split (3 MFMAs per product, ~fp32 accuracy so that ranks
 * agree with the reference; operand rows are kept [hi | lo] and one accumulator chain runs hi.hi, lo.hi, hi.lo).  Replaces ims.mm(caps.t()), reference alad/recall_auxiliary.py:30,51
 * and torch.mm at alad/evaluation.py:196,285.
 * workspace: aladin_sim_workspace_bytes(n_img, n_cap, D).
 * ------------------------------------------------------------------------------------------- */
ALADIN_API size_t aladin_sim_workspace_bytes(int n_img, int n_cap, int D);
ALADIN_API int aladin_sim_matrix(const float* img, int64_t img_rs, const float* cap, int64_t cap_rs,
                      int n_img, int n_cap, int D, float* sim, int64_t ld_sim,
                      void* workspace, void* stream);

/* Ranks for both retrieval directions from sim (n_img x n_cap), COCO protocol: captions
 * caps_per_img*i .. caps_per_img*i + caps_per_img-1 belong to image i.  rank = number of strictly
 * larger scores (== argsort position, reference alad/recall_auxiliary.py:34-56 and
 * alad/evaluation.py:213-223,303-308, except on exact ties).
 *   rank_i2t[n_img]: best rank among the image's captions;  top1_i2t[n_img]: argmax caption
 *   rank_t2i[n_cap]: rank of the caption's image;           top1_t2i[n_cap]: argmax image */
ALADIN_API size_t aladin_recall_workspace_bytes(int n_cap);
ALADIN_API int aladin_recall_ranks(const float* sim, int64_t ld_sim, int n_img, int n_cap, int caps_per_img,
                        int32_t* rank_i2t, int32_t* top1_i2t, int32_t* rank_t2i, int32_t* top1_t2i,
                        void* workspace, void* stream);

/* Top-k lists: for each of n_q queries the indices (out_idx, n_q x k int32, -1 past n_c) and optionally the
 * scores (out_val, may be NULL) of its k largest candidates M[q * q_stride + c * c_stride], c < n_c, in
 * descending order, ties -> lower index first.  With M = sim (n_img x n_cap), q_stride = 1, c_stride = ld_sim,
 * k = 50 it is the `top50` table t2i returns, reference alad/evaluation.py:262,309.  n_c <= 36864. */
ALADIN_API int aladin_topk(const float* M, int64_t q_stride, int64_t c_stride, int n_q, int n_c, int k, int32_t* out_idx,
                float* out_val, void* stream);

/* Fused retrieval: the same four outputs as aladin_sim_matrix + aladin_recall_ranks straight from the
 * embeddings, without ever writing the (n_img x n_cap) score matrix (reference
 * alad/recall_auxiliary.py:30-56 / alad/evaluation.py:196-223,285-308 in one pass), bit-identical to the
 * two-step path whatever the data (integer and packed-max atomics: independent of the tile order).
 * A rank is a count of DECISIONS "score > ground truth", so the GEMM runs the hi.hi third of the split
 * product only and bounds, per pair and rigorously (Cauchy-Schwarz on the two dropped segments of the
 * actual fp16 operands + the fp32 rounding of their accumulation: 2^-14 |s| covers D <= 16384, larger D takes the
 * exact path), what the rest can add.  Scores that beat their ground truth by more than the bound are counted in
 * registers; pairs the bound does not decide, and possible arg-maxima, are continued to the exact score -- through a
 * list of up to 512 per 256 x 384 tile (a second kernel first drops the arg-max candidates that the certified lower
 * bounds of all tiles rule out), a whole tile in place when it holds more.  Cost: a third of the three-product GEMM
 * when ground truths stand clear of the bulk of the scores, ~0.6 of it at Recall@1 75 / 41 %, all of it when they
 * sit deep inside; the result never depends on it.
 * aladin_retrieval_ranks_exact: every tile takes the three-product path (for A/B runs and tests).
 * aladin_retrieval_stats_offset: byte offset, inside the workspace of the last call, of int32[9]: [0] tiles continued in
 * place, [1] pairs listed, [5] listed pairs whose chains were continued, [6] tiles that ran the analysis, [7] of those,
 * tiles that overflowed their list, [8] tiles that skipped it ([2..4]: diagnostic build only).
 * The four rank / arg-max OUTPUTS are deterministic.  The STATISTICS, and the time a call takes, are not: a tile decides
 * whether to skip its analysis from what the tiles that finished before it have reported so far (relaxed loads of [6], [7]
 * while other tiles of the same launch update them), so which tiles skip -- and with it [0], [1], [5], [8] -- depends on
 * scheduling.  Callers may rely on [5] <= [1], [7] <= [6], [0] >= [8] and on nothing else. */
ALADIN_API size_t aladin_retrieval_workspace_bytes(int n_img, int n_cap, int D);
ALADIN_API size_t aladin_retrieval_stats_offset(int n_img, int n_cap, int D);
ALADIN_API int aladin_retrieval_ranks(const float* img, int64_t img_row_stride, const float* cap, int64_t cap_row_stride, int n_img,
                           int n_cap, int D, int caps_per_img, int32_t* rank_i2t, int32_t* top1_i2t, int32_t* rank_t2i,
                           int32_t* top1_t2i, void* workspace, void* stream);
ALADIN_API int aladin_retrieval_ranks_exact(const float* img, int64_t img_row_stride, const float* cap, int64_t cap_row_stride, int n_img,
                           int n_cap, int D, int caps_per_img, int32_t* rank_i2t, int32_t* top1_i2t, int32_t* rank_t2i,
                           int32_t* top1_t2i, void* workspace, void* stream);

/* Top-k gallery search straight from the embeddings: what aladin_sim_matrix + aladin_topk(..., out_val) give, bit for bit,
 * without writing the (n_img x n_cap) score matrix and without aladin_topk's limit on the candidates of a query.
 *   dim = 1: the n_img images are the queries, the captions the gallery;  dim = 0: the n_cap captions query the images
 *   (the operands keep their roles, as in aladin_topk on sim with q_stride = 1).
 *   out_idx (n_q x k int32): the k best gallery indices, best first, ties -> lower index, -1 past the gallery size;
 *   out_val (n_q x k fp32, may be NULL): their scores, the bits aladin_sim_matrix would store, -inf past the gallery size.
 *   NaN scores sort last.
 * The gallery is cut into groups of 16 neighbours; one pass of the three-product GEMM leaves every group's maximum, the k
 * best groups of a query hold its k best scores, a second pass collects them (csrc/search.hip).  No atomics: deterministic.
 * Limits: 1 <= k <= 256; at most 36864 groups = 589824 gallery items (ALADIN_ERR_UNSUPPORTED above).
 * workspace: aladin_search_workspace_bytes(n_img, n_cap, D, k, dim) (0 for arguments the call refuses): the packed operands
 * of aladin_sim_workspace_bytes + 6 bytes per (query, group) + 72 per (query, selected group). */
ALADIN_API size_t aladin_search_workspace_bytes(int n_img, int n_cap, int D, int k, int dim);
ALADIN_API int aladin_search_topk(const float* img, int64_t img_row_stride, const float* cap, int64_t cap_row_stride, int n_img,
                       int n_cap, int D, int k, int dim, int32_t* out_idx, float* out_val, void* workspace, void* stream);

/* Gallery index: a matching-head gallery prepared ONCE and searched many times (csrc/search.hip).
 * aladin_search_index_build packs the n x D fp32 gallery into `index`, a caller-owned device buffer of
 * aladin_search_index_bytes(n, D) bytes: a header (the power-of-two scale of the gallery's absmax, build scratch) and the rows
 * in the [hi | lo] operand format of aladin_sim_matrix, zero-padded so that the gallery can stand on either side.  The layout does
 * not depend on whether the rows are images or captions; the fp32 gallery is not needed after the build.  The index is
 * IMMUTABLE: a search never writes into it, so searches on several streams may share one.  It cannot be appended to -- a
 * new absmax would change the scale of the rows already packed; build a new one.
 * aladin_search_index_topk: aladin_search_topk's contract, word for word, with the gallery taken from the index --
 *   dim = 1: the n_q rows of q are images and query an index of captions;  dim = 0: they are captions and query an index of images;
 *   out_idx (n_q x k int32) best first, ties -> lower index, -1 past the gallery size; out_val (may be NULL) the bits
 *   aladin_sim_matrix would store for the pair, -inf past the gallery size; NaN scores sort last; positions past n count as -inf.
 * Only the queries are packed per call, their scale from the absmax of the whole n_q x D matrix of the call.  Up to 32 queries
 * of D <= 768 take ONE pass over the gallery (every row fetched once, scores of all n_q x n pairs left in the workspace, the k
 * best groups gathered from there); anything else runs the passes of aladin_search_topk on the packed gallery.  The results do
 * not depend on the route.
 * Limits: 1 <= k <= 256; at most 36864 groups = 589824 gallery items (ALADIN_ERR_UNSUPPORTED above; _bytes and
 * _workspace_bytes return 0 for arguments the calls refuse).  Arguments are checked before any launch.  No allocation, no
 * synchronisation, no atomics: graph-capturable.
 * workspace: aladin_search_index_workspace_bytes(n_q, n, D, k, dim): the packed queries, 6 bytes per (query, group), 8 per
 * (query, selected group) and 64 bytes per (query, group) of scores on the one-pass route / 64 per (query, selected group) otherwise. */
ALADIN_API size_t aladin_search_index_bytes(int n, int D);
ALADIN_API int aladin_search_index_build(const float* x, int64_t row_stride, int n, int D, void* index, void* stream);
ALADIN_API size_t aladin_search_index_workspace_bytes(int n_q, int n, int D, int k, int dim);
ALADIN_API int aladin_search_index_topk(const void* index, int n, int D, const float* q, int64_t q_row_stride, int n_q, int k, int dim,
                       int32_t* out_idx, float* out_val, void* workspace, void* stream);

/* Two-stage retrieval: alignment-head (MrSw) scores of LISTED pairs straight from two embedding stores, and the order of
 * every query's re-scored shortlist (csrc/rescore.hip).  Work and memory are proportional to n_q * k; no operand is repacked.
 *   x_* / y_*: the image / caption store as aladin_align_pack_store_x / _y take it (rows, offsets, counts, ids: view position
 *   -> sample, may be NULL), n_x / n_y the samples in the view, x_max_count / y_max_count a bound of their counts known to
 *   the host (the kernel clamps to it), D and precision those of BOTH stores.
 *   dim = 1: the n_x images are the queries and cand holds caption positions; dim = 0: the n_y captions query the images.
 *   cand (n_q x k int32): positions in the gallery view, -1 (or anything outside the view) = no candidate.
 *   x_full: the count at which an image fills the padded set (padded_len - 1 - tail); a shorter image takes the zero fill
 *   into every max over its regions (alad/loss.py:116,124).
 *   out (n_q x k fp32): the score of image q and caption cand[q][s] (dim = 1) / of image cand[q][s] and caption q (dim = 0);
 *   -inf where there is no candidate; exactly 0.0 for a caption without scored words.
 * A pair's bits depend on the pair alone: not on its slot, the other candidates, k, the number of queries or dim.
 * Limits (ALADIN_ERR_UNSUPPORTED past them, checked before any launch): 1 <= k <= 256, counts <= 96 on both sides, D one
 * that aladin_store_row_width accepts.  No allocation, no synchronisation, no atomics: graph-capturable.
 *
 * aladin_rerank_order: out_idx / out_val (n_q x k) = cand / scores of every query in descending score order, ties -> the
 * earlier shortlist slot (a stable sort), entries without a candidate last as -1 / -inf; NaN counts as -inf. */
ALADIN_API int aladin_align_rescore(const void* x_rows, const int64_t* x_offsets, const int32_t* x_counts, const int32_t* x_ids, int n_x,
                         int x_max_count, const void* y_rows, const int64_t* y_offsets, const int32_t* y_counts,
                         const int32_t* y_ids, int n_y, int y_max_count, int D, int precision, int dim, int x_full,
                         const int32_t* cand, int k, float* out, void* stream);
ALADIN_API int aladin_rerank_order(const int32_t* cand, const float* scores, int n_q, int k, int32_t* out_idx, float* out_val,
                        void* stream);

/* The alignment behind the score of LISTED pairs (csrc/rescore.hip, the main loop of aladin_align_rescore with another epilogue):
 * for every word of the caption the region that carried the max over regions and its cosine, for every region of the image the
 * word it matches best, and the pair's score.
 *   x_* / y_*, D, precision, dim, x_full, cand, k: exactly as aladin_align_rescore takes them.
 *   y_full: the count at which a caption fills the padded set (the caption store's padded_len - 1 - tail).
 *   out_score (n_q x k fp32): the bits aladin_align_rescore writes for the same pair.
 *   word_region (int32) / word_cos (fp32), n_q x k x word_ld, word_ld >= y_max_count: entry w of pair (q, s) = the region with
 *   the largest cosine to word w, and that cosine.
 *   region_word (int32) / region_cos (fp32), n_q x k x region_ld, region_ld >= x_max_count: entry r = the word with the largest
 *   cosine to region r, and that cosine.
 *   out_score may be NULL; word_region and word_cos may be NULL together, region_word and region_cos may be NULL together;
 *   ALADIN_ERR_ARG if nothing is asked for or if one output of a pair is NULL without the other.
 * Index convention: an index is the position among the sample's SCORED rows (0 .. count - 1), i.e. position idx + 1 of the
 * padded set (slot 0 is the global embedding).
 * Tie rule: equal cosines -> the lowest index, in both directions.
 * Fill rule: a side with fewer positions than its padded set (x_full / y_full) competes with the zero fill of
 * alad/loss.py:116,124: where every real cosine is < 0 the entry is -1 / 0.0f; a real position wins a tie with the fill (a
 * cosine of exactly 0 keeps its index).  A side that fills its set keeps its negative maximum and a real index.
 * Entries from the sample's count up to word_ld / region_ld are -1 / 0.0f; a slot without a candidate gets score -inf and all
 * entries -1 / 0.0f; a caption without scored words gives score 0.0f, every region -1 / 0.0f.  Cosines of split stores are
 * the accumulator times 2^-28 (exact).  Each entry is written once; a pair's bits depend on the pair alone.
 * Limits and their checks are those of aladin_align_rescore (1 <= k <= 256, counts <= 96, D, LDS; ALADIN_ERR_UNSUPPORTED, before
 * any launch).  No allocation, no synchronisation, no atomics: graph-capturable. */
ALADIN_API int aladin_align_pair_map(const void* x_rows, const int64_t* x_offsets, const int32_t* x_counts, const int32_t* x_ids, int n_x,
                          int x_max_count, const void* y_rows, const int64_t* y_offsets, const int32_t* y_counts,
                          const int32_t* y_ids, int n_y, int y_max_count, int D, int precision, int dim, int x_full, int y_full,
                          const int32_t* cand, int k, float* out_score, int32_t* word_region, float* word_cos, int64_t word_ld,
                          int32_t* region_word, float* region_cos, int64_t region_ld, void* stream);

/* nDCG of ranked lists against a relevance matrix (csrc/ndcg.hip): dcg_from_ranking / ndcg_from_ranking of reference
 * alad/evaluate_utils/dcg.py:169-216 for n_q queries at once, without the two host argsorts per query.
 *   rel: query q's relevance row is rel[q * q_stride + c * c_stride], c < n_c -- the stride pair of aladin_topk, so the columns
 *   of a row-major matrix serve as queries without a transpose.
 *   ranking (int32): ranking[q * ld_rank + r], r < rank, is the gallery position ranked r-th.  -1, or anything outside
 *   [0, n_c), is "no item": it adds nothing, keeps its position's discount and is never dereferenced.
 * Per query, with k = min(rank, n_c): gain = exp2f(rel) - 1.0f in float32, discount = log2(r + 2) in double,
 *   dcg   = sum over r < k of gain(rel[ranking[r]]) / discount(r)
 *   ideal = the same sum over the k largest relevances in descending order
 *   ndcg  = ideal == 0 ? 0 : dcg / ideal
 * both sums in double, in ascending r, by one instruction sequence: a ranking that lists the k largest relevances in descending
 * order gives ndcg == 1.0 exactly.  ndcg / dcg / ideal: n_q doubles each; dcg may be NULL, ideal may be NULL without the flag.
 * flags & ALADIN_NDCG_IDEAL_GIVEN: `ideal` is an INPUT (it depends on the data set and on rank, not on the ranking); nothing is
 * staged or selected, the listed relevances are read straight from memory, and ndcg / dcg are bit-equal to the other path's.
 * Relevances are expected finite; what a NaN does to the result is unspecified.
 * Limits: n_c <= 36864 without the flag (ALADIN_ERR_UNSUPPORTED, checked before any launch); none on n_c with it.
 * No workspace, no allocation, no synchronisation, no atomics: deterministic and graph-capturable. */
#define ALADIN_NDCG_IDEAL_GIVEN 1
ALADIN_API int aladin_ndcg(const float* rel, int64_t q_stride, int64_t c_stride, int n_q, int n_c, const int32_t* ranking,
                int64_t ld_rank, int rank, int flags, double* ndcg, double* dcg, double* ideal, void* stream);

/* ROUGE-L relevance of query captions against images (csrc/rouge.hip): Rouge.score of reference alad/evaluate_utils/rouge.py:46-76
 * for every (query, image) pair at once -- the matrix alad/evaluate_utils/compute_relevance.py fills with one Python LCS table per
 * (query, reference caption), and the `rel` aladin_ndcg grades against.
 *   Captions are token-id sequences in CSR form: q_tok / g_tok (int32 ids, any non-negative value: there is no vocabulary limit;
 *   equal ids = equal tokens) with q_off (n_q + 1) / g_off (n_g + 1) int64 offsets, the last one the token count.  A caption longer
 *   than q_max_len / g_max_len is truncated to it on the device; offsets are clamped into their token array, so nothing outside the
 *   arrays is read whatever they hold.  A gallery caption of no tokens is skipped, a query of none scores 0.
 *   grp_off (n_img + 1 int64): image j owns the gallery captions grp_off[j] .. grp_off[j + 1] - 1 (ragged groups).
 *   q_rows (n_q int32) or NULL: query i is written to row q_rows[i] of `out` (NULL: row i) -- a length class of a larger query
 *   set is one launch.  The rows must exist; they are not checked.
 * Per pair, with m the query's length, l_i the lengths of the image's references and lcs_i the longest common subsequences:
 *   P = max_i lcs_i / m,   R = max_i (lcs_i / l_i),   out = (P != 0 && R != 0) ? ((1 + b2) * P) * R / (R + b2 * P) : 0
 * with b2 = 1.2 * 1.2, in double, in this association and without contraction, rounded to float once on the store: the bits of the
 * reference's float32 file.  A caption against an image that holds it scores exactly 1.0f.
 * out[row * ld_out + j], j < n_img, ld_out >= n_img: each element written exactly once, columns past n_img untouched.
 * flags & ALADIN_ROUGE_LCS: out = max_i lcs_i, the length itself (my_lcs of the reference file for one reference).
 * Limits: 1 <= q_max_len, g_max_len <= 256 (ALADIN_ERR_UNSUPPORTED, checked before any launch); the kernel takes 1, 2 or 4
 * 64-bit words per query by q_max_len <= 64 / 128 / 256.
 * No workspace, no allocation, no synchronisation, no atomics on global memory: deterministic and graph-capturable. */
#define ALADIN_ROUGE_LCS 1
ALADIN_API int aladin_rouge_l(const int32_t* q_tok, const int64_t* q_off, const int32_t* q_rows, int n_q, int q_max_len,
                   const int32_t* g_tok, const int64_t* g_off, int n_g, int g_max_len, const int64_t* grp_off, int n_img, float* out,
                   int64_t ld_out, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALADIN_HIP_H */
