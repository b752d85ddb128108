"""GPU tier (-m gpu): no output and no workspace of the library may depend on what its memory held before the call, and no
kernel may write outside them.

Every result tensor and every workspace of aladin_amd is torch.empty memory.  tests/helpers/alloc_probe.py carves each of them
out of a guarded buffer and runs every row of the table below three times:

  1. 'record' on the DONOR problem X: every length full, dense non-zero upstream gradients -- every position of every output and
     every counter, list and accumulator of the workspaces is left non-zero and VALID for these shapes;
  2. 'stale'  on the probed problem Y (same shapes, other values, ragged lengths: one sample at the smallest length the op accepts,
     one full, an empty one where the op allows it), every allocation seeded with what step 1 left in its counterpart;
  3. 'clean'  on Y with every allocation zero-filled.

Asserted per row: the outputs of 2 and 3 are bit-identical; every guard band (4096 bytes each side of every allocation) is intact
in all three passes; seeded == intercepted >= 1 and nothing passed through; and the outputs of 3 pass the op's own check against
its float64 / exact-integer reference, with the gates of the op's own test file (imported, not copied; where a test file states
a gate inline, its figure is quoted with the test's name).

Run-to-run non-determinism: retrieval_ranks(return_stats=True)'s statistics are documented as scheduling-dependent
(ops_retrieval.retrieval_ranks) and are not compared; its four rank / top-1 outputs are.  The hinge's pair list is filled
through an atomic counter: its order is unspecified, and it is compared as a sorted prefix of `count` entries against the
oracle instead.  Every other output is held to bit-equality.

What a donor has to be: a stale accumulator shows only if it changes the result.  Sums and counters always do; a packed
MAXIMUM (retrieval's best_i2t) only if the donor's value beats the probe's, hence the donor of the separate_ground_truths rows.

The words a kernel reads before writing them, per entry point of the table, and what initialises each (read from csrc/):
  alignment_scores (no grad; MrSw / MwSr    pack + score launches only: operands, inverse norms and the side scratch are stored
    / symm; tiles and long)                 whole by the pack / side GEMM before the score launch reads them; S: every element stored
  alignment_scores with gradients           aladin_align_bwd, list path: counter[0] and the dS statistics counter[1..3] by a
    (aladin_align_bwd; long sets:             hipMemsetAsync of 256 bytes (aladin_internal_compact_pairs); the table is written for
    aladin_internal_long_bwd)                 the listed pairs, which are the pairs the row step reads (dS != 0); d_im / d_s: every row
                                              stored, dropped and masked rows as zeros
  alignment_triplet_loss, max_violation     aladin_align_triplet_fwd / _bwd: hinge statistics by hinge_stats_kernel; table by the pair
                                              blocks (exactly the non-zeros of dS) and dS, dS^T by every element of the finish blocks
                                              of the same launch; no counter
  alignment_triplet_loss, sum               aladin_hinge_fused: pair_count zeroed by hinge_stats_kernel block 0, the launch before the
                                              finish pass adds to it; then aladin_align_bwd with the caller's list; dense table
                                              (B = 128): near-tie flags by hipMemsetAsync (aladin_internal_align_argmax), counter by
                                              hipMemsetAsync (table_all_pairs), counter[1..3] by bwd_compact_flagged_kernel's atomics
  alignment_scan_scores                     forward: xn, yn, A, G stored whole before the pair kernel; backward: dA by hipMemsetAsync,
                                              H, dxn, dyn stored whole (one workgroup per caption, two GEMMs) before they are read
  alignment_sum_scores                      no workspace (normsum forward / backward, the fp32 GEMM): every output row stored
  hinge_loss, match_hinge (B > 64)          val[2B] | arg[2B] by hinge_stats_kernel, pair_count as above
  listnet_loss, distillation_loss mse /     per-line or per-block statistics and partials, each stored before the finish launch sums
    ordinal, cross_entropy_scores,            them in a fixed order; no atomics
    nn_entropy_loss, match_cross_entropy
  distillation_loss contrastive             col_count / row_count (atomicAdd in tcon_pick_kernel) by one hipMemsetAsync
  order_scores, dot_scores, l2norm_rows     no workspace
  small_batch_loss_heads,                   statistics by heads_small_stats_kernel; table and dS^T as for the triplet node; pair_count
    small_batch_match_distill, match_hinge    (sum mode) zeroed by the statistics kernel before the finish pass adds to it
  attention_distillation_loss               head[0] by attdistill_finish_kernel, partial[] one plain store per pair, stats one per
                                              (pair, word) by the forward kernel; the backward stores every row of d_im / d_s
  attention_window_mean                     no workspace
  sim_matrix                                packed operands, norms and scale by the pack launches; padded rows zero-filled
  recall_ranks                              packed column maxima and rank_t2i by two hipMemsetAsync; rank_i2t / top1_i2t plain stores
  retrieval_ranks (screened, exact)         ranks (= counters), statistics, lob_i2t / lob_t2i zeroed by the pack grid
                                              (sim_pack_prologue); list_cnt: every tile stores its own count, zero included; best_i2t /
                                              best_t2i: plain stores of the ground-truth pairs by sim_pack_gt_kernel, or -- an image's
                                              rows missing the packer's 64 KB of LDS -- hipMemsetAsync of best_i2t + sim_gt_kernel
  topk_indices                              no workspace
  search_topk, search_index_topk,           gmax, table, sel, sorted, strip, cand: each stored whole by the pass before the one that
    build_search_index                        reads it; the index's padding rows are zero-filled by the packer
  align_rescore, rerank_order,              no workspace; -1 slots and positions past a count stored as -inf / -1 / 0
    align_pair_map
  ndcg_from_ranking, rouge_l_relevance      no workspace (LDS only)
  store append, compute_sim_matrix          every row of a sample stored by aladin_store_append; then alignment_scores' launches
aladin_hinge_workspace_bytes returns 16 B + 256: the kernels use exactly the 16 B bytes, the 256 are slack nothing touches."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import alad_oracle as O                  # noqa: E402
import alloc_probe as P                  # noqa: E402
import attdistill_numpy as A             # noqa: E402
import entropy_numpy as EN               # noqa: E402
import matrix_losses_numpy as ML         # noqa: E402
import ndcg_numpy as ND                  # noqa: E402
import rouge_numpy as RG                 # noqa: E402
import secondary_numpy as SH             # noqa: E402
import teacher_numpy as TN               # noqa: E402
import xent_numpy as XE                  # noqa: E402

pytestmark = pytest.mark.gpu

UP = 1.75                                # the upstream gradient of every scalar loss


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())


def I(x, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def F(t):
    return float(t.detach())


def rng_of(*key):
    return ML._rng('uninitialised', *key)


class Row:
    """name; make(variant in 'donor' / 'probe') -> inputs; call(inputs) -> tuple of every returned tensor and produced gradient;
    check(outputs of the clean pass, inputs of the probe); before_pass(): reset host state that steers the allocation sequence"""

    def __init__(self, name, make, call, check, before_pass=None, skip_outputs=()):
        self.name, self.make, self.call, self.check, self.before_pass, self.skip_outputs = name, make, call, check, before_pass, skip_outputs


ROWS = []


def add(name, make, call, check, **kw):
    assert name not in [r.name for r in ROWS], name
    ROWS.append(Row(name, make, call, check, **kw))


class precision_of_the_backward:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from aladin_amd import ops
        self.old = ops.set_backward_precision(self.mode)

    def __exit__(self, *exc):
        from aladin_amd import ops
        ops.set_backward_precision(self.old)


# ------------------------------------------------------------------------------------------------
# inputs: the donor is full and dense, the probe ragged
# ------------------------------------------------------------------------------------------------
def ragged_lengths(B, full, tail, seed):
    """sample 0 EMPTY (length 1 + tail: slot 0 and the dropped tail only, nothing scored -- test_degenerate_lengths_and_zero_vectors),
    sample 1 full (the packed layout is cut at the longest sample: it has to be the donor's), sample 2 with ONE scored position,
    the rest anywhere between"""
    assert B >= 3
    lens = [int(v) for v in rng_of('len', B, full, seed).integers(2 + tail, full + 1, B)]
    lens[0], lens[1], lens[2] = 1 + tail, full, 2 + tail
    return lens


def assert_degenerate_samples(x, S=None, d_im=None, d_s=None):
    """what test_degenerate_lengths_and_zero_vectors requires of the probe's image 0 / caption 0 (nothing scored: a row and a column
    of S exactly 0, gradients exactly 0) and of image 2 / caption 2 (one scored position: nothing past it)"""
    assert x['il'][0] == 1 and x['sl'][0] == 3 and x['il'][2] == 2 and x['sl'][2] == 4
    if S is not None:
        S = N(S)
        assert np.isfinite(S).all() and not S[0, :].any() and not S[:, 0].any()
    for g in (d_im, d_s):
        if g is not None:
            g = N(g)
            assert np.isfinite(g).all() and not g[0].any() and not g[2, 2:].any() and not g[:, 0].any()


def sets(variant, Bi, Bc, R, Tn, D, seed, structured=None):
    """dict(im, s, il, sl, w): float32 sets, lengths, a dense upstream gradient (Bi, Bc) without a zero"""
    from aladin_amd import synth
    donor = variant == 'donor'
    sd = seed + (0 if donor else 1000)
    if structured is None:
        im, s, _, _ = synth.alignment_batch(Bi, R, Tn, D, seed=sd, ragged=False, Bc=Bc)
    else:
        im, s, _, _ = synth.structured_alignment_batch(Bi, R, Tn, D, seed=sd, noise=structured[0 if donor else 1], ragged=False)
    il, sl = ([R] * Bi, [Tn] * Bc) if donor else (ragged_lengths(Bi, R, 0, sd), ragged_lengths(Bc, Tn, 2, sd + 1))
    w = rng_of('w', Bi, Bc, sd).standard_normal((Bi, Bc)).astype(np.float32)
    w = np.where(np.abs(w) < 0.05, np.float32(0.05), w)
    return dict(im=im, s=s, il=il, sl=sl, w=w)


TILE, LONG = (9, 7, 37, 27, 100), (4, 5, 130, 101, 64)


# ------------------------------------------------------------------------------------------------
# alignment scores
# ------------------------------------------------------------------------------------------------
def add_alignment_rows():
    def no_grad_row(shape, agg, prec):
        long = shape is LONG

        def call(x):
            from aladin_amd import ops
            with torch.no_grad():
                return (ops.alignment_scores(T(x['im']), T(x['s']), x['il'], x['sl'], agg, precision=prec),)

        def check(out, x):
            import test_gpu_parity as G
            import test_long_sets_gpu as LS
            ref = O.alignment_scores(x['im'], x['s'], x['il'], x['sl'], agg, dtype=np.float64)
            S = N(out[0])
            assert S.shape == ref.shape
            assert_degenerate_samples(x, S=out[0])
            if prec == 'split':                           # test_alignment_scores_shape_sweep / test_long_scores_match_the_oracle
                np.testing.assert_allclose(S, ref, rtol=3e-6, atol=3e-6)
            else:
                (LS if long else G).assert_scores_close(S, ref)
        add('alignment_scores[%s-%s-%s]' % ('long' if long else 'tiles', agg, prec), lambda v: sets(v, *shape, seed=11), call, check)

    def grad_row(shape, agg, mode):
        long = shape is LONG

        def call(x):
            from aladin_amd import ops
            with precision_of_the_backward(mode):
                a, b = T(x['im']).requires_grad_(True), T(x['s']).requires_grad_(True)
                S = ops.alignment_scores(a, b, x['il'], x['sl'], agg)
                (S * T(x['w'])).sum().backward()
            return S.detach(), a.grad, b.grad

        def check(out, x):
            import faithful_torch as FT
            import test_gpu_parity as G
            import test_long_sets_gpu as LS
            ra, rb = torch.from_numpy(x['im']).double().requires_grad_(True), torch.from_numpy(x['s']).double().requires_grad_(True)
            Sr = FT.alignment_scores_faithful(ra, rb, x['il'], x['sl'], agg)
            (Sr * torch.from_numpy(x['w']).double()).sum().backward()
            assert_degenerate_samples(x, *out)
            if long:                                      # test_long_gradients_of_the_other_poolings
                LS.assert_scores_close(N(out[0]), Sr.detach().numpy())
                LS.assert_grads_close(out[1], ra.grad.numpy(), mode)
                LS.assert_grads_close(out[2], rb.grad.numpy(), mode)
                LS.assert_dropped_rows_zero(out[1], out[2], x['il'], x['sl'])
            else:                                         # test_leftover_regions_as_side_rows
                G.assert_scores_close(N(out[0]), Sr.detach().numpy())
                G.assert_grads_close(out[1], ra.grad, mode, exact_atol=5e-5)
                G.assert_grads_close(out[2], rb.grad, mode, exact_atol=5e-5)
        add('alignment_scores_grad[%s-%s-%s]' % ('long' if long else 'tiles', agg, mode), lambda v: sets(v, *shape, seed=13), call, check)

    for shape in (TILE, LONG):
        for agg in ('MrSw', 'MwSr', 'symm'):
            for prec in ('fp16', 'split'):
                no_grad_row(shape, agg, prec)
        for agg in ('MrSw', 'MwSr', 'symm'):
            for mode in ('exact', 'fp16'):
                grad_row(shape, agg, mode)


def reset_density_probes():
    """the sum-of-violations hinge steers its backward by the pair counts of earlier steps (ops._DensityProbe), and allocates its
    pinned slots during the first LAG + 1 of them: every pass starts from a new probe"""
    from aladin_amd import ops
    ops._density_probe = ops._DensityProbe()
    ops._generic_probes.clear()


def add_triplet_rows():
    def row(B, mv, mode, dense=False):
        shape = (B, B, 34, 50, 64)

        def call(x):
            from aladin_amd import _lib, ops
            old = ops.DENSE_GEMM_FORCE
            ops.DENSE_GEMM_FORCE = True if dense else old       # the row step does not follow the captions' fill: one workspace size
            try:
                with precision_of_the_backward(mode):
                    a, b = T(x['im']).requires_grad_(True), T(x['s']).requires_grad_(True)
                    loss, S = ops.alignment_triplet_loss(a, b, x['il'], x['sl'], 0.2, mv)
                    (loss * UP).backward()
            finally:
                ops.DENSE_GEMM_FORCE = old
            if not mv:                                    # (the hardest-negative node never reaches _align_backward)
                assert bool(ops._LAST_BWD_FLAGS[0] & _lib.BWD_DENSE) == dense
            return loss.detach(), S.detach(), a.grad, b.grad

        def check(out, x):
            import test_gpu_parity as G
            loss, S, d_im, d_s = out
            S_np = N(S)
            ref_loss, dS = O.hinge_loss(S_np, 0.2, mv, return_grad=True)
            np.testing.assert_allclose(F(loss), ref_loss, rtol=1e-5, atol=1e-6)        # test_alignment_backward_shape_sweep
            assert_degenerate_samples(x, S=S)
            for g in (d_im, d_s):                         # (a hinge's dS may leave the one-position sample without a gradient)
                g = N(g)
                assert np.isfinite(g).all() and not g[0].any() and not g[2, 2:].any() and not g[:, 0].any()
            if not dense:
                G.assert_scores_close(S_np, O.alignment_scores(x['im'], x['s'], x['il'], x['sl']))
                dim, ds = O.alignment_scores_backward(x['im'], x['s'], x['il'], x['sl'], dS * UP)
                G.assert_grads_close(d_im, dim, mode)
                G.assert_grads_close(d_s, ds, mode)
                return
            # test_dense_backward_table_equals_the_per_pair_path: the table's gradients against one workgroup per pair -- equal with
            # the gather row step, within 1e-5 of the largest entry with the GEMM row step (another summation order)
            from aladin_amd import ops
            old, ops.DENSE_BACKWARD = ops.DENSE_BACKWARD, False
            try:
                with precision_of_the_backward(mode):
                    a, b = T(x['im']).requires_grad_(True), T(x['s']).requires_grad_(True)
                    ref_l, ref_S = ops.alignment_triplet_loss(a, b, x['il'], x['sl'], 0.2, mv)
                    (ref_l * UP).backward()
            finally:
                ops.DENSE_BACKWARD = old
            assert F(ref_l) == F(loss) and torch.equal(ref_S, S)
            for got, ref in ((d_im, a.grad), (d_s, b.grad)):
                assert float(ref.abs().sum()) > 0
                assert float((ref - got).abs().max()) <= 1e-5 * float(ref.abs().max())
        name = 'alignment_triplet_loss[B%d-%s-%s%s]' % (B, 'max_violation' if mv else 'sum', mode, '-dense_table' if dense else '')
        add(name, lambda v: sets(v, *shape, seed=17 + B, structured=(1.0, 3.0)), call, check, before_pass=reset_density_probes)

    for mv in (True, False):
        for mode in ('exact', 'fp16'):
            row(12, mv, mode)
    row(128, False, 'exact', dense=True)


SCAN_SHAPE = (4, 6, 20, 24, 32)


def secondary_sets(variant):
    """the scan / sum shape: the donor full, the probe with an image without a scored region, one with one region, a caption
    without a word (a NaN column of scan scores, as the reference's) and one with one word"""
    x = sets(variant, *SCAN_SHAPE, seed=19)
    if variant == 'probe':
        x['il'], x['sl'] = [1, 2, 20, 11], [3, 4, 24, 9, 24, 15]
    return x


def add_secondary_rows():
    def scan_call(x):
        from aladin_amd import ops
        a, b = T(x['im']).requires_grad_(True), T(x['s']).requires_grad_(True)
        S = ops.alignment_scan_scores(a, b, x['il'], x['sl'])
        (S * T(x['w'])).sum().backward()
        return S.detach(), a.grad, b.grad

    def scan_check(out, x):                               # test_scan_scores_and_gradients_match_the_oracle
        S, d_im, d_s = (N(t) for t in out)
        So, do_im, do_s = O.scan_sentences_scores(x['im'], x['s'], x['il'], x['sl'], dS=x['w'])
        np.testing.assert_allclose(S, So, equal_nan=True, **SH.SCAN_SCORE_TOL)
        scale = max(1e-3, float(np.abs(do_im).max()), float(np.abs(do_s).max()))
        np.testing.assert_allclose(d_im, do_im, rtol=SH.SCAN_GRAD_RTOL, atol=SH.SCAN_GRAD_ATOL * scale)
        np.testing.assert_allclose(d_s, do_s, rtol=SH.SCAN_GRAD_RTOL, atol=SH.SCAN_GRAD_ATOL * scale)
        fs, fi, fc = SH.floor_ratio(S, So), SH.floor_ratio(d_im, do_im), SH.floor_ratio(d_s, do_s)
        print('scan: scores %.3g d_im %.3g d_s %.3g of the largest entry' % (fs, fi, fc))
        assert fs <= SH.SCAN_GATE['scores'] and fi <= SH.SCAN_GATE['grads'] and fc <= SH.SCAN_GATE['grads']
        assert not S[0].any() and not d_im[0].any() and np.isnan(S[1:, 0]).all() and not d_s[0].any()
        assert not d_im[:, 0].any() and not d_s[:, 0].any() and not d_s[:, -2:].any()
    add('alignment_scan_scores', secondary_sets, scan_call, scan_check)

    def sum_row(mean):
        def call(x):
            from aladin_amd import ops
            a, b = T(x['im']).requires_grad_(True), T(x['s']).requires_grad_(True)
            S = ops.alignment_sum_scores(a, b, x['il'], x['sl'], mean=mean)
            (S * T(x['w'])).sum().backward()
            return S.detach(), a.grad, b.grad

        def check(out, x):                                # test_normsum_and_sum_mean_scores_match_float64
            S64, di64, ds64, (ui, uc) = SH.sum_scores(x['im'], x['s'], x['il'], x['sl'], x['w'], mean=mean)
            fs = SH.floor_ratio(N(out[0]), S64)
            fi = SH.scaled_error(N(out[1]), di64, SH.normsum_scales(x['im'], x['il'], 0, ui)[1])
            fc = SH.scaled_error(N(out[2]), ds64, SH.normsum_scales(x['s'], x['sl'], 2, uc)[1])
            print('sum scores mean=%d: scores %.3g d_im %.3g d_s %.3g' % (mean, fs, fi, fc))
            assert fs <= SH.NORMSUM_GATE['scores'] and fi <= SH.NORMSUM_GATE['grad'] and fc <= SH.NORMSUM_GATE['grad']
        add('alignment_sum_scores[%s]' % ('mean' if mean else 'sum'), secondary_sets, call, check)

    sum_row(False)
    sum_row(True)


# ------------------------------------------------------------------------------------------------
# matrix losses and small heads
# ------------------------------------------------------------------------------------------------
def add_matrix_rows():
    def hinge_row(B, mv):
        kinds = {'donor': 'normal', 'probe': 'quantised'}       # another violation pattern, exact ties, another margin's worth of them

        def make(v):
            S, margin = ML.hinge_scores(B, kinds[v])
            return dict(S=S, margin=ML.HINGE_MARGIN_Q)

        def call(x):
            from aladin_amd import ops
            loss, dS, (pairs, count) = ops._hinge_raw(T(x['S']), x['margin'], mv, True, want_pairs=True)
            st = T(x['S']).requires_grad_(True)
            out = ops.hinge_loss(st, x['margin'], mv)
            (2.5 * out).backward()
            return loss, dS, count, out.detach(), st.grad, pairs

        def check(out, x):                                # test_hinge_equals_the_oracle / test_hinge_pair_list
            loss, dS, count, loss2, grad, pairs = out
            ref_loss, ref_dS = O.hinge_loss(x['S'].astype(np.float64), x['margin'], mv, return_grad=True)
            ref_dS = ref_dS.astype(np.float32)
            for got in (F(loss), F(loss2)):
                assert abs(got - float(ref_loss)) <= ML.HINGE_LOSS_RTOL * abs(float(ref_loss))
            assert np.array_equal(N(dS), ref_dS) and np.array_equal(N(grad), 2.5 * ref_dS)
            n = int(count.item())
            assert n == np.count_nonzero(ref_dS) and np.array_equal(np.sort(N(pairs)[:n]), np.flatnonzero(ref_dS))
        # the pair list's ORDER is unspecified (atomics) and its tail past the count is not an output: compared as a sorted prefix
        add('hinge_loss[B%d-%s]' % (B, 'max_violation' if mv else 'sum'), make, call, check, skip_outputs=(5,))

    def listnet_row(B):
        def make(v):
            t, m = ML.listnet_inputs(B, 'mild')
            if v == 'donor':
                t, m = ML.listnet_inputs(B + 1000, 'mild')
                t, m = t[:B, :B].copy(), m[:B, :B].copy()
            return dict(t=t, m=m)

        def call(x):
            from aladin_amd import ops
            st = T(x['m']).requires_grad_(True)
            loss = ops.listnet_loss(T(x['t']), st)
            (0.3 * loss).backward()
            return loss.detach(), st.grad

        def check(out, x):                                # test_listnet_equals_the_oracle
            ref_loss, ref_dM = O.listnet_loss(x['t'].astype(np.float64), x['m'].astype(np.float64), return_grad=True)
            np.testing.assert_allclose(F(out[0]), float(ref_loss), **ML.LISTNET_LOSS_TOL)
            ML.assert_cancelling_grad_close(N(out[1]), 0.3 * ref_dM, 'listnet B=%d' % B, 'mild')
        add('listnet_loss[B%d]' % B, make, call, check)

    def distill_row(B, mode):
        def make(v):
            if v == 'donor':
                return dict(t=SH.teacher(B, 'negative' if mode == 'contrastive' else 'dups'), m=SH.student_jittered(B), margin=SH.MARGIN_N)
            return dict(t=SH.teacher(B, 'normal'), m=SH.student_normal(B) if mode == 'mse' else SH.quantised(B, 'student'), margin=SH.MARGIN_Q)

        def call(x):
            from aladin_amd import ops
            st = T(x['m']).requires_grad_(True)
            wb = T(np.asarray(SH.WB, np.float32)).requires_grad_(True) if mode == 'mse' else None
            loss = ops.distillation_loss(T(x['t']), st, mode, x['margin'], 0.1, 3, wb=wb)
            loss.backward()
            return (loss.detach(), st.grad) + ((wb.grad,) if wb is not None else ())

        def check(out, x):
            import test_secondary_heads_gpu as TS
            loss, dM = F(out[0]), N(out[1])
            if mode == 'mse':                             # test_mse_within_the_derived_bound
                (l64, dM64, dwb64), (bl, bM, bwb) = SH.mse_ref(x['t'], x['m'], SH.WB)
                assert abs(loss - l64) <= bl and (np.abs(dM - dM64) <= bM).all() and (np.abs(N(out[2]) - dwb64) <= bwb).all()
            elif mode == 'contrastive':                   # test_contrastive_gradient_equals_the_oracle
                ref_loss, ref_dM, _ = SH.contrastive_eval(x['t'], x['m'], x['margin'])
                assert abs(loss - ref_loss) <= SH.HINGE_LOSS_RTOL * abs(ref_loss) and np.array_equal(dM, ref_dM)
            else:                                         # test_ordinal_activity_and_gradient
                TS.assert_ordinal(loss, dM, x['t'], x['m'], x['margin'], 0.1, 3, 'ordinal B=%d' % B)
        add('distillation_loss[%s-B%d]' % (mode, B), make, call, check)

    def xent_row(B):
        def make(v):
            S, t = XE.matrix_inputs(B, 'scaled' if v == 'donor' else 'sharp')
            return dict(S=S, t=XE.LN100 if v == 'probe' else 0.5)

        def call(x):
            from aladin_amd import ops
            s = T(x['S']).requires_grad_(True)
            tt = torch.full((1,), x['t'], dtype=torch.float32, device=dev(), requires_grad=True)
            loss = ops.cross_entropy_scores(s, tt)
            loss.backward()
            return loss.detach(), s.grad, tt.grad

        def check(out, x):                                # test_matrix_op_matches_float64
            ref_loss, ref_dS, ref_dt = XE.xent_f64(x['S'], x['t'])
            np.testing.assert_allclose(F(out[0]), ref_loss, **XE.LOSS_TOL)
            np.testing.assert_allclose(out[2].item(), ref_dt, **XE.LOSS_TOL)
            XE.assert_grad_close(N(out[1]), ref_dS, 'sharp', B)
        add('cross_entropy_scores[B%d]' % B, make, call, check)

    def entropy_row(B):
        D = 70

        def make(v):
            img, cap = EN.case_inputs('a' if v == 'donor' else 'b', B, D, 41 + B, 97 + B)
            return dict(img=img, cap=cap)

        def call(x):
            from aladin_amd import ops
            a, b = T(x['img']).requires_grad_(True), T(x['cap']).requires_grad_(True)
            loss, nn = ops.nn_entropy_loss(a, b, return_neighbours=True)
            (loss * UP).backward()
            return loss.detach(), nn, a.grad, b.grad

        def check(out, x):                                # test_every_fixture_case_matches_the_reference
            import test_entropy_gpu as TE
            assert EN.gaps(np.concatenate([x['img'], x['cap']], 0)).min() >= EN.MIN_GAP
            loss, nn, _, r_img, r_cap = EN.entropy_loss(x['img'], x['cap'], g=UP)
            np.testing.assert_allclose(F(out[0]), loss, **TE.LOSS_TOL)
            assert np.array_equal(N(out[1]), nn)
            np.testing.assert_allclose(N(out[2]), r_img, **TE.GRAD_TOL)
            np.testing.assert_allclose(N(out[3]), r_cap, **TE.GRAD_TOL)
        add('nn_entropy_loss[B%d]' % B, make, call, check)

    for B in (33, 257):
        hinge_row(B, True)
        hinge_row(B, False)
        listnet_row(B)
        for mode in ('mse', 'contrastive', 'ordinal'):
            distill_row(B, mode)
        xent_row(B)
        entropy_row(B)


def add_embedding_rows():
    B, D = 33, 100

    def gemm_make(v):
        A_, B_, W = ML.gemm_inputs(B, B, D, 'normal' if v == 'donor' else 'integer')
        return dict(a=A_, b=B_, w=W)

    def order_call(x):
        from aladin_amd import ops
        a, b = T(x['a']).requires_grad_(True), T(x['b']).requires_grad_(True)
        sc = ops.order_scores(a, b)
        (sc * T(x['w'])).sum().backward()
        return sc.detach(), a.grad, b.grad

    def order_make(v):
        im, s, G = SH.order_inputs(B, B, D)
        if v == 'donor':
            im, s, G = SH.order_inputs(B + 1, B + 1, D)
            im, s, G = im[:B].copy(), s[:B].copy(), G[:B, :B].copy()
        return dict(a=im, b=s, w=G)

    def order_check(out, x):                              # test_order_scores_and_gradients_match_the_oracle
        ref = O.order_scores(x['a'], x['b'])
        di, ds = O.order_scores_backward(x['a'], x['b'], x['w'])
        sc, gi, gs = (N(t) for t in out)
        np.testing.assert_allclose(sc, ref, **SH.ORDER_SCORE_TOL)
        scale = max(1.0, float(np.abs(di).max()))
        np.testing.assert_allclose(gi, di, rtol=SH.ORDER_GRAD_RTOL, atol=SH.ORDER_GRAD_ATOL * scale)
        np.testing.assert_allclose(gs, ds, rtol=SH.ORDER_GRAD_RTOL, atol=SH.ORDER_GRAD_ATOL * scale)
        assert SH.floor_ratio(sc, ref) <= SH.ORDER_GATE[0] and SH.floor_ratio(gi, di) <= SH.ORDER_GATE[1] and \
            SH.floor_ratio(gs, ds) <= SH.ORDER_GATE[1]
    add('order_scores', order_make, order_call, order_check)

    def dot_call(x):
        from aladin_amd import ops
        a, b = T(x['a']).requires_grad_(True), T(x['b']).requires_grad_(True)
        C_ = ops.dot_scores(a, b)
        C_.backward(T(x['w']))
        return C_.detach(), a.grad, b.grad

    def dot_check(out, x):                                # check_dot: integers, every partial sum exact in fp32
        refs, _ = ML.gemm_refs(x['a'], x['b'], x['w'])
        for g, r in zip(out, refs):
            assert np.array_equal(N(g), r)
    add('dot_scores', gemm_make, dot_call, dot_check)

    def l2_make(v):
        xx, g = ML.l2norm_inputs(B, D)
        if v == 'donor':
            xx, g = ML.l2norm_inputs(B, D + 1)
            xx, g = xx[:, :D].copy(), g[:, :D].copy()
        return dict(x=xx, g=g)

    def l2_call(x):
        from aladin_amd import ops
        leaf = T(x['x']).requires_grad_(True)
        out = ops.l2norm_rows(leaf)
        out.backward(T(x['g']))
        return out.detach(), leaf.grad

    def l2_check(out, x):
        import test_matrix_losses_gpu as TM
        TM.check_l2norm(N(out[0]), N(out[1]), x['x'], x['g'], 'l2norm_rows')
    add('l2norm_rows', l2_make, l2_call, l2_check)

    def emb_make(v):
        if v == 'donor':
            img, cap = EN.case_inputs('a', B, D, 51, 0)
            return dict(img=img, cap=cap)
        img, cap, _ = ML.small_batch_inputs(B, D)           # multiples of 1/16: M and the hinge's costs exact in fp32
        return dict(img=img, cap=cap)

    def xent_make(v):                                     # the two families of tests/golden/xent.npz, at this row's shape
        img, cap = XE.case_inputs('matched' if v == 'donor' else 'independent', B, D, 71, 72)
        return dict(img=img, cap=cap, t=0.5 if v == 'donor' else 1.5)

    def match_hinge_row(mv):
        def call(x):
            from aladin_amd import ops
            a, b = T(x['img']).requires_grad_(True), T(x['cap']).requires_grad_(True)
            loss, M = ops.match_hinge(a, b, ML.HINGE_MARGIN_Q, mv)
            loss.backward()
            return loss.detach(), M.detach(), a.grad, b.grad

        def check(out, x):                                # test_small_batch_heads_equal_the_oracle (the hinge alone: exact)
            M_ref = O.dot_scores(x['img'].astype(np.float64), x['cap'].astype(np.float64))
            lh_ref, dMh = O.hinge_loss(M_ref, ML.HINGE_MARGIN_Q, mv, return_grad=True)
            assert np.array_equal(N(out[1]), M_ref)
            assert abs(F(out[0]) - float(lh_ref)) <= ML.HINGE_LOSS_RTOL * abs(float(lh_ref))
            assert np.array_equal(N(out[2]), dMh @ x['cap'].astype(np.float64)) and np.array_equal(N(out[3]), dMh.T @ x['img'].astype(np.float64))
        add('match_hinge[%s]' % ('max_violation' if mv else 'sum'), emb_make, call, check)

    match_hinge_row(True)
    match_hinge_row(False)

    def mxe_call(x):
        from aladin_amd import ops
        a, b = T(x['img']).requires_grad_(True), T(x['cap']).requires_grad_(True)
        tt = torch.full((1,), x['t'], dtype=torch.float32, device=dev(), requires_grad=True)
        loss, M = ops.match_cross_entropy(a, b, tt, return_scores=True)
        loss.backward()
        return loss.detach(), M.detach(), a.grad, b.grad, tt.grad

    def mxe_check(out, x):                                # test_criterion_matches_every_fixture_case: the restatement, family gate
        r64 = XE.criterion_f64(x['img'], x['cap'], x['t'])
        np.testing.assert_allclose(F(out[0]), r64[0], **XE.LOSS_TOL)
        np.testing.assert_allclose(out[4].item(), r64[3], **XE.LOSS_TOL)
        XE.assert_grad_close(N(out[2]), r64[1], 'independent', 'd im')
        XE.assert_grad_close(N(out[3]), r64[2], 'independent', 'd s')
        (M_ref, _, _), (bound, _, _) = ML.gemm_refs(x['img'], x['cap'], np.zeros((B, B)))      # check_dot: k u |a| |b|
        assert (np.abs(N(out[1]).astype(np.float64) - M_ref) <= bound).all()
    add('match_cross_entropy', xent_make, mxe_call, mxe_check)


SMALL = (32, 34, 50, 64)                 # (B, R, T, D) of the small-batch rows


def small_make(v):
    B, R, Tn, D = SMALL
    x = sets(v, B, B, R, Tn, D, seed=23, structured=(1.0, 3.0))
    if v == 'donor':
        x['img'], x['cap'] = EN.case_inputs('a', B, D, 61, 0)
        x['teacher'] = ML.listnet_inputs(B + 1, 'mild')[0][:B, :B].copy()
    else:
        x['img'], x['cap'], x['teacher'] = ML.small_batch_inputs(B, D)
    return x


def add_small_batch_rows():
    W = {'matching': 1.0, 'alignment': 0.5, 'distillation': 0.25}

    def heads_row(mv, mode):
        def call(x):
            from aladin_amd import ops
            with precision_of_the_backward(mode):
                leaves = [T(x[k]).requires_grad_(True) for k in ('img', 'cap', 'im', 's')]
                total, terms, S, M = ops.small_batch_loss_heads(*leaves, x['il'], x['sl'], ML.HINGE_MARGIN_Q, mv,
                                                                ('matching', 'alignment', 'distillation'), W)
                (total * UP).backward()
            return (total.detach(), terms, S, M) + tuple(t.grad for t in leaves)

        def check(out, x):
            """test_small_batch_single_node_step_equals_the_composition: the node against the same terms composed from the separate
            differentiable pieces (each of them a row of this table with its own oracle check), with that test's gates; S and M
            against the oracle as well"""
            import test_gpu_parity as G
            from aladin_amd import ops
            total, terms, S, M = out[:4]
            assert np.array_equal(N(M), O.dot_scores(x['img'].astype(np.float64), x['cap'].astype(np.float64)))
            G.assert_scores_close(N(S), O.alignment_scores(x['im'], x['s'], x['il'], x['sl']))
            assert_degenerate_samples(x, S=S)
            for g in out[6:]:
                g = N(g)
                assert np.isfinite(g).all() and not g[0].any() and not g[2, 2:].any() and not g[:, 0].any()
            with precision_of_the_backward(mode):
                t0 = [T(x[k]).requires_grad_(True) for k in ('img', 'cap', 'im', 's')]
                la, S0 = ops.alignment_triplet_loss(t0[2], t0[3], x['il'], x['sl'], ML.HINGE_MARGIN_Q, mv)
                lm, ld, _ = ops.small_batch_match_distill(t0[0], t0[1], S0, ML.HINGE_MARGIN_Q, mv)
                ref = lm * W['matching'] + la * W['alignment'] + ld * W['distillation']
                (ref * UP).backward()
            np.testing.assert_allclose(F(total), F(ref), rtol=1e-6)
            np.testing.assert_allclose(N(terms), [F(lm), F(la), F(ld)], rtol=1e-6, atol=1e-7)
            for got, leaf in zip(out[4:], t0):
                scale = float(leaf.grad.abs().max())
                assert scale > 0
                np.testing.assert_allclose(N(got), N(leaf.grad), rtol=1e-5, atol=1e-6 * scale)
        add('small_batch_loss_heads[%s-%s]' % ('max_violation' if mv else 'sum', mode), small_make, call, check,
            before_pass=reset_density_probes)

    heads_row(True, 'fp16')
    heads_row(True, 'exact')
    heads_row(False, 'fp16')

    def distill_row(mv):
        def call(x):
            from aladin_amd import ops
            a, b = T(x['img']).requires_grad_(True), T(x['cap']).requires_grad_(True)
            lh, ll, M = ops.small_batch_match_distill(a, b, T(x['teacher']), ML.HINGE_MARGIN_Q, mv)
            (ML.SMALL_G_HINGE * lh + ML.SMALL_G_LISTNET * ll).backward()
            return lh.detach(), ll.detach(), M.detach(), a.grad, b.grad

        def check(out, x):                                # test_small_batch_heads_equal_the_oracle
            img64, cap64 = x['img'].astype(np.float64), x['cap'].astype(np.float64)
            M_ref = O.dot_scores(img64, cap64)
            ll_ref, dMl = O.listnet_loss(x['teacher'].astype(np.float64), M_ref, return_grad=True)
            lh_ref, dMh = O.hinge_loss(M_ref, ML.HINGE_MARGIN_Q, mv, return_grad=True)
            assert np.array_equal(N(out[2]), M_ref)
            assert abs(F(out[0]) - float(lh_ref)) <= ML.HINGE_LOSS_RTOL * abs(float(lh_ref))
            np.testing.assert_allclose(F(out[1]), float(ll_ref), **ML.LISTNET_LOSS_TOL)
            coef = ML.SMALL_G_HINGE * dMh + ML.SMALL_G_LISTNET * dMl
            ML.assert_cancelling_grad_close(N(out[3]), coef @ cap64, 'd_img')
            ML.assert_cancelling_grad_close(N(out[4]), coef.T @ img64, 'd_cap')
        add('small_batch_match_distill[%s]' % ('max_violation' if mv else 'sum'), small_make, call, check)

    distill_row(True)
    distill_row(False)


# ------------------------------------------------------------------------------------------------
# attention distillation, attention window
# ------------------------------------------------------------------------------------------------
def add_attention_rows():
    cases = dict(A.GPU_CASES)

    def row(name, both):
        def make(v):
            kw = dict(cases[name])
            if v == 'donor':
                kw.update(seed=kw['seed'] + 100, im_kind='full', s_kind='full')
            return A.make_inputs(**kw)

        def call(x):
            from aladin_amd import ops
            im, s = T(x['im']).requires_grad_(True), T(x['s']).requires_grad_(both)
            loss = ops.attention_distillation_loss(im, s, x['im_len'], x['s_len'], T(x['teacher']))
            (loss * UP).backward()
            return (loss.detach(), im.grad) + ((s.grad,) if both else ())

        def check(out, x):                                # test_loss_and_gradients_match_the_float64_restatement
            ref = A.attdistill(x['im'], x['s'], x['im_len'], x['s_len'], x['teacher'], rounded='split')
            d_im = N(out[1])
            d_s = N(out[2]) if both else ref[2] * UP
            el, ei, es = A.errors((F(out[0]), d_im, d_s), (ref[0], ref[1] * UP, ref[2] * UP))
            print('%s: loss rel %.2e [gate %.1e]  d_im %.2e  d_s %.2e [gate %.1e]' % (name, el, A.GATE_LOSS_REL, ei, es, A.GATE_GRAD_MAXNORM))
            assert el <= A.GATE_LOSS_REL and ei <= A.GATE_GRAD_MAXNORM and es <= A.GATE_GRAD_MAXNORM
            n, m = A.counts(x['im_len'], x['s_len'], x['im'].shape[1] - 1, x['s'].shape[1] - 1)
            assert not d_im[:, 0].any() and all(not d_im[i, 1 + n[i]:].any() for i in range(len(n)))
            if both:
                assert not d_s[:, 0].any() and all(not d_s[j, 1 + m[j]:].any() for j in range(len(m)))
        add('attention_distillation_loss[%s-%s]' % (name, 'both' if both else 'd_im'), make, call, check)

    for name in ('b5x3_r15_t16_d20_ragged', 'b9x9_r33_t17_d64_ragged'):
        row(name, True)
        row(name, False)

    # the smallest kernel case whose window starts off a 16-row boundary (teacher_numpy.KERNEL_CASES is ordered by size of its
    # families; every case starts at row 1 or later: the first)
    name, (n_, H, dh, L, rows, cols) = next(c for c in TN.KERNEL_CASES if c[1][4][0] % 16)

    def win_make(v):
        q, k = TN.qk(n_, L, H, dh, 7 if v == 'probe' else 17)
        mask = TN.ragged_mask(n_, L, 9) if v == 'probe' else np.ones((n_, L), np.int64)
        return dict(q=q, k=k, mask=mask)

    def win_call(x):
        from aladin_amd import ops
        return (ops.attention_window_mean(T(x['q']), T(x['k']), I(x['mask'], np.int64), H, rows, cols),)

    def win_check(out, x):                                # test_window_matches_the_float64_restatement
        import test_teacher_gpu as TT
        floor, ref = TN.fp32_floor(x['q'], x['k'], x['mask'], H, rows, cols)
        TT.check(name, out[0], ref, floor)
        assert bool((N(out[0])[ref == 0.0] == 0.0).all())
    add('attention_window_mean[%s]' % name, win_make, win_call, win_check)


# ------------------------------------------------------------------------------------------------
# retrieval
# ------------------------------------------------------------------------------------------------
def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def counting_ranks(sim, cpi):
    """test_topk_gpu.test_recall_ranks_equal_counting: rank = #(scores strictly above the ground truth), top-1 = first maximum"""
    n_cap = sim.shape[1]
    cols = np.arange(n_cap)
    gt_t2i = sim[cols // cpi, cols]
    gt_i2t = gt_t2i.reshape(sim.shape[0], cpi).max(axis=1)
    return ((sim > gt_i2t[:, None]).sum(axis=1), sim.argmax(axis=1), (sim > gt_t2i[None, :]).sum(axis=0), sim.argmax(axis=0))


def add_retrieval_rows():
    n_img, cpi, D = 300, 5, 100

    def make(v, n_img=n_img, cpi=cpi, D=D, donor_copies=False):
        if v == 'donor':                                  # lists, overflowed tiles and continued chains all leave state
            import test_gpu_parity as G
            img, cap = G._adversarial_retrieval('bulk', n_img, cpi, D, seed=n_img + 7 * cpi)
            if donor_copies:
                cap[::cpi] = img                          # every image's first caption is the image: row maxima of 1.0
        else:                                             # clean, separated data
            rng = rng_of('retrieval')
            img = unit(rng.standard_normal((n_img, D)))
            cap = unit(np.repeat(img, cpi, axis=0) + 0.05 * rng.standard_normal((n_img * cpi, D)))
        return dict(img=img, cap=cap)

    def sim_call(x):
        from aladin_amd import ops
        return (ops.sim_matrix(T(x['img']), T(x['cap'])),)

    def sim_check(out, x):                                # test_recall_vs_reference: atol 2e-6 on unit-norm rows
        np.testing.assert_allclose(N(out[0]), x['img'].astype(np.float64) @ x['cap'].astype(np.float64).T, rtol=0, atol=2e-6)
    add('sim_matrix', make, sim_call, sim_check)

    def recall_make(v):
        import test_topk_gpu as TK
        sim = TK.int_scores((n_img, n_img * cpi), 5 if v == 'donor' else 6)      # small integers: ties everywhere
        return dict(sim=sim if v == 'probe' else sim + 0.5)

    def recall_call(x):
        from aladin_amd import ops
        return ops.recall_ranks(T(x['sim']), caps_per_img=cpi)

    def recall_check(out, x):
        for g, w in zip(out, counting_ranks(x['sim'], cpi)):
            np.testing.assert_array_equal(N(g), w.astype(np.int32))
    add('recall_ranks', recall_make, recall_call, recall_check)

    def ranks_row(exact, n_img=n_img, cpi=cpi, D=D, tag='', donor_copies=False):
        def call(x):
            from aladin_amd import ops
            *ranks, stats = ops.retrieval_ranks(T(x['img']), T(x['cap']), cpi, exact=exact, return_stats=True)
            assert stats['rescored_pairs'] <= stats['listed_pairs'] and stats['skipped_tiles'] <= stats['exact_tiles'] <= stats['tiles']
            return tuple(ranks)                           # the statistics depend on scheduling (documented): not compared

        def check(out, x):                                # test_fused_retrieval_ranks_equal_two_step + counting on the stored scores
            from aladin_amd import ops
            sim = ops.sim_matrix(T(x['img']), T(x['cap']))
            for g, w in zip(out, ops.recall_ranks(sim, cpi)):
                assert torch.equal(g, w)
            for g, w in zip(out, counting_ranks(N(sim), cpi)):
                np.testing.assert_array_equal(N(g), w.astype(np.int32))
            assert (N(out[0]) == 0).all() and (N(out[2]) == 0).all()      # separated data: every ground truth first
        add('retrieval_ranks[%s%s]' % ('exact' if exact else 'screened', tag), lambda v: make(v, n_img, cpi, D, donor_copies), call, check)

    ranks_row(False)
    ranks_row(True)
    # an image's row and its captions' do not fit the packer's 64 KB of LDS: the ground truths come from their own kernel, behind
    # the memset of the packed row maxima (test_fused_retrieval_ranks_equal_two_step's (20, 40, 768)).  Those are MAXIMA, of scores
    # in units of the call's own operand scale: a stale one shows only if it beats the probe's, so every image of this donor has
    # a caption equal to itself (cosine 1.0; the probe's ground truths reach 0.6 at this D)
    ranks_row(False, 20, 40, 768, '-separate_ground_truths', donor_copies=True)
    ranks_row(True, 20, 40, 768, '-separate_ground_truths', donor_copies=True)

    def topk_row(dim):
        def mk(v):
            import test_topk_gpu as TK
            q = TK.int_scores((4, 257), 257050 if v == 'probe' else 9)
            return dict(q=q if v == 'probe' else q * 2 + 1)

        def call(x):
            from aladin_amd import ops
            return (ops.topk_indices(T(x['q'] if dim == 1 else x['q'].T), 50, dim=dim),)

        def check(out, x):
            import test_topk_gpu as TK
            np.testing.assert_array_equal(N(out[0]), TK.topk_reference(x['q'], 50))
        add('topk_indices[dim%d]' % dim, mk, call, check)

    def search_mk(n_q, n_g, dim):
        def mk(v):
            import test_search_gpu as TS
            sd = 0 if v == 'probe' else 500
            q, g = TS.randn((n_q, D), 11 + n_q + sd), TS.randn((n_g, D), 12 + n_g + sd)
            return dict(q=q, g=g)
        return mk

    def sides(x, dim):
        return (T(x['q']), T(x['g'])) if dim == 1 else (T(x['g']), T(x['q']))

    def stored(x, dim, k):
        import test_search_gpu as TS
        from aladin_amd import ops
        return TS.stored_topk(ops.sim_matrix(*sides(x, dim)), k, dim)

    def search_check(dim, k):
        def check(out, x):                                # assert_equals_stored: int for int, bit for bit
            ref_idx, ref_val = stored(x, dim, k)
            assert torch.equal(out[0], ref_idx) and P.same_bits(out[1], ref_val)
        return check

    def search_row(dim):
        def call(x):
            from aladin_amd import ops
            return ops.search_topk(*sides(x, dim), 50, dim=dim, return_scores=True)
        add('search_topk[dim%d]' % dim, search_mk(37, 1003, dim) if dim == 1 else search_mk(1003, 37, dim), call, search_check(dim, 50))

    def index_row(n_q, dim):
        def call(x):
            from aladin_amd import ops
            index = ops.build_search_index(T(x['g']))
            # Of the index itself: its scale (the header's first float) and every packed row, the zero rows of the padding
            # included.  The rest of the header is the build's scratch (csrc/search.hip: "dead after it"); that no search reads
            # it is what this row shows -- the stale pass's index carries the donor build's header bytes, the clean one's zeros,
            # and the indices and scores above are the same bits.  The header's extent comes from the library's own size query:
            # an index is header + rows x padded width, so twice the size at D = 64 minus the size at D = 128 is the header.
            from aladin_amd import _lib
            lib, n = _lib.load(), x['g'].shape[0]
            header = 2 * int(lib.aladin_search_index_bytes(n, 64)) - int(lib.aladin_search_index_bytes(n, 128))
            assert 256 <= header < index.buf.numel()
            return ops.search_index_topk(index, T(x['q']), 50, dim=dim, return_scores=True) + (index.buf[:4], index.buf[header:])

        def check(out, x):
            search_check(dim, 50)(out[:2], x)
        add('search_index_topk[q%d-dim%d]' % (n_q, dim), search_mk(n_q, 1003, dim), call, check)

    for dim in (1, 0):
        topk_row(dim)
        search_row(dim)
        index_row(5, dim)
        index_row(40, dim)


def add_store_rows():
    """through the smallest stores of tests/test_rerank_gpu.py: test_last_sample_of_an_exactly_full_store -- the allocation of the
    rows ends with the last sample's last row, so the back guard band stands where the allocator's slack used to"""
    D = 64
    counts = {'probe': ([16, 5, 13], [9, 20, 11]), 'donor': ([13, 16, 5], [20, 11, 9])}      # the same totals and maxima: the same shapes

    def make(v):
        import test_rerank_gpu as TR
        ic, cc = counts[v]
        images, il = TR.make_sets(ic, 0, D, 31 if v == 'probe' else 41)
        captions, cl = TR.make_sets(cc, 2, D, 32 if v == 'probe' else 42)
        return dict(images=images, il=il, captions=captions, cl=cl, ic=ic, cc=cc, cand=np.array([[2, 0, 1, 2]] * 3, np.int32))

    def stores(x, precision):
        import test_rerank_gpu as TR
        si = TR.fill_store(x['images'], x['il'], 0, precision, batch=3, capacity_rows=sum(x['ic']))
        sc = TR.fill_store(x['captions'], x['cl'], 2, precision, batch=3, capacity_rows=sum(x['cc']))
        assert si.rows.shape[0] == si.n_rows == sum(x['ic']) and sc.rows.shape[0] == sc.n_rows == sum(x['cc'])
        return si, sc

    def row(precision, direction):
        def call(x):
            from aladin_amd import ops
            from aladin_amd.store import alignment_map_for_pairs, alignment_scores_for_pairs
            si, sc = stores(x, precision)
            cand = I(x['cand'])
            scores = alignment_scores_for_pairs(si, sc, cand, direction)
            order = ops.rerank_order(cand, scores)
            pa = alignment_map_for_pairs(si, sc, cand, direction)
            return (scores,) + tuple(order) + tuple(pa) + (si.rows, sc.rows)

        def check(out, x):
            import test_align_map_gpu as TA
            import test_rerank_gpu as TR
            ref = O.alignment_scores(x['images'], x['captions'], x['il'], x['cl'], dtype=np.float64)
            want = (ref if direction == 'i2t' else ref.T)[:, [2, 0, 1, 2]]
            TR.assert_close(N(out[0]), want, precision, D)
            idx, val = TR.np_stable(x['cand'], N(out[0]))                               # a stable sort of the device's own scores
            assert np.array_equal(N(out[1]), idx) and np.array_equal(N(out[2]), val)
            assert P.same_bits(out[3], out[0])                                        # the map's score: the rescore call's bits
            TA.check_map(tuple(N(t) for t in out[3:8]), x['cand'], direction, TA.Model(x['images'], x['il'], x['captions'], x['cl']),
                         precision, ref)
        add('store_rescore_rerank_pair_map[%s-%s]' % (precision, direction), make, call, check)

    for precision in ('split', 'fp16'):
        for direction in ('i2t', 't2i'):
            row(precision, direction)

    # store append + the alignment-mode evaluation grid on ragged stores of 8 x 12 samples
    def eval_make(v):
        import test_rerank_gpu as TR
        donor = v == 'donor'
        ic = [70, 33, 1, 48, 17, 50, 16, 35]
        cc = [68, 9, 0, 41, 1, 16, 17, 35, 8, 40, 12, 30]
        if donor:
            ic, cc = ic[::-1], cc[::-1]
        images, il = TR.make_sets(ic, 0, D, 51 + donor)
        captions, cl = TR.make_sets(cc, 2, D, 53 + donor)
        return dict(images=images, il=il, captions=captions, cl=cl, ic=ic, cc=cc)

    def eval_row(precision):
        def call(x):
            import test_rerank_gpu as TR
            from aladin_amd import evaluation as E
            si = TR.fill_store(x['images'], x['il'], 0, precision, batch=3, capacity_rows=sum(x['ic']))
            sc = TR.fill_store(x['captions'], x['cl'], 2, precision, batch=5, capacity_rows=sum(x['cc']))
            return E.compute_sim_matrix(si, sc, mode='alignment'), si.rows, sc.rows

        def check(out, x):
            import test_rerank_gpu as TR
            ref = O.alignment_scores(x['images'], x['captions'], x['il'], x['cl'], dtype=np.float64)
            TR.assert_close(N(out[0]), ref, precision, D)
        add('store_append_compute_sim_matrix[%s]' % precision, eval_make, call, check, before_pass=clear_eval_caches)

    eval_row('split')
    eval_row('fp16')


def clear_eval_caches():
    from aladin_amd import eval_grid
    from aladin_amd import evaluation as E
    E.clear_eval_cache()
    eval_grid._PLAN_CACHE.clear()


def add_ndcg_rouge_rows():
    # test_rank_past_the_gallery_and_entries_that_are_no_item: rank past the gallery, -1 entries, an all -1 row, entries outside
    n_q, n_c, rank = 6, 30, 40

    def ndcg_make(v):
        import test_ndcg_gpu as TD
        if v == 'donor':
            return dict(rel=TD.relevance_rows(n_q, n_c, 31) + np.float32(0.25), lists=TD.random_lists(n_q, n_c, rank, 32))
        rel, lists = TD.relevance_rows(n_q, n_c, 21), TD.random_lists(n_q, n_c, rank, 22)
        lists[2] = -1
        lists[3, [0, 5, 9]] = -1
        lists[4, [1, 2, 3, 4]] = [n_c, n_c + 1000, -2, np.iinfo(np.int32).min]
        lists[5, [0, 29]] = [np.iinfo(np.int32).max, 2 ** 20]
        return dict(rel=rel, lists=lists)

    def ndcg_row(dim):
        def call(x):
            from aladin_amd import ops
            return ops.ndcg_from_ranking(T(x['rel'] if dim == 1 else x['rel'].T), I(x['lists']), dim=dim, return_parts=True)

        def check(out, x):
            import test_ndcg_gpu as TD
            want = ND.ndcg_table(x['rel'], x['lists'])
            TD.assert_within_bound(N(out[0]), want[0], want[2], n_c, 'no-item entries dim %d' % dim)
            assert out[0][2].item() == 0.0 and out[1][2].item() == 0.0 and out[2][2].item() >= 1.0
        add('ndcg_from_ranking[dim%d]' % dim, ndcg_make, call, check)

    ndcg_row(1)
    ndcg_row(0)

    # test_ragged_groups_and_the_extreme_length_pairs: 13 queries against 70 images of 1 .. 7 captions
    def rouge_make(v):
        import test_rouge_gpu as TG
        rng = np.random.RandomState(11)
        groups = TG.ragged_groups(rng, 70, 1, 7)
        gallery = TG.random_seqs(rng, rng.randint(4, 21, size=groups[-1]), 12)
        queries = TG.random_seqs(rng, rng.randint(4, 21, size=13), 12)
        if v == 'donor':                                  # the same counts, longer captions over a small vocabulary: no zero relevance
            rng = np.random.RandomState(12)
            gallery = TG.random_seqs(rng, [21] * groups[-1], 3)
            queries = TG.random_seqs(rng, [21] * 13, 3)
        return dict(queries=queries, gallery=gallery, groups=groups)

    def rouge_row(lcs):
        def call(x):
            import test_rouge_gpu as TG
            return (TG.relevance(x['queries'], x['gallery'], x['groups'], lcs=lcs),)

        def check(out, x):
            import test_rouge_gpu as TG
            want = RG.relevance(x['queries'], x['gallery'], x['groups'], **({'fn': RG.max_lcs} if lcs else {}))
            TG.same_bits(out[0], want)
        add('rouge_l_relevance[%s]' % ('lcs' if lcs else 'f_measure'), rouge_make, call, check)

    rouge_row(False)
    rouge_row(True)


add_alignment_rows()
add_triplet_rows()
add_secondary_rows()
add_matrix_rows()
add_embedding_rows()
add_small_batch_rows()
add_attention_rows()
add_retrieval_rows()
add_store_rows()
add_ndcg_rouge_rows()


@functools.lru_cache(maxsize=None)
def inputs_of(name, variant):
    """a row's inputs: built once, shared between the passes and the check, never written to"""
    return next(r for r in ROWS if r.name == name).make(variant)


@pytest.mark.parametrize('row', ROWS, ids=[r.name for r in ROWS])
def test_outputs_do_not_depend_on_stale_memory_and_stay_inside_their_allocations(row):
    X, Y = inputs_of(row.name, 'donor'), inputs_of(row.name, 'probe')
    probes, stale, clean = P.run_three_passes(row.call, X, Y, before_pass=row.before_pass)      # (verifies guards and counts per pass)
    record, seeded, zeroed = probes
    print('%s: %d allocations per pass' % (row.name, record.intercepted))
    for p in probes:
        assert p.intercepted >= 1 and p.passed_through_device == 0, (p.mode, p.intercepted, p.passed_through_device)
        assert p.intercepted == record.intercepted
    assert seeded.seeded == seeded.intercepted >= 1 and record.seeded == zeroed.seeded == 0
    keep = [i for i in range(len(stale)) if i not in row.skip_outputs]
    P.assert_same_outputs(seeded, [stale[i] for i in keep], zeroed, [clean[i] for i in keep], names=['output %d' % i for i in keep])
    row.check(clean, Y)
