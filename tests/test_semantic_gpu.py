"""GPU tier (-m gpu): the semantic contrastive loss -- aladin_semantic_hinge_fwd_bwd (csrc/semantic.hip) through
ops.semantic_hinge_loss, loss.SemanticContrastiveLoss and loss.AlignmentSemanticContrastiveLoss.

References are never the code under test: the reference's recorded float64 run (tests/golden/semantic.npz,
make_golden_semantic.py) and the float64 restatement tests/helpers/semantic_numpy.py that the CPU tier pins to it.  Under the
input condition stated there dS and the positives are integers and must EQUAL the reference's; the loss is held to
HINGE_LOSS_RTOL = 1e-5, the existing hinge gate.  The quantised family (multiples of 1/16, margin 0.25) is exact in fp32 and must
equal the restatement, ties included.  Every value test prints its figures before asserting."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_alignment_inputs, load_golden
import alad_oracle as O

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import alloc_probe as P                  # noqa: E402
import matrix_losses_numpy as ML         # noqa: E402
import rouge_numpy as RG                 # noqa: E402
import semantic_numpy as X               # noqa: E402

pytestmark = pytest.mark.gpu

MEASURES = ['dot', 'cosine', 'order']
LOSS_RTOL = ML.HINGE_LOSS_RTOL
MAX_B = 8192                             # ALADIN_SEM_MAX_B


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(dev())               # a copy: the shared inputs are read-only


def D32(draws):
    return torch.from_numpy(np.array(draws, dtype=np.int32)).to(dev())


def bits(v):
    return v.contiguous().view(torch.int32)


def run_op(S, rel, draws, margin=X.MARGIN, threshold=X.THRESHOLD, max_violation=False, g=None, leaf=None, **kw):
    """ops.semantic_hinge_loss forward + backward -> (loss, dS, positives); S, rel, draws: device tensors (S a view of `leaf` when given)"""
    from aladin_amd import ops
    s = S.detach().requires_grad_(True) if leaf is None else S
    loss, pos = ops.semantic_hinge_loss(s, rel, margin, threshold, max_violation, draws=draws, return_positives=True, **kw)
    assert pos.dtype == torch.int32 and tuple(pos.shape) == (2 * S.shape[0],) and not pos.requires_grad
    (loss if g is None else loss * g).backward()
    return loss.detach(), (s if leaf is None else leaf).grad, pos


def assert_matches(got, want, what):
    """(loss, dS, pos) of the op against (loss, dS, pos) of a reference: figures first, then the gates"""
    loss, dS, pos = got[0].item(), got[1].cpu().numpy(), got[2].cpu().numpy()
    wrong = int((dS != want[1]).sum())
    print('semantic %s: loss %.9g ref %.9g rel diff %.2e;  dS entries differing %d of %d;  positives differing %d'
          % (what, loss, want[0], abs(loss - want[0]) / max(abs(want[0]), 1e-30), wrong, dS.size, int((pos != want[2]).sum())))
    assert np.array_equal(pos, want[2]), what
    assert wrong == 0, what
    np.testing.assert_allclose(loss, want[0], rtol=LOSS_RTOL, atol=0)


@functools.lru_cache(maxsize=None)
def fixture():
    """(golden, matrix cases [(ci, B, family, S, rel, draws)], class cases [(ci, measure, B, D, im, s, rel, draws)]): inputs rebuilt
    from the recorded seeds, checksums checked; shared, never written to"""
    g = load_golden('semantic')
    same = lambda got, want: abs(got - float(want)) <= 1e-9 * max(1.0, abs(float(want)))      # noqa: E731
    mats, classes = [], []
    for ci, ((B, fam), seed) in enumerate(zip(g['matrix_cases'], g['matrix_seeds'])):
        S, rel, draws = X.matrix_inputs(int(B), X.FAMILIES[int(fam)], int(seed))
        assert same(X.checksum(S), g['m%d_S_checksum' % ci]) and same(X.checksum(rel), g['m%d_rel_checksum' % ci]) and np.array_equal(draws, g['m%d_draws' % ci])
        mats.append((ci, int(B), X.FAMILIES[int(fam)], S, rel, draws))
    for ci, ((m, B, D), seed) in enumerate(zip(g['class_cases'], g['class_seeds'])):
        im, s, rel, draws = X.class_inputs(MEASURES[int(m)], int(B), int(D), int(seed))
        assert same(X.checksum(im), g['c%d_im_checksum' % ci]) and same(X.checksum(s), g['c%d_s_checksum' % ci]) and np.array_equal(draws, g['c%d_draws' % ci])
        classes.append((ci, MEASURES[int(m)], int(B), int(D), im, s, rel, draws))
    assert len(mats) == len(X.SIZES) * len(X.FAMILIES) and len(classes) == len(X.CLASS_CASES)
    return g, mats, classes


@functools.lru_cache(maxsize=None)
def restated(B, family, seed, max_violation, order='reference', mask_positives=False, kind='grid'):
    """(S, rel, draws, margin, float64 (loss, dS, pos)) of a helper input: computed once, shared, never written to.  kind 'grid': the
    2^-16 grid with margin 0.2; 'quantised': the project's multiples of 1/16 with margin 0.25"""
    S, rel, draws = X.matrix_inputs(B, family, seed)
    margin = X.MARGIN
    if kind == 'quantised':
        S, margin = ML.hinge_scores(B, 'quantised')
    ref = X.semantic_f64(S, rel, margin, X.THRESHOLD, draws, max_violation, order, mask_positives)
    if kind == 'grid':
        # against the restatement, which shares the lowest-index rule, an exact tie of equal scores is no ambiguity
        min_x, gap, ok = X.condition_figures(S, rel, margin, X.THRESHOLD, draws, max_violation, order, mask_positives, exact_ties=True)
        assert ok, (B, family, seed, min_x, gap)
    for a in (S, rel, draws, ref[1], ref[2]):
        a.setflags(write=False)
    return S, rel, draws, margin, ref


def test_matrix_op_matches_every_fixture_case():
    """Fails without the feature: ops has no semantic_hinge_loss."""
    g, mats, _ = fixture()
    for ci, B, fam, S, rel, draws in mats:
        for mv in X.MODES:
            p = 'm%d_%s_' % (ci, 'max' if mv else 'sum')
            got = run_op(T(S), T(rel), D32(draws), max_violation=mv)
            assert_matches(got, (float(g[p + 'loss']), g[p + 'dS'], g[p + 'pos']), 'fixture matrix %d B %d %s %s' % (ci, B, fam, 'max' if mv else 'sum'))
            if B == 1:
                assert got[0].item() == 0.0 and not got[1].any()


def run_class(crit, im, s, rel, draws):
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    loss, scores = crit(a, b, T(rel), return_similarity_mat=True, draws=D32(draws))
    scores.retain_grad()
    loss.backward()
    return loss.detach(), scores.grad, a.grad, b.grad


def test_class_matches_every_fixture_case_with_each_measure():
    from aladin_amd.loss import SemanticContrastiveLoss
    g, _, classes = fixture()
    assert sorted({m for _, m, *_ in classes}) == sorted(MEASURES)
    for ci, measure, B, D, im, s, rel, draws in classes:
        for mv in X.MODES:
            p = 'c%d_%s_' % (ci, 'max' if mv else 'sum')
            crit = SemanticContrastiveLoss(margin=X.MARGIN, threshold=X.THRESHOLD, measure=measure, max_violation=mv)
            loss, dS, d_im, d_s = run_class(crit, im, s, rel, draws)
            want_dS = g[p + 'dS'].astype(np.float64)
            wrong = int((dS.cpu().numpy() != want_dS).sum())
            print('semantic class %d %-6s (%2d, %2d) %s: loss %.9g ref %.9g;  dS entries differing %d' % (ci, measure, B, D, 'max' if mv else 'sum',
                                                                                                    loss.item(), float(g[p + 'loss']), wrong))
            assert wrong == 0
            np.testing.assert_allclose(loss.item(), float(g[p + 'loss']), rtol=LOSS_RTOL, atol=0)
            for got, key in ((d_im, 'dim'), (d_s, 'ds')):
                ref = g[p + key].astype(np.float64)
                if measure == 'dot':
                    # integers times multiples of 2^-6, summed far below 2^24 units: exact in fp32 in any order (and in the fixture's float32)
                    assert np.array_equal(got.cpu().numpy(), ref), (ci, key)
                else:
                    assert (np.abs(got.cpu().numpy() - ref) <= ML.l2norm_bwd_tol(ref)).all(), (ci, key)


@pytest.mark.parametrize('family', X.FAMILIES)
@pytest.mark.parametrize('mv', X.MODES, ids=['sum', 'max'])
def test_matrix_op_matches_the_restatement_past_one_strip_and_one_chunk(family, mv):
    """B = 1025: 17 column strips, five 256-column chunks of the finish pass, 65 wave-line blocks; the fixture sizes are covered by
    test_matrix_op_matches_every_fixture_case (the CPU tier holds restatement == fixture there)."""
    S, rel, draws, margin, ref = restated(1025, family, 0, mv)
    assert_matches(run_op(T(S), T(rel), D32(draws), max_violation=mv), ref, 'B 1025 %s %s' % (family, 'max' if mv else 'sum'))


@pytest.mark.parametrize('B', [16, 17, 48, 49, 113])
def test_matrix_op_matches_the_restatement_at_the_line_walk_edges(B):
    """The edges of the walk sem_stats_kernel shares (line_walk.hpp) that the sizes above miss: 16 / 17, the last block of 16 wave-rows
    full and one over; 48 / 49, the last size at which a strip's waves run the tail loop only and the first at which wave 0 has four
    rows in flight; 113, both loops in waves 1 to 15."""
    for mv in X.MODES:
        S, rel, draws, margin, ref = restated(B, 'dense', 0, mv)
        assert_matches(run_op(T(S), T(rel), D32(draws), max_violation=mv), ref, 'B %d dense %s' % (B, 'max' if mv else 'sum'))


@pytest.mark.parametrize('B', [5, 65, 257])
def test_quantised_family_equals_the_restatement_ties_included(B):
    for mv in X.MODES:
        for order in ('reference', 'aligned'):
            S, rel, draws, margin, ref = restated(B, 'dense', 0, mv, order, kind='quantised')
            assert margin == 0.25
            if mv and B >= 65:
                assert ML.hinge_tied_rows(S, margin) > 0                                  # ties are there to be broken
            got = run_op(T(S), T(rel), D32(draws), margin=margin, max_violation=mv, column_positives=order)
            assert_matches(got, ref, 'quantised B %d %s %s' % (B, 'max' if mv else 'sum', order))
            if B <= 65:
                assert got[0].item() == ref[0]                                             # multiples of 1/16 far below 2^24 units: exact


@pytest.mark.parametrize('family', ['groups', 'dense'])
def test_mask_positives_and_aligned_columns(family):
    B = 65
    for mv in X.MODES:
        for order, mask in (('aligned', False), ('reference', True), ('aligned', True)):
            S, rel, draws, margin, ref = restated(B, family, 0, mv, order, mask)
            got = run_op(T(S), T(rel), D32(draws), max_violation=mv, column_positives=order, mask_positives=mask)
            assert_matches(got, ref, 'B %d %s %s %s mask %d' % (B, family, 'max' if mv else 'sum', order, mask))
    plain = restated(B, family, 0, False)[4]
    assert plain[0] != restated(B, family, 0, False, 'aligned')[4][0] and plain[0] > restated(B, family, 0, False, 'reference', True)[4][0]


def test_a_line_without_candidates_falls_back_to_its_diagonal_cell():
    B = 65
    S, rel, draws, margin, _ = restated(B, 'dense', 0, False)
    rel = rel.copy()
    rel[7, :] = 0.1                                                                        # row 7 and column 40: nothing above the threshold
    rel[:, 40] = np.nan                                                                    # NaN compares false
    rel[64, :] = 0.0
    for mv in X.MODES:
        ref = X.semantic_f64(S, rel, margin, X.THRESHOLD, draws, mv)
        assert ref[2][7] == 7 and ref[2][64] == 64 and ref[2][B + 40] == 40
        assert X.condition_figures(S, rel, margin, X.THRESHOLD, draws, mv, exact_ties=True)[2]
        assert_matches(run_op(T(S), T(rel), D32(draws), max_violation=mv), ref, 'no candidates %s' % ('max' if mv else 'sum'))
    # nothing anywhere: the VSE++ hinge
    none = torch.zeros((B, B), device=dev())
    got = run_op(T(S), none, D32(draws))
    want_loss, want_dS = O.hinge_loss(S.astype(np.float64), margin, False, return_grad=True)
    assert_matches(got, (float(want_loss), want_dS, np.tile(np.arange(B), 2)), 'no candidates at all')


def test_relevance_views_are_read_in_place_and_score_views_send_the_gradient_to_the_base():
    B = 65
    for mv in X.MODES:
        S, rel, draws, margin, ref = restated(B, 'dense', 0, mv)
        want = run_op(T(S), T(rel), D32(draws), max_violation=mv)
        assert_matches(want, ref, 'contiguous')
        # (a) relevances as the transpose of a (captions x images) matrix -- what rouge.relevance_matrix(...).t() is
        rel_t = T(rel.T.copy()).t()
        assert rel_t.stride() == (1, B)
        # (b) a column slice of a wider matrix, (c) every second row and column
        wide = torch.full((B, B + 9), 0.9, device=dev())
        wide[:, 4:4 + B] = T(rel)
        sparse = torch.full((2 * B, 2 * B), 0.9, device=dev())
        sparse[::2, ::2] = T(rel)
        for view in (rel_t, wide[:, 4:4 + B], sparse[::2, ::2]):
            assert not view.is_contiguous()
            got = run_op(T(S), view, D32(draws), max_violation=mv)
            for u, v in zip(got, want):
                assert torch.equal(bits(u), bits(v))
        # scores: a row-strided view is used in place, a column-strided one is copied; the gradient lands in the base either way
        base = torch.zeros((B, B + 5), device=dev())
        base[:, 2:2 + B] = T(S)
        base.requires_grad_(True)
        got = run_op(base[:, 2:2 + B], T(rel), D32(draws), max_violation=mv, leaf=base)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1][:, 2:2 + B]), bits(want[1]))
        assert not got[1][:, :2].any() and not got[1][:, 2 + B:].any()
        wide_s = torch.zeros((B, 2 * B), device=dev())
        wide_s[:, ::2] = T(S)
        wide_s.requires_grad_(True)
        got = run_op(wide_s[:, ::2], T(rel), D32(draws), max_violation=mv, leaf=wide_s)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1][:, ::2]), bits(want[1])) and not got[1][:, 1::2].any()
        colmajor = T(S).t().contiguous().requires_grad_(True)
        got = run_op(colmajor.t(), T(rel), D32(draws), max_violation=mv, leaf=colmajor)
        assert torch.equal(bits(got[1].t()), bits(want[1]))


def test_upstream_gradient_loss_only_and_no_positives():
    from aladin_amd import ops
    B = 257
    S, rel, draws, margin, ref = restated(B, 'groups', 0, False)
    base = run_op(T(S), T(rel), D32(draws))
    scaled = run_op(T(S), T(rel), D32(draws), g=2.5)
    assert torch.equal(bits(scaled[0]), bits(base[0])) and torch.equal(bits(scaled[2]), bits(base[2]))
    assert np.array_equal(scaled[1].cpu().numpy(), 2.5 * ref[1])                           # integers times 2.5: exact
    # positives = NULL: the same loss and gradient
    x = T(S).requires_grad_(True)
    loss = ops.semantic_hinge_loss(x, T(rel), margin, draws=D32(draws))
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0
    loss.backward()
    assert torch.equal(bits(loss.detach()), bits(base[0])) and torch.equal(bits(x.grad), bits(base[1]))
    # dS = NULL: no B x B buffer is allocated, the same loss and positives
    torch.cuda.synchronize()
    rel_d, draws_d = T(rel), D32(draws)
    for want_grad in (False, True):
        x = T(S).requires_grad_(want_grad)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out, pos = ops.semantic_hinge_loss(x, rel_d, margin, draws=draws_d, return_positives=True)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - before
        assert (grew >= 4 * B * B) == want_grad, (want_grad, grew)
        assert out.requires_grad == want_grad and torch.equal(bits(out.detach()), bits(base[0])) and torch.equal(bits(pos), bits(base[2]))
    with torch.no_grad():
        quiet = ops.semantic_hinge_loss(T(S).requires_grad_(True), rel_d, margin, draws=draws_d)
    assert not quiet.requires_grad and torch.equal(bits(quiet), bits(base[0]))


@pytest.mark.parametrize('B', [5, 257])
def test_a_nan_score_gives_a_nan_loss(B):
    from aladin_amd import ops
    S, rel, draws, margin, _ = restated(B, 'dense', 0, False)
    pos = X.positives(rel, X.THRESHOLD, draws)
    r = next(i for i in range(B) if pos[i] != i)
    cells = [(1, 3), (B - 1, 0), (r, int(pos[r]))]                                         # two costs and a row's anchor
    for mv in X.MODES:
        for i, j in cells:
            bad = S.copy()
            bad[i, j] = np.nan
            assert np.isnan(X.semantic_f64(bad, rel, margin, X.THRESHOLD, draws, mv)[0])
            x = T(bad).requires_grad_(True)
            loss = ops.semantic_hinge_loss(x, T(rel), margin, max_violation=mv, draws=D32(draws))
            loss.backward()
            assert torch.isnan(loss).item(), (B, mv, i, j)
            assert torch.isfinite(x.grad).all()                                            # integer counts throughout
        assert torch.isfinite(ops.semantic_hinge_loss(T(S), T(rel), margin, max_violation=mv, draws=D32(draws))).item()
    # a NaN on the diagonal that is nobody's anchor is cleared with the diagonal, as the reference's masked_fill_ does
    rel_off = rel.copy()
    rel_off[2, 2] = 0.0
    bad = S.copy()
    bad[2, 2] = np.nan
    if X.positives(rel_off, X.THRESHOLD, draws)[2] != 2 and X.positives(rel_off, X.THRESHOLD, draws)[B + 2] != 2:
        want = X.semantic_f64(bad, rel_off, margin, X.THRESHOLD, draws, False)[0]
        assert np.isfinite(want)
        got = ops.semantic_hinge_loss(T(bad), T(rel_off), margin, draws=D32(draws))
        np.testing.assert_allclose(got.item(), want, rtol=LOSS_RTOL)


def test_two_runs_give_the_same_bits_and_a_graph_replay_follows_refreshed_draws():
    from aladin_amd import ops
    B = 257
    for mv in X.MODES:
        S, rel, draws, margin, ref = restated(B, 'dense', 0, mv)
        r1, r2 = run_op(T(S), T(rel), D32(draws), max_violation=mv), run_op(T(S), T(rel), D32(draws), max_violation=mv)
        for u, v in zip(r1, r2):
            assert torch.equal(bits(u), bits(v))
        x = T(S).requires_grad_(True)
        rel_d, draws_d = T(rel), D32(draws)
        out = {}

        def run():
            loss, pos = ops.semantic_hinge_loss(x, rel_d, margin, max_violation=mv, draws=draws_d, return_positives=True)
            out['loss'], out['pos'] = loss.detach(), pos
            (out['dS'],) = torch.autograd.grad(loss, (x,))
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            run()                                                                          # warm-up outside the capture
        cur.wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        seen = []
        other = restated(B, 'dense', 1, mv)
        # fresh contents; then the draws alone change; then the scores too
        for S2, draws2 in ((S, draws), (S, X.make_draws(B, 7)), (other[0], other[2])):
            with torch.no_grad():
                x.copy_(T(S2))
                draws_d.copy_(D32(draws2))
            graph.replay()
            torch.cuda.synchronize()
            eager = run_op(T(S2), rel_d, D32(draws2), max_violation=mv)
            for k, v in (('loss', eager[0]), ('dS', eager[1]), ('pos', eager[2])):
                assert torch.equal(bits(out[k]), bits(v)), k
            want = X.semantic_f64(S2, rel, margin, X.THRESHOLD, draws2, mv)
            assert np.array_equal(out['pos'].cpu().numpy(), want[2]) and np.array_equal(out['dS'].cpu().numpy(), want[1])
            np.testing.assert_allclose(out['loss'].item(), want[0], rtol=LOSS_RTOL)
            seen.append(out['pos'].clone())
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])     # the draws are read on the device


@pytest.mark.parametrize('B', [1, 2, 65, 257])
def test_diagonal_relevances_give_the_plain_hinge_exactly(B):
    from aladin_amd import ops
    S = X.grid_scores(B, 3)
    rel, draws = T(np.eye(B)), D32(X.make_draws(B, 3))
    for mv in X.MODES:
        x = T(S).requires_grad_(True)
        plain = ops.hinge_loss(x, X.MARGIN, mv)
        plain.backward()
        for order in ('reference', 'aligned'):
            got = run_op(T(S), rel, draws, max_violation=mv, column_positives=order)
            assert torch.equal(got[1], x.grad), (B, mv, order)                              # as values: the hinge writes an empty diagonal as -0.0
            np.testing.assert_allclose(got[0].item(), plain.item(), rtol=LOSS_RTOL)
            assert got[2].tolist() == list(range(B)) * 2


# The backward's row step, as tests/test_gpu_parity.py runs every comparison of alignment gradient VALUES: under both modes, with
# that file's per-mode absolute term (a fraction of the largest reference entry) on top of rtol 1e-3.
EXACT_BWD_GATE, FP16_BWD_GATE = 3e-5, 5e-4


@pytest.fixture(params=['exact', 'fp16'])
def bwd_mode(request):
    from aladin_amd import ops
    old = ops.set_backward_precision(request.param)
    yield request.param
    ops.set_backward_precision(old)


def test_alignment_head_semantic_loss(bwd_mode):
    """AlignmentSemanticContrastiveLoss('MrSw') on the align_b5_d64 golden's sets.  Loss: the restatement on the ORACLE's score matrix
    (rtol 1e-3 / atol 1e-3, the alignment losses' tolerance: the scores come from fp16 operands).  Set gradients: the oracle's
    alignment_scores_backward fed with the restatement's dS -- taken at the HIP scores, where the kernel's dS must equal it."""
    from aladin_amd.loss import AlignmentSemanticContrastiveLoss
    g = load_golden('align_b5_d64')
    im, s, il, sl = golden_alignment_inputs(g)
    B = len(il)
    rel, draws = X.relevances(B, 'dense', 5), X.make_draws(B, 5)
    for mv in X.MODES:
        crit = AlignmentSemanticContrastiveLoss(margin=X.MARGIN, threshold=X.THRESHOLD, max_violation=mv)
        a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
        loss, S = crit(a, b, il, sl, T(rel), return_similarity_mat=True, draws=D32(draws))
        S.retain_grad()
        loss.backward()
        S_oracle = O.alignment_scores(im, s, il, sl, 'MrSw', dtype=np.float64)
        S_hip = S.detach().cpu().numpy()
        ref_loss = X.semantic_f64(S_oracle, rel, X.MARGIN, X.THRESHOLD, draws, mv)[0]
        hip_loss, dS, pos = X.semantic_f64(S_hip, rel, X.MARGIN, X.THRESHOLD, draws, mv)
        min_x, gap, ok = X.condition_figures(S_hip, rel, X.MARGIN, X.THRESHOLD, draws, mv)
        print('alignment semantic (%s, %s): loss %.7g, restatement on the oracle\'s scores %.7g, on the HIP scores %.7g;  min |x| %.3g, '
              'min gap %.3g' % (bwd_mode, 'max' if mv else 'sum', loss.item(), ref_loss, hip_loss, min_x, gap))
        assert ok                                                                          # the decisions at the HIP scores are unambiguous
        np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(S_hip, S_oracle, rtol=1e-3, atol=3e-4)
        np.testing.assert_allclose(loss.item(), hip_loss, rtol=LOSS_RTOL)
        assert np.array_equal(S.grad.cpu().numpy(), dS)
        d_im, d_s = O.alignment_scores_backward(im, s, il, sl, dS)
        gate = EXACT_BWD_GATE if bwd_mode == 'exact' else FP16_BWD_GATE
        for got, ref, what in ((a.grad, d_im, 'd im_set'), (b.grad, d_s, 'd s_seq')):
            got = got.cpu().numpy()
            scale = float(np.abs(ref).max())
            print('   %s (%s): max |err| / max |ref| %.3g (gate %.3g)' % (what, bwd_mode, np.abs(got - ref).max() / scale, gate))
            np.testing.assert_allclose(got, ref, rtol=1e-3, atol=gate * scale)


CAPTIONS = ['a man rides a horse on the beach', 'a man riding a horse along the beach', 'two dogs play in the snow',
            'a dog plays in the snow', 'a plate of food on a table', 'a man rides a brown horse', 'a table with a plate of food on it',
            'children playing football in a park', 'a red bus on a city street']


def test_end_to_end_from_strings():
    """rouge.relevance_matrix(captions, caps_per_img=1).t() feeds the loss as the transposed view it is"""
    from aladin_amd import ops, rouge
    B = len(CAPTIONS)
    rel = rouge.relevance_matrix(CAPTIONS, caps_per_img=1).t()                             # images x captions
    assert tuple(rel.shape) == (B, B) and rel.stride() == (1, B)
    want_rel = RG.caption_relevance(CAPTIONS, 1).T
    assert np.array_equal(rel.cpu().numpy(), want_rel)
    above = want_rel > X.THRESHOLD
    assert above.sum() > B and (np.diag(want_rel) == 1).all()                              # paraphrases are positives beside the diagonal
    S, draws = X.grid_scores(B, 11), X.make_draws(B, 11)
    for mv in X.MODES:
        assert X.condition_figures(S, want_rel, X.MARGIN, X.THRESHOLD, draws, mv, exact_ties=True)[2]
        x = T(S).requires_grad_(True)
        loss, pos = ops.semantic_hinge_loss(x, rel, X.MARGIN, X.THRESHOLD, mv, draws=D32(draws), return_positives=True)
        loss.backward()
        assert_matches((loss.detach(), x.grad, pos), X.semantic_f64(S, want_rel, X.MARGIN, X.THRESHOLD, draws, mv), 'from strings')
    # device draws: a generator makes them repeatable, and every choice is a candidate
    gen = torch.Generator(device=dev())
    picks = []
    for _ in range(2):
        gen.manual_seed(1234)
        picks.append(ops.semantic_hinge_loss(T(S), rel, X.MARGIN, generator=gen, return_positives=True)[1].cpu().numpy())
    assert np.array_equal(picks[0], picks[1])
    assert all(above[i, picks[0][i]] for i in range(B)) and all(above[picks[0][B + j], j] for j in range(B))


def test_out_of_range_and_bad_input_are_refused_without_a_launch():
    import ctypes as C
    from aladin_amd import _lib, ops
    lib = _lib.load()
    assert _lib.SEM_MAX_B == MAX_B
    out = torch.full((64,), 7.0, device=dev())
    p = lambda x: C.c_void_p(x.data_ptr())                                                  # noqa: E731
    B = MAX_B + 1
    rc = lib.aladin_semantic_hinge_fwd_bwd(p(out), B, p(out), B, 1, B, 0.2, 0.4, 0, p(out), p(out), p(out), p(out), p(out), None)
    assert rc == 2 and str(MAX_B) in lib.aladin_last_error().decode()                      # ALADIN_ERR_UNSUPPORTED
    assert lib.aladin_semantic_hinge_fwd_bwd(p(out), 3, p(out), 4, 1, 4, 0.2, 0.4, 0, p(out), p(out), p(out), p(out), p(out), None) == 1
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 64                                                      # nothing ran
    big = torch.zeros(1, device=dev()).expand(B, B)
    with pytest.raises(ValueError, match=str(MAX_B)):
        ops.semantic_hinge_loss(big, big, 0.2)
    sq = torch.zeros((4, 4), device=dev())
    with pytest.raises(ValueError, match='square'):
        ops.semantic_hinge_loss(torch.zeros((4, 5), device=dev()), sq, 0.2)
    with pytest.raises(ValueError, match='aligned with the scores'):
        ops.semantic_hinge_loss(sq, torch.zeros((5, 5), device=dev()), 0.2)
    with pytest.raises(ValueError, match='draws'):
        ops.semantic_hinge_loss(sq, sq, 0.2, draws=torch.zeros(8, dtype=torch.int64, device=dev()))
    with pytest.raises(RuntimeError, match='draws must live on the device'):
        ops.semantic_hinge_loss(sq, sq, 0.2, draws=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.semantic_hinge_loss(sq, torch.zeros((4, 4)), 0.2)


@pytest.mark.parametrize('variant', ['sum-reference', 'max-aligned-masked'])
def test_outputs_and_workspace_do_not_depend_on_stale_memory_and_stay_inside_their_allocations(variant):
    """loss, dS, the positives and the workspace are torch.empty memory: a pass seeded with another problem's final bytes and a
    zero-filled pass give the same bits, the restatement's, and no guard band is touched"""
    from aladin_amd import ops
    B = 65
    mv, order, mask = (False, 'reference', False) if variant == 'sum-reference' else (True, 'aligned', True)
    donor, probe = restated(B, 'groups', 1, mv, order, mask), restated(B, 'dense', 0, mv, order, mask)

    def call(case):
        S, rel, draws, margin, _ = case
        x = T(S).requires_grad_(True)
        loss, pos = ops.semantic_hinge_loss(x, T(rel), margin, X.THRESHOLD, mv, draws=D32(draws), column_positives=order, mask_positives=mask,
                                            return_positives=True)
        loss.backward()
        return loss.detach(), x.grad, pos
    probes, stale, clean = P.run_three_passes(call, donor, probe)
    record, seeded, zeroed = probes
    print('semantic_hinge_loss[%s]: %d allocations per pass' % (variant, record.intercepted))
    assert record.intercepted == seeded.intercepted == zeroed.intercepted == 4             # loss, dS, positives, workspace
    assert seeded.seeded == 4 and all(p.passed_through_device == 0 for p in probes)
    P.assert_same_outputs(seeded, stale, zeroed, clean, names=['loss', 'dS', 'positives'])
    assert_matches(clean, probe[4], 'probed %s' % variant)
