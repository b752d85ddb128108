"""CPU tier of the score-matrix tests: the inputs of tests/test_matrix_losses_gpu.py deserve the gates that file holds the kernels
to.  Every input comes from tests/helpers/matrix_losses_numpy.py, the same functions the GPU tier calls.

  * hinge: on the quantised scores the oracle's dS is identical in float32 and float64 (so "bit for bit" is a fair demand), and
    exact ties of the hardest negative are plentiful (the tie rule is actually exercised);
  * GEMM: the integer products, forward and both backward products, are exactly representable in fp32 in any summation order;
  * ListNet: the extreme family stays finite in float32; the float32 restatement is pinned to the oracle on the reference's own
    fixtures; the absolute gate of the cancelling gradients, LISTNET_A = 4 x the float32 restatement's worst distance from float64
    over every input of a family, is measured here and asserted not to exceed its recorded value."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import alad_oracle as O                  # noqa: E402
import matrix_losses_numpy as H          # noqa: E402


@pytest.mark.parametrize('B', H.HINGE_BS)
def test_quantised_hinge_is_exact_in_both_precisions(B):
    S, margin = H.hinge_scores(B, 'quantised')
    assert S.dtype == np.float32 and np.array_equal(S * 16, np.round(S * 16)) and np.abs(S).max() <= 4
    for mv in (True, False):
        l32, d32 = O.hinge_loss(S, margin, mv, return_grad=True)
        l64, d64 = O.hinge_loss(S.astype(np.float64), margin, mv, return_grad=True)
        assert d32.dtype == np.float32 and d64.dtype == np.float64
        assert np.array_equal(d32, d64), (B, mv)
        assert abs(float(l32) - float(l64)) <= H.HINGE_LOSS_RTOL * abs(float(l64))
    # the costs themselves: margin + s - diag computed in float32 is the float64 value
    c32 = np.float32(margin) + S - np.diag(S)[:, None]
    assert np.array_equal(c32.astype(np.float64), margin + S.astype(np.float64) - np.diag(S).astype(np.float64)[:, None])


@pytest.mark.parametrize('B', [B for B in H.HINGE_BS if B >= 63])
def test_quantised_hinge_has_exact_ties(B):
    S, margin = H.hinge_scores(B, 'quantised')
    tied_rows, tied_cols = H.hinge_tied_rows(S, margin), H.hinge_tied_rows(S.T, margin)
    assert tied_rows > 0 and tied_cols > 0
    if B >= 255:
        assert 4 * tied_rows >= B and 4 * tied_cols >= B, (B, tied_rows, tied_cols)


@pytest.mark.parametrize('where', ['nan_off', 'nan_diag', 'inf_off'])
@pytest.mark.parametrize('B', H.HINGE_NAN_BS)
def test_oracle_propagates_non_finite_scores(B, where):
    S, margin, rows, cols = H.hinge_nonfinite(B, where)
    ref, _ = H.hinge_scores(B, 'quantised')
    for mv in (True, False):
        with np.errstate(invalid='ignore'):
            loss, dS = O.hinge_loss(S.astype(np.float64), margin, mv, return_grad=True)
        assert (np.isposinf(loss) if where == 'inf_off' else np.isnan(loss)), (where, mv, loss)
        # the lines the non-finite entry does not touch keep a finite gradient block
        assert np.isfinite(dS[np.ix_(rows, cols)]).all()
    assert np.array_equal(S[np.ix_(rows, cols)], ref[np.ix_(rows, cols)])


@pytest.mark.parametrize('M,N,K', H.GEMM_SHAPES)
def test_integer_gemm_products_are_exactly_representable(M, N, K):
    A, B, W = H.gemm_inputs(M, N, K, 'integer')
    assert K <= 3000 and max(np.abs(x).max() for x in (A, B, W)) <= 8
    assert H.fp32_sums_exact(A, B.T) and H.fp32_sums_exact(W, B) and H.fp32_sums_exact(W.T, A)
    (C, d_im, d_s), _ = H.gemm_refs(A, B, W)
    for ref in (C, d_im, d_s):
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    # the float32 product numpy itself computes agrees, whatever order its BLAS sums in
    assert np.array_equal(A @ B.T, C) and np.array_equal(W @ B, d_im) and np.array_equal(W.T @ A, d_s)


def test_normal_gemm_bound_holds_for_a_float32_product():
    """the derived elementwise bound k u (|X| |Y|) covers numpy's own float32 products of the standard-normal inputs"""
    for M, N, K in H.GEMM_SHAPES:
        A, B, W = H.gemm_inputs(M, N, K, 'normal')
        refs, bounds = H.gemm_refs(A, B, W)
        for got, ref, bound in zip((A @ B.T, W @ B, W.T @ A), refs, bounds):
            assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (M, N, K)


@pytest.mark.parametrize('B', H.LISTNET_BS)
def test_extreme_listnet_family_is_finite_in_float32(B):
    T, M = H.listnet_inputs(B, 'extreme')
    loss, dM = H.listnet_f32(T, M)
    ref, dref = O.listnet_loss(T.astype(np.float64), M.astype(np.float64), return_grad=True)
    assert np.isfinite(loss) and np.isfinite(dM).all() and np.isfinite(ref) and np.isfinite(dref).all()
    np.testing.assert_allclose(loss, ref, **H.LISTNET_LOSS_TOL)
    if B >= 63:
        assert float(np.abs(H.LISTNET_TAU * M).max()) > 200          # the un-shifted exponential would overflow float32 ...
        assert 40 < float(ref) < 52                                   # ... and log(Q + eps) sits near log(1e-10) = -23 per side


@pytest.mark.parametrize('name', ['distill_b16', 'distill_b5'])
def test_float32_restatement_matches_the_oracle_on_the_fixtures(name):
    g = load_golden(name)
    T, M = g['teacher'], g['student']
    loss, dM = H.listnet_f32(T, M)
    ref, dref = O.listnet_loss(T.astype(np.float64), M.astype(np.float64), return_grad=True)
    np.testing.assert_allclose(loss, ref, **H.LISTNET_LOSS_TOL)
    np.testing.assert_allclose(loss, g['loss_listnet'], **H.LISTNET_LOSS_TOL)
    H.assert_cancelling_grad_close(dM, dref, name)
    H.assert_cancelling_grad_close(dM, g['dstudent_listnet'], name + ' (recorded)')


def small_refs(B, D, mv):
    """float64 references of the small-batch heads: (M, hinge loss, dM_hinge, listnet loss, dM_listnet, d_img, d_cap)"""
    img, cap, teacher = H.small_batch_inputs(B, D)
    M = O.dot_scores(img.astype(np.float64), cap.astype(np.float64))
    lh, dMh = O.hinge_loss(M, H.HINGE_MARGIN_Q, mv, return_grad=True)
    ll, dMl = O.listnet_loss(teacher.astype(np.float64), M, return_grad=True)
    coef = H.SMALL_G_HINGE * dMh + H.SMALL_G_LISTNET * dMl
    return M, lh, dMh, ll, dMl, coef @ cap.astype(np.float64), coef.T @ img.astype(np.float64)


def test_small_batch_products_are_exact():
    for B in H.SMALL_BS:
        for D in H.SMALL_DS:
            img, cap, _ = H.small_batch_inputs(B, D)
            assert H.fp32_sums_exact(img * 16, (cap * 16).T)
            M = O.dot_scores(img.astype(np.float64), cap.astype(np.float64))
            assert np.array_equal(M.astype(np.float32).astype(np.float64), M)
            for mv in (True, False):
                _, d32 = O.hinge_loss(M.astype(np.float32), H.HINGE_MARGIN_Q, mv, return_grad=True)
                _, d64 = O.hinge_loss(M, H.HINGE_MARGIN_Q, mv, return_grad=True)
                assert np.array_equal(d32, d64)


def test_listnet_floor_is_within_its_recorded_value():
    """max|float32 restatement - float64| / max|float64| of the cancelling gradients on every input the GPU tier gates with
    LISTNET_A: dM of ListNet (both families, every B) and d_img / d_cap of the small-batch heads."""
    floors = {}
    for B in H.LISTNET_BS:
        for fam in H.LISTNET_FAMILIES:
            T, M = H.listnet_inputs(B, fam)
            _, dM = H.listnet_f32(T, M)
            _, dref = O.listnet_loss(T.astype(np.float64), M.astype(np.float64), return_grad=True)
            floors['listnet %s B=%d' % (fam, B)] = H.floor_ratio(dM, dref)
    for B in H.SMALL_BS:
        for D in H.SMALL_DS:
            img, cap, teacher = H.small_batch_inputs(B, D)
            for mv in (True, False):
                _, _, dMh, _, _, d_img, d_cap = small_refs(B, D, mv)
                g_img, g_cap = H.small_heads_f32(img, cap, teacher, dMh)
                floors['small B=%d D=%d mv=%d' % (B, D, mv)] = max(H.floor_ratio(g_img, d_img), H.floor_ratio(g_cap, d_cap))
    print('\n'.join('%-32s %.3e' % kv for kv in sorted(floors.items())))
    for fam in H.LISTNET_FAMILIES:
        mine = {k: v for k, v in floors.items() if k.startswith('listnet ' + fam) or (fam == 'mild' and k.startswith('small'))}
        worst = max(mine, key=mine.get)
        print('worst %s: %s %.3e; recorded floor %.3e, a = %.3e' % (fam, worst, mine[worst], H.LISTNET_FLOOR[fam], H.LISTNET_A[fam]))
        assert mine[worst] <= H.LISTNET_FLOOR[fam], (worst, mine[worst])
        assert H.LISTNET_A[fam] == 4 * H.LISTNET_FLOOR[fam]


def test_l2norm_backward_gate_covers_a_float32_restatement():
    """the float32 evaluation of the l2norm formulas meets test_l2norm_and_cosine_measure's tolerances at every shape (D = 3000
    included), so the GPU tier keeps them as they are"""
    f = np.float32
    for rows, D in H.L2NORM_SHAPES:
        x, g = H.l2norm_inputs(rows, D)
        out, dx = H.l2norm_ref(x, g)
        ss = (x * x).sum(1, keepdims=True, dtype=f)
        nrm = np.sqrt(ss)
        proj = (x * g).sum(1, keepdims=True, dtype=f) / ss
        np.testing.assert_allclose(x / nrm, out, **H.L2NORM_FWD_TOL)
        assert (np.abs(((g - x * proj) / nrm).astype(np.float64) - dx) <= H.l2norm_bwd_tol(dx)).all(), (rows, D)
