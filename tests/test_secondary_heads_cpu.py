"""CPU tier of the secondary heads' tests: the inputs of tests/test_secondary_heads_gpu.py deserve the gates that file holds the
kernels to.  Every input comes from tests/helpers/secondary_numpy.py, the same functions the GPU tier calls.

  * the helper's float64 restatements ARE the oracle (scan, contrastive, ordinal, mse, order) or agree with its masked-tensor form
    ('sum' / 'mean'), so a gate measured against them is a gate against the oracle;
  * preconditions, asserted: valid scan cosines stay 1e-6 away from the A > 0 gate, teacher arg-maxes are exact ties or 1e-3 apart,
    the ordinal teachers' values are distinct (or exactly equal, by construction), non-quantised hinge arguments stay 1e-4 from 0;
  * quantised students: hinge arguments are exact in float32, so dM of the contrastive mode is the same in both precisions;
  * floors: the float32 restatements' distance from float64, printed and asserted not to exceed the recorded constants from which
    the GPU gates (4 x) are derived;
  * slips, emulated in numpy: each moves the result by far more than the gate of the family it is aimed at."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import alad_oracle as O                  # noqa: E402
import secondary_numpy as H              # noqa: E402

SCAN_CASES = [('shape', sh) for sh in H.SCAN_SHAPES] + [(fam, None) for fam in H.SCAN_FAMILIES[1:]]
_SCAN = {}


def scan_both(family, shape):
    """(inputs, float64 evaluation, float32 evaluation), once per case"""
    key = (family, shape)
    if key not in _SCAN:
        inp = H.scan_inputs(family, shape)
        _SCAN[key] = (inp, H.scan_eval(*inp, dtype=np.float64), H.scan_eval(*inp, dtype=np.float32))
    return _SCAN[key]


# ------------------------------------------------------------------------------------------------
# scan-sentences
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,shape', SCAN_CASES)
def test_scan_restatement_is_the_oracle(family, shape):
    (im, s, il, sl, w), (S, d_im, d_s, min_abs), _ = scan_both(family, shape)
    So, do_im, do_s = O.scan_sentences_scores(im, s, il, sl, dS=w)                      # float32 casts of its float64 results
    np.testing.assert_allclose(S, So, rtol=2e-7, atol=1e-30)
    np.testing.assert_allclose(d_im, do_im, rtol=1e-6, atol=2e-7 * np.abs(do_im).max())
    np.testing.assert_allclose(d_s, do_s, rtol=1e-6, atol=2e-7 * np.abs(do_s).max())
    assert H.row_ratio(d_im, do_im) <= 2e-7 and H.row_ratio(d_s, do_s) <= 2e-7
    # precondition: no valid cosine of two non-zero vectors sits on the A > 0 gate (a discontinuity of the gradient)
    print('scan %s %s: smallest valid |A| %.3g' % (family, shape, min_abs))
    assert min_abs >= 1e-6, (family, shape, min_abs)


def test_scan_special_inputs_are_what_they_claim():
    im, s, il, sl, w = H.scan_inputs('zero')
    assert not im[H.SCAN_ZERO_REGION].any() and not s[H.SCAN_ZERO_WORD].any()
    assert 1 <= H.SCAN_ZERO_REGION[1] < il[1] and 1 <= H.SCAN_ZERO_WORD[1] < sl[2] - 2                    # inside the valid range
    S, d_im, d_s = O.scan_sentences_scores(im, s, il, sl, dS=w)
    assert np.isfinite(S).all() and np.isfinite(d_im).all() and np.isfinite(d_s).all()
    # the zero region's gradient is the reference's finite value, 1e8 (cosine eps) x 1e12 (normalize eps) x O(1), not 0
    assert 1e18 < np.abs(d_im[H.SCAN_ZERO_REGION]).max() < 1e22
    assert np.abs(np.delete(d_im.reshape(-1, im.shape[2]), H.SCAN_ZERO_REGION[0] * im.shape[1] + H.SCAN_ZERO_REGION[1], 0)).max() < 1e3
    im, s, il, sl, w = H.scan_inputs('opposite')
    A = O.masked_alignments(im, s, il, sl, np.float64)
    assert (A[0, 1, :, 1] < 0).all() and (A[1:, 1, :, 1] > 0).any()                                       # raw word 2 is scored word 1
    im, s, il, sl, w = H.scan_inputs('ragged')
    S = O.scan_sentences_scores(im, s, il, sl)
    assert not S[0].any() and np.isnan(S[1:, 0]).all() and np.isfinite(S[:, 1:]).all()
    # the pair kernels' LDS (3 R'T' + T'^2 + T' + 3 R' floats, forward and backward alike) fits 160 KiB at the bound
    Rq, Tq = H.SCAN_MAX_SHAPE[2] - 1, H.SCAN_MAX_SHAPE[3] - 3
    assert (Rq, Tq) == (96, 96) and (3 * Rq * Tq + Tq * Tq + Tq + 3 * Rq) * 4 <= 160 * 1024


def test_scan_floors_are_within_their_recorded_values():
    worst = {k: 0.0 for k in H.SCAN_FLOOR}
    for family, shape in SCAN_CASES:
        _, (S, d_im, d_s, _), (S32, d_im32, d_s32, _) = scan_both(family, shape)
        fs, fg = H.floor_ratio(S32, S), max(H.floor_ratio(d_im32, d_im), H.floor_ratio(d_s32, d_s))
        print('scan floor %-8s %-22s scores %.3g gradients %.3g' % (family, shape, fs, fg))
        worst['scores'], worst['grads'] = max(worst['scores'], fs), max(worst['grads'], fg)
        if family == 'zero':
            worst['zero_rows'] = max(H.row_ratio(d_im32, d_im), H.row_ratio(d_s32, d_s))
    print('scan floors', {k: '%.3g' % v for k, v in worst.items()}, 'recorded', H.SCAN_FLOOR)
    for k, v in worst.items():
        assert v <= H.SCAN_FLOOR[k] <= 1.1 * v, (k, v)                  # within, and recorded no more than a last digit above


def test_scan_slips_move_the_result_past_the_gate():
    sh = (3, 2, 9, 68, 31)
    (im, s, il, sl, w), (S, d_im, d_s, _), _ = scan_both('shape', sh)
    S2, d_im2, d_s2, _ = H.scan_eval(im, s, il, sl, w, max_words=64)                    # words >= 64 ignored
    moved = (H.floor_ratio(S2, S), H.floor_ratio(d_im2, d_im), H.floor_ratio(d_s2, d_s))
    print('slip scan words >= 64 ignored: scores %.3g d_im %.3g d_s %.3g' % moved)
    assert moved[0] > 100 * H.SCAN_GATE['scores'] and min(moved[1:]) > 100 * H.SCAN_GATE['grads']
    sh = (2, 3, 70, 21, 100)
    (im, s, il, sl, w), (S, d_im, d_s, _), _ = scan_both('shape', sh)
    for what in ('the partial slab', 'a whole slab'):
        S2, d_im2, d_s2, _ = H.scan_eval(im, s, il, sl, w, gram_features=96) if what == 'the partial slab' else \
            scan_without_second_slab(im, s, il, sl, w)
        moved = (H.floor_ratio(S2, S), H.floor_ratio(d_im2, d_im))
        print('slip scan Gram drops %s: scores %.3g d_im %.3g' % ((what,) + moved))
        assert moved[0] > 100 * H.SCAN_GATE['scores'] and moved[1] > 100 * H.SCAN_GATE['grads']


def scan_without_second_slab(im, s, il, sl, w):
    """scan_eval whose Gram matrix misses features 32 .. 63: the features reordered (which changes no product), the kept ones first"""
    keep = np.r_[0:32, 64:s.shape[2], 32:64]
    return H.scan_eval(im[:, :, keep], s[:, :, keep], il, sl, w, gram_features=s.shape[2] - 32)


# ------------------------------------------------------------------------------------------------
# sum / mean
# ------------------------------------------------------------------------------------------------
def test_sum_restatement_agrees_with_the_masked_tensor():
    for D in H.NORMSUM_DS:
        for minimal in (False, True):
            im, s, il, sl, w = H.normsum_inputs(D, minimal)
            for mean in (False, True):
                ref = O.alignment_scores(im, s, np.minimum(il, im.shape[1]), np.minimum(sl, s.shape[1]), 'mean' if mean else 'sum',
                                         dtype=np.float64)
                got = H.sum_scores(im, s, il, sl, mean=mean)
                np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-13)
    im, s, il, sl, w = H.normsum_inputs(64)
    assert not im[H.NORMSUM_ZERO].any() and not s[H.NORMSUM_ZERO].any() and il[H.NORMSUM_ZERO[0]] - 1 >= H.NORMSUM_ZERO[1]
    assert sorted(L - 1 for L in il) == sorted(H.NORMSUM_L) == sorted(L - 3 for L in sl)
    # the gradient is a directional derivative: check it against a central difference of the float64 scores
    S, d_im, d_s, _ = H.sum_scores(im, s, il, sl, w, mean=True)
    rng = np.random.default_rng(0)
    di, ds = rng.standard_normal(im.shape), rng.standard_normal(s.shape)
    di[H.NORMSUM_ZERO], ds[H.NORMSUM_ZERO] = 0, 0                                       # (the zero rows' 1e12 slope is one-sided)
    h = 1e-6
    num = ((H.sum_scores(im + h * di, s + h * ds, il, sl, mean=True) - H.sum_scores(im - h * di, s - h * ds, il, sl, mean=True)) * w).sum() / (2 * h)
    ana = (d_im * di).sum() + (d_s * ds).sum()
    assert abs(num - ana) <= 1e-6 * max(1.0, abs(ana)), (num, ana)


def test_normsum_floors_are_within_their_recorded_values():
    worst = {'out': 0.0, 'grad': 0.0, 'scores': 0.0}
    for D in H.NORMSUM_DS:
        for minimal in (False, True):
            im, s, il, sl, w = H.normsum_inputs(D, minimal)
            g = np.random.default_rng(D).standard_normal((im.shape[0], D)).astype(np.float32)
            for x, lens, tail in ((im, il, 0), (s, sl, 2)):
                o64, d64 = H.normsum(x, lens, tail, g)
                o32, d32 = H.normsum(x, lens, tail, g, np.float32)
                so, sg = H.normsum_scales(x, lens, tail, g)
                worst['out'] = max(worst['out'], H.floor_ratio(o32, o64))
                assert not o32[so == 0].any() and not o64[so == 0].any()
                worst['grad'] = max(worst['grad'], H.scaled_error(d32, d64, sg))
            S64, di64, ds64, (gi, gc) = H.sum_scores(im, s, il, sl, w)
            S32, di32, ds32, _ = H.sum_scores(im, s, il, sl, w, dtype=np.float32)
            worst['scores'] = max(worst['scores'], H.floor_ratio(S32, S64))
            worst['grad'] = max(worst['grad'], H.scaled_error(di32, di64, H.normsum_scales(im, il, 0, gi)[1]),
                                H.scaled_error(ds32, ds64, H.normsum_scales(s, sl, 2, gc)[1]))
    print('normsum floors', {k: '%.3g' % v for k, v in worst.items()}, 'recorded', H.NORMSUM_FLOOR)
    for k, v in worst.items():
        assert v <= H.NORMSUM_FLOOR[k] <= 1.1 * v, (k, v)


def test_normsum_slip_moves_the_result_past_the_gate():
    im, s, il, sl, w = H.normsum_inputs(65)
    S = H.sum_scores(im, s, il, sl)
    S2 = H.sum_scores(im, s, il, sl, count_len=True)                                    # len instead of len - 1 - tail
    moved = H.floor_ratio(S2, S)
    print('slip normsum counts len: scores %.3g' % moved)
    assert moved > 100 * H.NORMSUM_GATE['scores']


# ------------------------------------------------------------------------------------------------
# distillation modes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', H.DISTILL_BS)
def test_teachers_are_what_they_claim(B):
    for kind in H.CONTRASTIVE_TEACHERS:
        gap, ties = H.argmax_gaps(H.teacher(B, kind))
        print('teacher B=%d %-12s arg-max gap %.3g tied lines %d' % (B, kind, gap, ties))
        assert gap >= 1e-3, (B, kind, gap)                                             # every arg-max an exact tie or well separated
        if kind == 'normal':
            assert ties == 0 or B <= 2
        if kind == 'ties' and B >= 5:
            assert ties >= B // 2
    T0 = H.teacher(B, 'negative').astype(np.float64)
    np.fill_diagonal(T0, 0)
    assert (np.argmax(T0, 1) == np.arange(B)).all() and (np.argmax(T0, 0) == np.arange(B)).all()     # the zeroed diagonal wins
    T0 = H.teacher(B, 'concentrated').astype(np.float64)
    np.fill_diagonal(T0, 0)
    assert np.bincount(np.argmax(T0, 1), minlength=B)[min(2, B - 1)] == B                              # c_2 = B
    if B > 1:
        t = H.teacher(B, 'normal')
        # ordinal: a line's values are pairwise distinct or exactly equal -- float32 values order the same way in float64, and equal
        # ones keep their index order in the oracle's stable sort as in the kernel's (key, index) sort
        for m in (t, t.T):
            assert np.array_equal(np.argsort(m, 1, kind='stable'), np.argsort(m.astype(np.float64), 1, kind='stable'))
        t = H.teacher(B, 'dups')
        assert np.array_equal(t, np.round(t)) and (B < 16 or all(len(np.unique(line)) < B for line in t))
        t = H.teacher(B, 'inf')
        assert np.isposinf(t[0]).all() and np.isfinite(t).any() and not np.isnan(t).any()


@pytest.mark.parametrize('B', H.DISTILL_BS)
def test_contrastive_restatement_is_the_oracle_and_quantised_students_are_exact(B):
    M = H.quantised(B, 'student')
    assert M.dtype == np.float32 and np.array_equal(M * 16, np.round(M * 16)) and np.abs(M).max() <= 4
    for kind in H.CONTRASTIVE_TEACHERS:
        for margin in (H.MARGIN_Q, 0.0):
            T = H.teacher(B, kind)
            lo, dMo = O.distill_contrastive(T, M, margin, True)
            l64, d64, _ = H.contrastive_eval(T, M, margin)
            l32, d32, _ = H.contrastive_eval(T, M, margin, np.float32)
            assert np.array_equal(d64, dMo) and np.array_equal(d32, d64), (B, kind, margin)
            assert abs(l64 - float(lo)) <= 1e-6 * abs(l64) and l32 == l64
    # the non-quantised case: no hinge argument within 1e-4 of 0, so a float32 evaluation has the float64 activity
    T, M = H.teacher(B, 'normal'), H.student_jittered(B)
    _, d64, gap = H.contrastive_eval(T, M, H.MARGIN_N)
    print('contrastive normal B=%d: smallest |hinge argument| %.3g' % (B, gap))
    assert gap >= 1e-4 and np.array_equal(H.contrastive_eval(T, M, H.MARGIN_N, np.float32)[1], d64)
    assert np.array_equal(d64, O.distill_contrastive(T, M, H.MARGIN_N, True)[1])


@pytest.mark.parametrize('B', [5, 257])
def test_cancelling_diagonal_family_separates_the_precisions(B):
    """with margin 1e-6 and scores near 100, float32 margin + s - diag is 0 where s equals the diagonal.  The float32
    activity differs from the float64 one there, the diagonal gradient is still minus the off-diagonal activity, and a
    rule that adds c_k + r_k to the diagonal whenever margin > 0 (assuming margin + S_kk - S_kk == margin) is wrong by c_k + r_k."""
    T, M = H.teacher(B, 'normal'), H.cancelling_diagonal(B)
    assert (np.float32(H.MARGIN_TINY) + M == M).all()
    _, d32, _ = H.contrastive_eval(T, M, H.MARGIN_TINY, np.float32)
    _, d64, _ = H.contrastive_eval(T, M, H.MARGIN_TINY)
    assert not np.array_equal(d32, d64) and np.array_equal(d64, O.distill_contrastive(T, M, H.MARGIN_TINY, True)[1])
    assert np.array_equal(np.diag(d32), -diag_share(T, M))
    T0 = T.astype(np.float64)
    np.fill_diagonal(T0, 0)
    extra = np.bincount(np.argmax(T0, 1), minlength=B) + np.bincount(np.argmax(T0, 0), minlength=B)
    print('cancelling diagonal B=%d: assuming margin + S_kk - S_kk == margin adds up to %d to a diagonal gradient of size up to %d' % (B, extra.max(), np.abs(np.diag(d32)).max()))
    assert (extra > 0).sum() > B // 2


def diag_share(T, M):
    """minus the diagonal of dM from first principles, in float32 arithmetic: sum_{j != k} c_j [a_kj > 0] + sum_{i != k} r_i [b_ik > 0]"""
    B = M.shape[0]
    T0 = T.astype(np.float64)
    np.fill_diagonal(T0, 0)
    cc, rc = np.bincount(np.argmax(T0, 1), minlength=B), np.bincount(np.argmax(T0, 0), minlength=B)
    m, d = np.float32(H.MARGIN_TINY), np.diag(M)
    out = np.zeros(B)
    for k in range(B):
        for j in range(B):
            if j != k:
                out[k] += cc[j] * ((m + M[k, j]) - d[k] > 0) + rc[j] * ((m + M[j, k]) - d[k] > 0)
    return out


@pytest.mark.parametrize('B', H.ORDINAL_BS)
def test_ordinal_parts_are_the_oracle(B):
    M = H.quantised(B, 'student')
    for kind in H.ORDINAL_TEACHERS:
        T = H.teacher(B, kind)
        for stride in sorted({1, min(3, B - 1), B - 1}):
            for thr in (0.1, -np.inf, float(T[B - 1, 0])):
                lo, dMo = O.distill_ordinal(T, M, H.MARGIN_Q, thr, stride, True)
                loss, gr, gc, nr, nc, _ = H.ordinal_parts(T, M, H.MARGIN_Q, thr, stride)
                assert np.array_equal((gr + gc).astype(np.float32), dMo), (B, kind, stride, thr)
                assert (np.isnan(lo) and np.isnan(loss)) or abs(loss - float(lo)) <= 1e-6 * abs(loss)
    T, Mn = H.teacher(B, 'normal'), H.student_jittered(B)
    gap = H.ordinal_parts(T, Mn, H.MARGIN_N, 0.1, min(3, B - 1))[5]
    print('ordinal normal B=%d: smallest |hinge argument| %.3g' % (B, gap))
    assert gap >= 1e-4


def test_distillation_slips_move_the_result():
    B = 257
    M, T = H.quantised(B, 'student'), H.teacher(B, 'ties')
    # arg-max ties to the last index
    d = H.contrastive_eval(T, M, H.MARGIN_Q)[1]
    d2 = H.contrastive_eval(T, M, H.MARGIN_Q, last_index=True)[1]
    print('slip contrastive ties to the last index: %d of %d gradient entries change' % ((d != d2).sum(), d.size))
    assert (d != d2).sum() > B
    # ordinal ties ordered by the highest index
    T = H.teacher(B, 'dups')
    _, gr, gc, _, _, _ = H.ordinal_parts(T, M, H.MARGIN_Q, 0.1, 3)
    _, gr2, gc2, _, _, _ = H.ordinal_parts(T, M, H.MARGIN_Q, 0.1, 3, highest_index=True)
    print('slip ordinal ties by the highest index: %d of %d gradient entries change' % (((gr + gc) != (gr2 + gc2)).sum(), gr.size))
    assert ((gr + gc) != (gr2 + gc2)).sum() > B
    # ld taken as B: the rows of a (B, B + 5) buffer read with stride B
    for mode in ('mse', 'contrastive', 'ordinal'):
        wide_t, wide_m = np.zeros((B, B + 5), np.float32), np.zeros((B, B + 5), np.float32)
        rng = np.random.default_rng(1)
        wide_t[:], wide_m[:] = rng.standard_normal((B, B + 5)) + 3, rng.integers(-64, 65, (B, B + 5)) / 16 - 3
        wide_t[:, :B], wide_m[:, :B] = H.teacher(B, 'normal'), M
        wrong_t, wrong_m = wide_t.ravel()[:B * B].reshape(B, B), wide_m.ravel()[:B * B].reshape(B, B)
        f = {'mse': lambda t, m: O.distill_mse(t, m, H.WB, True)[:2], 'contrastive': lambda t, m: O.distill_contrastive(t, m, H.MARGIN_Q, True),
             'ordinal': lambda t, m: O.distill_ordinal(t, m, H.MARGIN_Q, 0.1, 3, True)}[mode]
        (l, g), (l2, g2) = f(wide_t[:, :B], wide_m[:, :B]), f(wrong_t, wrong_m)
        print('slip ld taken as B, %s: loss %.6g -> %.6g, %d gradient entries change' % (mode, l, l2, (g != g2).sum()))
        assert abs(l - l2) > 1e-3 * abs(l) and (g != g2).sum() > B


@pytest.mark.parametrize('B', H.DISTILL_BS)
def test_mse_bounds_cover_a_float32_evaluation(B):
    T, M = H.teacher(B, 'normal'), H.student_normal(B)
    (loss, dM, dwb), (bl, bM, bwb) = H.mse_ref(T, M, H.WB)
    lo, dMo, dwbo = O.distill_mse(T, M, np.float32(H.WB), True)
    assert abs(loss - float(lo)) <= 2 * H.U32 * loss and np.abs(dM - dMo).max() <= 2 * H.U32 * np.abs(dM).max()
    assert (np.abs(dwb - dwbo) <= 2 * H.U32 * np.abs(dwb) + 1e-12).all()
    l32, d32, w32 = H.mse_f32(T, M, H.WB)
    print('mse B=%d: loss error %.3g of bound %.3g; dM worst error / bound %.3g' % (B, abs(float(l32) - loss), bl, (np.abs(d32 - dM) / bM).max()))
    assert abs(float(l32) - loss) <= bl and (np.abs(d32 - dM) <= bM).all() and (np.abs(w32 - dwb) <= bwb).all()
    assert bl <= 1e-6 * loss and (bM <= 2e-6 * np.abs(dM).max()).all()                  # "a few float32 ulps of the result"


# ------------------------------------------------------------------------------------------------
# order_sim
# ------------------------------------------------------------------------------------------------
def test_order_restatement_is_the_oracle_and_floors_are_within_their_recorded_values():
    ws, wg = 0.0, 0.0
    for Bi, Bc, D in H.ORDER_SHAPES:
        im, s, G = H.order_inputs(Bi, Bc, D)
        sc, di, ds = H.order_eval(im, s, G)
        assert (sc < 0).all()                                                          # every pair has a violation: finite gradients
        np.testing.assert_allclose(sc, O.order_scores(im, s), rtol=2e-7)
        dio, dso = O.order_scores_backward(im, s, G)
        np.testing.assert_allclose(di, dio, rtol=1e-6, atol=2e-7 * np.abs(dio).max())
        np.testing.assert_allclose(ds, dso, rtol=1e-6, atol=2e-7 * np.abs(dso).max())
        sc32, di32, ds32 = H.order_eval(im, s, G, np.float32)
        fs, fg = H.floor_ratio(sc32, sc), max(H.floor_ratio(di32, di), H.floor_ratio(ds32, ds))
        print('order floor %s: scores %.3g gradients %.3g' % ((Bi, Bc, D), fs, fg))
        ws, wg = max(ws, fs), max(wg, fg)
    assert ws <= H.ORDER_FLOOR[0] <= 1.1 * ws and wg <= H.ORDER_FLOOR[1] <= 1.1 * wg, (ws, wg)
    im, s, G = H.order_inputs(33, 31, 32, covered_row=True)
    sc, di, ds = H.order_eval(im, s, G)
    assert not sc[0].any() and (sc[1:] < 0).all() and np.isnan(di[0]).all() and np.isfinite(di[1:]).all() and np.isnan(ds).all()
