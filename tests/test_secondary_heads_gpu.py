"""GPU tier (-m gpu) of the secondary poolings and distillation modes against the oracle and float64 numpy at every edge of their
kernels: aggregation='scan-sentences' (csrc/scan.hip), 'sum' / 'mean' (csrc/pool.hip normsum_*), DistillationLoss 'mse' / 'ordinal' /
'contrastive' and order_sim (csrc/distill.hip).

Inputs and gates come from tests/helpers/secondary_numpy.py; tests/test_secondary_heads_cpu.py proves what is relied on here:

  * scan: scores and gradients within the tolerances test_gpu_parity already holds AND within 4 x the float32 restatement's measured
    distance from float64, recorded rounded up in its last digit (scores 1.67e-7 -> 1.7e-7 -> gate 6.8e-7, gradients 3.58e-7 -> 3.6e-7
    -> 1.44e-6 of the largest entry; the zero-vector family row by row, 2.46e-7 -> 2.5e-7 -> 1.0e-6 of each row's largest entry);
  * sum / mean: 4 x the recorded floors (output 1.14e-7 -> 1.2e-7 -> 4.8e-7, gradient 2.48e-7 -> 2.5e-7 -> 1.0e-6 of each row's scale
    |g| / |x|, scores 2.31e-7 -> 2.4e-7 -> 9.6e-7);
  * contrastive: dM EQUALS the oracle's (quantised students: exact in both precisions; jittered students: no hinge argument within
    0.0085 of 0), loss rtol 1e-5;  ordinal: each of the row and column parts is +-1 / n exactly, their sum within 2 ulp;
  * mse: the bound derived in secondary_numpy.mse_ref (three float32 roundings of the residual, sums in double);
  * order_sim: test_gpu_parity's tolerances and 4 x the recorded floors (scores 1.0e-7 -> 1.1e-7 -> 4.4e-7, gradients 1.86e-7 ->
    1.9e-7 -> 7.6e-7)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import alad_oracle as O                  # noqa: E402
import secondary_numpy as H              # noqa: E402

pytestmark = pytest.mark.gpu

SCAN_CASES = [('shape', sh) for sh in H.SCAN_SHAPES] + [(fam, None) for fam in H.SCAN_FAMILIES[1:]]


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def F(t):
    return float(t.detach())


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------
# scan-sentences
# ------------------------------------------------------------------------------------------------
def scan_case(family, shape=None):
    """(inputs, the oracle's (S, d_im, d_s)), once per case"""
    def make():
        inp = H.scan_inputs(family, shape)
        return inp, O.scan_sentences_scores(*inp[:4], dS=inp[4])
    return cached(('scan', family, shape), make)


def run_scan(im, s, il, sl, w):
    from aladin_amd import ops
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    S = ops.alignment_scan_scores(a, b, il, sl)
    (S * T(w)).sum().backward()
    return N(S), N(a.grad), N(b.grad)


@pytest.mark.parametrize('family,shape', SCAN_CASES)
def test_scan_scores_and_gradients_match_the_oracle(family, shape):
    """every shape edge, the documented maximum R' = T' = 96 WITH its backward, ragged lengths, zero vectors inside the
    valid range (row by row: a zero region's gradient is 1e20 times an ordinary one) and a word opposite to every region of an image"""
    (im, s, il, sl, w), (So, do_im, do_s) = scan_case(family, shape)
    S, d_im, d_s = run_scan(im, s, il, sl, w)
    fs, fi, fc = H.floor_ratio(S, So), H.floor_ratio(d_im, do_im), H.floor_ratio(d_s, do_s)
    print('scan %s %s: scores %.3g d_im %.3g d_s %.3g of the largest entry (gates %.3g / %.3g)'
          % (family, shape, fs, fi, fc, H.SCAN_GATE['scores'], H.SCAN_GATE['grads']))
    np.testing.assert_allclose(S, So, equal_nan=True, **H.SCAN_SCORE_TOL)
    scale = max(1e-3, float(np.abs(do_im).max()), float(np.abs(do_s).max()))
    np.testing.assert_allclose(d_im, do_im, rtol=H.SCAN_GRAD_RTOL, atol=H.SCAN_GRAD_ATOL * scale)
    np.testing.assert_allclose(d_s, do_s, rtol=H.SCAN_GRAD_RTOL, atol=H.SCAN_GRAD_ATOL * scale)
    assert fs <= H.SCAN_GATE['scores'] and fi <= H.SCAN_GATE['grads'] and fc <= H.SCAN_GATE['grads']
    assert not d_im[:, 0].any() and not d_s[:, 0].any() and not d_s[:, -2:].any()
    if family == 'zero':
        ri, rc = H.row_ratio(d_im, do_im), H.row_ratio(d_s, do_s)
        print('scan zero: worst row d_im %.3g d_s %.3g (gate %.3g)' % (ri, rc, H.SCAN_GATE['zero_rows']))
        assert ri <= H.SCAN_GATE['zero_rows'] and rc <= H.SCAN_GATE['zero_rows']
        assert np.isfinite(d_im).all() and np.isfinite(d_s).all()
    if family == 'opposite':
        assert np.isfinite(S).all() and np.isfinite(d_im).all() and np.isfinite(d_s).all()
    if family == 'ragged':
        R, Tn = im.shape[1], s.shape[1]
        assert il[0] == 1 and not S[0].any() and not d_im[0].any()                   # nothing scored: exactly 0
        assert sl[0] == 3 and np.isnan(S[1:, 0]).all() and not d_s[0].any()          # no word: NaN where Li > 0, 0 where Li = 0
        assert np.isfinite(S[:, 1:]).all() and np.isfinite(d_im).all() and np.isfinite(d_s).all()
        for i, L in enumerate(il):
            assert not d_im[i, min(L, R):].any()
            assert L < 2 or d_im[i, 1:min(L, R)].any()
        for j, L in enumerate(sl):
            assert not d_s[j, max(min(L, Tn) - 2, 1):].any()
    if family == 'max':
        from aladin_amd import ops
        with torch.no_grad():
            assert same(N(ops.alignment_scan_scores(T(im), T(s), il, sl)), S)


def test_scan_views_and_determinism():
    """a permuted (S, B, D) -> (B, S, D) view is consumed in place, a feature slice is copied, a transposed upstream gradient is made
    contiguous: all bit-equal to the contiguous run, and the run to itself"""
    from aladin_amd import ops
    from aladin_amd._ops_common import _rows_inner_contig
    (im, s, il, sl, w), _ = scan_case('ragged')
    S0, gi0, gs0 = run_scan(im, s, il, sl, w)
    S1, gi1, gs1 = run_scan(im, s, il, sl, w)
    assert same(S0, S1) and same(gi0, gi1) and same(gs0, gs1)
    # permuted bases
    a, b = T(im.transpose(1, 0, 2)).requires_grad_(True), T(s.transpose(1, 0, 2)).requires_grad_(True)
    va, vb = a.permute(1, 0, 2), b.permute(1, 0, 2)
    assert not va.is_contiguous() and _rows_inner_contig(va) is va and _rows_inner_contig(vb) is vb
    S = ops.alignment_scan_scores(va, vb, il, sl)
    (S * T(w)).sum().backward()
    assert same(N(S), S0) and same(N(a.grad).transpose(1, 0, 2), gi0) and same(N(b.grad).transpose(1, 0, 2), gs0)
    # feature slices of wider buffers
    D = im.shape[2]
    wa, wb = np.full(im.shape[:2] + (D + 2,), 7, np.float32), np.full(s.shape[:2] + (D + 2,), -7, np.float32)
    wa[:, :, 1:D + 1], wb[:, :, 1:D + 1] = im, s
    a, b = T(wa).requires_grad_(True), T(wb).requires_grad_(True)
    va, vb = a[:, :, 1:D + 1], b[:, :, 1:D + 1]
    assert _rows_inner_contig(va) is not va
    S = ops.alignment_scan_scores(va, vb, il, sl)
    (S.t() * T(w).t()).sum().backward()                                               # and a transposed upstream gradient
    ga, gb = N(a.grad), N(b.grad)
    assert same(N(S), S0) and same(ga[:, :, 1:D + 1], gi0) and same(gb[:, :, 1:D + 1], gs0)
    assert not ga[:, :, 0].any() and not ga[:, :, -1].any() and not gb[:, :, 0].any() and not gb[:, :, -1].any()


@pytest.mark.parametrize('pooling', ['scan', 'sum', 'mean'])
def test_feature_size_mismatch_is_rejected(pooling):
    """captions WIDER than images (the orientation in which a missing check still reads in bounds) raise in every pooling"""
    from aladin_amd import ops
    im, s = T(np.ones((2, 5, 8))), T(np.ones((2, 7, 12)))
    with pytest.raises(ValueError, match='feature sizes differ'):
        if pooling == 'scan':
            ops.alignment_scan_scores(im, s, [5, 5], [7, 7])
        else:
            ops.alignment_sum_scores(im, s, [5, 5], [7, 7], mean=(pooling == 'mean'))


# ------------------------------------------------------------------------------------------------
# sum / mean
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('minimal', [False, True])
@pytest.mark.parametrize('D', H.NORMSUM_DS)
def test_normsum_and_sum_mean_scores_match_float64(D, minimal):
    """every scored length 0, 1, 3, 4, 5, N - 1 - tail and one above N over the 4-wave split, a zero row inside the range, both tails;
    gradient exactly 0 at position 0, on the dropped tail and beyond the length (scaled_error demands it)"""
    from aladin_amd import ops
    im, s, il, sl, w = H.normsum_inputs(D, minimal)
    g = np.random.default_rng(D).standard_normal((im.shape[0], D)).astype(np.float32)
    for x, lens, tail in ((im, il, 0), (s, sl, 2)):
        o64, d64 = H.normsum(x, lens, tail, g)
        xt = T(x).requires_grad_(True)
        out = ops._NormSum.apply(xt, ops.lengths_tensor(lens, dev()), tail)
        out.backward(T(g))
        so, sg = H.normsum_scales(x, lens, tail, g)
        fo, fg = H.floor_ratio(N(out), o64), H.scaled_error(N(xt.grad), d64, sg)
        assert not N(out)[so == 0].any()                                              # nothing scored: exactly 0
        print('normsum D=%d tail=%d minimal=%d: out %.3g of the largest entry, grad %.3g of the scale of each row' % (D, tail, minimal, fo, fg))
        assert fo <= H.NORMSUM_GATE['out'] and fg <= H.NORMSUM_GATE['grad']
    for mean in (False, True):
        S64, di64, ds64, (ui, uc) = H.sum_scores(im, s, il, sl, w, mean=mean)
        a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
        S = ops.alignment_sum_scores(a, b, il, sl, mean=mean)
        (S * T(w)).sum().backward()
        fs = H.floor_ratio(N(S), S64)
        fi = H.scaled_error(N(a.grad), di64, H.normsum_scales(im, il, 0, ui)[1])
        fc = H.scaled_error(N(b.grad), ds64, H.normsum_scales(s, sl, 2, uc)[1])
        print('sum scores D=%d mean=%d minimal=%d: scores %.3g d_im %.3g d_s %.3g' % (D, mean, minimal, fs, fi, fc))
        assert fs <= H.NORMSUM_GATE['scores'] and fi <= H.NORMSUM_GATE['grad'] and fc <= H.NORMSUM_GATE['grad']


def test_sum_scores_take_a_permuted_view_in_place():
    from aladin_amd import ops
    from aladin_amd._ops_common import _rows_inner_contig
    im, s, il, sl, w = H.normsum_inputs(64)
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    S0 = ops.alignment_sum_scores(a, b, il, sl)
    (S0 * T(w)).sum().backward()
    pa, pb = T(im.transpose(1, 0, 2)).requires_grad_(True), T(s.transpose(1, 0, 2)).requires_grad_(True)
    va, vb = pa.permute(1, 0, 2), pb.permute(1, 0, 2)
    assert _rows_inner_contig(va) is va and _rows_inner_contig(vb) is vb
    S = ops.alignment_sum_scores(va, vb, il, sl)
    (S * T(w)).sum().backward()
    assert same(N(S), N(S0)) and same(N(pa.grad).transpose(1, 0, 2), N(a.grad)) and same(N(pb.grad).transpose(1, 0, 2), N(b.grad))


# ------------------------------------------------------------------------------------------------
# distillation modes
# ------------------------------------------------------------------------------------------------
def run_distill(teacher, student, mode, margin=H.MARGIN_Q, threshold=0.1, stride=3, wb=None, scale=None):
    """(loss, dM, dwb) through ops.distillation_loss on contiguous copies"""
    from aladin_amd import ops
    st = T(student).requires_grad_(True)
    wbt = T(np.asarray(wb, np.float32)).requires_grad_(True) if wb is not None else None
    loss = ops.distillation_loss(T(teacher), st, mode, margin, threshold, stride, wb=wbt)
    (loss if scale is None else scale * loss).backward()
    return F(loss), N(st.grad), (N(wbt.grad) if wbt is not None else None)


@pytest.mark.parametrize('B', H.DISTILL_BS)
def test_mse_within_the_derived_bound(B):
    teacher, student = H.teacher(B, 'normal'), H.student_normal(B)
    (loss64, dM64, dwb64), (bl, bM, bwb) = H.mse_ref(teacher, student, H.WB)
    loss, dM, dwb = run_distill(teacher, student, 'mse', wb=H.WB)
    print('mse B=%d: loss error %.3g (bound %.3g), dM worst error / bound %.3g, dwb error / bound %s'
          % (B, abs(loss - loss64), bl, (np.abs(dM - dM64) / bM).max(), np.abs(dwb - dwb64) / bwb))
    assert abs(loss - loss64) <= bl and (np.abs(dM - dM64) <= bM).all() and (np.abs(dwb - dwb64) <= bwb).all()
    (ref0, _, _), (bl0, _, _) = H.mse_ref(teacher, student, (0.0, 0.3))               # wb0 = 0: the student drops out
    loss0, dM0, _ = run_distill(teacher, student, 'mse', wb=(0.0, 0.3))
    assert not dM0.any() and abs(loss0 - ref0) <= bl0


@pytest.mark.parametrize('kind', H.CONTRASTIVE_TEACHERS)
@pytest.mark.parametrize('B', H.DISTILL_BS)
def test_contrastive_gradient_equals_the_oracle(B, kind):
    """quantised students: dM equal, ties of the teacher's arg-max to the lowest index, the zeroed diagonal winning, one column picked
    by every row, margin 0; and the jittered (inexact) student"""
    teacher = H.teacher(B, kind)
    for student, margin in ((H.quantised(B, 'student'), H.MARGIN_Q), (H.quantised(B, 'student'), 0.0), (H.student_jittered(B), H.MARGIN_N)):
        ref_loss, ref_dM, _ = H.contrastive_eval(teacher, student, margin)
        loss, dM, _ = run_distill(teacher, student, 'contrastive', margin, scale=2.5)
        print('contrastive B=%d %s margin %g: loss %.9g oracle %.9g' % (B, kind, margin, loss, ref_loss))
        assert abs(loss - ref_loss) <= H.HINGE_LOSS_RTOL * abs(ref_loss)
        assert np.array_equal(dM, 2.5 * ref_dM), (B, kind, margin, int((dM != 2.5 * ref_dM).sum()))      # small integers x 2.5: exact


@pytest.mark.parametrize('B', [5, 257])
def test_contrastive_diagonal_gradient_cancels_in_float32(B):
    """margin 1e-6 under scores near 100 -- float32 margin + S_kk - S_kk is 0, and the diagonal's own +c_k + r_k must not
    be added on the assumption that it is `margin`.  The activity is the float32 one (secondary_numpy.contrastive_eval in float32)."""
    teacher, student = H.teacher(B, 'normal'), H.cancelling_diagonal(B)
    ref_loss, ref_dM, _ = H.contrastive_eval(teacher, student, H.MARGIN_TINY, np.float32)
    loss, dM, _ = run_distill(teacher, student, 'contrastive', H.MARGIN_TINY)
    bad = dM != ref_dM
    print('contrastive cancelling diagonal B=%d: %d entries differ (%d on the diagonal)' % (B, bad.sum(), np.diag(bad).sum()))
    assert abs(loss - ref_loss) <= H.HINGE_LOSS_RTOL * abs(ref_loss)
    assert not bad.any()


def assert_ordinal(loss, dM, teacher, student, margin, thr, stride, what):
    ref_loss, gr, gc, nr, nc, _ = H.ordinal_parts(teacher, student, margin, thr, stride)
    np.testing.assert_allclose(loss, ref_loss, equal_nan=True, err_msg=what, **H.ORDINAL_LOSS_TOL)
    one = (gr == 0) | (gc == 0)
    assert np.array_equal(dM[one], (gr + gc)[one].astype(np.float32)), what          # a single part: +-1 / n, rounded once
    ulp = np.spacing(np.maximum(np.abs(gr), np.abs(gc)).astype(np.float32)).astype(np.float64)
    assert (np.abs(dM - (gr + gc)) <= 2 * ulp)[~one].all(), what


@pytest.mark.parametrize('kind', H.ORDINAL_TEACHERS)
@pytest.mark.parametrize('B', H.ORDINAL_BS)
def test_ordinal_activity_and_gradient(B, kind):
    """stride 1, 3 and B - 1; threshold 0.1, -inf and exactly a teacher value (>=); duplicated teacher values (stable by index); +inf
    teacher entries beside the sort's +inf padding; the jittered student.  (A selection that is empty for the rows alone cannot
    exist: it needs every teacher entry below the threshold, which empties the columns' too -- test_gpu_parity covers that case.)"""
    teacher = H.teacher(B, kind)
    for student, margin in ((H.quantised(B, 'student'), H.MARGIN_Q), (H.student_jittered(B), H.MARGIN_N)):
        for stride in sorted({1, min(3, B - 1), B - 1}):
            for thr in (0.1, -np.inf, float(teacher[B - 1, 0])):
                loss, dM, _ = run_distill(teacher, student, 'ordinal', margin, thr, stride)
                assert_ordinal(loss, dM, teacher, student, margin, thr, stride, 'ordinal B=%d %s stride %d thr %r' % (B, kind, stride, thr))


def test_ordinal_needs_two_lines():
    from aladin_amd import ops
    with pytest.raises(ValueError):
        ops.distillation_loss(T(np.ones((1, 1))), T(np.ones((1, 1))), 'ordinal', 0.2, 0.1, 1)


@pytest.mark.parametrize('mode', ['mse', 'contrastive', 'ordinal'])
def test_distillation_views(mode, monkeypatch):
    """teacher and student views with ld = B + 5 are consumed in place (the leading dimension handed to the kernel is B + 5, and no
    other is computed); a ::2 view and a transposed view are copied (the kernel sees ld = B); all
    give the contiguous run's bits, the gradient lands in the view's elements of the base tensor (zero elsewhere), a student without
    requires_grad gives the same loss, and an upstream factor multiplies the gradient"""
    from aladin_amd import ops, ops_losses
    from aladin_amd.loss import DistillationLoss
    B = H.DISTILL_VIEW_B
    lds, real_ld = [], ops_losses._ld
    monkeypatch.setattr(ops_losses, '_ld', lambda t: lds.append(real_ld(t)) or lds[-1])      # every ld the wrapper hands to a kernel
    teacher, student = H.teacher(B, 'normal'), H.quantised(B, 'student')
    wb = H.WB if mode == 'mse' else None
    loss0, dM0, dwb0 = run_distill(teacher, student, mode, wb=wb)

    def call(t, m, scale=None):
        wbt = T(np.asarray(wb, np.float32)).requires_grad_(True) if wb is not None else None
        loss = ops.distillation_loss(t, m, mode, H.MARGIN_Q, 0.1, 3, wb=wbt)
        if m.requires_grad:
            (loss if scale is None else scale * loss).backward()
        return F(loss), (N(wbt.grad) if wbt is not None and m.requires_grad else None)

    rng = np.random.default_rng(3)
    wide_t = (rng.standard_normal((B + 3, B + 5)) + 3).astype(np.float32)
    wide_m = (rng.integers(-64, 65, (B + 3, B + 5)) / 16 - 3).astype(np.float32)
    wide_t[:B, :B], wide_m[:B, :B] = teacher, student
    base_t, base_m = T(wide_t), T(wide_m).requires_grad_(True)
    vt, vm = base_t[:B, :B], base_m[:B, :B]
    assert vt.stride() == (B + 5, 1) and vm.stride() == (B + 5, 1)
    del lds[:]
    loss, dwb = call(vt, vm, scale=2.5)
    assert vt.stride(1) == 1 and vm.stride(1) == 1 and lds == [B + 5, B + 5], lds     # the no-copy branch: teacher and student in place
    want = np.zeros_like(wide_m)
    want[:B, :B] = dM0 * np.float32(2.5)
    assert loss == loss0 and np.array_equal(N(base_m.grad), want), mode
    assert dwb is None or np.array_equal(dwb, dwb0 * np.float32(2.5))
    # copied views
    two_t, two_m = np.zeros((B, 2 * B), np.float32), np.zeros((B, 2 * B), np.float32)
    two_t[:, ::2], two_m[:, ::2] = teacher, student
    base_m = T(two_m).requires_grad_(True)
    del lds[:]
    loss, _ = call(T(two_t)[:, ::2], base_m[:, ::2])
    assert lds == [B, B], lds
    assert loss == loss0 and np.array_equal(N(base_m.grad)[:, ::2], dM0) and not N(base_m.grad)[:, 1::2].any(), mode
    base_m = T(student.T).requires_grad_(True)
    del lds[:]
    loss, _ = call(T(teacher.T).t(), base_m.t())
    assert lds == [B, B], lds
    assert loss == loss0 and np.array_equal(N(base_m.grad).T, dM0), mode
    # no gradient requested, and the module
    assert call(T(teacher), T(student))[0] == loss0
    crit = DistillationLoss(mode=mode, margin=H.MARGIN_Q, threshold=0.1, stride=3).to(dev())
    if mode == 'mse':
        with torch.no_grad():
            crit.wb.copy_(T(np.asarray(H.WB, np.float32)))
    assert F(crit(T(teacher), T(student))) == loss0


@pytest.mark.parametrize('B', [5, 257])
def test_a_nan_student_score_reaches_the_loss(B):
    """relu / clamp(min=0) keep a NaN, so one NaN student score that a hinge compares makes the loss NaN: on the diagonal, in the
    column every row picks (c_j = B), in a row a column picks (r_i > 0) -- and ONLY then: at (2, 3), a column no row picks in a row no
    column picks, the reference never selects the element and the loss stays finite.  For ordinal: wherever the oracle compares it
    (everywhere at stride 1 and threshold -inf)."""
    teacher = H.teacher(B, 'concentrated')
    T0 = teacher.astype(np.float64)
    np.fill_diagonal(T0, 0)
    cc, rc = np.bincount(np.argmax(T0, 1), minlength=B), np.bincount(np.argmax(T0, 0), minlength=B)
    picked_row = int(np.argmax(T0, 0)[2])
    assert cc[2] == B and cc[3] == 0 and rc[2] == 0 and rc[picked_row] > 0 and rc[B - 1] == 1
    for i, j in ((2, 2), (1, 2), (picked_row, 3), (B - 1, B - 2), (2, 3)):
        student = H.quantised(B, 'student').copy()
        student[i, j] = np.nan
        loss = run_distill(teacher, student, 'contrastive')[0]
        ref = H.contrastive_eval(teacher, student, H.MARGIN_Q)[0]
        assert np.isnan(ref) == ((i, j) != (2, 3))
        if (i, j) == (2, 3):
            assert abs(loss - ref) <= H.HINGE_LOSS_RTOL * abs(ref), ('contrastive', B, i, j, loss, ref)
        else:
            assert np.isnan(loss), ('contrastive', B, i, j)
        for stride in (1, min(3, B - 1)):
            tn = H.teacher(B, 'normal')
            want = np.isnan(H.ordinal_parts(tn, student, H.MARGIN_Q, -np.inf, stride)[0])
            assert want or stride > 1                                                 # stride 1 compares every position of a line
            assert np.isnan(run_distill(tn, student, 'ordinal', threshold=-np.inf, stride=stride)[0]) == want, ('ordinal', B, i, j)
    assert np.isfinite(run_distill(teacher, H.quantised(B, 'student'), 'contrastive')[0])


# ------------------------------------------------------------------------------------------------
# order_sim
# ------------------------------------------------------------------------------------------------
def run_order(im, s, G, grad_im=True, grad_s=True):
    from aladin_amd import ops
    a, b = T(im).requires_grad_(grad_im), T(s).requires_grad_(grad_s)
    sc = ops.order_scores(a, b)
    (sc * T(G)).sum().backward()
    return N(sc), (N(a.grad) if grad_im else None), (N(b.grad) if grad_s else None)


@pytest.mark.parametrize('Bi,Bc,D', H.ORDER_SHAPES)
def test_order_scores_and_gradients_match_the_oracle(Bi, Bc, D):
    """31 / 32 / 33 rows on either side of the 32 x 32 tile, D around the 32-wide slab; ld > D views in place; one side's gradient only"""
    from aladin_amd import ops
    im, s, G = H.order_inputs(Bi, Bc, D)
    ref, di, ds = cached(('order', Bi, Bc, D), lambda: (O.order_scores(im, s),) + O.order_scores_backward(im, s, G))
    sc, gi, gs = run_order(im, s, G)
    fs, fi, fc = H.floor_ratio(sc, ref), H.floor_ratio(gi, di), H.floor_ratio(gs, ds)
    print('order (%d, %d, %d): scores %.3g d_im %.3g d_s %.3g (gates %.3g / %.3g)' % ((Bi, Bc, D, fs, fi, fc) + H.ORDER_GATE))
    np.testing.assert_allclose(sc, ref, **H.ORDER_SCORE_TOL)
    scale = max(1.0, float(np.abs(di).max()))
    np.testing.assert_allclose(gi, di, rtol=H.ORDER_GRAD_RTOL, atol=H.ORDER_GRAD_ATOL * scale)
    np.testing.assert_allclose(gs, ds, rtol=H.ORDER_GRAD_RTOL, atol=H.ORDER_GRAD_ATOL * scale)
    assert fs <= H.ORDER_GATE[0] and fi <= H.ORDER_GATE[1] and fc <= H.ORDER_GATE[1]
    # one side only
    sc1, gi1, gs1 = run_order(im, s, G, grad_s=False)
    sc2, gi2, gs2 = run_order(im, s, G, grad_im=False)
    assert gs1 is None and gi2 is None and same(sc1, sc) and same(sc2, sc) and same(gi1, gi) and same(gs2, gs)
    # ld > D
    wi, wc = np.full((Bi, D + 3), 9, np.float32), np.full((Bc, D + 3), -9, np.float32)
    wi[:, :D], wc[:, :D] = im, s
    a, b = T(wi).requires_grad_(True), T(wc).requires_grad_(True)
    va, vb = a[:, :D], b[:, :D]
    assert va.stride() == (D + 3, 1)
    scv = ops.order_scores(va, vb)
    (scv * T(G)).sum().backward()
    assert same(N(scv), sc) and same(N(a.grad)[:, :D], gi) and same(N(b.grad)[:, :D], gs)
    assert not N(a.grad)[:, D:].any() and not N(b.grad)[:, D:].any()


def test_order_pair_without_violation_and_nan_embeddings():
    """an image that dominates every caption: score -0 / 0 and NaN gradients wherever the oracle has them; a NaN in an
    embedding makes its row / column of scores NaN and leaves the others alone"""
    Bi, Bc, D = 33, 31, 32
    im, s, G = H.order_inputs(Bi, Bc, D, covered_row=True)
    ref, (di, ds) = O.order_scores(im, s), O.order_scores_backward(im, s, G)
    sc, gi, gs = run_order(im, s, G)
    assert not sc[0].any() and np.isnan(di[0]).all() and np.isnan(ds).all()
    np.testing.assert_allclose(sc, ref, **H.ORDER_SCORE_TOL)
    assert np.array_equal(np.isnan(gi), np.isnan(di)) and np.array_equal(np.isnan(gs), np.isnan(ds))
    np.testing.assert_allclose(gi[1:], di[1:], rtol=H.ORDER_GRAD_RTOL, atol=H.ORDER_GRAD_ATOL * max(1.0, float(np.abs(di[1:]).max())))
    for Bi, Bc, D in ((33, 31, 32), (31, 33, 1)):
        im, s, G = H.order_inputs(Bi, Bc, D)
        im, s = im.copy(), s.copy()
        im[1, 0], s[2, D - 1] = np.nan, np.nan
        with np.errstate(invalid='ignore'):
            ref = O.order_scores(im, s)
        sc = run_order(im, s, G)[0]
        bad = np.zeros((Bi, Bc), bool)
        bad[1, :], bad[:, 2] = True, True
        assert np.array_equal(np.isnan(ref), bad) and np.array_equal(np.isnan(sc), bad), (Bi, Bc, D)
        np.testing.assert_allclose(sc[~bad], ref[~bad], **H.ORDER_SCORE_TOL)


def test_order_backward_limit_is_reported_at_forward_time():
    """more than 16384 partner rows cannot be back-propagated; say so when the differentiable forward is requested"""
    from aladin_amd import ops
    from aladin_amd.ops_losses import ORDER_BWD_PARTNERS
    rng = np.random.default_rng(7)
    im, s = rng.standard_normal((ORDER_BWD_PARTNERS + 1, 1)).astype(np.float32), rng.standard_normal((2, 1)).astype(np.float32)
    with pytest.raises(ValueError, match='at most 16384'):
        ops.order_scores(T(im).requires_grad_(True), T(s))
    with pytest.raises(ValueError, match='at most 16384'):
        ops.order_scores(T(s), T(im).requires_grad_(True))
    with torch.no_grad():
        sc = ops.order_scores(T(im).requires_grad_(True), T(s))
    np.testing.assert_allclose(N(sc), O.order_scores(im, s), **H.ORDER_SCORE_TOL)
    assert not ops.order_scores(T(im), T(s)).requires_grad
