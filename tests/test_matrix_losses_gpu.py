"""GPU tier (-m gpu) of the exact-fp32 score-matrix ops against the oracle and float64 numpy at every edge of their kernels: the
VSE++ hinge and ListNet (csrc/losses.hip, matrix_losses.hpp), aladin_sgemm_strided behind ops.dot_scores (sgemm_tile.hpp), l2norm
(csrc/pool.hip), order_scores' single-row strides and the B <= 64 fused heads (csrc/small_batch.hip).

Inputs come from tests/helpers/matrix_losses_numpy.py; tests/test_matrix_losses_cpu.py proves what is relied on here:

  * hinge, quantised scores (multiples of 1/16, margin 0.25): every cost is exact, so dS must EQUAL the oracle's in both modes --
    which pins the tie rule (lowest index, rows and columns) across lanes, waves and the 256-stride loop; loss rtol 1e-5;
  * GEMM, integer operands: C, d_im and d_s must EQUAL the float64 products whatever the summation order; standard-normal
    operands are held to the derived bound |C - ref| <= k 2^-24 (|A| |B|^T), k the contraction length of each product;
  * ListNet: loss rtol 1e-5 / atol 1e-6; gradients |got - ref64| <= 1e-4 |ref64| + a max|ref64| with a = 4 x the distance of a plain
    float32 numpy restatement from float64, measured per input family by the CPU tier: worst 5.05e-7 on the mild family (recorded
    floor 5.5e-7, a = 2.2e-6) and 2.98e-6 on the extreme one (recorded 3.2e-6, a = 1.28e-5);
  * l2norm: the tolerances of test_gpu_parity.test_l2norm_and_cosine_measure, unchanged (the CPU tier shows a float32 evaluation
    meets them at D = 3000 too)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import alad_oracle as O                  # noqa: E402
import matrix_losses_numpy as H          # noqa: E402

pytestmark = pytest.mark.gpu

MODES = (True, False)                    # max_violation


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def F(t):
    return float(t.detach())


_ORACLE = {}


def hinge_oracle(B, kind, mv):
    """(loss float64, dS) of the oracle: float64 on the quantised scores (identical to its float32 run, CPU tier), on the float32
    scores themselves for dS of the standard-normal case.  Computed once per case."""
    key = (B, kind, mv)
    if key not in _ORACLE:
        S, margin = H.hinge_scores(B, kind)
        loss, dS = O.hinge_loss(S.astype(np.float64), margin, mv, return_grad=True)
        if kind == 'normal':
            dS = O.hinge_loss(S, margin, mv, return_grad=True)[1]
        _ORACLE[key] = (float(np.float64(loss)), dS.astype(np.float32))
    return _ORACLE[key]


def assert_hinge_loss(got, ref, what):
    print('%s: loss %.9g oracle %.9g' % (what, got, ref))
    assert abs(got - ref) <= H.HINGE_LOSS_RTOL * abs(ref), (what, got, ref)


# ------------------------------------------------------------------------------------------------
# hinge
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['quantised', 'normal'])
@pytest.mark.parametrize('B', H.HINGE_BS)
def test_hinge_equals_the_oracle(B, kind):
    from aladin_amd import ops
    S, margin = H.hinge_scores(B, kind)
    for mv in MODES:
        ref_loss, ref_dS = hinge_oracle(B, kind, mv)
        what = 'hinge B=%d %s mv=%d' % (B, kind, mv)
        # the raw call
        loss, dS, pairs = ops._hinge_raw(T(S), margin, mv, True)
        assert pairs is None
        assert_hinge_loss(F(loss), ref_loss, what + ' raw')
        assert np.array_equal(N(dS), ref_dS), (what, int((N(dS) != ref_dS).sum()))
        # autograd, a scaled upstream gradient
        st = T(S).requires_grad_(True)
        out = ops.hinge_loss(st, margin, mv)
        assert F(out) == F(loss)
        (2.5 * out).backward()
        assert np.array_equal(N(st.grad), 2.5 * ref_dS), what                        # small integers x 2.5: exact
        # loss only
        only = ops.hinge_loss(T(S), margin, mv)
        assert not only.requires_grad and F(only) == F(loss)
        raw_only = ops._hinge_raw(T(S), margin, mv, False)
        assert raw_only[1] is None and raw_only[2] is None and float(raw_only[0]) == F(loss)


@pytest.mark.parametrize('B', H.HINGE_VIEW_BS)
def test_hinge_views(B):
    """a view used in place with ld = B + 5 (rows not 16-byte aligned), a ::2 view (copied) and a transposed view: the contiguous
    run's results exactly, and the gradient in the right elements of the base tensor, zero elsewhere"""
    from aladin_amd import ops
    S, margin = H.hinge_scores(B, 'quantised')
    rng = np.random.default_rng(B)
    for mv in MODES:
        ref_loss, ref_dS = hinge_oracle(B, 'quantised', mv)
        contig = float(ops._hinge_raw(T(S), margin, mv, True)[0])

        big = (rng.integers(-64, 65, (B + 3, B + 5)) / 16).astype(np.float32)        # the surroundings: other quantised scores
        big[:B, :B] = S
        base = T(big).requires_grad_(True)
        view = base[:B, :B]
        assert view.stride() == (B + 5, 1)
        loss, dS, _ = ops._hinge_raw(view.detach(), margin, mv, True)
        assert F(loss) == contig and np.array_equal(N(dS), ref_dS), ('ld > B', B, mv)
        (2.5 * ops.hinge_loss(view, margin, mv)).backward()
        want = np.zeros_like(big)
        want[:B, :B] = 2.5 * ref_dS
        assert np.array_equal(N(base.grad), want), ('ld > B grad', B, mv)

        wide = (rng.integers(-64, 65, (B, 2 * B)) / 16).astype(np.float32)
        wide[:, ::2] = S
        base = T(wide).requires_grad_(True)
        out = ops.hinge_loss(base[:, ::2], margin, mv)
        assert F(out) == contig
        out.backward()
        want = np.zeros_like(wide)
        want[:, ::2] = ref_dS
        assert np.array_equal(N(base.grad), want), ('::2', B, mv)

        base = T(S.T).requires_grad_(True)                                           # base.t() is S
        out = ops.hinge_loss(base.t(), margin, mv)
        assert F(out) == contig
        out.backward()
        assert np.array_equal(N(base.grad), ref_dS.T), ('.t()', B, mv)


@pytest.mark.parametrize('B', H.HINGE_PAIR_BS)
def test_hinge_pair_list(B):
    from aladin_amd import ops
    S, margin = H.hinge_scores(B, 'quantised')
    for mv in MODES:
        _, ref_dS = hinge_oracle(B, 'quantised', mv)
        loss, dS, (pairs, count) = ops._hinge_raw(T(S), margin, mv, True, want_pairs=True)
        n = int(count.item())
        assert np.array_equal(N(dS), ref_dS)
        assert n == np.count_nonzero(ref_dS), (B, mv, n)
        assert np.array_equal(np.sort(N(pairs)[:n]), np.flatnonzero(ref_dS)), (B, mv)      # the order is unspecified
        if mv:
            assert n <= 3 * B


@pytest.mark.parametrize('where', ['nan_off', 'nan_diag', 'inf_off'])
@pytest.mark.parametrize('B', H.HINGE_NAN_BS)
def test_hinge_propagates_non_finite_scores(B, where):
    """a NaN score gives a NaN loss and +inf a +inf loss, as in the oracle (fmaxf(NaN, 0) = 0 would swallow it); the gradient is
    checked only on the rows and columns none of whose costs is touched"""
    from aladin_amd import ops
    S, margin, rows, cols = H.hinge_nonfinite(B, where)
    for mv in MODES:
        with np.errstate(invalid='ignore'):
            ref_loss, ref_dS = O.hinge_loss(S.astype(np.float64), margin, mv, return_grad=True)
        loss, dS, _ = ops._hinge_raw(T(S), margin, mv, True)
        only = ops._hinge_raw(T(S), margin, mv, False)[0]
        print('hinge %s B=%d mv=%d: loss %r oracle %r' % (where, B, mv, F(loss), float(ref_loss)))
        for got in (F(loss), F(only)):
            assert (got == np.inf and ref_loss == np.inf) if where == 'inf_off' else (np.isnan(got) and np.isnan(ref_loss)), (where, B, mv, got)
        assert np.array_equal(N(dS)[np.ix_(rows, cols)], ref_dS[np.ix_(rows, cols)].astype(np.float32)), (where, B, mv)


@pytest.mark.parametrize('side', ['img', 'cap'])
def test_small_batch_hinge_propagates_nan(side):
    """one NaN component in an embedding row makes a row (column) of M NaN: the fused heads' hinge term is NaN, as the separate
    kernels' and the oracle's"""
    from aladin_amd import ops
    img, cap, teacher = H.small_batch_inputs(5, 8)
    img, cap = img.copy(), cap.copy()
    (img if side == 'img' else cap)[2, 3] = np.nan
    M_ref = O.dot_scores(img.astype(np.float64), cap.astype(np.float64))
    assert np.isnan(M_ref[2] if side == 'img' else M_ref[:, 2]).all() and np.isnan(M_ref).sum() == 5
    for mv in MODES:
        with np.errstate(invalid='ignore'):
            assert np.isnan(O.hinge_loss(M_ref, H.HINGE_MARGIN_Q, mv))
        for t in (None, T(teacher)):
            lh, _, M = ops.small_batch_match_distill(T(img), T(cap), t, H.HINGE_MARGIN_Q, mv)
            assert np.array_equal(np.isnan(N(M)), np.isnan(M_ref))
            assert np.isnan(F(lh)), (side, mv, F(lh))
            assert np.isnan(float(ops.hinge_loss(M, H.HINGE_MARGIN_Q, mv)))          # the big-batch kernel on the same M agrees


# ------------------------------------------------------------------------------------------------
# ListNet
# ------------------------------------------------------------------------------------------------
def listnet_ref(teacher, student):
    loss, dM = O.listnet_loss(teacher.astype(np.float64), student.astype(np.float64), return_grad=True)
    return float(loss), dM


@pytest.mark.parametrize('family', H.LISTNET_FAMILIES)
@pytest.mark.parametrize('B', H.LISTNET_BS)
def test_listnet_equals_the_oracle(B, family):
    from aladin_amd import ops
    teacher, student = H.listnet_inputs(B, family)
    ref_loss, ref_dM = listnet_ref(teacher, student)
    st = T(student).requires_grad_(True)
    loss = ops.listnet_loss(T(teacher), st)
    (0.3 * loss).backward()                                                          # a scaled upstream gradient
    got = N(st.grad)
    print('listnet B=%d %s: loss %.9g oracle %.9g, grad max|err|/max|ref| %.3e' % (B, family, F(loss), ref_loss,
                                                                                   H.floor_ratio(got, 0.3 * ref_dM)))
    assert np.isfinite(F(loss))
    np.testing.assert_allclose(F(loss), ref_loss, **H.LISTNET_LOSS_TOL)
    H.assert_cancelling_grad_close(got, 0.3 * ref_dM, 'listnet B=%d %s' % (B, family), family)
    with torch.no_grad():                                                            # forward only: no gradient buffer, one workgroup
        only = ops.listnet_loss(T(teacher), T(student))
    assert F(only) == F(loss)


@pytest.mark.parametrize('family', H.LISTNET_FAMILIES)
def test_listnet_views(family):
    """teacher and student as ld > B views with different leading dimensions; a ::2 student with the gradient in its base"""
    from aladin_amd import ops
    B = H.LISTNET_VIEW_B
    teacher, student = H.listnet_inputs(B, family)
    ref_loss, ref_dM = listnet_ref(teacher, student)
    contig = T(student).requires_grad_(True)
    loss0 = ops.listnet_loss(T(teacher), contig)
    loss0.backward()

    big_t = np.full((B + 2, B + 7), 1e30, np.float32)                                # a stray read would blow the softmax up
    big_s = np.full((B + 1, B + 3), 1e30, np.float32)
    big_t[:B, :B], big_s[:B, :B] = teacher, student
    base = T(big_s).requires_grad_(True)
    loss = ops.listnet_loss(T(big_t)[:B, :B], base[:B, :B])
    loss.backward()
    assert F(loss) == F(loss0)
    np.testing.assert_allclose(F(loss), ref_loss, **H.LISTNET_LOSS_TOL)
    g = N(base.grad)
    assert np.array_equal(g[:B, :B], N(contig.grad)) and not g[B:].any() and not g[:, B:].any()
    H.assert_cancelling_grad_close(g[:B, :B], ref_dM, 'listnet ld > B ' + family, family)

    wide = np.full((B, 2 * B), 1e30, np.float32)
    wide[:, ::2] = student
    base = T(wide).requires_grad_(True)
    loss = ops.listnet_loss(T(teacher), base[:, ::2])
    loss.backward()
    g = N(base.grad)
    assert F(loss) == F(loss0)
    assert np.array_equal(g[:, ::2], N(contig.grad)) and not g[:, 1::2].any()


def test_listnet_propagates_nan():
    from aladin_amd import ops
    teacher, student = H.listnet_inputs(63, 'mild')
    student = student.copy()
    student[4, 9] = np.nan
    assert np.isnan(listnet_ref(teacher, student)[0])
    assert np.isnan(float(ops.listnet_loss(T(teacher), T(student))))


@pytest.mark.parametrize('op', ['hinge', 'listnet', 'distill_contrastive'])
def test_an_expanded_row_is_copied_not_refused(op):
    """A (B, B) expand of one row has unit column stride and row stride 0: the matrix ops copy it (the C ABI refuses ld < B) and give
    the bits of the .contiguous() input, loss and gradient."""
    from aladin_amd import ops
    B = 5
    rng = np.random.default_rng(7)
    row, trow = T(rng.standard_normal(B).astype(np.float32)), T(rng.standard_normal(B).astype(np.float32))
    run = {'hinge': lambda t, s: ops.hinge_loss(s, 0.2, False),
           'listnet': lambda t, s: ops.listnet_loss(t, s),
           'distill_contrastive': lambda t, s: ops.distillation_loss(t, s, 'contrastive')}[op]
    teacher = trow.expand(B, B)
    view = row.expand(B, B).detach().requires_grad_(True)
    contig = row.expand(B, B).contiguous().requires_grad_(True)
    assert view.stride() == (0, 1) and teacher.stride() == (0, 1)
    loss_v, loss_c = run(teacher, view), run(teacher.contiguous(), contig)
    (loss_v * 1.5).backward()
    (loss_c * 1.5).backward()
    assert torch.equal(loss_v.detach(), loss_c.detach()) and torch.isfinite(loss_c)
    assert tuple(view.grad.shape) == (B, B) and torch.equal(view.grad, contig.grad) and contig.grad.any()


# ------------------------------------------------------------------------------------------------
# dot_scores / sgemm
# ------------------------------------------------------------------------------------------------
def operand(x, layout):
    """(leaf, view): view holds x (rows, K); 'n' row-major, 't' the .t() of a (K, rows) buffer, 'c' columns 3 : 3 + K of a wider
    buffer (ld > K, rows misaligned), 's' every second column of a (rows, 2 K) buffer (inner stride 2).  -> also the function
    that takes the leaf's gradient back to x's layout."""
    rows, K = x.shape
    if layout == 'n':
        leaf = T(x).requires_grad_(True)
        return leaf, leaf, lambda g: g
    if layout == 't':
        leaf = T(x.T).requires_grad_(True)
        return leaf, leaf.t(), lambda g: g.T
    if layout == 'c':
        big = np.full((rows, K + 7), 1e30, np.float32)
        big[:, 3:3 + K] = x
        leaf = T(big).requires_grad_(True)
        return leaf, leaf[:, 3:3 + K], lambda g: _only(g, (slice(None), slice(3, 3 + K)))
    assert layout == 's'
    big = np.full((rows, 2 * K), 1e30, np.float32)
    big[:, ::2] = x
    leaf = T(big).requires_grad_(True)
    return leaf, leaf[:, ::2], lambda g: _only(g, (slice(None), slice(None, None, 2)))


def _only(g, index):
    """g[index], after checking that g is zero everywhere else"""
    rest = g.copy()
    rest[index] = 0
    assert not rest.any(), 'gradient outside the view'
    return g[index]


def run_dot(A, Bm, W, la, lb, w_transposed=False):
    from aladin_amd import ops
    leaf_a, a, back_a = operand(A, la)
    leaf_b, b, back_b = operand(Bm, lb)
    assert a.shape == A.shape and b.shape == Bm.shape
    C = ops.dot_scores(a, b)
    w = T(W.T).t() if w_transposed else T(W)
    C.backward(w)
    return N(C), back_a(N(leaf_a.grad)), back_b(N(leaf_b.grad))


def check_dot(M_, N_, K, layouts, w_transposed=False):
    A, Bm, W = H.gemm_inputs(M_, N_, K, 'integer')
    refs, _ = H.gemm_refs(A, Bm, W)
    for la, lb in layouts:
        got = run_dot(A, Bm, W, la, lb, w_transposed)
        for g, r, name in zip(got, refs, ('C', 'd_im', 'd_s')):
            assert g.shape == r.shape and np.array_equal(g, r), ((M_, N_, K), la + lb, name, int((g != r).sum()))
    A, Bm, W = H.gemm_inputs(M_, N_, K, 'normal')
    refs, bounds = H.gemm_refs(A, Bm, W)
    la, lb = layouts[0]
    got = run_dot(A, Bm, W, la, lb, w_transposed)
    for g, r, bound, name in zip(got, refs, bounds, ('C', 'd_im', 'd_s')):
        err = np.abs(g.astype(np.float64) - r)
        print('dot %s %s%s %s: max err / bound %.3f' % ((M_, N_, K), la, lb, name, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), ((M_, N_, K), la + lb, name)


@pytest.mark.parametrize('M_,N_,K', H.GEMM_SHAPES)
def test_dot_scores_is_exact_in_the_four_storage_layouts(M_, N_, K):
    check_dot(M_, N_, K, [(la, lb) for la, lb in H.GEMM_LAYOUTS])


@pytest.mark.parametrize('M_,N_,K', H.GEMM_VIEW_SHAPES)
def test_dot_scores_views(M_, N_, K):
    check_dot(M_, N_, K, [('c', 'c'), ('s', 's'), ('c', 't'), ('n', 's')])
    check_dot(M_, N_, K, [('n', 'n'), ('t', 't')], w_transposed=True)


# ------------------------------------------------------------------------------------------------
# l2norm
# ------------------------------------------------------------------------------------------------
def run_l2norm(view, leaf, g):
    from aladin_amd import ops
    out = ops.l2norm_rows(view)
    out.backward(T(g))
    return N(out), N(leaf.grad)


def check_l2norm(out, dx, x, g, what):
    ref_out, ref_dx = H.l2norm_ref(x, g)
    bad = np.isnan(ref_out).any(1)                                                   # zero rows: NaN exactly there
    assert np.array_equal(np.isnan(out), np.isnan(ref_out)) and np.array_equal(np.isnan(dx), np.isnan(ref_dx)), what
    np.testing.assert_allclose(out[~bad], ref_out[~bad], err_msg=what, **H.L2NORM_FWD_TOL)
    if (~bad).any():
        assert (np.abs(dx[~bad] - ref_dx[~bad]) <= H.l2norm_bwd_tol(ref_dx[~bad])).all(), what


@pytest.mark.parametrize('rows,D', H.L2NORM_SHAPES)
def test_l2norm_contiguous_and_in_place_view(rows, D):
    x, g = H.l2norm_inputs(rows, D)
    leaf = T(x).requires_grad_(True)
    out0, dx0 = run_l2norm(leaf, leaf, g)
    check_l2norm(out0, dx0, x, g, ('contiguous', rows, D))
    big = np.full((rows, D + 5), 1e30, np.float32)                                   # a stray read would swamp the norm
    big[:, 2:2 + D] = x
    leaf = T(big).requires_grad_(True)
    view = leaf[:, 2:2 + D]
    assert view.stride(1) == 1                                                       # used in place: row_stride > D
    out, dbig = run_l2norm(view, leaf, g)
    assert np.array_equal(out, out0) and np.array_equal(_only(dbig, (slice(None), slice(2, 2 + D))), dx0), (rows, D)
    if rows == 1 and D == 200:                                                       # one row over column storage: stride(0) = 1 < D
        leaf = T(x.reshape(D, 1)).requires_grad_(True)
        view = leaf.t()
        assert view.shape == (1, D) and view.stride(1) == 1
        out, dcol = run_l2norm(view, leaf, g)
        assert np.array_equal(out, out0) and np.array_equal(dcol.reshape(1, D), dx0)


@pytest.mark.parametrize('rows,D', [(5, 65), (9, 1000)])
def test_l2norm_zero_row(rows, D):
    x, g = H.l2norm_inputs(rows, D, zero_row=rows // 2)
    leaf = T(x).requires_grad_(True)
    out, dx = run_l2norm(leaf, leaf, g)
    assert np.isnan(out[rows // 2]).all() and np.isnan(dx[rows // 2]).all()
    check_l2norm(out, dx, x, g, ('zero row', rows, D))
    x1, _ = H.l2norm_inputs(rows, D)                                                 # the other rows: as without the zero row
    leaf = T(x1).requires_grad_(True)
    out1, dx1 = run_l2norm(leaf, leaf, g)
    keep = np.arange(rows) != rows // 2
    assert np.array_equal(out[keep], out1[keep]) and np.array_equal(dx[keep], dx1[keep])


# ------------------------------------------------------------------------------------------------
# single-row / single-column operands whose size-1 dimension reports an arbitrary stride
# ------------------------------------------------------------------------------------------------
def one_row_views(x):
    """views of a (1, D) array whose row stride is arbitrary -> [(leaf, view, gradient-of-leaf -> (1, D))]"""
    D = x.shape[1]
    col = T(x.reshape(D, 1)).requires_grad_(True)                                    # .t() of column storage: strides (1, 1)
    flat = T(x.reshape(D)).requires_grad_(True)
    return [(col, col.t(), lambda g: g.reshape(1, D)),
            (flat, flat.as_strided((1, D), (7, 1)), lambda g: g.reshape(1, D)),      # an odd row stride, not a multiple of 4
            (flat, flat.as_strided((1, D), (0, 1)), lambda g: g.reshape(1, D))]


@pytest.mark.parametrize('op', ['dot_scores', 'order_scores'])
@pytest.mark.parametrize('D', [1, 33, 200])
def test_single_row_operands_with_arbitrary_row_stride(op, D):
    """Bi = 1 and Bc = 1 through dot_scores and order_scores: the results of the contiguous copy, forward and backward"""
    from aladin_amd import ops
    fn = getattr(ops, op)
    rng = np.random.default_rng(D)
    for Bi, Bc in ((1, 9), (9, 1), (1, 1)):
        im = rng.standard_normal((Bi, D)).astype(np.float32)
        s = (rng.standard_normal((Bc, D)) + 0.3).astype(np.float32)
        w = rng.standard_normal((Bi, Bc)).astype(np.float32)
        a0, b0 = T(im).requires_grad_(True), T(s).requires_grad_(True)
        out0 = fn(a0, b0)
        out0.backward(T(w))
        ga0, gb0 = N(a0.grad).copy(), N(b0.grad).copy()
        if op == 'dot_scores':
            (ref, _, _), (bound, _, _) = H.gemm_refs(im, s, w)
            assert (np.abs(N(out0) - ref) <= bound).all()
        else:                                                                        # the figures tests/fuzz/fuzz_losses.py holds order_scores to
            np.testing.assert_allclose(N(out0), O.order_scores(im, s), rtol=5e-6, atol=1e-6)
        keep = lambda leaf: [(leaf, leaf, lambda g: g)]
        for la, va, back_a in (one_row_views(im) if Bi == 1 else keep(a0)):
            for lb, vb, back_b in (one_row_views(s) if Bc == 1 else keep(b0)):
                la.grad = lb.grad = None
                out = fn(va, vb)
                out.backward(T(w))
                assert torch.equal(out, out0), (op, Bi, Bc, D, va.stride(), vb.stride())
                # order_scores: 0 / 0 = NaN where a pair has no violation, as autograd in the reference
                assert np.array_equal(back_a(N(la.grad)), ga0, equal_nan=True), (op, Bi, Bc, D, va.stride())
                assert np.array_equal(back_b(N(lb.grad)), gb0, equal_nan=True), (op, Bi, Bc, D, vb.stride())


@pytest.mark.parametrize('D', [1, 63, 200, 3000])
def test_l2norm_single_row_with_arbitrary_row_stride(D):
    from aladin_amd import ops
    x, g = H.l2norm_inputs(1, D)
    leaf0 = T(x).requires_grad_(True)
    out0, dx0 = run_l2norm(leaf0, leaf0, g)
    check_l2norm(out0, dx0, x, g, ('single row', D))
    for leaf, view, back in one_row_views(x):
        leaf.grad = None
        out, dleaf = run_l2norm(view, leaf, g)
        assert np.array_equal(out, out0) and np.array_equal(back(dleaf), dx0), (D, view.stride())
    col = T(np.ascontiguousarray(np.broadcast_to(x.reshape(D, 1), (D, 3)))).requires_grad_(True)    # single COLUMN inputs: (D, 1), row stride 3
    out = ops.l2norm_rows(col[:, 1:2])
    np.testing.assert_allclose(N(out), np.sign(x).reshape(D, 1), **H.L2NORM_FWD_TOL)


# ------------------------------------------------------------------------------------------------
# small-batch fused heads against the oracle (not against the separate kernels: a shared mistake would cancel)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', H.SMALL_DS)
@pytest.mark.parametrize('B', H.SMALL_BS)
def test_small_batch_heads_equal_the_oracle(B, D):
    from aladin_amd import ops
    img, cap, teacher = H.small_batch_inputs(B, D)
    M_ref = O.dot_scores(img.astype(np.float64), cap.astype(np.float64))
    ll_ref, dMl = O.listnet_loss(teacher.astype(np.float64), M_ref, return_grad=True)
    for mv in MODES:
        lh_ref, dMh = O.hinge_loss(M_ref, H.HINGE_MARGIN_Q, mv, return_grad=True)
        a, b = T(img).requires_grad_(True), T(cap).requires_grad_(True)
        lh, ll, M = ops.small_batch_match_distill(a, b, T(teacher), H.HINGE_MARGIN_Q, mv)
        what = 'small B=%d D=%d mv=%d' % (B, D, mv)
        print('%s: hinge %.9g (%.9g) listnet %.9g (%.9g)' % (what, F(lh), float(lh_ref), F(ll), float(ll_ref)))
        assert np.array_equal(N(M), M_ref), what                                     # exact products (CPU tier)
        assert abs(F(lh) - float(lh_ref)) <= H.HINGE_LOSS_RTOL * abs(float(lh_ref)), what
        np.testing.assert_allclose(F(ll), float(ll_ref), **H.LISTNET_LOSS_TOL)
        # the hinge gradient on M alone: integer coefficients times multiples of 1/16, exact -> must EQUAL the float64 chain
        lh.backward(retain_graph=True)
        assert np.array_equal(N(a.grad), dMh @ cap.astype(np.float64)) and np.array_equal(N(b.grad), dMh.T @ img.astype(np.float64)), what
        a.grad = b.grad = None
        (H.SMALL_G_HINGE * lh + H.SMALL_G_LISTNET * ll).backward()
        coef = H.SMALL_G_HINGE * dMh + H.SMALL_G_LISTNET * dMl
        H.assert_cancelling_grad_close(N(a.grad), coef @ cap.astype(np.float64), what + ' d_img')
        H.assert_cancelling_grad_close(N(b.grad), coef.T @ img.astype(np.float64), what + ' d_cap')
