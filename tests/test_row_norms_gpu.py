"""GPU tier (-m gpu): the row-norm contract of every kernel that normalises rows -- the row encoder of csrc/pack_rows.hpp and its
inverse-norm slots [xm | xe | y], the slot look-ups of the backward row step (csrc/align_bwd.hip) and their long-set copies
(csrc/align_long.hip), the dense backward's own normalisers (csrc/align_bwd_dense.hip, csrc/bwd_common.hpp), the private ones of
csrc/pool.hip and csrc/scan.hip, and the store packers (csrc/store.hip).

Every other alignment input of the suite has rows of practically ONE norm, so a row that met a neighbour's inverse norm would be a
few per cent off on one row, and a gradient tolerance scaled by the tensor's largest entry sees only the largest rows.  Here each
case is run on the synthetic inputs (base) and on the same inputs with every row multiplied by its own factor, both sides
independently, same lengths, same upstream gradient (tests/helpers/row_scaling.py):

  1. determinism: two base calls are bit-equal, outputs and gradients;
  2. exact covariance under powers of two (exponents in [-30, 30], adversarial positions forced per packed row map): outputs
     bit-equal, and 2^k times the gradient of a scaled row bit-equal to the gradient of the unscaled row; dropped positions
     (position 0, the tail, everything past the length) exactly 0 in both.  No tolerance: any row paired with the wrong norm
     breaks it;
  3. the float64 oracle on decade factors 10^U(-3, 3): scores through test_gpu_parity's assert_scores_close (split operands: the
     tolerances of test_alignment_scores_shape_sweep), gradients through its assert_grads_close gates AFTER each row of `got` and
     `ref` is multiplied by that row's input norm.  That removes the 1 / |row| factor: what is compared is the projected sum of
     partner unit vectors per row, the quantity the existing tests compare on equal-norm data, and the same gates now bind on
     every row.  exact_atol is what the neighbouring test of the same op passes (named at each use).
Every gradient case runs under the three row steps of ops.set_backward_precision; the inverse-norm slots are read by 'fp16-own'
alone.  The dense backward is reached from B = 128 (B * B >= ops.DENSE_MIN_PAIRS).

tests/test_row_norms_cpu.py shows that the reference's restatements themselves satisfy 2 and that the forced positions land on the
packed rows they are meant for."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import alad_oracle as O
import faithful_torch as FT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import row_scaling as RS                 # noqa: E402

pytestmark = pytest.mark.gpu

ids = lambda s: 'x'.join(map(str, s))    # noqa: E731


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(dev())          # a copy: the cases' arrays are shared and read-only


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(params=['exact', 'fp16', 'fp16-own'])
def bwd_mode(request):
    """The row steps of the alignment backward: the two of test_gpu_parity.bwd_mode, and the opt-in 'fp16-own' -- the ONLY mode in
    which the row step reads a row's inverse norm from the packers' [xm | xe | y] slots (packed_x_rnorm / packed_y_rnorm of
    csrc/align_bwd.hip, their copies in csrc/align_long.hip) instead of normalising the raw row again."""
    from aladin_amd import ops
    old = ops.set_backward_precision(request.param)
    yield request.param
    ops.set_backward_precision(old)


@pytest.fixture
def fresh_density_probes():
    """The dense / list choice of the backward follows earlier steps' pair counts: start every case from the same state."""
    from aladin_amd import ops
    ops._density_probe.__init__()
    ops._generic_probes.clear()
    yield
    ops._density_probe.__init__()
    ops._generic_probes.clear()


# ------------------------------------------------------------------------------------------------
# the three checks
# ------------------------------------------------------------------------------------------------
def assert_same_bits(got, want, what, k=None):
    """np.array_equal on float32 arrays, with the rows that differ (and their exponents) in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.isfinite(want).all(), what
    if np.array_equal(got, want):
        return
    bad = np.argwhere((got != want).reshape(got.shape[0], -1).any(-1) if got.ndim < 3 else (got != want).any(-1))
    rows = [tuple(int(v) for v in r) for r in bad[:12]]
    detail = []
    for r in rows[:6]:
        g, w = got[r], want[r]
        detail.append('%s%s: max|got| %.4g max|want| %.4g' % (r, '' if k is None or got.ndim < 3 else ' k=%d' % k[r],
                                                               np.abs(g).max(), np.abs(w).max()))
    raise AssertionError('%s: %d of %d rows differ, first %s; %s' % (what, len(bad), int(np.prod(got.shape[:-1])) if got.ndim > 1 else got.size,
                                                                  rows, '; '.join(detail)))


def assert_dropped_rows_zero(d_im, d_s, il, sl):
    """Region 0, token 0, the last two tokens and every padded position carry exactly no gradient."""
    for i, L in enumerate(il):
        assert not d_im[i, 0].any() and not d_im[i, L:].any(), ('image', i)
    for j, L in enumerate(sl):
        assert not d_s[j, 0].any() and not d_s[j, max(L - 2, 1):].any(), ('caption', j)


def check_determinism(first, second, what):
    for n, (a, b) in enumerate(zip(first, second)):
        assert_same_bits(b, a, '%s: output %d of two base calls' % (what, n))


def check_covariance(c, base, scaled, what, n_out=1):
    """base / scaled: (outputs..., d_im, d_s) of the call on (c.im, c.s) and on (c.im2, c.s2)."""
    for n in range(n_out):
        assert_same_bits(scaled[n], base[n], '%s: output %d, scaled rows vs base' % (what, n))
    (gi0, gs0), (gi1, gs1) = base[n_out:n_out + 2], scaled[n_out:n_out + 2]
    assert np.abs(gi0).max() > 0 and np.abs(gs0).max() > 0, what
    RS.assert_grad_unscaling_is_exact(gi1)
    RS.assert_grad_unscaling_is_exact(gs1)
    assert_same_bits(RS.unscale_grad(gi1, c.kx), gi0, '%s: 2^k x (max-side gradient of the scaled rows) vs base' % what, c.kx)
    assert_same_bits(RS.unscale_grad(gs1, c.ky), gs0, '%s: 2^k x (sum-side gradient of the scaled rows) vs base' % what, c.ky)
    for gi, gs in ((gi0, gs0), (gi1, gs1)):
        assert_dropped_rows_zero(gi, gs, c.il, c.sl)


def check_row_weighted_grads(got, ref, x, mode, exact_atol, D):
    """assert_grads_close of test_gpu_parity on rows multiplied by their input norms (float64, host).  'fp16-own' is no mode of
    that function: it is held to what test_default_backward_row_step_vs_reference holds it to, rtol 1e-3 + 1e-3 of the largest
    entry (the row's own unit vector carries an fp16 rounding too: 5.8e-4 measured on equal-norm data, which is why it is an
    opt-in)."""
    import test_gpu_parity as G
    n = RS.row_norms(x)
    got, ref = np.asarray(got, np.float64) * n, np.asarray(ref, np.float64) * n
    scale = max(1e-9, float(np.abs(ref).max()))
    print('row-weighted gradient (%s, D=%d): max |err| / max |ref| %.3g' % (mode, D, np.abs(got - ref).max() / scale))
    if mode == 'fp16-own':
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-3 * scale)
    else:
        G.assert_grads_close(got, ref, mode, exact_atol=exact_atol, D=D)


def check_scores(S, ref, precision):
    import test_gpu_parity as G
    assert S.shape == ref.shape and np.isfinite(S).all()
    if precision == 'split':
        np.testing.assert_allclose(S, ref, rtol=3e-6, atol=3e-6)          # test_alignment_scores_shape_sweep
    else:
        G.assert_scores_close(S, ref)


_REFS = {}


def faithful_reference(c, agg):
    """The reference's dataflow in double on the DECADE-scaled inputs, upstream gradient c.w: (S, d_im, d_s), once per case."""
    key = (c.shape, agg)
    if key not in _REFS:
        a, b = torch.from_numpy(np.array(c.im10)).double().requires_grad_(True), torch.from_numpy(np.array(c.s10)).double().requires_grad_(True)
        S = FT.alignment_scores_faithful(a, b, c.il, c.sl, agg)
        (S * torch.from_numpy(np.array(c.w)).double()).sum().backward()
        _REFS[key] = tuple(v.copy() for v in (S.detach().numpy(), a.grad.numpy(), b.grad.numpy()))
        for v in _REFS[key]:
            v.setflags(write=False)
    return _REFS[key]


def oracle_backward(c, dS, tag):
    """alad_oracle.alignment_scores_backward on the decade-scaled inputs for the dS of the HIP scores, once per case (dS is a
    function of the forward's fp16 scores, which do not depend on the backward's mode)."""
    key = (c.shape, tag)
    if key not in _REFS:
        _REFS[key] = (np.array(dS),) + O.alignment_scores_backward(c.im10, c.s10, c.il, c.sl, dS)
    assert np.array_equal(_REFS[key][0], dS), 'the hinge gradient of the HIP scores changed between two runs of one case'
    return _REFS[key][1:]


# ------------------------------------------------------------------------------------------------
# ops.alignment_scores
# ------------------------------------------------------------------------------------------------
def scores_no_grad(im, s, il, sl, agg, precision):
    from aladin_amd import ops
    with torch.no_grad():
        return (N(ops.alignment_scores(T(im), T(s), il, sl, agg, precision=precision)),)


def scores_with_grad(im, s, il, sl, w, agg):
    from aladin_amd import ops
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    S = ops.alignment_scores(a, b, il, sl, agg)
    (S * T(w)).sum().backward()
    return N(S), N(a.grad), N(b.grad)


@pytest.mark.parametrize('shape', RS.TILE_SHAPES + [RS.FORWARD_ONLY_SHAPE] + RS.LONG_SHAPES, ids=ids)
@pytest.mark.parametrize('precision', ['fp16', 'split'])
def test_scores_without_grad(shape, precision):
    """No-grad 'MrSw' scores in both evaluation precisions: the packers (vector, scalar at D % 8 != 0, streamed at D = 1088,
    long-set) and the score kernels.  The split operands hi / lo are rounded from x * inv * 2^14: bit-equal as well."""
    c = RS.alignment_case(shape)
    what = 'alignment_scores[no grad, %s]' % precision
    base = scores_no_grad(c.im, c.s, c.il, c.sl, 'MrSw', precision)
    check_determinism(base, scores_no_grad(c.im, c.s, c.il, c.sl, 'MrSw', precision), what)
    assert_same_bits(scores_no_grad(c.im2, c.s2, c.il, c.sl, 'MrSw', precision)[0], base[0], what + ': scaled rows vs base')
    # one side scaled at a time: a slot mix-up inside one operand cannot hide behind the other
    assert_same_bits(scores_no_grad(c.im2, c.s, c.il, c.sl, 'MrSw', precision)[0], base[0], what + ': scaled images vs base')
    assert_same_bits(scores_no_grad(c.im, c.s2, c.il, c.sl, 'MrSw', precision)[0], base[0], what + ': scaled captions vs base')
    S10 = scores_no_grad(c.im10, c.s10, c.il, c.sl, 'MrSw', precision)[0]
    check_scores(S10, O.alignment_scores(c.im10, c.s10, c.il, c.sl, 'MrSw', dtype=np.float64), precision)


@pytest.mark.parametrize('shape', RS.TILE_SHAPES + RS.LONG_SHAPES, ids=ids)
def test_scores_with_grad(shape, bwd_mode):
    """Differentiable 'MrSw' scores, a gradient on S: the pair kernels' exact re-decision, the row step's own normalisers ('exact':
    own row and partners; 'fp16': own row, partners from the packed operands) and its inverse-norm slot look-ups ('fp16-own'), tile
    classes and long sets."""
    c = RS.alignment_case(shape)
    what = 'alignment_scores[grad, %s]' % bwd_mode
    base = scores_with_grad(c.im, c.s, c.il, c.sl, c.w, 'MrSw')
    check_determinism(base, scores_with_grad(c.im, c.s, c.il, c.sl, c.w, 'MrSw'), what)
    check_covariance(c, base, scores_with_grad(c.im2, c.s2, c.il, c.sl, c.w, 'MrSw'), what)
    S10, gi, gs = scores_with_grad(c.im10, c.s10, c.il, c.sl, c.w, 'MrSw')
    Sr, ri, rs = faithful_reference(c, 'MrSw')
    check_scores(S10, Sr, 'fp16')
    # exact_atol: test_leftover_regions_as_side_rows (a gradient on S against the reference's dataflow) passes 5e-5; the long-set
    # neighbour test_long_gradients_of_the_other_poolings keeps the default
    atol = 2e-5 if shape in RS.LONG_SHAPES else 5e-5
    check_row_weighted_grads(gi, ri, c.im10, bwd_mode, atol, shape[4])
    check_row_weighted_grads(gs, rs, c.s10, bwd_mode, atol, shape[4])
    assert_dropped_rows_zero(gi, gs, c.il, c.sl)


@pytest.mark.parametrize('shape', RS.TILE_SHAPES[:2], ids=ids)
@pytest.mark.parametrize('agg', ['MwSr', 'symm'])
@pytest.mark.parametrize('precision', ['fp16', 'split'])
def test_other_aggregations_without_grad(shape, agg, precision):
    """'MwSr' / 'symm': the same kernels with the sets' roles swapped -- captions in the [xm | xe] slots, images in y."""
    c = RS.alignment_case(shape)
    what = 'alignment_scores[no grad, %s, %s]' % (agg, precision)
    base = scores_no_grad(c.im, c.s, c.il, c.sl, agg, precision)
    check_determinism(base, scores_no_grad(c.im, c.s, c.il, c.sl, agg, precision), what)
    assert_same_bits(scores_no_grad(c.im2, c.s2, c.il, c.sl, agg, precision)[0], base[0], what + ': scaled rows vs base')
    S10 = scores_no_grad(c.im10, c.s10, c.il, c.sl, agg, precision)[0]
    check_scores(S10, O.alignment_scores(c.im10, c.s10, c.il, c.sl, agg, dtype=np.float64), precision)


@pytest.mark.parametrize('shape', RS.TILE_SHAPES[:2], ids=ids)
@pytest.mark.parametrize('agg', ['MwSr', 'symm'])
def test_other_aggregations_with_grad(shape, agg, bwd_mode):
    c = RS.alignment_case(shape)
    what = 'alignment_scores[grad, %s, %s]' % (agg, bwd_mode)
    base = scores_with_grad(c.im, c.s, c.il, c.sl, c.w, agg)
    check_determinism(base, scores_with_grad(c.im, c.s, c.il, c.sl, c.w, agg), what)
    check_covariance(c, base, scores_with_grad(c.im2, c.s2, c.il, c.sl, c.w, agg), what)
    S10, gi, gs = scores_with_grad(c.im10, c.s10, c.il, c.sl, c.w, agg)
    Sr, ri, rs = faithful_reference(c, agg)
    check_scores(S10, Sr, 'fp16')
    # exact_atol 3e-5: test_alignment_other_modes_loss_and_gradients
    check_row_weighted_grads(gi, ri, c.im10, bwd_mode, 3e-5, shape[4])
    check_row_weighted_grads(gs, rs, c.s10, bwd_mode, 3e-5, shape[4])


# ------------------------------------------------------------------------------------------------
# 'sum' / 'mean' pooling (csrc/pool.hip) and scan-sentences (csrc/scan.hip): normalisers of their own, fp32 end to end
# ------------------------------------------------------------------------------------------------
def sum_scores_with_grad(im, s, il, sl, w, mean):
    from aladin_amd import ops
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    S = ops.alignment_sum_scores(a, b, il, sl, mean=mean)
    (S * T(w)).sum().backward()
    return N(S), N(a.grad), N(b.grad)


@pytest.mark.parametrize('shape', RS.TILE_SHAPES[:2], ids=ids)
@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
def test_sum_and_mean_pooling(shape, mean):
    c = RS.alignment_case(shape)
    what = 'alignment_sum_scores[mean=%s]' % mean
    base = sum_scores_with_grad(c.im, c.s, c.il, c.sl, c.w, mean)
    check_determinism(base, sum_scores_with_grad(c.im, c.s, c.il, c.sl, c.w, mean), what)
    check_covariance(c, base, sum_scores_with_grad(c.im2, c.s2, c.il, c.sl, c.w, mean), what)
    S10, gi, gs = sum_scores_with_grad(c.im10, c.s10, c.il, c.sl, c.w, mean)
    Sr, ri, rs = faithful_reference(c, 'mean' if mean else 'sum')
    # scores: the tolerance of test_alignment_module_modes for these poolings; gradients: 'exact' gate with exact_atol 3e-5, as
    # test_alignment_other_modes_loss_and_gradients holds them (no fp16 operand anywhere on this path)
    np.testing.assert_allclose(S10, Sr, rtol=1e-4, atol=2e-6 * max(1e-6, float(np.abs(Sr).max())) + 1e-6)
    check_row_weighted_grads(gi, ri, c.im10, 'exact', 3e-5, shape[4])
    check_row_weighted_grads(gs, rs, c.s10, 'exact', 3e-5, shape[4])


def scan_scores_with_grad(im, s, il, sl, w):
    from aladin_amd import ops
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    S = ops.alignment_scan_scores(a, b, il, sl)
    (S * T(w)).sum().backward()
    return N(S), N(a.grad), N(b.grad)


@pytest.mark.parametrize('shape', RS.TILE_SHAPES[:2], ids=ids)
def test_scan_sentences(shape):
    c = RS.alignment_case(shape)
    what = 'alignment_scan_scores'
    base = scan_scores_with_grad(c.im, c.s, c.il, c.sl, c.w)
    check_determinism(base, scan_scores_with_grad(c.im, c.s, c.il, c.sl, c.w), what)
    check_covariance(c, base, scan_scores_with_grad(c.im2, c.s2, c.il, c.sl, c.w), what)
    S10, gi, gs = scan_scores_with_grad(c.im10, c.s10, c.il, c.sl, c.w)
    Sr, ri, rs = O.scan_sentences_scores(c.im10, c.s10, c.il, c.sl, dS=np.asarray(c.w, np.float64))
    # the tolerances of test_scan_sentences_ragged_vs_oracle, on row-norm-weighted gradients
    np.testing.assert_allclose(S10, Sr, rtol=3e-5, atol=5e-6)
    ni, ns = RS.row_norms(c.im10), RS.row_norms(c.s10)
    scale = max(1e-3, float(np.abs(ri * ni).max()), float(np.abs(rs * ns).max()))
    np.testing.assert_allclose(gi.astype(np.float64) * ni, ri * ni, rtol=2e-4, atol=1e-5 * scale)
    np.testing.assert_allclose(gs.astype(np.float64) * ns, rs * ns, rtol=2e-4, atol=1e-5 * scale)


# ------------------------------------------------------------------------------------------------
# ops.alignment_triplet_loss: the fused node (pair-list backward) and the sum of violations (list and dense backward)
# ------------------------------------------------------------------------------------------------
DENSE_B = 128            # the smallest batch with B * B >= ops.DENSE_MIN_PAIRS (1 << 14): below it the backward never takes the dense path


def triplet_step(im, s, il, sl, mv):
    from aladin_amd import ops
    ops._density_probe.__init__()
    ops._LAST_BWD_FLAGS[0] = 0                                            # (the fused node's own backward does not report)
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    loss, S = ops.alignment_triplet_loss(a, b, il, sl, 0.2, mv)
    loss.backward()
    return N(loss).reshape(1), N(S), N(a.grad), N(b.grad), ops._LAST_BWD_FLAGS[0]


def check_triplet(shape, mv, bwd_mode, what, dense_bits=None):
    from aladin_amd import _lib
    import test_gpu_parity as G
    c = RS.alignment_case(shape, structured=True)
    runs = [triplet_step(x, y, c.il, c.sl, mv) for x, y in ((c.im, c.s), (c.im, c.s), (c.im2, c.s2), (c.im10, c.s10))]
    if dense_bits is not None:
        for r in runs:
            assert r[4] & (_lib.BWD_DENSE | _lib.BWD_DENSE_GATHER) == dense_bits, (r[4], dense_bits)
    base, again, scaled, decade = (r[:4] for r in runs)
    check_determinism(base, again, what)
    check_covariance(c, base, scaled, what, n_out=2)
    loss, S10, gi, gs = decade
    G.assert_scores_close(S10, O.alignment_scores(c.im10, c.s10, c.il, c.sl, dtype=np.float64))
    # as test_alignment_backward_shape_sweep: the oracle chained on the HIP scores, default exact_atol
    ref_loss, dS = O.hinge_loss(S10, 0.2, mv, return_grad=True)
    np.testing.assert_allclose(loss[0], ref_loss, rtol=1e-5, atol=1e-6)
    assert (dS != 0).any()
    ri, rs = oracle_backward(c, dS, ('triplet', mv))
    check_row_weighted_grads(gi, ri, c.im10, bwd_mode, 2e-5, shape[4])
    check_row_weighted_grads(gs, rs, c.s10, bwd_mode, 2e-5, shape[4])


@pytest.mark.parametrize('shape', [(10, 10, 51, 38, 128), (12, 12, 34, 50, 64)], ids=ids)
@pytest.mark.parametrize('mv', [True, False], ids=['hardest', 'sum'])
def test_triplet_loss_pair_list_backward(shape, mv, bwd_mode, fresh_density_probes):
    """max_violation=True: the fused forward's arg-max table + the row step; False at this size: pack + scores + hinge and the
    pair-list backward."""
    check_triplet(shape, mv, bwd_mode, 'alignment_triplet_loss[mv=%s, %s]' % (mv, bwd_mode), dense_bits=0)


@pytest.mark.parametrize('shape', [(DENSE_B, DENSE_B, 51, 38, 128), (DENSE_B, DENSE_B, 34, 50, 64)], ids=ids)
@pytest.mark.parametrize('rows', ['gemm', 'gather'])
def test_triplet_loss_dense_backward(shape, rows, bwd_mode, fresh_density_probes, monkeypatch):
    """Sum of violations at B = 128: the dense arg-max table (split-precision tile kernel, its own normaliser) and both of its row
    steps -- the two GEMMs over re-normalised operands and the per-row gather."""
    from aladin_amd import _lib, ops
    monkeypatch.setattr(ops, 'DENSE_MIN_FRACTION', 0.0)                   # whatever the density of this batch's dS
    if rows == 'gemm':
        monkeypatch.setattr(ops, 'DENSE_GEMM_FORCE', True)                # ... and however full its captions
    else:
        monkeypatch.setattr(ops, 'DENSE_ROWS_GEMM', False)
    check_triplet(shape, False, bwd_mode, 'alignment_triplet_loss[dense %s, %s]' % (rows, bwd_mode),
                  dense_bits=_lib.BWD_DENSE | (_lib.BWD_DENSE_GATHER if rows == 'gather' else 0))


# ------------------------------------------------------------------------------------------------
# the single-node loss heads at B <= 64 (csrc/small_batch.hip + the alignment kernels): only the sets are scaled
# ------------------------------------------------------------------------------------------------
HEADS = ('matching', 'alignment', 'distillation')
HEAD_WEIGHTS = {'matching': 0.1, 'alignment': 1.0, 'distillation': 0.75}


def heads_step(ge, gc, im, s, il, sl):
    from aladin_amd import ops
    x, y, a, b = (T(v).requires_grad_(True) for v in (ge, gc, im, s))
    total, terms, S, M = ops.small_batch_loss_heads(x, y, a, b, il, sl, 0.2, True, HEADS, HEAD_WEIGHTS)
    total.backward()
    return N(total).reshape(1), N(terms), N(S), N(M), N(x.grad), N(y.grad), N(a.grad), N(b.grad)


@pytest.mark.parametrize('B', [8, 33])
def test_small_batch_loss_heads(B, bwd_mode):
    from aladin_amd import ops, synth
    import test_gpu_parity as G
    assert B <= ops.SMALL_BATCH_MAX
    shape = (B, B, 34, 50, 64)
    c = RS.alignment_case(shape, structured=True)
    ge, gc = synth.global_embeddings(B, 64, seed=500 + B, noise=1.0)
    what = 'small_batch_loss_heads[B=%d, %s]' % (B, bwd_mode)
    base = heads_step(ge, gc, c.im, c.s, c.il, c.sl)
    check_determinism(base, heads_step(ge, gc, c.im, c.s, c.il, c.sl), what)
    # total, terms, S, M and the embeddings' gradients: bit-equal; the sets' gradients: exactly 2^-k per row
    check_covariance(c, base, heads_step(ge, gc, c.im2, c.s2, c.il, c.sl), what, n_out=6)
    total, terms, S10, M, _, _, gi, gs = heads_step(ge, gc, c.im10, c.s10, c.il, c.sl)
    G.assert_scores_close(S10, O.alignment_scores(c.im10, c.s10, c.il, c.sl, dtype=np.float64))
    ref_loss, dS = O.hinge_loss(S10, 0.2, True, return_grad=True)
    np.testing.assert_allclose(terms[1], ref_loss, rtol=1e-5, atol=1e-6)
    # only the alignment hinge reaches the sets (ListNet's teacher is detached), weight 1: as test_alignment_backward_shape_sweep
    ri, rs = oracle_backward(c, dS * HEAD_WEIGHTS['alignment'], ('heads',))
    check_row_weighted_grads(gi, ri, c.im10, bwd_mode, 2e-5, 64)
    check_row_weighted_grads(gs, rs, c.s10, bwd_mode, 2e-5, 64)


# ------------------------------------------------------------------------------------------------
# store.PackedSetStore (csrc/store.hip): the packed rows themselves, and everything scored from them
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_packed_set_stores(precision):
    """Stores filled from scaled and from unscaled sets (the edge problem of tests/test_rerank_gpu.py at D = 64) hold the same
    bits -- a store keeps unit rows only, no norms -- and so do the grid scores, the scores of listed pairs and their alignment
    maps, arg-max indices included; the grid of decade-scaled sets against the float64 oracle."""
    import test_rerank_gpu as RR
    from aladin_amd.store import alignment_map_for_pairs, alignment_scores_for_pairs, alignment_scores_from_stores
    D, n_img, n_cap = 64, 23, 27
    rng = np.random.RandomState(D)
    ic = [RR.IMG_COUNTS[k % len(RR.IMG_COUNTS)] for k in range(n_img)]
    cc = [RR.CAP_COUNTS[k % len(RR.CAP_COUNTS)] for k in rng.permutation(n_cap)]
    images, il = RR.make_sets(ic, 0, D, 100 + D)
    captions, cl = RR.make_sets(cc, 2, D, 200 + D)
    # first and last scored position of every sample at opposite extremes, the rest drawn
    kx = RS.pow2_row_scales(images.shape[:2], 61, forced={(b, p): e for b, L in enumerate(il) for p, e in ((1, RS.KMAX), (L - 1, RS.KMIN)) if L > 2})
    ky = RS.pow2_row_scales(captions.shape[:2], 62, forced={(b, p): e for b, L in enumerate(cl) for p, e in ((1, RS.KMIN), (L - 3, RS.KMAX)) if L > 4})
    RS.assert_pow2_scaling_is_exact(images, kx)
    RS.assert_pow2_scaling_is_exact(captions, ky)
    sets = {'base': (images, captions), 'again': (images, captions), 'scaled': (RS.scale_rows(images, kx), RS.scale_rows(captions, ky))}
    cands = {d: torch.from_numpy(RR.random_shortlist(nq, ng, 7, 11)).to(dev()) for d, nq, ng in (('i2t', n_img, n_cap), ('t2i', n_cap, n_img))}
    out = {}
    for name, (x, y) in sets.items():
        si, sc = RR.fill_store(x, il, 0, precision), RR.fill_store(y, cl, 2, precision)
        res = [si.rows[:si.n_rows].clone(), sc.rows[:sc.n_rows].clone(), alignment_scores_from_stores(si, sc)]
        for d in ('i2t', 't2i'):
            res.append(alignment_scores_for_pairs(si, sc, cands[d], d))
            res.extend(alignment_map_for_pairs(si, sc, cands[d], d))
        out[name] = res
    assert out['base'][0].numel() > 0 and out['base'][0].dtype == torch.float16
    for name in ('again', 'scaled'):
        for n, (a, b) in enumerate(zip(out['base'], out[name])):
            assert a.dtype == b.dtype and torch.equal(RR.bits(a) if a.dtype == torch.float32 else a, RR.bits(b) if b.dtype == torch.float32 else b), \
                'packed stores: result %d of the %s stores differs from the base stores' % (n, name)
    fx, fy = RS.decade_row_scales(images.shape[:2], 63), RS.decade_row_scales(captions.shape[:2], 64)
    x10, y10 = RS.scale_rows_by(images, fx), RS.scale_rows_by(captions, fy)
    got = alignment_scores_from_stores(RR.fill_store(x10, il, 0, precision), RR.fill_store(y10, cl, 2, precision)).cpu().numpy()
    RR.assert_close(got, O.alignment_scores(x10, y10, il, cl, dtype=np.float64), precision, D)


# ------------------------------------------------------------------------------------------------
# the eps edge, forward only
# ------------------------------------------------------------------------------------------------
def test_rows_at_the_normalisation_eps():
    """Three scored rows with norms 2^-39, 2^-40 and 2^-41 straddle F.normalize's 1e-12: the reference divides the two short ones by
    the eps instead of their norm.  Scores: finite and the float64 oracle's, in both evaluation precisions and from the
    differentiable forward; gradients: finite (what the backward does for clamped rows is not judged here)."""
    from aladin_amd import ops
    import test_gpu_parity as G
    shape = RS.TILE_SHAPES[0]
    c = RS.alignment_case(shape)
    im, s = np.array(c.im), np.array(c.s)
    rows = ((im, 0, 3, -39), (s, 0, 2, -40), (im, 1, 1, -41))              # in range for their samples; (1, 1) is what the tile filling copies
    assert c.il[0] > 3 and c.sl[0] - 2 > 2 and c.il[1] > 1
    for x, b, p, e in rows:
        x[b, p] = (x[b, p].astype(np.float64) * (2.0 ** e / np.linalg.norm(x[b, p].astype(np.float64)))).astype(np.float32)
        n = float(np.linalg.norm(x[b, p].astype(np.float64)))
        assert abs(n / 2.0 ** e - 1) < 1e-6 and (n > 1e-12) == (e == -39)
    ref = O.alignment_scores(im, s, c.il, c.sl, dtype=np.float64)
    for precision in ('fp16', 'split'):
        check_scores(scores_no_grad(im, s, c.il, c.sl, 'MrSw', precision)[0], ref, precision)
    for mode in ('exact', 'fp16', 'fp16-own'):
        old = ops.set_backward_precision(mode)
        try:
            S, gi, gs = scores_with_grad(im, s, c.il, c.sl, c.w, 'MrSw')
        finally:
            ops.set_backward_precision(old)
        G.assert_scores_close(S, ref)
        assert np.isfinite(gi).all() and np.isfinite(gs).all()
