"""CPU tier: the expectations of the row-norm contract tests (tests/test_row_norms_gpu.py) hold for the REFERENCE's restatements
alone, before any kernel is involved -- the float64 oracle's scores do not move when rows are multiplied by powers of two, its
gradients (and the reference's dataflow under autograd, oracle/faithful_torch.py in double) scale by exactly 2^-k per row -- and
the adversarial positions of tests/helpers/row_scaling.py land on the packed rows its docstring names, for every geometry the
GPU tier runs.  The geometry comes from aladin_align_geometry itself (host code: no kernel is launched)."""
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

ALL_SHAPES = RS.TILE_SHAPES + [RS.FORWARD_ONLY_SHAPE] + RS.LONG_SHAPES
ids = lambda s: 'x'.join(map(str, s))    # noqa: E731


@pytest.mark.parametrize('shape', sorted(RS.EXPECTED_ROW_MAP), ids=ids)
def test_forced_positions_land_on_the_rows_they_are_meant_for(shape):
    """mrows / rem / trows of every shape are those of the class comment of aladin_align_geometry (RS.EXPECTED_ROW_MAP, copied
    out of it) and of the library itself; with them, the forced positions are the packed rows the helper's docstring names."""
    from aladin_amd import ops
    Bi, Bc, R, T, D = shape
    g = ops.align_geometry(Bi, Bc, R, T, D, layout='auto')
    assert (g.mrows, g.rem, g.trows) == RS.EXPECTED_ROW_MAP[shape]
    c = RS.alignment_case(shape, structured=Bi == Bc and Bi >= 8)
    assert (c.mrows, c.rem, c.trows) == RS.EXPECTED_ROW_MAP[shape] and (c.Rq, c.Tq) == (R - 1, T - 3)
    # lengths: full, one short, exactly the main tile (where the set is long enough for that to differ)
    assert c.il[0] == R and c.il[1] == R - 1 and c.sl[0] == T and c.sl[1] == T - 1
    if Bi > 2 and c.mrows + 1 <= R:
        assert c.il[2] - 1 == c.mrows
    if Bc > 2 and 19 <= T:
        assert c.sl[2] - 3 == 16
    fx, fy = c.forced_x, c.forced_y
    for (b, p), e in fx.items():                            # every forced exponent is in the draw the cases use
        assert c.kx[b, p] == e
    for (b, p), e in fy.items():
        assert c.ky[b, p] == e
    # position p is scored region p - 1; a region below mrows is main row p - 1 of its image, region mrows + q side row q
    last_main = min(c.mrows, c.Rq)                          # position of main row mrows - 1 (with tile-filling copies: of the last scored region)
    assert c.rem == max(c.Rq - c.mrows, 0) and (c.rem > 0) == (c.mrows + 1 <= c.Rq)
    for b in range(Bi):
        assert fx[(b, 1)] == RS.KMAX                        # main row 0, what rows Rq .. mrows - 1 copy
        assert fx[(b, last_main)] == RS.KMIN
        if c.rem:
            assert fx[(b, c.mrows + 1)] == RS.K_SIDE        # region mrows: side row 0, slot xe_row0 + b * rem
            assert c.kx[b, c.mrows] == RS.KMIN              # ... right after the last main row at the other end of the range
    # first and last scored position of the last image: far apart (KMIN, unless the last position is side row 0, which keeps K_SIDE)
    assert c.kx[Bi - 1, 1] == RS.KMAX and c.kx[Bi - 1, c.il[Bi - 1] - 1] == (RS.K_SIDE if c.il[Bi - 1] - 1 == c.mrows + 1 and c.rem else RS.KMIN)
    if c.half_tiles:
        # caption 0's last word and caption 1's first word: rows Tq - 1 and trows of y, inside ONE 16-row tile
        assert c.trows in (8, 24, 40) and c.sl[0] - 3 == c.Tq
        assert fy[(0, c.Tq)] == RS.KMAX and fy[(1, 1)] == RS.KMIN
        assert (c.Tq - 1) // 16 == (c.trows + 0) // 16
    else:
        assert c.trows % 16 == 0
    b = Bc - 1
    assert c.ky[b, 1] == (RS.KMIN if (c.half_tiles and b == 1) else RS.KMAX) and c.ky[b, c.sl[b] - 3] in (RS.KMIN, RS.KMAX)
    assert c.ky[b, 1] != c.ky[b, c.sl[b] - 3] or c.sl[b] - 3 == 1
    # the draw really spreads the norms: both signs of the exponent on both sides, scaled inputs differ from the base
    assert c.kx.min() == RS.KMIN and c.kx.max() == RS.KMAX and c.ky.min() == RS.KMIN and c.ky.max() == RS.KMAX
    assert not np.array_equal(c.im2, c.im) and not np.array_equal(c.s2, c.s)


def test_the_helpers_bounds_reject_what_would_not_be_exact():
    x = np.ones((1, 2, 64), np.float32)
    RS.assert_pow2_scaling_is_exact(x, np.array([[30, -30]]))
    with pytest.raises(AssertionError):
        RS.assert_pow2_scaling_is_exact(x * np.float32(2.0 ** -40), np.array([[0, -30]]))       # a component below 2^-30
    with pytest.raises(AssertionError):
        RS.assert_pow2_scaling_is_exact(x, np.array([[31, 0]]))
    with pytest.raises(AssertionError):
        RS.assert_grad_unscaling_is_exact(np.array([1.0, 2.0 ** -120]))
    RS.assert_grad_unscaling_is_exact(np.array([0.0, 2.0 ** -60]))
    g = np.array([[[3.0, -5.0]]], np.float32)
    k = np.array([[7]])
    assert np.array_equal(RS.unscale_grad(RS.scale_rows(g, -k), k), g)
    f = RS.decade_row_scales((4, 50), 3)
    assert f.min() >= 1e-3 and f.max() <= 1e3 and f.min() < 1e-2 and f.max() > 1e2


@pytest.mark.parametrize('shape', ALL_SHAPES, ids=ids)
def test_oracle_scores_do_not_move_under_power_of_two_row_scales(shape):
    """alad_oracle.alignment_scores in float64, every pooling it restates, and the scan-sentences restatement."""
    c = RS.alignment_case(shape)
    for mode in ('MrSw', 'MrAVGw', 'MwSr', 'symm', 'sum', 'mean'):
        base = O.alignment_scores(c.im, c.s, c.il, c.sl, mode, dtype=np.float64)
        scaled = O.alignment_scores(c.im2, c.s2, c.il, c.sl, mode, dtype=np.float64)
        np.testing.assert_allclose(scaled, base, rtol=0, atol=1e-12, err_msg=mode)
        assert np.isfinite(base).all() and np.abs(base).max() > 0
    if shape[4] <= 128:
        np.testing.assert_allclose(O.scan_sentences_scores(c.im2, c.s2, c.il, c.sl), O.scan_sentences_scores(c.im, c.s, c.il, c.sl),
                                   rtol=0, atol=1e-12)


def _faithful_grads(im, s, il, sl, mode, w):
    a, b = torch.from_numpy(np.array(im)).double().requires_grad_(True), torch.from_numpy(np.array(s)).double().requires_grad_(True)
    S = FT.alignment_scores_faithful(a, b, il, sl, mode)
    (S * torch.from_numpy(np.array(w)).double()).sum().backward()
    return S.detach().numpy(), a.grad.numpy(), b.grad.numpy()


# every pooling on the shapes the GPU tier runs it on: 'MrSw' everywhere, the others on the first two shapes
GRAD_CASES = [(shape, 'MrSw') for shape in RS.TILE_SHAPES + RS.LONG_SHAPES] + \
    [(shape, mode) for shape in RS.TILE_SHAPES[:2] for mode in ('MwSr', 'symm', 'sum', 'mean', 'scan-sentences')]


@pytest.mark.parametrize('shape,mode', GRAD_CASES, ids=lambda v: v if isinstance(v, str) else ids(v))
def test_reference_gradients_scale_by_the_inverse_row_factor(shape, mode):
    """The reference's dataflow under autograd, in double: unscale_grad maps the scaled rows' gradients back to the unscaled ones
    (rtol 1e-10), dropped and padded positions get exactly 0 on both, and the scores agree to 1e-12."""
    c = RS.alignment_case(shape)
    S0, gi0, gs0 = _faithful_grads(c.im, c.s, c.il, c.sl, mode, c.w)
    S1, gi1, gs1 = _faithful_grads(c.im2, c.s2, c.il, c.sl, mode, c.w)
    np.testing.assert_allclose(S1, S0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(RS.unscale_grad(gi1, c.kx), gi0, rtol=1e-10, atol=0)
    np.testing.assert_allclose(RS.unscale_grad(gs1, c.ky), gs0, rtol=1e-10, atol=0)
    assert np.abs(gi0).max() > 0 and np.abs(gs0).max() > 0
    for g in (gi0, gi1):
        assert not g[:, 0].any() and all(not g[i, L:].any() for i, L in enumerate(c.il))
    for g in (gs0, gs1):
        assert not g[:, 0].any() and all(not g[j, max(L - 2, 1):].any() for j, L in enumerate(c.sl))
    # a row 2^30 times longer really has a gradient 2^30 times smaller: a whole-tensor tolerance would not see it
    i, p = 0, 1
    assert c.kx[i, p] == RS.KMAX and (np.abs(gi1[i, p]).max() == np.abs(gi0[i, p]).max() * 2.0 ** -30)


@pytest.mark.parametrize('shape', RS.TILE_SHAPES[:3] + RS.LONG_SHAPES[:1] + [(10, 10, 51, 38, 128)], ids=ids)
def test_oracle_backward_scales_by_the_inverse_row_factor(shape):
    """alad_oracle.alignment_scores_backward (what the GPU tier holds the triplet and small-batch gradients to) and the gradients
    of the scan-sentences restatement."""
    c = RS.alignment_case(shape, structured=shape[0] == shape[1])
    gi0, gs0 = O.alignment_scores_backward(c.im, c.s, c.il, c.sl, c.w)
    gi1, gs1 = O.alignment_scores_backward(c.im2, c.s2, c.il, c.sl, c.w)
    np.testing.assert_allclose(RS.unscale_grad(gi1, c.kx), gi0, rtol=1e-10, atol=0)
    np.testing.assert_allclose(RS.unscale_grad(gs1, c.ky), gs0, rtol=1e-10, atol=0)
    assert np.abs(gi0).max() > 0 and np.abs(gs0).max() > 0
    if shape in RS.TILE_SHAPES[:2]:
        _, di0, ds0 = O.scan_sentences_scores(c.im, c.s, c.il, c.sl, dS=c.w)
        _, di1, ds1 = O.scan_sentences_scores(c.im2, c.s2, c.il, c.sl, dS=c.w)
        np.testing.assert_allclose(RS.unscale_grad(di1, c.kx), di0, rtol=1e-10, atol=0)
        np.testing.assert_allclose(RS.unscale_grad(ds1, c.ky), ds0, rtol=1e-10, atol=0)


@pytest.mark.parametrize('shape', RS.TILE_SHAPES[:2], ids=ids)
def test_row_norm_weighted_gradients_do_not_depend_on_the_row_factors(shape):
    """What the GPU tier's oracle check judges: gradient rows multiplied by their row's input norm.  On the power-of-two scaling
    that quantity is the unscaled problem's, to 1e-10 of its largest entry -- the 1 / |row| factor is gone and every row weighs
    in at its own size."""
    c = RS.alignment_case(shape)
    _, gi0, gs0 = _faithful_grads(c.im, c.s, c.il, c.sl, 'MrSw', c.w)
    _, gi1, gs1 = _faithful_grads(c.im2, c.s2, c.il, c.sl, 'MrSw', c.w)
    for g0, x0, g1, x1 in ((gi0, c.im, gi1, c.im2), (gs0, c.s, gs1, c.s2)):
        n0, n1 = g0 * RS.row_norms(x0), g1 * RS.row_norms(x1)
        np.testing.assert_allclose(n1, n0, rtol=0, atol=1e-10 * np.abs(n0).max())
        rowmax = np.abs(g1).max(-1)
        assert rowmax.max() > 1e6 * rowmax[rowmax > 0].min()          # the raw gradient rows differ by orders of magnitude
