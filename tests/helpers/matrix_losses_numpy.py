"""Inputs and numpy references of the score-matrix tier's tests (tests/test_matrix_losses_cpu.py, tests/test_matrix_losses_gpu.py):
the VSE++ hinge and ListNet (csrc/losses.hip, matrix_losses.hpp), the strided fp32 GEMM behind dot_scores (sgemm_tile.hpp), l2norm
(csrc/pool.hip) and the B <= 64 fused heads (csrc/small_batch.hip).

Both tiers build every input HERE, from (kind, shape) alone, so that what the CPU tier proves about an input (exactness in fp32,
exact ties, the float32 noise floor of ListNet) holds for the very array the GPU tier feeds the kernels.

References: oracle/alad_oracle.py (hinge_loss, listnet_loss, dot_scores) and float64 numpy.  The float32 restatements below
(listnet_f32, small_heads_f32) follow the kernels' formulas term by term in numpy float32; they are NOT references:
their own distance from float64 is the measured floor from which the cancelling gradients' absolute gate is derived
(LISTNET_A = 4 x a family's worst floor, asserted by the CPU tier)."""
import zlib

import numpy as np

# ------------------------------------------------------------------------------------------------
# case lists
# ------------------------------------------------------------------------------------------------
HINGE_BS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 2049)        # 2049: past the 2048-block clamp of hinge_finish_kernel
HINGE_VIEW_BS = (65, 257)
HINGE_PAIR_BS = (63, 257, 513)
HINGE_NAN_BS = (5, 257)
HINGE_MARGIN_Q = 0.25                                          # with the quantised scores: every cost exact in fp32
HINGE_MARGIN_N = 0.2                                           # with the standard-normal scores
HINGE_LOSS_RTOL = 1e-5

LISTNET_BS = (1, 2, 63, 257, 1500)                             # 1500: past the finish kernel's clamp (B >= 1449)
LISTNET_FAMILIES = ('mild', 'extreme')
LISTNET_VIEW_B = 63
LISTNET_TAU = 6.0
LISTNET_EPS = 1e-10
LISTNET_LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
LISTNET_GRAD_RTOL = 1e-4
# worst max|float32 restatement - float64| / max|float64| of the cancelling gradients per input family, measured by
# tests/test_matrix_losses_cpu.py::test_listnet_floor_is_within_its_recorded_value (it prints the figure of every input):
#   mild     5.05e-7 (ListNet B = 1500; the small-batch heads, whose teacher is this family's, reach 4.9e-7)  recorded as 5.5e-7
#   extreme  2.98e-6 (ListNet B = 2: tau * M ~ 100 carries an absolute rounding of 4e-6 into the exponent)     recorded as 3.2e-6
# The gate's absolute term is 4 x the family's floor: the device's expf / logf are a few ulp looser than numpy's and its sums run
# in another order.
LISTNET_FLOOR = {'mild': 5.5e-7, 'extreme': 3.2e-6}
LISTNET_A = {fam: 4 * v for fam, v in LISTNET_FLOOR.items()}

GEMM_SHAPES = ((1, 1, 1), (1, 70, 33), (70, 1, 33), (63, 65, 31), (64, 64, 32), (65, 129, 33), (33, 40, 127), (33, 40, 128),
               (33, 40, 129), (129, 63, 160), (70, 66, 257), (20, 24, 3000))
GEMM_VIEW_SHAPES = ((65, 129, 33), (33, 40, 129))
GEMM_LAYOUTS = ('nn', 'nt', 'tn', 'tt')                        # im, s: 'n' row-major (rows, K); 't' the .t() of a (K, rows) buffer
U32 = 2.0 ** -24                                               # unit roundoff of float32

L2NORM_SHAPES = ((1, 1), (1, 200), (5, 63), (5, 64), (5, 65), (9, 1000), (6, 3000), (257, 8))
L2NORM_FWD_TOL = dict(rtol=2e-6, atol=1e-7)
L2NORM_BWD_RTOL, L2NORM_BWD_ATOL = 1e-4, 1e-6                  # atol x max(1, max|ref|)

SMALL_BS = (1, 2, 63, 64)
SMALL_DS = (8, 30, 100)                                        # 30: no multiple of 4, the kernels' scalar loads
SMALL_G_HINGE, SMALL_G_LISTNET = 1.5, 0.75                     # upstream gradients of the two small-batch loss terms


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------
# hinge
# ------------------------------------------------------------------------------------------------
def hinge_scores(B, kind):
    """(S float32 (B, B), margin).  'quantised': multiples of 1/16 in [-4, 4] with margin 0.25 -- margin + s - diag is exact in fp32
    and in float64, so the oracle's dS is the same in both and exact ties are plentiful;  'normal': standard normal, margin 0.2."""
    rng = _rng('hinge', B, kind)
    if kind == 'quantised':
        return (rng.integers(-64, 65, (B, B)) / 16).astype(np.float32), HINGE_MARGIN_Q
    assert kind == 'normal'
    return rng.standard_normal((B, B)).astype(np.float32), HINGE_MARGIN_N


def hinge_tied_rows(S, margin):
    """number of rows whose hardest negative (largest positive off-diagonal cost) is attained at more than one column"""
    S = np.asarray(S, np.float64)
    c = np.clip(margin + S - np.diag(S)[:, None], 0, None)
    np.fill_diagonal(c, 0)
    top = c.max(1, keepdims=True)
    return int(((top[:, 0] > 0) & ((c == top).sum(1) > 1)).sum())


def hinge_nonfinite(B, where):
    """quantised scores with one non-finite entry -> (S, margin, rows_clean, cols_clean): the boolean row / column masks of the lines
    none of whose costs is touched.  where: 'nan_off' (1, 3) | 'nan_diag' (2, 2) | 'inf_off' (1, 3)"""
    S, margin = hinge_scores(B, 'quantised')
    S = S.copy()
    i, j, v = {'nan_off': (1, 3, np.nan), 'nan_diag': (2, 2, np.nan), 'inf_off': (1, 3, np.inf)}[where]
    S[i, j] = v
    rows, cols = np.ones(B, bool), np.ones(B, bool)
    rows[i] = False
    cols[j] = False
    return S, margin, rows, cols


# ------------------------------------------------------------------------------------------------
# ListNet
# ------------------------------------------------------------------------------------------------
def listnet_inputs(B, family):
    """(teacher, student) float32 (B, B).  'mild': 2 N + 3 and clip(0.3 N, -1, 1) (tests/fuzz/fuzz_losses.py);  'extreme': 40 N and
    10 N -- tau * student spans +-hundreds: the softmax must be max-shifted, most Q underflow and log(Q + eps) sits at log(1e-10)."""
    rng = _rng('listnet', B, family)
    if family == 'mild':
        return (rng.standard_normal((B, B)) * 2 + 3).astype(np.float32), np.clip(rng.standard_normal((B, B)) * 0.3, -1, 1).astype(np.float32)
    assert family == 'extreme'
    return (40 * rng.standard_normal((B, B))).astype(np.float32), (10 * rng.standard_normal((B, B))).astype(np.float32)


def listnet_f32(T, M, tau=LISTNET_TAU, eps=LISTNET_EPS):
    """(loss, dM) of ListNet by the kernels' formulas (csrc/losses.hip) in numpy float32 throughout:
    P = softmax(T), Q = softmax(tau M) max-shifted, term = -sum P log(Q + eps), W = P Q / (Q + eps),
    dM = (tau / B) [Q^r Wsum^r - W^r + Q^c Wsum^c - W^c], loss = mean of the column terms + mean of the row terms."""
    f = np.float32
    T, M = np.asarray(T, f), np.asarray(M, f)
    B = M.shape[0]
    tau, eps = f(tau), f(eps)
    m = tau * M
    loss = f(0)
    dM = np.zeros((B, B), f)
    with np.errstate(under='ignore'):
        for axis in (0, 1):                                       # columns, then rows: the order the kernel adds the two means in
            te = np.exp(T - T.max(axis=axis, keepdims=True))
            se = np.exp(m - m.max(axis=axis, keepdims=True))
            P = te / te.sum(axis=axis, keepdims=True, dtype=f)
            Q = se / se.sum(axis=axis, keepdims=True, dtype=f)
            loss = loss + (-(P * np.log(Q + eps))).sum(axis=axis, dtype=f).sum(dtype=f) / f(B)
            W = P * Q / (Q + eps)
            dM += Q * W.sum(axis=axis, keepdims=True, dtype=f) - W
    return f(loss), (tau / f(B)) * dM


def floor_ratio(got, ref):
    """max|got - ref| / max|ref| (0 where the reference is identically zero and got is too)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    err = np.abs(got - ref).max()
    if top == 0.0:
        assert err == 0.0
        return 0.0
    return float(err / top)


def assert_cancelling_grad_close(got, ref64, what='', family='mild'):
    """the gate of the gradients that cancel (dM ~ (tau / B)(Q - P)): |got - ref| <= rtol |ref| + LISTNET_A[family] max|ref|"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert np.isfinite(got).all(), what
    tol = LISTNET_GRAD_RTOL * np.abs(ref64) + LISTNET_A[family] * np.abs(ref64).max()
    bad = np.abs(got - ref64) > tol
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(got - ref64).max()), float(np.abs(ref64).max()))


# ------------------------------------------------------------------------------------------------
# GEMM (dot_scores and its two backward products)
# ------------------------------------------------------------------------------------------------
def gemm_inputs(M, N, K, kind):
    """(A (M, K), B (N, K), W (M, N)) float32; C = A B^T, d_im = W B, d_s = W^T A.  'integer': integers in [-8, 8] -- every partial
    sum of every one of the three products stays below 2^24, so the float64 product is the fp32 result whatever the summation
    order;  'normal': standard normal."""
    rng = _rng('gemm', M, N, K, kind)
    if kind == 'integer':
        draw = lambda shape: rng.integers(-8, 9, shape).astype(np.float32)
    else:
        assert kind == 'normal'
        draw = lambda shape: rng.standard_normal(shape).astype(np.float32)
    return draw((M, K)), draw((N, K)), draw((M, N))


def gemm_refs(A, B, W):
    """float64 (C, d_im, d_s) and the elementwise error bounds of a float32 evaluation in any order: k u (|X| |Y|), k the
    contraction length of each product"""
    A, B, W = (np.asarray(x, np.float64) for x in (A, B, W))
    K, N, M = A.shape[1], B.shape[0], A.shape[0]
    refs = (A @ B.T, W @ B, W.T @ A)
    bounds = (K * U32 * (np.abs(A) @ np.abs(B).T), N * U32 * (np.abs(W) @ np.abs(B)), M * U32 * (np.abs(W).T @ np.abs(A)))
    return refs, bounds


def fp32_sums_exact(X, Y):
    """True when sum_k |X[i, k] Y[k, j]| < 2^24 for integer-valued X, Y: every partial sum, in any order, is an integer below
    2^24 in magnitude and therefore a float32"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    return bool((X == np.round(X)).all() and (Y == np.round(Y)).all() and (np.abs(X) @ np.abs(Y)).max() < 2.0 ** 24)


# ------------------------------------------------------------------------------------------------
# l2norm
# ------------------------------------------------------------------------------------------------
def l2norm_inputs(rows, D, zero_row=None):
    """(x, upstream gradient) float32 (rows, D); zero_row: that row of x is all zero (NaN in the reference, forward and backward)"""
    rng = _rng('l2norm', rows, D)
    x = rng.standard_normal((rows, D)).astype(np.float32)
    g = rng.standard_normal((rows, D)).astype(np.float32)
    if zero_row is not None:
        x[zero_row] = 0
    return x, g


def l2norm_ref(x, g):
    """float64 (out, dx) of x / sqrt(sum x^2) (no eps): dx = (g - n <n, g>) / ||x||"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        nrm = np.sqrt((x * x).sum(1, keepdims=True))
        n = x / nrm
        return n, (g - n * (n * g).sum(1, keepdims=True)) / nrm


def l2norm_bwd_tol(ref):
    """the absolute + relative gate of the l2norm backward on a finite float64 reference"""
    ref = np.asarray(ref, np.float64)
    return L2NORM_BWD_RTOL * np.abs(ref) + L2NORM_BWD_ATOL * max(1.0, float(np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------
# small-batch fused heads
# ------------------------------------------------------------------------------------------------
def small_batch_inputs(B, D):
    """(img, cap (B, D), teacher (B, B)) float32.  Embeddings are multiples of 1/16 in [-1/4, 1/4]: M = img cap^T is a sum of
    multiples of 1/256 far below 2^16, exact in fp32 in any order, and margin 0.25 + M - diag is exact too (hinge dM bit-equal to
    the oracle's, ties included); the teacher is the mild ListNet family's."""
    rng = _rng('small', B, D)
    img = (rng.integers(-4, 5, (B, D)) / 16).astype(np.float32)
    cap = (rng.integers(-4, 5, (B, D)) / 16).astype(np.float32)
    teacher = (rng.standard_normal((B, B)) * 2 + 3).astype(np.float32)
    return img, cap, teacher


def small_heads_f32(img, cap, teacher, dMh):
    """float32 restatement of the small-batch backward: coef = g_h dM_hinge + g_l dM_listnet, d_img = coef cap, d_cap = coef^T img"""
    f = np.float32
    M = (np.asarray(img, np.float64) @ np.asarray(cap, np.float64).T).astype(f)
    _, dMl = listnet_f32(teacher, M)
    coef = f(SMALL_G_HINGE) * np.asarray(dMh, f) + f(SMALL_G_LISTNET) * dMl
    return coef @ np.asarray(cap, f), coef.T @ np.asarray(img, f)
