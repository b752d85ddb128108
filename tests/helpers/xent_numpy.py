"""Numpy restatements of the symmetric cross-entropy (InfoNCE) criterion that aladin_xent_fwd_bwd computes (include/aladin_hip.h;
reference alad/loss.py:190-201, CrossEntropyCriterion), and the inputs of its tests.

    S = im s^T,  L = S e^t,  loss = 1/(2B) [ sum_i (LSE_j L_ij - L_ii) + sum_j (LSE_i L_ij - L_jj) ]
    dL = (P^r + P^c - 2 I) / (2B),  dS = e^t dL,  dt = sum_ij dL_ij L_ij,  d_im = dS s,  d_s = dS^T im

xent_f64 / criterion_f64 are the float64 REFERENCES (tests/test_xent_cpu.py pins them to the reference's recorded float64 run,
tests/golden/xent.npz).  xent_f32 / criterion_f32 follow the same formulas in plain numpy float32; they are NOT references: their
own distance from float64 is the measured floor from which the gradients' absolute gate is derived (XENT_A = 4 x a family's
floor, the rule of matrix_losses_numpy.LISTNET_A).

Both tiers build every input HERE, so that what the CPU tier measures holds for the very arrays the GPU tier feeds the kernels."""
import numpy as np

LN100 = float(np.float32(np.log(100.0)))             # the float32 the modules' parameter holds, widened

# ------------------------------------------------------------------------------------------------
# the fixture tests/golden/xent.npz (make_golden_xent.py): embeddings through CrossEntropyCriterion
# ------------------------------------------------------------------------------------------------
SHAPES = [(1, 8), (2, 8), (5, 30), (33, 64), (65, 768)]       # D = 30: no multiple of 4; B = 65: more than one wave and one strip
TEMPERATURES = (0.0, 1.5, LN100)
FIXTURE_FAMILIES = ('matched', 'independent')
SEED_MATCHED, SEED_INDEPENDENT = 151, (161, 261)
MATCHED_NOISE = 2.0                  # matched cosines ~0.2: at t = ln 100 a diagonal ~20 above off-diagonals of spread ~100 / sqrt(D)
# The reference forms the diagonal of its gradient as softmax - 1, which float64 rounds at 1e-16 ABSOLUTE whatever is left of it.
# The recorded gradients are good to 1e-16 / (the largest off-diagonal softmax mass of any line) of their largest entry; every
# fixture case with B > 1 keeps that mass above MIN_TOP_MASS (asserted by the generator and the CPU tier), i.e. 1e-13.
MIN_TOP_MASS = 1e-3
GRAD_COLUMN_STEP = 4                 # cases with B * D > GRAD_FULL_MAX record every 4th gradient column (make_golden_entropy.py's rule)
GRAD_FULL_MAX = 4096
MODEL_MAX_B = 33                     # cases up to this B also record the model's weighted totals and their gradients
MODEL_LOSS_TYPE, MODEL_WEIGHTS = 'matching-crossentropy', [1.0, 0.5]

# ------------------------------------------------------------------------------------------------
# the matrix-level tests: ops.cross_entropy_scores on a score matrix
# ------------------------------------------------------------------------------------------------
# 63 / 64 / 65: the wave and the 64-column strip; 257: the finish kernel's 256-column chunk and the stats kernel's 16-wave row
# stride several times over; 1500: past the finish kernel's clamp of about 2048 workgroups (6 column chunks x 341 row groups: the
# rows are dealt to the groups with a stride) and the four-rows-in-flight loop of the column strips.
SIZES = (1, 2, 63, 64, 65, 257, 1500)
FAMILIES = ('mild', 'sharp', 'scaled')
LOSS_TOL = dict(rtol=1e-5, atol=1e-6)                # loss and dt: the values ListNet uses (LISTNET_LOSS_TOL)
GRAD_RTOL = 1e-4

# worst max|float32 restatement - float64| / max|float64| of the gradients per input family, measured by
# tests/test_xent_cpu.py::test_float32_floor_is_within_its_recorded_value (it prints the figure of every input):
#   mild         dS  1.96e-7 (B = 63)                                                                          recorded as 2.2e-7
#   sharp        dS  3.78e-6 (B = 2: L ~ 64 carries an absolute rounding of 4e-6 into the exponent; 4.4e-7 elsewhere)  recorded as 4.2e-6
#   scaled       dS  1.79e-7 (B = 1500)                                                                        recorded as 2.0e-7
#   matched      d im / d s  6.69e-6 ((65, 768) at t = ln 100: the float32 products' rounding times e^t in the exponent;
#                            below 6e-7 in every other case)                                                   recorded as 7.4e-6
#   independent  d im / d s  8.90e-7 ((65, 768) at t = ln 100)                                                 recorded as 1.0e-6
# The gate's absolute term is 4 x the family's floor: the device's expf / logf are a few ulp looser than numpy's and its sums
# (the products' too) run in another order.
XENT_FLOOR = {'mild': 2.2e-7, 'sharp': 4.2e-6, 'scaled': 2.0e-7, 'matched': 7.4e-6, 'independent': 1.0e-6}
XENT_A = {fam: 4 * v for fam, v in XENT_FLOOR.items()}


def case_inputs(family, B, D, seed, seed2=0):
    """(img, cap) float32 unit-norm rows of a fixture case.  'matched': the pairs of one synth.global_embeddings draw (a sharp
    diagonal);  'independent': the image half of the draw `seed`, the caption half of the independent draw `seed2`."""
    from aladin_amd import synth
    if family == 'independent':
        return synth.global_embeddings(B, D, seed, 1.0)[0], synth.global_embeddings(B, D, seed2, 1.0)[1]
    assert family == 'matched'
    return synth.global_embeddings(B, D, seed, MATCHED_NOISE)


def fixture_cases():
    """[(family, B, D, t, seed, seed2)] in the fixture's order"""
    out = []
    for B, D in SHAPES:
        for t in TEMPERATURES:
            out.append(('matched', B, D, t, SEED_MATCHED, 0))
            out.append(('independent', B, D, t) + SEED_INDEPENDENT)
    return out


def grad_columns(B, D):
    """the gradient columns a fixture case records"""
    return slice(None, None, GRAD_COLUMN_STEP if B * D > GRAD_FULL_MAX else 1)


def matrix_inputs(B, family):
    """(S float32 (B, B), t).  'mild': cosines of independent unit vectors, t = 0;  'sharp': cosines of matched pairs
    (diagonal ~0.64, the rest ~N(0, 1/8)) at t = ln 100 -- both softmaxes near one-hot, most of them saturated in float32;
    'scaled': uniform in [0, 47] like MrSw scores of 50-token captions, t = 0."""
    from aladin_amd import synth
    if family == 'mild':
        img = synth.global_embeddings(B, 32, 171, 1.0)[0]
        cap = synth.global_embeddings(B, 32, 271, 1.0)[1]
        return (img.astype(np.float64) @ cap.astype(np.float64).T).astype(np.float32), 0.0
    if family == 'sharp':
        img, cap = synth.global_embeddings(B, 64, 181, 0.75)
        return (img.astype(np.float64) @ cap.astype(np.float64).T).astype(np.float32), LN100
    assert family == 'scaled'
    return (47.0 * synth.uniform((B, B), 191)).astype(np.float32), 0.0


# ------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------
def _lse(L, axis):
    m = L.max(axis=axis, keepdims=True)
    return m + np.log(np.exp(L - m).sum(axis=axis, keepdims=True))


def offdiag_mass(S, t):
    """per line (rows, then columns) the softmax mass off the diagonal, float64 (2B,)"""
    L = np.asarray(S, np.float64) * np.exp(np.float64(t))
    off = ~np.eye(len(L), dtype=bool)
    out = []
    for axis in (1, 0):
        E = np.exp(L - L.max(axis=axis, keepdims=True))
        out.append((E * off).sum(axis=axis) / E.sum(axis=axis))
    return np.concatenate(out)


def xent_f64(S, t, g=1.0):
    """-> (loss, dS, dt) in float64 for the upstream gradient g; NaN in, NaN out"""
    S = np.asarray(S, np.float64)
    B = S.shape[0]
    assert S.shape == (B, B)
    L = S * np.exp(np.float64(t))
    with np.errstate(invalid='ignore', under='ignore'):
        lr, lc = _lse(L, 1), _lse(L, 0)
        d = np.diag(L)
        loss = ((lr[:, 0] - d).sum() + (lc[0] - d).sum()) / (2 * B)
        dL = (np.exp(L - lr) + np.exp(L - lc) - 2 * np.eye(B)) / (2 * B)
        # P^r_ii - 1 and P^c_ii - 1 without the cancellation: minus the line's off-diagonal mass
        off = ~np.eye(B, dtype=bool)
        dL[np.diag_indices(B)] = -((np.exp(L - lr) * off).sum(1) + (np.exp(L - lc) * off).sum(0)) / (2 * B)
        # the separable form of dt: per line, sum P (L - L_dd); it does not cancel where the softmaxes are one-hot
        dt = ((np.exp(L - lr) * (L - d[:, None])).sum() + (np.exp(L - lc) * (L - d[None, :])).sum()) / (2 * B)
    return float(loss), g * np.exp(np.float64(t)) * dL, float(g * dt)


def criterion_f64(im, s, t, g=1.0):
    """CrossEntropyCriterion from embeddings -> (loss, d_im, d_s, dt, S), float64"""
    im, s = np.asarray(im, np.float64), np.asarray(s, np.float64)
    S = im @ s.T
    loss, dS, dt = xent_f64(S, t, g)
    return loss, dS @ s, dS.T @ im, dt, S


# ------------------------------------------------------------------------------------------------
# plain float32 restatements (the measured floor)
# ------------------------------------------------------------------------------------------------
def xent_f32(S, t):
    """(loss, dS, dt) by the same formulas in numpy float32 throughout: per line the max-shifted exponentials E = e^(L - m), their
    sum s, P = E / s, the diagonal's P - 1 as -(off-diagonal sum of E) / s, LSE - L_dd = (m - L_dd) + log s and the line's share of
    dt as sum(E (L - m)) / s + (m - L_dd)."""
    f = np.float32
    S = np.asarray(S, f)
    B = S.shape[0]
    et = np.exp(f(t))
    L = S * et
    d = np.diag(L)
    off = ~np.eye(B, dtype=bool)
    inv = f(1) / (f(2) * f(B))
    g = np.zeros((B, B), f)
    loss = dt = f(0)
    with np.errstate(under='ignore'):
        for axis in (1, 0):                                          # rows, then columns
            m = L.max(axis=axis, keepdims=True)
            E = np.exp(L - m)
            s = E.sum(axis=axis, keepdims=True, dtype=f)
            P = E / s
            mass = (E * off).sum(axis=axis, keepdims=True, dtype=f)
            P[np.diag_indices(B)] = (-(mass / s)).ravel()
            g += P
            shift = m.ravel() - d
            loss = loss + (shift + np.log(s).ravel()).sum(dtype=f)
            dt = dt + ((E * (L - m)).sum(axis=axis, dtype=f) / s.ravel() + shift).sum(dtype=f)
    return f(loss * inv), (et * inv) * g, f(dt * inv)


def criterion_f32(im, s, t):
    """(loss, d_im, d_s, dt) from embeddings in numpy float32 throughout, products included"""
    f = np.float32
    im, s = np.asarray(im, f), np.asarray(s, f)
    loss, dS, dt = xent_f32(im @ s.T, t)
    return loss, dS @ s, dS.T @ im, dt


def floor_ratio(got, ref):
    """max|got - ref| / max|ref| (0 where the reference is identically zero and got is too)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    err = np.abs(got - ref).max()
    if top == 0.0:
        assert err == 0.0
        return 0.0
    return float(err / top)


def assert_grad_close(got, ref64, family, what=''):
    """the gate of the gradients: |got - ref| <= GRAD_RTOL |ref| + XENT_A[family] max|ref| (assert_cancelling_grad_close's rule)"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert np.isfinite(got).all(), what
    tol = GRAD_RTOL * np.abs(ref64) + XENT_A[family] * np.abs(ref64).max()
    bad = np.abs(got - ref64) > tol
    assert not bad.any(), (what, family, int(bad.sum()), float(np.abs(got - ref64).max()), float(np.abs(ref64).max()))
