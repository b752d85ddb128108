"""Inputs and numpy references of the secondary heads' tests (tests/test_secondary_heads_cpu.py, tests/test_secondary_heads_gpu.py):
aggregation='scan-sentences' (csrc/scan.hip), 'sum' / 'mean' (csrc/pool.hip normsum_*), DistillationLoss 'mse' / 'ordinal' /
'contrastive' and order_sim (csrc/distill.hip).

Both tiers build every input HERE, from its name alone, so that what the CPU tier proves about an input holds for the very array
the GPU tier feeds the kernels.

References: oracle/alad_oracle.py (scan_sentences_scores, distill_*, order_scores*) and the float64 restatements below where the
oracle has none (normsum, 'sum' / 'mean').  scan_eval, normsum, order_eval and contrastive_eval take a dtype: in float64 they
are pinned to the oracle by the CPU tier; in float32 they follow the kernels' formulas term by term and are NOT references --
their distance from float64 is the measured floor, and the GPU tier's gate is 4 x the worst floor of a family (the kernels sum
in another order and use the device's expf), recorded below with the measurement beside it."""
import zlib

import numpy as np

U32 = 2.0 ** -24                                               # unit roundoff of float32
F_EPS = 1e-12                                                  # F.normalize
COS_EPS = 1e-8                                                 # F.cosine_similarity


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def floor_ratio(got, ref):
    """max|got - ref| / max|ref| over the finite entries of ref; non-finite entries must agree in kind"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    if not fin.any():
        return 0.0
    top = np.abs(ref[fin]).max()
    err = np.abs(got[fin] - ref[fin]).max()
    if top == 0.0:
        assert err == 0.0
        return 0.0
    return float(err / top)


def row_ratio(got, ref):
    """the worst floor_ratio of a single row (last axis): what a zero vector's 1e8 times larger gradient cannot hide behind.
    A row whose reference is identically zero must be exactly zero."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return max(floor_ratio(g, r) for g, r in zip(got, ref))


# ------------------------------------------------------------------------------------------------
# scan-sentences
# ------------------------------------------------------------------------------------------------
# (Bi, Bc, R, T, D), full lengths: minimum size | one-row / one-column dS, Bi R' no multiple of 4 | T' = 65: the 64-lane word loops
# wrap, D < 32 | T'^2 > 256: more than one Gram accumulator per thread, R' above 4 waves x 16, D with a partial 32-slab
SCAN_SHAPES = ((1, 1, 2, 4, 1), (1, 5, 6, 20, 33), (5, 1, 6, 20, 33), (3, 2, 9, 68, 31), (2, 3, 70, 21, 100))
SCAN_MAX_SHAPE = (2, 2, 97, 99, 8)                             # R' = T' = 96, the bound of scan_check, forward and backward
SCAN_FAMILIES = ('shape', 'max', 'ragged', 'zero', 'opposite')
SCAN_RAGGED = (8, 8, 12, 16, 64)
SCAN_RAGGED_IM_LEN = [1, 2, 12, 15, 5, 12, 7, 3]               # 1: nothing scored; 2: one region; 15 > R: clamped
SCAN_RAGGED_S_LEN = [3, 4, 16, 20, 9, 16, 5, 10]               # 3: no word (NaN column); 4: one word; 20 > T: clamped
SCAN_ZERO = (3, 3, 6, 9, 16)                                   # region 2 of image 1 and word 3 of caption 2 are zero vectors
SCAN_ZERO_REGION, SCAN_ZERO_WORD = (1, 2), (2, 3)              # (sample, position in the raw set)
SCAN_OPPOSITE = (3, 2, 5, 8, 16)                               # word 2 of caption 1 is opposite to every region of image 0
SCAN_SCORE_TOL = dict(rtol=3e-5, atol=5e-6)                    # test_gpu_parity.test_scan_sentences_ragged_vs_oracle, kept
SCAN_GRAD_RTOL, SCAN_GRAD_ATOL = 2e-4, 1e-5                    # the same test: atol x max(1e-3, max|d_im|, max|d_s|), kept
# worst max|float32 restatement - float64| / max|float64| over every input above, measured by
# tests/test_secondary_heads_cpu.py::test_scan_floors_are_within_their_recorded_values (it prints the figure of every input):
#   scores     1.67e-7 at (2, 3, 70, 21, 100)                                                    recorded as 1.7e-7
#   grads      3.58e-7 at (3, 2, 9, 68, 31), the larger of d_im and d_s                          recorded as 3.6e-7
#   zero_rows  2.46e-7, the zero family's gradients PER ROW (row_ratio): each row against its own largest entry, so that
#              the zero region's 1e20 cannot hide the other rows                                 recorded as 2.5e-7
# Recorded: the measured floor rounded up in its last digit.  The gate is 4 x the recorded floor x max|reference| (of the row, in the zero family), held ON TOP of the test_gpu_parity
# tolerances above: whichever is tighter decides.
SCAN_FLOOR = {'scores': 1.7e-7, 'grads': 3.6e-7, 'zero_rows': 2.5e-7}
SCAN_GATE = {k: 4 * v for k, v in SCAN_FLOOR.items()}


def scan_inputs(family, shape=None):
    """(im (Bi, R, D), s (Bc, T, D), im_len, s_len, dS (Bi, Bc)) float32 / lists"""
    if family == 'shape':
        Bi, Bc, R, Tn, D = shape
    else:
        Bi, Bc, R, Tn, D = {'max': SCAN_MAX_SHAPE, 'ragged': SCAN_RAGGED, 'zero': SCAN_ZERO, 'opposite': SCAN_OPPOSITE}[family]
    rng = _rng('scan', family, Bi, Bc, R, Tn, D)
    im = rng.standard_normal((Bi, R, D)).astype(np.float32)
    s = rng.standard_normal((Bc, Tn, D)).astype(np.float32)
    w = rng.standard_normal((Bi, Bc)).astype(np.float32)
    il, sl = [R] * Bi, [Tn] * Bc
    if family == 'ragged':
        il, sl = list(SCAN_RAGGED_IM_LEN), list(SCAN_RAGGED_S_LEN)
    elif family == 'zero':
        im[SCAN_ZERO_REGION] = 0
        s[SCAN_ZERO_WORD] = 0
    elif family == 'opposite':
        base = rng.standard_normal(D).astype(np.float32)
        im[0] = base + 0.25 * im[0]                            # every region of image 0 within a narrow cone around base
        s[1, 2] = -base
    return im, s, il, sl, w


def scan_eval(im_set, s_seq, im_len, s_len, dS, dtype=np.float64, max_words=None, gram_features=None):
    """(S, d_im, d_s) of 'scan-sentences' by the formulas of oracle.scan_sentences_scores / csrc/scan.hip, every operation in `dtype`
    (float64: the oracle itself, which the CPU tier asserts; float32: the floor).  Also returns the valid cosines' smallest |A|.
    Slips: max_words -- words at or beyond that index are ignored;  gram_features -- the Gram matrix sees only the first so many
    features."""
    f = dtype
    im, s = np.asarray(im_set, f), np.asarray(s_seq, f)
    Bi, Bc = im.shape[0], s.shape[0]
    ni = np.sqrt((im * im).sum(-1, keepdims=True, dtype=f))
    ns = np.sqrt((s * s).sum(-1, keepdims=True, dtype=f))
    xn = (im / np.maximum(ni, f(F_EPS)))[:, 1:, :]
    yn = (s / np.maximum(ns, f(F_EPS)))[:, 1:-2, :]
    S = np.zeros((Bi, Bc), f)
    dxn, dyn = np.zeros_like(xn), np.zeros_like(yn)
    min_abs = np.inf
    for i in range(Bi):
        Li = min(max(int(im_len[i]) - 1, 0), xn.shape[1])
        for j in range(Bc):
            Lj = min(max(int(s_len[j]) - 3, 0), yn.shape[1])
            if max_words is not None:
                Lj = min(Lj, max_words)
            if Li == 0:
                continue
            if Lj == 0:
                S[i, j] = np.nan
                continue
            x, y = xn[i, :Li], yn[j, :Lj]
            A = x @ y.T
            live = np.abs(A)[np.ix_(np.abs(x).sum(1) > 0, np.abs(y).sum(1) > 0)]
            if live.size:
                min_abs = min(min_abs, float(live.min()))
            P = np.maximum(A, f(0))
            c = np.maximum(np.sqrt((P * P).sum(0, dtype=f)), f(1e-12))
            Nn = P / c
            E = np.exp(Nn - Nn.max(1, keepdims=True))
            W = E / E.sum(1, keepdims=True, dtype=f)
            yg = y if gram_features is None else y[:, :gram_features]
            G = yg @ yg.T
            u = (W * A).sum(1, dtype=f)
            t = W @ G
            q = (W * t).sum(1, dtype=f)
            n = np.sqrt(np.maximum(q, f(0)))
            a = np.maximum(np.sqrt((x * x).sum(1, dtype=f)), f(COS_EPS))
            a = np.where(a > f(0.5), f(1), a)                  # a unit vector's norm is 1 in the kernel (and 1 +- 1 ulp in the oracle)
            m = np.maximum(n, f(COS_EPS))
            cos = u / (a * m)
            S[i, j] = cos.sum(dtype=f)
            g = f(dS[i, j])
            if g == 0:
                continue
            k = np.where(n > f(COS_EPS), cos / (m * m), f(0))
            dW = g * (A / (a * m)[:, None] - k[:, None] * t)
            dZ = W * (dW - (W * dW).sum(1, keepdims=True, dtype=f))
            dot = (Nn * dZ).sum(0, dtype=f)
            dP = (dZ - Nn * dot) / c
            dA = g * W / (a * m)[:, None] + dP * (A > 0)
            Hm = g * (W * k[:, None]).T @ W
            dxn[i, :Li] += dA @ y
            dyn[j, :Lj] += dA.T @ x - Hm @ y
    with np.errstate(over='ignore'):
        d_im, d_s = np.zeros_like(im), np.zeros_like(s)
        d_im[:, 1:, :] = (dxn - xn * (xn * dxn).sum(-1, keepdims=True, dtype=f)) / np.maximum(ni[:, 1:, :], f(F_EPS))
        d_s[:, 1:-2, :] = (dyn - yn * (yn * dyn).sum(-1, keepdims=True, dtype=f)) / np.maximum(ns[:, 1:-2, :], f(F_EPS))
    return S, d_im, d_s, min_abs


# ------------------------------------------------------------------------------------------------
# 'sum' / 'mean': the masked sum of unit vectors
# ------------------------------------------------------------------------------------------------
NORMSUM_DS = (1, 63, 64, 65, 257)                              # the 64-lane loop and the 256-thread final sum wrap
NORMSUM_R, NORMSUM_T = 10, 12                                  # N - 1 - tail = 9 scored positions on either side
NORMSUM_L = (0, 1, 3, 4, 5, 9, 14, 2)                          # scored length of each sample (14: above N, clamped)
NORMSUM_ZERO = (4, 2)                                          # (sample, position) of a zero row inside the range, both sides
# worst distance of the float32 restatement from float64 over every D, both sides and the minimal sets, measured by
# tests/test_secondary_heads_cpu.py::test_normsum_floors_are_within_their_recorded_values:
#   out     1.14e-7 of the output's largest entry (rows without a scored position exactly 0)             recorded as 1.2e-7
#   grad    2.48e-7 of each row's scale max|g_b| / |x| (normsum_scales), alone and behind 'sum' scores    recorded as 2.5e-7
#   scores  2.31e-7 of the largest 'sum' score                                                          recorded as 2.4e-7
# (the measured floor rounded up in its last digit); gate = 4 x the recorded floor
NORMSUM_FLOOR = {'out': 1.2e-7, 'grad': 2.5e-7, 'scores': 2.4e-7}
NORMSUM_GATE = {k: 4 * v for k, v in NORMSUM_FLOOR.items()}


def normsum_inputs(D, minimal=False):
    """(im, s, im_len, s_len, dS).  minimal: N = 2 regions / 4 tokens, the smallest sets the entry point takes"""
    R, Tn = (2, 4) if minimal else (NORMSUM_R, NORMSUM_T)
    Ls = (1, 0, 3) if minimal else NORMSUM_L
    B = len(Ls)
    rng = _rng('normsum', D, minimal)
    im = rng.standard_normal((B, R, D)).astype(np.float32)
    s = rng.standard_normal((B, Tn, D)).astype(np.float32)
    w = rng.standard_normal((B, B)).astype(np.float32)
    if not minimal:
        im[NORMSUM_ZERO] = 0
        s[NORMSUM_ZERO] = 0
    return im, s, [L + 1 for L in Ls], [L + 3 for L in reversed(Ls)], w


def normsum(x, lens, tail, g=None, dtype=np.float64, count_len=False):
    """out[b] = sum_{p = 1 .. min(len - 1 - tail, N - 1 - tail)} x[b, p] / max(|x[b, p]|, 1e-12) and, with the upstream g (B, D), its
    gradient (g - n <n, g>) / max(|x|, 1e-12) on those positions, 0 elsewhere.  Slip: count_len -- positions 1 .. len are summed."""
    f = dtype
    x = np.asarray(x, f)
    B, N, D = x.shape
    nrm = np.maximum(np.sqrt((x * x).sum(-1, keepdims=True, dtype=f)), f(F_EPS))
    n = x / nrm
    out = np.zeros((B, D), f)
    dx = np.zeros_like(x)
    for b in range(B):
        L = int(lens[b]) if count_len else int(lens[b]) - 1 - tail
        L = min(max(L, 0), N - 1 - tail)
        out[b] = n[b, 1:1 + L].sum(0, dtype=f)
        if g is not None:
            gb = np.asarray(g, f)[b]
            with np.errstate(over='ignore'):
                dx[b, 1:1 + L] = (gb - n[b, 1:1 + L] * (n[b, 1:1 + L] * gb).sum(-1, keepdims=True, dtype=f)) / nrm[b, 1:1 + L]
    return (out, dx) if g is not None else out


def normsum_scales(x, lens, tail, g):
    """the natural size of each row's terms, against which a float32 evaluation's error is measured: the output row b is a sum of
    L_b unit vectors (scale L_b); the gradient row (b, p) is g_b / |x| minus its projection (scale max|g_b| / max(|x|, 1e-12)) --
    the two cancel entirely at D = 1, so the row's own largest entry is no yardstick.  0 where nothing is scored: exact zeros."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    B, N, _ = x.shape
    nrm = np.maximum(np.sqrt((x * x).sum(-1)), F_EPS)
    so, sg = np.zeros(B), np.zeros((B, N))
    for b in range(B):
        L = min(max(int(lens[b]) - 1 - tail, 0), N - 1 - tail)
        so[b] = L
        sg[b, 1:1 + L] = np.abs(g[b]).max() / nrm[b, 1:1 + L]
    return so, sg


def scaled_error(got, ref, scale):
    """max over rows (last axis) of max|got - ref| / scale; a row of scale 0 must be exactly zero"""
    got, ref, scale = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(scale, np.float64)
    assert got.shape == ref.shape and scale.shape == ref.shape[:-1]
    err = np.abs(got - ref).max(-1)
    dead = scale == 0
    assert not got[dead].any() and not ref[dead].any()
    return float((err[~dead] / scale[~dead]).max()) if (~dead).any() else 0.0


def sum_scores(im, s, il, sl, dS=None, mean=False, dtype=np.float64, count_len=False):
    """'sum' / 'mean' scores (alad/loss.py:120-123) as <sum of unit regions, sum of unit words>; 'mean' divides by the PADDED
    (R - 1)(T - 3).  With dS: also (d_im, d_s) and the two upstream gradients (B, D) the normsum backward received."""
    f = dtype
    scale = f(1.0 / ((im.shape[1] - 1) * (s.shape[1] - 3))) if mean else f(1)
    a, b = normsum(im, il, 0, dtype=f, count_len=count_len), normsum(s, sl, 2, dtype=f, count_len=count_len)
    S = (a @ b.T) * scale
    if dS is None:
        return S
    dS = np.asarray(dS, f) * scale
    return S, normsum(im, il, 0, dS @ b, f)[1], normsum(s, sl, 2, dS.T @ a, f)[1], (dS @ b, dS.T @ a)


# ------------------------------------------------------------------------------------------------
# distillation modes
# ------------------------------------------------------------------------------------------------
DISTILL_BS = (1, 2, 5, 256, 257, 513)                          # the sort's power-of-two edges, the 256-thread line loop, the mse grid
ORDINAL_BS = DISTILL_BS[1:]
DISTILL_VIEW_B = 257
MARGIN_Q = 0.25                                                # with the quantised students: every hinge argument exact in fp32
MARGIN_N = 0.2
HINGE_LOSS_RTOL = 1e-5                                         # matrix_losses_numpy.HINGE_LOSS_RTOL
ORDINAL_LOSS_TOL = dict(rtol=5e-6, atol=1e-6)                  # test_gpu_parity.test_distillation_modes_vs_oracle_random, kept
WB = (0.7, -0.2)
CONTRASTIVE_TEACHERS = ('normal', 'ties', 'negative', 'concentrated')
ORDINAL_TEACHERS = ('normal', 'dups', 'inf')


# (B, kind) -> reseed of a family whose first draw missed a CPU-tier precondition (an arg-max less than 1e-3 above the runner-up)
TEACHER_SALT = {(256, 'normal'): 1, (257, 'normal'): 2, (513, 'normal'): 7}


def quantised(B, *key):
    """multiples of 1/16 in [-4, 4], float32"""
    return (_rng('q', B, *key).integers(-64, 65, (B, B)) / 16).astype(np.float32)


def teacher(B, kind):
    """'normal': standard normal (arg-max separated, values distinct: asserted by the CPU tier);  'ties' / 'dups': integers in
    [-3, 3] -- exact arg-max ties and duplicated values in every line;  'negative': every off-diagonal entry below 0, so the zeroed
    diagonal wins every arg-max;  'concentrated': column 2 is 10 and the rest negative: every row picks column 2 (row 2 through its
    zeroed diagonal), c_2 = B;  'inf': normal with +inf sprinkled in (they tie with the sort's padding keys)."""
    rng = _rng('teacher', B, kind, TEACHER_SALT.get((B, kind), 0))
    t = rng.standard_normal((B, B)).astype(np.float32)
    if kind in ('ties', 'dups'):
        t = rng.integers(-3, 4, (B, B)).astype(np.float32)
    elif kind == 'negative':
        t = -np.abs(t) - np.float32(0.5)
    elif kind == 'concentrated':
        t = -np.abs(t) - np.float32(0.5)
        t[:, min(2, B - 1)] = 10
    elif kind == 'inf':
        t[rng.random((B, B)) < 0.1] = np.inf
        t[0, :] = np.inf                                       # a whole line of them
    else:
        assert kind == 'normal'
    return t


def student_normal(B):
    return _rng('student', B).standard_normal((B, B)).astype(np.float32)


def student_jittered(B):
    """the non-quantised student of the two hinge modes, to go with MARGIN_N = 0.2: multiples of 1/16 plus a jitter below 0.002.
    A hinge argument is 0.2 + k / 16 + (two jitters): 0.2 is 0.0125 away from the nearest multiple of 1/16, so every argument stays
    0.0085 away from 0 at any B (standard-normal students put one within 1e-5 of 0 as soon as B reaches a few hundred), while no
    argument is exact in float32."""
    return (quantised(B, 'jittered') + _rng('jitter', B).uniform(-0.002, 0.002, (B, B))).astype(np.float32)


def argmax_gaps(T):
    """(smallest gap between the best and the second-best DISTINCT value, number of lines whose best value is attained twice) over
    the rows and columns of the teacher with its diagonal zeroed"""
    T0 = np.array(T, np.float64)
    np.fill_diagonal(T0, 0.0)
    gap, ties = np.inf, 0
    for M in (T0, T0.T):
        for line in M:
            top = line.max()
            ties += int((line == top).sum() > 1)
            rest = line[line < top]
            if rest.size:
                gap = min(gap, float(top - rest.max()))
    return gap, ties


def contrastive_eval(T, M, margin, dtype=np.float64, last_index=False):
    """(loss, dM, smallest |hinge argument|) of oracle.distill_contrastive with margin + s - diag evaluated in `dtype`, left to right
    as the kernel does (float64: the oracle itself).  The diagonal of dM is minus the off-diagonal activity of its row and column:
    element (k, k) enters its own cost with +1 and -1.  Slip: last_index -- arg-max ties go to the last index."""
    f = dtype
    T0 = np.array(T, np.float64)
    M = np.asarray(M, f)
    B = M.shape[0]
    np.fill_diagonal(T0, 0.0)
    pick = (lambda X: B - 1 - np.argmax(X[:, ::-1], axis=1)) if last_index else (lambda X: np.argmax(X, axis=1))
    cc = np.bincount(pick(T0), minlength=B).astype(np.float64)
    rc = np.bincount(pick(T0.T), minlength=B).astype(np.float64)
    d = np.diag(M)
    with np.errstate(invalid='ignore'):
        a = ((f(margin) + M) - d[:, None]).astype(np.float64)
        b = ((f(margin) + M) - d[None, :]).astype(np.float64)
        loss = np.sum(np.where(cc[None, :] > 0, cc[None, :] * np.where(a < 0, 0.0, a), 0.0)) + \
            np.sum(np.where(rc[:, None] > 0, rc[:, None] * np.where(b < 0, 0.0, b), 0.0))       # unpicked lines are never selected
    ga, gb = cc[None, :] * (a > 0), rc[:, None] * (b > 0)
    dM = ga + gb
    off = ~np.eye(B, dtype=bool)
    dM[np.arange(B), np.arange(B)] = -((ga * off).sum(1) + (gb * off).sum(0))
    return float(loss), dM, float(min(np.abs(a[off]).min(), np.abs(b[off]).min())) if B > 1 else np.inf


def ordinal_parts(T, M, margin, threshold, stride, highest_index=False):
    """float64 (loss, row part, column part, n_rows, n_cols, smallest |hinge argument| compared) of oracle.distill_ordinal: dM is
    the sum of the two parts, each +-1 / n on the active positions.  Slip: highest_index -- equal teacher values are ordered by
    descending index."""
    T, M = np.asarray(T, np.float64), np.asarray(M, np.float64)
    loss, parts, ns, gap = 0.0, [], [], np.inf
    for axis in (1, 0):
        Tt, Mt = (T, M) if axis == 1 else (T.T, M.T)
        if highest_index:
            order = np.array([sorted(range(Tt.shape[1]), key=lambda c, r=r: (Tt[r, c], -c)) for r in range(Tt.shape[0])])
        else:
            order = np.argsort(Tt, axis=1, kind='stable')
        ts = np.take_along_axis(Tt, order, axis=1)
        so = np.take_along_axis(Mt, order, axis=1)
        with np.errstate(invalid='ignore'):
            arg = margin + (so[:, :-stride] - so[:, stride:])
        valid = ts[:, stride:] >= threshold
        n = int(valid.sum())
        if valid.any():
            gap = min(gap, float(np.abs(arg[valid]).min()))
        with np.errstate(invalid='ignore', divide='ignore'):
            loss += np.sum(np.where(arg < 0, 0.0, arg)[valid]) / n if n else np.nan
        act = (valid & (arg > 0)).astype(np.float64) / max(n, 1)
        gs = np.zeros(Mt.shape)
        gs[:, :-stride] += act
        gs[:, stride:] -= act
        g = np.zeros(Mt.shape)
        np.put_along_axis(g, order, gs, axis=1)
        parts.append(g if axis == 1 else g.T)
        ns.append(n)
    return float(loss), parts[0], parts[1], ns[0], ns[1], gap


def mse_ref(T, M, wb):
    """float64 (loss, dM, dwb) of mean((M w0 + w1 - T)^2) and the bounds a float32 evaluation of r = M w0 + w1 - T with the sums in
    double must meet.  With u = 2^-24 and g3 = 3u / (1 - 3u), three float32 roundings (product, sum, difference; two with a fused
    multiply-add) give |r^ - r| <= e = g3 (|M w0| + |w1| + |T|), hence
      loss:  sum(2 |r| e + e^2) / n + 2u |loss|                (the double sums' own rounding is below 1e-13 relative)
      dM = k r^, k = fl(2 w0 / fl(B B)):  (2 |w0| / n) e (1 + g3) + g3 |dM|
      dwb0 = 2 sum(r^ M) / n:  2 sum(e |M|) / n + 2u |dwb0|;      dwb1 = 2 sum(r^) / n:  2 sum(e) / n + 2u |dwb1|."""
    T, M = np.asarray(T, np.float64), np.asarray(M, np.float64)
    w0, w1 = float(np.float32(wb[0])), float(np.float32(wb[1]))
    n = M.size
    u, g3 = U32, 3 * U32 / (1 - 3 * U32)
    r = M * w0 + w1 - T
    e = g3 * (np.abs(M * w0) + abs(w1) + np.abs(T))
    loss, dM = np.mean(r * r), 2.0 * r * w0 / n
    dwb = np.array([np.sum(2.0 * r * M) / n, np.sum(2.0 * r) / n])
    bounds = (np.sum(2 * np.abs(r) * e + e * e) / n + 2 * u * abs(loss), (2 * abs(w0) / n) * e * (1 + g3) + g3 * np.abs(dM),
              np.array([2 * np.sum(e * np.abs(M)) / n + 2 * u * abs(dwb[0]), 2 * np.sum(e) / n + 2 * u * abs(dwb[1])]))
    return (loss, dM, dwb), bounds


def mse_f32(T, M, wb):
    """the kernel's evaluation in numpy: r in float32 (product, sum, difference), the three sums in double"""
    f = np.float32
    T, M = np.asarray(T, f), np.asarray(M, f)
    w0, w1 = f(wb[0]), f(wb[1])
    r = M * w0 + w1 - T
    n = M.size
    k = f(2) * w0 / (f(M.shape[0]) * f(M.shape[0]))
    r64 = r.astype(np.float64)
    return (f(np.sum(r64 * r64) / n), k * r, np.array([2 * np.sum(r64 * M) / n, 2 * np.sum(r64) / n]).astype(f))


def cancelling_diagonal(B):
    """students whose diagonal cost rounds to 0: 100 + multiples of 1/16 everywhere, to go with margin 1e-6 -- below half an ulp of the scores (3.8e-6), so
    float32 margin + s is s, margin + s - diag is 0 wherever s equals the diagonal, and the float64 activity differs there"""
    M = (np.float32(100) + quantised(B, 'cancel') / np.float32(4)).astype(np.float32)
    if B > 1:
        M[0, 1] = M[0, 0]                                      # cost_s[0][1] = margin + 0
        M[B - 1, 0] = M[0, 0]                                  # cost_im[B-1][0] = margin + 0
    return M


MARGIN_TINY = 1e-6


# ------------------------------------------------------------------------------------------------
# order_sim
# ------------------------------------------------------------------------------------------------
ORDER_SHAPES = ((31, 33, 1), (32, 32, 31), (33, 31, 32), (32, 33, 33), (33, 32, 65))
ORDER_SCORE_TOL = dict(rtol=3e-6, atol=1e-6)                   # test_gpu_parity.test_order_sim_vs_oracle_odd_shapes, kept
ORDER_GRAD_RTOL, ORDER_GRAD_ATOL = 1e-4, 2e-5                  # the same test: atol x max(1, max|d_im|), kept
# worst floor_ratio of the float32 restatement over ORDER_SHAPES: scores 1.00e-7, gradients 1.86e-7 (tests/test_secondary_heads_cpu.py::
# test_order_restatement_is_the_oracle_and_floors_are_within_their_recorded_values); recorded rounded up in the last digit, gate = 4 x the recorded floor
ORDER_FLOOR = (1.1e-7, 1.9e-7)
ORDER_GATE = tuple(4 * v for v in ORDER_FLOOR)


def order_inputs(Bi, Bc, D, covered_row=False):
    """(im (Bi, D), s (Bc, D), G (Bi, Bc)) float32; covered_row: im[0] = 10 dominates every caption -- no violation in row 0 (score -0, NaN gradients)"""
    rng = _rng('order', Bi, Bc, D)
    im = rng.standard_normal((Bi, D)).astype(np.float32)
    s = (rng.standard_normal((Bc, D)) + 0.5).astype(np.float32)
    G = rng.standard_normal((Bi, Bc)).astype(np.float32)
    im[:, 0], s[:, 0] = -np.abs(im[:, 0]), np.abs(s[:, 0]) + 1        # feature 0 violates in every pair: finite gradients at D = 1 too
    if covered_row:
        im[0] = 10
    return im, s, G


def order_eval(im, s, G, dtype=np.float64):
    """(scores, d_im, d_s) of -|max(s_j - im_i, 0)| in `dtype` (float64: oracle.order_scores / order_scores_backward)"""
    f = dtype
    im, s, G = np.asarray(im, f), np.asarray(s, f), np.asarray(G, f)
    c = np.maximum(s[None, :, :] - im[:, None, :], f(0))
    nrm = np.sqrt((c * c).sum(2, dtype=f))
    with np.errstate(invalid='ignore', divide='ignore'):
        u = (G / nrm)[:, :, None] * c
    return -nrm, u.sum(1, dtype=f), -u.sum(0, dtype=f)
