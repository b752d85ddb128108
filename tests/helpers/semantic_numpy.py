"""Inputs and the float64 restatement of the semantic contrastive loss's tests (tests/test_semantic_cpu.py,
tests/test_semantic_gpu.py, tests/golden/make_golden_semantic.py): aladin_semantic_hinge_fwd_bwd (csrc/semantic.hip),
ops.semantic_hinge_loss, loss.SemanticContrastiveLoss, loss.AlignmentSemanticContrastiveLoss.

The restatement follows the specification in include/aladin_hip.h step by step (positives, anchors, costs, loss, dS); the CPU
tier pins it to the reference's recorded float64 run (tests/golden/semantic.npz).  Every input is built HERE from (size, family,
seed) alone, so that what the CPU tier proves about an input (the condition below) holds for the very array the GPU tier feeds
the kernels.

THE INPUT CONDITION.  The hinge is discontinuous: a comparison of decisions (dS, the arg-max) is meaningful only where the
reference's decisions do not hang on the last bits.  Every non-quantised case meets, in float64 on the float32 inputs,
    every off-diagonal |margin + S - anchor| >= COND_EPS = 2^-19, for the row anchor and for the column anchor, and
    every line's largest and second-largest cost differ by >= COND_EPS unless both are 0.
A float32 evaluation of margin + S - anchor rounds at 2.4e-7 at the most (|value| < 4), an eighth of COND_EPS."""
import zlib

import numpy as np

MARGIN = 0.2
THRESHOLD = 0.4
COND_EPS = 2.0 ** -19
SIZES = (1, 2, 5, 33, 65, 257)
FAMILIES = ('diag', 'groups', 'dense')
MODES = (False, True)                                        # max_violation
CLASS_CASES = (('dot', 5, 8), ('dot', 33, 64), ('dot', 65, 64), ('cosine', 5, 8), ('order', 5, 8))
CLASS_FAMILY = 'dense'
MAX_SEEDS = 16


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def grid_scores(B, seed):
    """float32 (B, B): multiples of 2^-16 in [-1, 1]"""
    return (_rng('sem-scores', B, seed).integers(-65536, 65537, (B, B)) / 65536.0).astype(np.float32)


def relevances(B, family, seed=0):
    """float32 (B, B).  'diag': the identity;  'groups': blocks of 5 at 0.7, diagonal 1;  'dense': uniform [0, 1), diagonal 1"""
    if family == 'diag':
        return np.eye(B, dtype=np.float32)
    if family == 'groups':
        g = np.arange(B) // 5
        rel = np.where(g[:, None] == g[None, :], 0.7, 0.0).astype(np.float32)
    else:
        assert family == 'dense'
        rel = _rng('sem-rel', B, seed).random((B, B)).astype(np.float32)
    np.fill_diagonal(rel, 1.0)
    return rel


def make_draws(B, seed):
    """int32 (2B,) in [0, 2^31 - 1): rows, then columns"""
    return _rng('sem-draws', B, seed).integers(0, 2 ** 31 - 1, 2 * B).astype(np.int32)


def matrix_inputs(B, family, seed):
    """(S, rel, draws) of a matrix-level case"""
    return grid_scores(B, seed), relevances(B, family, seed), make_draws(B, seed)


def embeddings(B, D, seed):
    """(im, s) float32 (B, D): entries multiples of 2^-6 in [-1/4, 1/4] -- the products are multiples of 2^-12 and their sums stay
    far below 2^12, exact in fp32 whatever the summation order"""
    rng = _rng('sem-emb', B, D, seed)
    return (rng.integers(-16, 17, (B, D)) / 64.0).astype(np.float32), (rng.integers(-16, 17, (B, D)) / 64.0).astype(np.float32)


def class_scores(measure, im, s):
    """float64 scores of a measure on float32 embeddings"""
    im, s = np.asarray(im, np.float64), np.asarray(s, np.float64)
    if measure == 'dot':
        return im @ s.T
    if measure == 'cosine':
        return (im / np.sqrt((im * im).sum(1, keepdims=True))) @ (s / np.sqrt((s * s).sum(1, keepdims=True))).T
    assert measure == 'order'
    return -np.sqrt((np.clip(s[None, :, :] - im[:, None, :], 0, None) ** 2).sum(2))


def class_inputs(measure, B, D, seed):
    """(im, s, rel, draws) of a class-level case"""
    im, s = embeddings(B, D, seed)
    return im, s, relevances(B, CLASS_FAMILY, seed + 1000), make_draws(B, seed)


def first_good_seed(build, margin=MARGIN, threshold=THRESHOLD):
    """the first seed in [0, MAX_SEEDS) at which build(seed) -> (S float64-able, rel, draws) meets the input condition in both modes"""
    for seed in range(MAX_SEEDS):
        S, rel, draws = build(seed)
        if all(condition_figures(S, rel, margin, threshold, draws, mv)[2] for mv in MODES):
            return seed
    raise AssertionError('no seed below %d meets the input condition' % MAX_SEEDS)


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def positives(rel, threshold, draws):
    """step 1 -> int64 (2B,): every row's column, then every column's row.  A line without candidates: its diagonal cell."""
    rel = np.asarray(rel)
    B = rel.shape[0]
    with np.errstate(invalid='ignore'):
        cand = rel > threshold                               # NaN compares false
    pos = np.empty(2 * B, np.int64)
    for v in range(2 * B):
        idx = np.nonzero(cand[v] if v < B else cand[:, v - B])[0]
        pos[v] = idx[int(draws[v]) % len(idx)] if len(idx) else v % B
    return pos


def anchors(S, pos, order='reference'):
    """step 2 -> (a1 (B,), a2 (B,), cells): cells[m] = (row, column) of the cell whose score is a2[m]"""
    B = S.shape[0]
    a1 = S[np.arange(B), pos[:B]]
    cells = [(int(pos[B + j]), j) for j in range(B)]
    if order == 'reference':
        cells = sorted(cells)                                # row-major: what scores[cols_mask] reads back
    else:
        assert order == 'aligned'
    a2 = np.array([S[r, c] for r, c in cells], S.dtype).reshape(B)
    return a1, a2, cells


def costs(S, rel, margin, threshold, a1, a2, mask_positives=False):
    """step 3 -> (cs, ci): NaN where a cost is NaN, 0 on the diagonal and, with mask_positives, wherever rel > threshold"""
    cs = np.clip(margin + S - a1[:, None], 0, None)
    ci = np.clip(margin + S - a2[None, :], 0, None)
    zero = np.eye(S.shape[0], dtype=bool)
    if mask_positives:
        with np.errstate(invalid='ignore'):
            zero = zero | (np.asarray(rel) > threshold)
    cs[zero] = 0
    ci[zero] = 0
    return cs, ci


def semantic_f64(S, rel, margin, threshold, draws, max_violation, order='reference', mask_positives=False):
    """-> (loss, dS float64 (integer valued), pos int64 (2B,)) for an upstream gradient of 1; ties go to the lowest index"""
    S = np.asarray(S, np.float64)
    B = S.shape[0]
    pos = positives(rel, threshold, draws)
    a1, a2, cells = anchors(S, pos, order)
    cs, ci = costs(S, rel, margin, threshold, a1, a2, mask_positives)
    dS = np.zeros((B, B))
    if max_violation:
        loss = cs.max(1).sum() + ci.max(0).sum()
        js, is_ = cs.argmax(1), ci.argmax(0)                 # the first (lowest) index of the maximum
        for i in range(B):
            if cs[i, js[i]] > 0:
                dS[i, js[i]] += 1
                dS[i, pos[i]] -= 1
        for m in range(B):
            if ci[is_[m], m] > 0:
                dS[is_[m], m] += 1
                dS[cells[m]] -= 1
    else:
        loss = cs.sum() + ci.sum()
        P, Q = cs > 0, ci > 0
        dS += P
        dS += Q
        for i in range(B):
            dS[i, pos[i]] -= P[i].sum()
        for m in range(B):
            dS[cells[m]] -= Q[:, m].sum()
    return float(loss), dS, pos


def condition_figures(S, rel, margin, threshold, draws, max_violation, order='reference', mask_positives=False, exact_ties=False):
    """-> (smallest off-diagonal |margin + S - anchor|, smallest top-two gap of a line's costs (inf outside max mode or where both
    are 0), whether the input condition holds).  exact_ties: the gap is taken to the largest cost BELOW the line's maximum -- for
    comparisons with the restatement, which shares the kernels' lowest-index rule: equal scores give equal costs in float64 and in
    fp32 alike, so an exact tie is decided the same way on both sides"""
    S = np.asarray(S, np.float64)
    B = S.shape[0]
    if B == 1:
        return np.inf, np.inf, True
    pos = positives(rel, threshold, draws)
    a1, a2, _ = anchors(S, pos, order)
    off = ~np.eye(B, dtype=bool)
    min_x = min(np.abs(margin + S - a1[:, None])[off].min(), np.abs(margin + S - a2[None, :])[off].min())
    gap = np.inf
    if max_violation:
        cs, ci = costs(S, rel, margin, threshold, a1, a2, mask_positives)
        for lines in (cs, ci.T):
            if exact_ties:
                for line in lines:
                    u = np.unique(line)
                    if len(u) > 1:
                        gap = min(gap, float(u[-1] - u[-2]))
                continue
            top = np.sort(lines, axis=1)[:, -2:]
            live = top[:, 1] > 0
            if live.any():
                gap = min(gap, float((top[live, 1] - top[live, 0]).min()))
    return float(min_x), float(gap), bool(min_x >= COND_EPS and gap >= COND_EPS)


# ------------------------------------------------------------------------------------------------
# the fixture's case list (tests/golden/semantic.npz), in file order
# ------------------------------------------------------------------------------------------------
def matrix_cases():
    return [(B, fam) for B in SIZES for fam in FAMILIES]


def checksum(a):
    """order-sensitive float64 checksum of an array (the rule of aladin_amd.synth.checksum, for integer arrays too)"""
    a = np.asarray(a, np.float64).ravel()
    return float((a * (1.0 + (np.arange(a.size) % 7))).sum())
