"""CPU tier of the semantic contrastive loss (aladin_semantic_hinge_fwd_bwd, ops.semantic_hinge_loss, loss.SemanticContrastiveLoss,
loss.AlignmentSemanticContrastiveLoss): the float64 restatement (tests/helpers/semantic_numpy.py) pinned to the reference's recorded
float64 run of tests/golden/semantic.npz, the fixture's coverage and input condition, the restatement's properties (diagonal-only
positives are the plain hinge, the two column orders, the line without candidates), the binding's new symbols, the drop-in
signatures, and the checks that must hold before a device is touched."""
import ctypes as C
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import alad_oracle as O

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import semantic_numpy as X               # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 2          # ALADIN_ERR_* of include/aladin_hip.h
MAX_B = 8192                             # ALADIN_SEM_MAX_B
MEASURES = ['dot', 'cosine', 'order']


def same(got, want):
    return abs(got - float(want)) <= 1e-9 * max(1.0, abs(float(want)))


def matrix_fixture(g):
    """-> [(case index, B, family, S, rel, draws)] of the fixture's matrix level, inputs rebuilt from the seeds and checksummed"""
    out = []
    for ci, ((B, fam), seed) in enumerate(zip(g['matrix_cases'], g['matrix_seeds'])):
        B, fam = int(B), X.FAMILIES[int(fam)]
        S, rel, draws = X.matrix_inputs(B, fam, int(seed))
        assert same(X.checksum(S), g['m%d_S_checksum' % ci]) and same(X.checksum(rel), g['m%d_rel_checksum' % ci])
        assert np.array_equal(draws, g['m%d_draws' % ci])
        out.append((ci, B, fam, S, rel, draws))
    return out


def class_fixture(g):
    """-> [(case index, measure, B, D, im, s, rel, draws)] of the fixture's class level"""
    out = []
    for ci, ((m, B, D), seed) in enumerate(zip(g['class_cases'], g['class_seeds'])):
        measure, B, D = MEASURES[int(m)], int(B), int(D)
        im, s, rel, draws = X.class_inputs(measure, B, D, int(seed))
        assert same(X.checksum(im), g['c%d_im_checksum' % ci]) and same(X.checksum(s), g['c%d_s_checksum' % ci])
        assert same(X.checksum(rel), g['c%d_rel_checksum' % ci]) and np.array_equal(draws, g['c%d_draws' % ci])
        out.append((ci, measure, B, D, im, s, rel, draws))
    return out


def test_fixture_covers_the_cases_and_meets_the_input_condition():
    g = load_golden('semantic')
    assert float(g['margin']) == X.MARGIN == 0.2 and float(g['threshold']) == X.THRESHOLD == 0.4 and float(g['cond_eps']) == X.COND_EPS == 2.0 ** -19
    cases = matrix_fixture(g)
    assert [(B, fam) for _, B, fam, _, _, _ in cases] == X.matrix_cases()
    assert X.SIZES == (1, 2, 5, 33, 65, 257) and X.FAMILIES == ('diag', 'groups', 'dense')
    worst_x, worst_gap = np.inf, np.inf
    for ci, B, fam, S, rel, draws in cases:
        assert np.array_equal(S * 65536, np.round(S * 65536)) and np.abs(S).max() <= 1           # the 2^-16 grid
        assert (np.diag(rel) == 1).all() and draws.dtype == np.int32 and draws.min() >= 0 and draws.max() < 2 ** 31 - 1
        for mv in X.MODES:
            min_x, gap, ok = X.condition_figures(S, rel, X.MARGIN, X.THRESHOLD, draws, mv)
            p = 'm%d_%s_' % (ci, 'max' if mv else 'sum')
            assert ok and min_x == float(g[p + 'min_x']) and gap == float(g[p + 'min_gap']), (ci, B, fam, mv, min_x, gap)
            assert g[p + 'dS'].dtype == np.int16 and g[p + 'dS'].shape == (B, B) and g[p + 'pos'].shape == (2 * B,)
            worst_x, worst_gap = min(worst_x, min_x), min(worst_gap, gap)
    ccases = class_fixture(g)
    assert [(m, B, D) for _, m, B, D, _, _, _, _ in ccases] == list(X.CLASS_CASES)
    for ci, measure, B, D, im, s, rel, draws in ccases:
        assert np.array_equal(im * 64, np.round(im * 64)) and np.array_equal(s * 64, np.round(s * 64))      # the 2^-6 grid
        if measure == 'dot':                                                                  # exact in fp32 in any order
            assert (np.abs(im.astype(np.float64)) @ np.abs(s.astype(np.float64)).T).max() * 4096 < 2 ** 24
        S = X.class_scores(measure, im, s)
        for mv in X.MODES:
            min_x, gap, ok = X.condition_figures(S, rel, X.MARGIN, X.THRESHOLD, draws, mv)
            assert ok, (ci, measure, mv, min_x, gap)
            worst_x, worst_gap = min(worst_x, min_x), min(worst_gap, gap)
    print('input condition: smallest |x| %.3g, smallest top-two gap %.3g, bound %.3g' % (worst_x, worst_gap, X.COND_EPS))


def test_restatement_gives_the_reference_values():
    """loss to 1e-12 relative, dS and the positives equal; the reference asked randint for the restatement's candidate counts"""
    g = load_golden('semantic')
    worst = 0.0
    runs = [('m%d' % ci, S.astype(np.float64), rel, draws) for ci, B, fam, S, rel, draws in matrix_fixture(g)]
    runs += [('c%d' % ci, X.class_scores(m, im, s), rel, draws) for ci, m, B, D, im, s, rel, draws in class_fixture(g)]
    assert len(runs) == 18 + 5
    for key, S, rel, draws in runs:
        B = S.shape[0]
        for mv in X.MODES:
            p = '%s_%s_' % (key, 'max' if mv else 'sum')
            loss, dS, pos = X.semantic_f64(S, rel, X.MARGIN, X.THRESHOLD, draws, mv)
            want = float(g[p + 'loss'])
            assert abs(loss - want) <= 1e-12 * max(1.0, abs(want)), (p, loss, want)
            worst = max(worst, abs(loss - want) / max(1.0, abs(want)))
            assert np.array_equal(dS, g[p + 'dS']), p
            assert np.array_equal(pos, g[p + 'pos']), p
            cand = rel > X.THRESHOLD
            assert np.array_equal(g[p + 'asked'], np.concatenate([cand.sum(1), cand.sum(0)]))
            assert dS.sum() == 0                                                              # every active term has its anchor
            if B == 1:
                assert loss == 0.0 and not dS.any()
    print('restatement vs recorded reference: worst relative loss diff %.3g' % worst)


def test_diagonal_positives_are_the_plain_hinge():
    """'diag' relevances: both column orders, and the oracle's VSE++ hinge, loss and dS"""
    for B in X.SIZES:
        S, rel, draws = X.matrix_inputs(B, 'diag', 0)
        S64 = S.astype(np.float64)
        for mv in X.MODES:
            want_loss, want_dS = O.hinge_loss(S64, X.MARGIN, mv, return_grad=True)
            for order in ('reference', 'aligned'):
                loss, dS, pos = X.semantic_f64(S64, rel, X.MARGIN, X.THRESHOLD, draws, mv, order=order)
                assert abs(loss - float(want_loss)) <= 1e-12 * max(1.0, abs(float(want_loss))) and np.array_equal(dS, want_dS)
                assert np.array_equal(pos, np.tile(np.arange(B), 2))


def test_the_two_column_orders_differ_off_the_diagonal_family():
    for fam in ('groups', 'dense'):
        for B in (33, 65, 257):                                                                # (at B = 5 the picks may come out sorted)
            S, rel, draws = X.matrix_inputs(B, fam, 0)
            for mv in X.MODES:
                ref = X.semantic_f64(S, rel, X.MARGIN, X.THRESHOLD, draws, mv, order='reference')
                ali = X.semantic_f64(S, rel, X.MARGIN, X.THRESHOLD, draws, mv, order='aligned')
                assert np.array_equal(ref[2], ali[2])                                          # the same positives
                # sum mode tells the orders apart.  In max mode they may coincide: where every column's maximum is positive the loss
                # is sum_j (margin + max_i S_ij) minus the sum of the anchors and every chosen cell receives -1, whatever the order
                if not mv:
                    assert ref[0] != ali[0] and not np.array_equal(ref[1], ali[1]), (fam, B)
    # the quirk itself: the column anchors are handed out in row-major order of the chosen cells
    S = np.arange(9, dtype=np.float64).reshape(3, 3)
    pos = np.array([0, 1, 2, 2, 0, 1])                                                         # columns 0, 1, 2 chose rows 2, 0, 1
    a1, a2, cells = X.anchors(S, pos, 'reference')
    assert cells == [(0, 1), (1, 2), (2, 0)] and a2.tolist() == [1.0, 5.0, 6.0]
    a1, a2, cells = X.anchors(S, pos, 'aligned')
    assert cells == [(2, 0), (0, 1), (1, 2)] and a2.tolist() == [6.0, 1.0, 5.0]


def test_a_line_without_candidates_falls_back_to_its_diagonal_cell_and_mask_positives_clears_them():
    B = 5
    S, rel, draws = X.matrix_inputs(B, 'dense', 0)
    rel = rel.copy()
    rel[2, :] = 0.1                                                                            # row 2: no candidate, the diagonal included
    rel[:, 4] = np.nan                                                                         # column 4: NaN compares false
    pos = X.positives(rel, X.THRESHOLD, draws)
    assert pos[2] == 2 and pos[B + 4] == 4
    for v in range(2 * B):
        line = rel[v] if v < B else rel[:, v - B]
        with np.errstate(invalid='ignore'):
            idx = np.nonzero(line > X.THRESHOLD)[0]
        assert pos[v] == (idx[draws[v] % len(idx)] if len(idx) else v % B)
    rel = X.relevances(33, 'groups')
    S, _, draws = X.matrix_inputs(33, 'groups', 0)
    a1, a2, _ = X.anchors(S.astype(np.float64), X.positives(rel, X.THRESHOLD, draws))
    cs, ci = X.costs(S.astype(np.float64), rel, X.MARGIN, X.THRESHOLD, a1, a2, mask_positives=True)
    assert not cs[rel > X.THRESHOLD].any() and not ci[rel > X.THRESHOLD].any() and cs[rel <= X.THRESHOLD].any()
    plain = X.semantic_f64(S, rel, X.MARGIN, X.THRESHOLD, draws, False)
    masked = X.semantic_f64(S, rel, X.MARGIN, X.THRESHOLD, draws, False, mask_positives=True)
    assert masked[0] < plain[0] and masked[1].sum() == 0
    bad = S.astype(np.float64).copy()
    bad[1, 3] = np.nan
    assert all(np.isnan(X.semantic_f64(bad, rel, X.MARGIN, X.THRESHOLD, draws, mv)[0]) for mv in X.MODES)


def test_new_symbols_are_declared_exported_and_bound():
    from aladin_amd import _lib
    names = ['aladin_semantic_hinge_workspace_bytes', 'aladin_semantic_hinge_fwd_bwd']
    assert [n for n in _lib.SIGNATURES if 'semantic' in n] == names and all(n in _lib.SYMBOLS for n in names)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    assert _lib.ABI_VERSION == lib.aladin_version() == 13                 # added entry points do not move the version
    assert _lib.SEM_MAX_B == MAX_B >= 2048
    assert (_lib.SEM_MAX_VIOLATION, _lib.SEM_COLUMNS_ALIGNED, _lib.SEM_MASK_POSITIVES) == (1, 2, 4)
    hdr = open(os.path.join(ROOT, 'include', 'aladin_hip.h')).read()
    for line in ('#define ALADIN_SEM_MAX_B %d' % MAX_B, '#define ALADIN_SEM_MAX_VIOLATION 1', '#define ALADIN_SEM_COLUMNS_ALIGNED 2',
                 '#define ALADIN_SEM_MASK_POSITIVES 4', 'ALADIN_API size_t aladin_semantic_hinge_workspace_bytes(int B);',
                 'ALADIN_API int aladin_semantic_hinge_fwd_bwd(const float* S, int64_t ldS, const float* rel,'):
        assert line in hdr, line
    assert '#define ALADIN_ABI_VERSION 13' in hdr.replace('  ', ' ')
    mk = open(os.path.join(ROOT, 'aladin_amd', 'csrc', 'Makefile')).read()
    assert ' semantic.hip ' in next(line for line in mk.splitlines() if line.startswith('SRCS'))
    assert 'aladin_*' in open(os.path.join(ROOT, 'aladin_amd', 'csrc', 'exports.map')).read()


def _aligned_host_pointer(keep):
    buf = (C.c_char * 4096)()
    keep.append(buf)
    return C.c_void_p((C.addressof(buf) + 255) // 256 * 256)


def test_entry_point_checks_arguments_and_the_limit_before_touching_a_device():
    from aladin_amd import _lib
    lib = _lib.load()
    keep = []
    p, null = _aligned_host_pointer(keep), C.c_void_p(0)

    def call(**kw):
        a = dict(S=p, ld=4, rel=p, rs=4, cs=1, B=4, flags=0, draws=p, loss=p, dS=p, pos=p, ws=p)
        a.update(kw)
        return lib.aladin_semantic_hinge_fwd_bwd(a['S'], a['ld'], a['rel'], a['rs'], a['cs'], a['B'], 0.2, 0.4, a['flags'], a['draws'], a['loss'],
                                                 a['dS'], a['pos'], a['ws'], None)
    for kw in ({'S': null}, {'rel': null}, {'draws': null}, {'loss': null}, {'ws': null}, {'B': 0}, {'B': -3}, {'ld': 3}, {'rs': -1}, {'cs': -4},
               {'flags': 8}, {'ws': C.c_void_p(p.value + 4)}):
        assert call(**kw) == ERR_ARG, kw
        assert b'semantic_hinge_fwd_bwd' in lib.aladin_last_error()
    assert call(B=MAX_B + 1, ld=MAX_B + 1) == ERR_UNSUPPORTED
    msg = lib.aladin_last_error().decode()
    assert 'semantic' in msg and str(MAX_B) in msg and str(MAX_B + 1) in msg, msg
    assert call(B=MAX_B + 1, ld=4) == ERR_ARG                               # the argument check comes first
    ws = lib.aladin_semantic_hinge_workspace_bytes
    assert ws(0) == ws(-1) == ws(MAX_B + 1) == 0
    assert all(ws(b) >= 9 * 4 * b for b in (1, 2, 65, 1500, MAX_B))        # per sample: two lines' (value, arg, positive), two anchors, a rank
    assert all(ws(b) < ws(b + 1) for b in (1, 2, 63, 64, 65, 1000))


def test_ops_and_modules_refuse_bad_input_before_a_device_is_touched():
    from aladin_amd import ops
    from aladin_amd.loss import AlignmentSemanticContrastiveLoss, SemanticContrastiveLoss
    x, sq = torch.zeros((4, 8)), torch.zeros((4, 4))
    sets, seq = torch.zeros((4, 5, 8)), torch.zeros((4, 7, 8))
    crit, acrit = SemanticContrastiveLoss(margin=0.2, measure='dot'), AlignmentSemanticContrastiveLoss(margin=0.2)
    draws = torch.zeros(8, dtype=torch.int32)
    for call in (lambda: ops.semantic_hinge_loss(sq, sq, 0.2), lambda: ops.semantic_hinge_loss(sq, sq, 0.2, draws=draws, max_violation=True),
                 lambda: crit(x, x, sq), lambda: acrit(sets, seq, [5] * 4, [7] * 4, sq)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    for call in (lambda: ops.semantic_hinge_loss(torch.zeros((4, 5)), torch.zeros((4, 5)), 0.2), lambda: ops.semantic_hinge_loss(torch.zeros(4), sq, 0.2),
                 lambda: ops.semantic_hinge_loss(torch.zeros((0, 0)), torch.zeros((0, 0)), 0.2), lambda: acrit(sets, seq[:3], [5] * 4, [7] * 3, sq)):
        with pytest.raises(ValueError, match='square'):
            call()
    for rel in (torch.zeros((4, 5)), torch.zeros((3, 3)), torch.zeros(16)):
        with pytest.raises(ValueError, match='aligned with the scores'):
            ops.semantic_hinge_loss(sq, rel, 0.2)
    for bad in (torch.zeros(8, dtype=torch.int64), torch.zeros(7, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32),
                torch.zeros(8, dtype=torch.float32)):
        with pytest.raises(ValueError, match='draws'):
            ops.semantic_hinge_loss(sq, sq, 0.2, draws=bad)
    with pytest.raises(TypeError):
        ops.semantic_hinge_loss(sq, sq, 0.2, draws=[0] * 8)
    with pytest.raises(TypeError):
        ops.semantic_hinge_loss(sq.numpy(), sq, 0.2)
    big = torch.zeros(1).expand(MAX_B + 1, MAX_B + 1)                       # no memory behind it
    with pytest.raises(ValueError, match=str(MAX_B)):
        ops.semantic_hinge_loss(big, big, 0.2)
    for make in (lambda: ops.semantic_hinge_loss(sq, sq, 0.2, column_positives='nope'), lambda: SemanticContrastiveLoss(column_positives='nope'),
                 lambda: AlignmentSemanticContrastiveLoss(column_positives='nope')):
        with pytest.raises(ValueError, match='column_positives'):
            make()
    with pytest.raises(ValueError, match='aggregation'):
        AlignmentSemanticContrastiveLoss(aggregation='nope')
    assert acrit.aggregation == 'MrSw' and 'not in the reference' in AlignmentSemanticContrastiveLoss.__doc__.lower()
    assert ops.semantic_hinge_loss is __import__('aladin_amd.ops_losses', fromlist=['x']).semantic_hinge_loss      # re-exported from ops


def test_drop_in_signatures_match_the_reference():
    """The reference's parameters, in its order and with its defaults; whatever this port adds is keyword-only."""
    from aladin_amd import loss as L
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'signatures_semantic.json')))
    crit = L.SemanticContrastiveLoss
    homes = {'SemanticContrastiveLoss.__init__': crit.__init__, 'SemanticContrastiveLoss.forward': crit.forward,
             'SemanticContrastiveLoss.compute_semantic_contrastive_loss': crit.compute_semantic_contrastive_loss}
    assert set(ref) == set(homes)
    for key, want in ref.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(homes[key]).parameters.values()]
        assert got[:len(want)] == want, (key, got, want)
        assert all(kind == 'KEYWORD_ONLY' and default is not None for _, kind, default in got[len(want):]), (key, got)
    assert ref['SemanticContrastiveLoss.forward'] == [['self', 'POSITIONAL_OR_KEYWORD', None], ['im', 'POSITIONAL_OR_KEYWORD', None],
                                                      ['s', 'POSITIONAL_OR_KEYWORD', None], ['relevances', 'POSITIONAL_OR_KEYWORD', None],
                                                      ['return_similarity_mat', 'POSITIONAL_OR_KEYWORD', 'False']]
    assert [n for n in inspect.signature(crit.__init__).parameters][5:] == ['column_positives', 'mask_positives']
    assert [n for n in inspect.signature(crit.forward).parameters][5:] == ['draws']
    c = crit(margin=0.2, threshold=0.3, measure='cosine', max_violation=True)
    assert (c.margin, c.threshold, c.max_violation, c.sim) == (0.2, 0.3, True, L.cosine_sim) and not list(c.state_dict())
    assert crit(measure='dot').sim is L.dot_sim and crit(measure='order').sim is L.order_sim and not hasattr(crit(), 'sim')
    params = list(inspect.signature(L.AlignmentSemanticContrastiveLoss.forward).parameters)
    assert params == ['self', 'im_set', 's_seq', 'im_len', 's_len', 'relevances', 'return_similarity_mat', 'draws']
    init = inspect.signature(L.AlignmentSemanticContrastiveLoss.__init__).parameters
    assert [(n, p.default) for n, p in init.items()][1:] == [('margin', 0), ('threshold', 0.4), ('max_violation', False), ('aggregation', 'MrSw'),
                                                             ('column_positives', 'reference'), ('mask_positives', False)]
    assert 'SemanticContrastiveLoss' in L.__doc__ and 'alad/loss.py:203-270' in L.__doc__
