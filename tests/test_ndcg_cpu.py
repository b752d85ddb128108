"""CPU tier: the host side of nDCG evaluation (aladin_ndcg, ops.ndcg_from_ranking, aladin_amd.dcg, evaluation.search_ndcg / i2t /
t2i) -- argument and limit checks that must hold before a device is touched, the drop-in signatures, the scorer's files and window
arithmetic -- and the numpy restatement (tests/helpers/ndcg_numpy.py) pinned to the reference's recorded values, which is what the
GPU tier compares the kernel with."""
import ctypes as C
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import ndcg_numpy as N                   # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 2          # ALADIN_ERR_* of include/aladin_hip.h
IDEAL_GIVEN = 1                          # ALADIN_NDCG_IDEAL_GIVEN
KINDS = ['image', 'sentence']
METHODS = ['rougeL', 'spice']
# The restatement repeats the reference's arithmetic, but numpy's float32 power is not the same function everywhere: its SIMD and
# scalar loops, hence two CPUs, may differ in the last bit.  Both are within the 1 ulp the derived bound assumes, so the recorded
# values bind the restatement to that bound -- 3.9e-6 at k = 25 and ideal DCG >= 1, smaller than the bound at the fixture's k = 30.
TOL = 3.9e-6


def lib():
    from aladin_amd import _lib
    return _lib.load()


def fixture_cases(g):
    """-> [(case index, npts, fold, retrieval, rank, lists, expected (n_q, 2))] of tests/golden/ndcg_small.npz."""
    return [(ci, int(npts), int(fold), KINDS[int(kind)], int(rank), g['list_%d' % ci], g['expect_%d' % ci])
            for ci, (npts, fold, kind, rank) in enumerate(g['cases'])]


def fixture_window(r, npts, fold, kind):
    """(queries, gallery) of a fold window of a (captions, images) relevance matrix, reference dcg.py:22-29."""
    blk = r[5 * npts * fold:5 * npts * (fold + 1), npts * fold:npts * (fold + 1)]
    return blk if kind == 'image' else blk.T


def _ndcg(p, **kw):
    """aladin_ndcg on HOST buffers: every call below must be refused before a launch."""
    a = dict(rel=p, q_stride=64, c_stride=1, n_q=2, n_c=30, ranking=p, ld_rank=25, rank=25, flags=0, ndcg=p, dcg=p, ideal=p)
    a.update(kw)
    return lib().aladin_ndcg(a['rel'], a['q_stride'], a['c_stride'], a['n_q'], a['n_c'], a['ranking'], a['ld_rank'], a['rank'],
                             a['flags'], a['ndcg'], a['dcg'], a['ideal'], None)


def test_entry_point_checks_arguments_before_touching_a_device():
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    for kw in ({'rel': null}, {'ranking': null}, {'ndcg': null}, {'n_q': 0}, {'n_c': 0}, {'rank': 0}, {'ld_rank': 24},
               {'flags': IDEAL_GIVEN, 'ideal': null}, {'flags': IDEAL_GIVEN, 'ideal': null, 'n_c': 40000}):
        assert _ndcg(p, **kw) == ERR_ARG, kw
        assert b'ndcg' in lib().aladin_last_error()
    # the limit of the selection, named; dcg and ideal may be NULL without the flag (the call gets past the argument check)
    assert _ndcg(p, n_c=36865, dcg=null, ideal=null) == ERR_UNSUPPORTED
    msg = lib().aladin_last_error().decode()
    assert 'ndcg' in msg and '36864' in msg and '36865' in msg, msg
    assert lib().aladin_version() == 13                  # 13: the alignment geometry's layout field (this entry point: unchanged since it was added)


def test_ops_wrapper_raises_value_error_before_the_device():
    from aladin_amd import ops
    rel = torch.zeros((4, 30))
    rk = torch.zeros((4, 25), dtype=torch.int32)
    bad = [dict(rel=torch.zeros(30)), dict(rel=rel.double()), dict(rel=rel.numpy()), dict(dim=2), dict(rel=torch.zeros((0, 30))),
           dict(ranking=rk.long()), dict(ranking=torch.zeros((3, 25), dtype=torch.int32)), dict(ranking=torch.zeros(25, dtype=torch.int32)),
           dict(ranking=rk.tolist()), dict(rank=0), dict(rank=26), dict(ranking=torch.zeros((4, 0), dtype=torch.int32)),
           dict(dim=0),                                                     # 30 queries along dim 0, 4 rankings
           dict(ideal=torch.zeros(4)), dict(ideal=torch.zeros(3, dtype=torch.float64)), dict(ideal=[0.0] * 4)]
    for kw in bad:
        a = dict(rel=rel, ranking=rk)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.ndcg_from_ranking(a.pop('rel'), a.pop('ranking'), **a)
    wide = torch.zeros((1, 36865))
    one = torch.zeros((1, 25), dtype=torch.int32)
    with pytest.raises(ValueError, match='36864'):
        ops.ndcg_from_ranking(wide, one)
    with pytest.raises(ValueError, match='36864'):
        ops.ndcg_from_ranking(wide.t(), one, dim=0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):            # with the ideal given the limit is gone: refused for the device only
        ops.ndcg_from_ranking(wide, one, ideal=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):            # inside the limits: refused, never computed
        ops.ndcg_from_ranking(rel, rk)


def test_scorer_and_evaluation_layers_raise_value_error(monkeypatch):
    from aladin_amd import dcg as D
    from aladin_amd import evaluation as E
    r = np.zeros((20, 4), np.float32)
    with pytest.raises(ValueError, match='methods'):
        D.DCG(None, 20, 'test', relevance_methods=['rougeL', 'spice'], relevances=[r])
    with pytest.raises(ValueError, match='n_queries'):
        D.DCG(None, 21, 'test', relevances=[r])
    with pytest.raises(ValueError, match='rank'):
        D.DCG(None, 20, 'test', rank=0, relevances=[r])
    sc = D.DCG(None, 20, 'test', relevances=[r])
    rk = torch.zeros((10, 3), dtype=torch.int32)
    for call in (lambda: sc.compute_ndcg_batch(2, rk, retrieval='both'), lambda: sc.compute_ndcg_batch(5, rk),        # 25 captions of 20
                 lambda: sc.compute_ndcg_batch(2, rk, fold_index=2), lambda: sc.compute_ndcg_batch(0, rk),
                 lambda: sc.compute_ndcg_batch(2, rk, fold_index=-1), lambda: sc.compute_ndcg(2, 10, [0, 1]),
                 lambda: sc.compute_ndcg(2, 2, [0, 1], retrieval='sentence'), lambda: sc.compute_ndcg(2, 0, [0], retrieval='x')):
        with pytest.raises(ValueError, match='DCG'):
            call()
    monkeypatch.setattr(D, '_device', lambda: torch.device('cpu'))        # past the host checks nothing may be computed off the GPU
    with pytest.raises(ValueError, match='rankings'):
        sc.compute_ndcg_batch(2, torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match='rankings'):
        sc.compute_ndcg(2, 0, [])
    with pytest.raises(ValueError, match='11 rankings'):
        sc.compute_ndcg_batch(2, torch.zeros((11, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        sc.compute_ndcg_batch(2, rk)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        D.ndcg_from_ranking([0.5, 0.25, 1.0], [2, 0])
    with pytest.raises(ValueError, match='y_true'):
        D.dcg_from_ranking([[0.5, 0.25]], [0])
    with pytest.raises(ValueError, match='direction'):
        E.search_ndcg(rk, sc, direction='both')
    with pytest.raises(ValueError, match='scorer'):
        E.search_ndcg(rk, None)
    with pytest.raises(ValueError, match='table'):
        E.search_ndcg(torch.zeros(10, dtype=torch.int32), sc, direction='t2i')
    with pytest.raises(ValueError, match='DCG'):
        E.search_ndcg(rk, sc, direction='i2t')                             # npts defaults to 10 images: 50 captions of 20


def test_i2t_t2i_demand_the_fold_window_as_gallery_and_keep_zeros_without_a_scorer(monkeypatch):
    from aladin_amd import dcg as D
    from aladin_amd import evaluation as E
    sim = torch.zeros((4, 20))
    monkeypatch.setattr(E, '_eval_scores', lambda *a: sim)
    monkeypatch.setattr(E, '_ranks', lambda s: (np.arange(4.0), np.zeros(4), np.arange(20.0), np.zeros(20)))
    images, captions = torch.zeros((20, 3, 8)), torch.zeros((20, 3, 8))
    sc = D.DCG(None, 20, 'test', relevances=[np.zeros((20, 4), np.float32)])
    with pytest.raises(ValueError, match=r'20 captions ranked, 10 in the window of npts=2'):
        E.i2t(images, captions, None, None, npts=2, ndcg_scorer=sc)
    with pytest.raises(ValueError, match=r'4 images ranked, 2 in the window of npts=2'):
        E.t2i(images, captions, None, None, npts=2, ndcg_scorer=sc)
    for fn, n in ((E.i2t, 4), (E.t2i, 20)):
        m = fn(images, captions, None, None)
        assert len(m) == 7 and m[5:] == (0, 0) and type(m[5]) is int
        assert fn(images, captions, None, None, None, False, None, 1) == m
    m, (ranks, top1) = E.i2t(images, captions, None, None, return_ranks=True, ndcg_scorer=None, fold_index=3)
    assert m[5:] == (0, 0) and len(ranks) == 4


def test_drop_in_signatures_match_the_reference():
    """The rule of test_boundary_cpu.test_drop_in_signatures_match_the_reference for the scorer's surface: same names, order, kinds
    and defaults; trailing parameters only with a default."""
    from aladin_amd import dcg as D
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'signatures_ndcg.json')))
    homes = {'DCG.__init__': D.DCG.__init__, 'DCG.compute_ndcg': D.DCG.compute_ndcg, 'ndcg_from_ranking': D.ndcg_from_ranking,
             'dcg_from_ranking': D.dcg_from_ranking}
    assert set(ref) == set(homes)
    for key, want in ref.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(homes[key]).parameters.values()]
        assert got[:len(want)] == want, (key, got, want)
        for extra in got[len(want):]:
            assert extra[2] is not None or extra[1] in ('VAR_POSITIONAL', 'VAR_KEYWORD'), (key, 'extra parameter without a default', extra)
    assert [p[0] for p in ref['DCG.__init__']] == ['self', 'config', 'n_queries', 'split', 'rank', 'relevance_methods']


def test_restatement_gives_the_reference_values():
    """Every recorded query of the fixture: the restatement repeats the reference's float32 / float64 arithmetic and is held to
    the derived per-query bound (see TOL above; the measured difference is printed); the all-zero windows give exactly 0; the
    data condition behind the GPU tolerance (ideal DCG >= 1 wherever it is not 0) holds."""
    g = load_golden('ndcg_small')
    assert [str(m) for m in g['methods']] == METHODS
    assert g['rel_rougeL'].shape == g['rel_spice'].shape == (300, 60) and g['rel_rougeL'].dtype == np.float32
    assert (g['rel_spice'] == 0).mean() > 0.6 and (g['rel_rougeL'] == 0).mean() < 0.05
    galleries, zeros, worst = set(), 0, 0.0
    for ci, npts, fold, kind, rank, lists, expect in fixture_cases(g):
        for mi, m in enumerate(METHODS):
            win = fixture_window(g['rel_' + m], npts, fold, kind)
            galleries.add(win.shape[1])
            assert lists.shape == (win.shape[0], rank) and expect.shape == (win.shape[0], 2)
            nd, dc, best = N.ndcg_table(win, lists, rank=rank)
            allzero = ~win.any(axis=1)
            zeros += int(allzero.sum())
            assert (nd[allzero] == 0).all() and (expect[allzero, mi] == 0).all() and (best[allzero] == 0).all()
            assert (best[~allzero] >= 1.0).all() and (win[~allzero].max(axis=1) == 1.0).all()
            err = np.abs(nd - expect[:, mi])
            assert (err <= N.ndcg_bound(best, min(rank, win.shape[1]))).all(), (ci, m, err.max())
            worst = max(worst, float(err.max()))
    assert galleries == {30, 60, 150, 300} and zeros >= 8
    print('restatement vs recorded reference values: worst |diff| %.3g' % worst)          # ~1e-16 where the fixture was generated
    assert abs(float(N.ndcg_bound(1.0, 25)) - 3.9e-6) < 0.05e-6          # the figure the derivation states for k = 25, best >= 1


def test_restatement_rules_the_reference_leaves_open():
    rel = np.array([0.5, 0.0, 1.0, 0.25], np.float32)
    nd, dc, best = N.ndcg_parts(rel, [2, 0, 3, 1])
    assert nd == 1.0 and dc == best                                       # the ideal order
    assert N.ndcg_parts(rel, [2, 0, 3, 1, -1, -1], rank=6)[1:] == (dc, best)          # k = min(rank, gallery)
    a = N.ndcg_parts(rel, [7, 2, -5, 0])
    b = N.ndcg_parts(rel, [-1, 2, -1, 0])
    assert a == b and 0 < a[0] < 1                                        # "no item" keeps the position's discount
    assert abs(a[1] - (1.0 / np.log2(3) + (2 ** np.float32(0.5) - 1) / np.log2(5))) < 1e-15
    assert N.ndcg_parts(np.zeros(5, np.float32), [0, 1]) == (0.0, 0.0, 0.0)


def _numpy_device_op(calls):
    """A stand-in for ops.ndcg_from_ranking on host tensors (the restatement), recording how it was called."""
    def op(rel, ranking, dim=1, rank=None, ideal=None, return_parts=False):
        calls.append(dict(shape=tuple(rel.shape), dim=dim, rank=rank, ideal=ideal is not None, n_q=ranking.shape[0]))
        nd, dc, best = (torch.from_numpy(v) for v in N.ndcg_table(rel.numpy(), ranking.numpy(), dim=dim, rank=rank))
        if ideal is not None:
            assert torch.equal(ideal, best)
        return (nd, dc, best) if return_parts else nd
    return op


def test_scorer_reads_the_raw_files_and_cuts_the_reference_windows(tmp_path, monkeypatch):
    """DCG over raw float32 files named as the reference names them, through a config dict; its windows, query axis and caches for
    both retrieval kinds and fold indices, checked on the host by replacing the device op with the restatement: the recorded
    reference values come out for every case of the fixture."""
    from aladin_amd import dcg as D
    g = load_golden('ndcg_small')
    os.makedirs(tmp_path / 'toy' / 'relevances')
    for m in METHODS:
        g['rel_' + m].tofile(str(tmp_path / 'toy' / 'relevances' / ('toy-test-%s.npy' % m)))
    config = {'dataset': {'data': str(tmp_path), 'name': 'toy'}}
    calls = []
    monkeypatch.setattr(D, '_device', lambda: torch.device('cpu'))
    monkeypatch.setattr(D.ops, 'ndcg_from_ranking', _numpy_device_op(calls), raising=False)
    one = D.DCG(config, 300, 'test')
    assert one.rank == 25 and one.relevance_methods == ['rougeL'] and len(one.relevances) == 1
    scorers = {}
    for ci, npts, fold, kind, rank, lists, expect in fixture_cases(g):
        sc = scorers.setdefault(rank, D.DCG(config, 300, 'test', rank=rank, relevance_methods=METHODS))
        assert [r.shape for r in sc.relevances] == [(300, 60)] * 2 and np.array_equal(sc.relevances[1], g['rel_spice'])
        del calls[:]
        got = sc.compute_ndcg_batch(npts, lists, fold_index=fold, retrieval=kind)
        assert list(got) == METHODS
        for mi, m in enumerate(METHODS):
            assert got[m].dtype == torch.float64 and np.abs(got[m].numpy() - expect[:, mi]).max() <= TOL
            assert torch.equal(sc._window(mi, npts, fold), torch.from_numpy(np.ascontiguousarray(fixture_window(g['rel_' + m], npts, fold, 'image'))))
        k = min(rank, lists.shape[1])
        assert [c['dim'] for c in calls] == [1 if kind == 'image' else 0] * 2 and all(c['rank'] == k and not c['ideal'] for c in calls)
        again = sc.compute_ndcg_batch(npts, torch.from_numpy(lists), fold_index=fold, retrieval=kind)
        assert all(c['ideal'] for c in calls[2:]) and len(calls) == 4           # the kept ideal DCG is passed from the second call on
        assert all(torch.equal(again[m], got[m]) for m in METHODS)
        for q in (0, lists.shape[0] // 2, lists.shape[0] - 1):                     # the reference's per-query call, full ranking in
            full = [int(v) for v in lists[q] if v >= 0]
            single = sc.compute_ndcg(npts, q, full, fold_index=fold, retrieval=kind)
            assert list(single) == METHODS and all(isinstance(v, float) for v in single.values())
            assert max(abs(single[m] - expect[q, mi]) for mi, m in enumerate(METHODS)) <= TOL
        assert calls[-1]['n_q'] == 1
    sc = scorers[25]
    assert len(sc._windows) == 6 and len(sc._ideals) == 12                        # 3 folds x 2 methods; x 2 retrieval kinds
    sc.clear()
    assert not sc._windows and not sc._ideals
    # relevances= takes arrays or tensors instead of files
    mem = D.DCG(None, 300, 'test', relevance_methods=METHODS, relevances=[g['rel_rougeL'], torch.from_numpy(g['rel_spice'])])
    ci, npts, fold, kind, rank, lists, expect = fixture_cases(g)[3]
    got = mem.compute_ndcg_batch(npts, lists, fold_index=fold, retrieval=kind)
    assert all(np.abs(got[m].numpy() - expect[:, mi]).max() <= TOL for mi, m in enumerate(METHODS))
