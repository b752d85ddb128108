"""CPU tier: the host side of two-stage retrieval (aladin_align_rescore / aladin_rerank_order, ops.align_rescore,
store.alignment_scores_for_pairs, evaluation.search_rerank) -- argument and limit checks that must hold before a device is
touched -- and a numpy model of the ordering rule the GPU tier holds the kernel to."""
import ctypes as C

import numpy as np
import pytest
import torch

ERR_ARG, ERR_UNSUPPORTED = 1, 2          # ALADIN_ERR_* of include/aladin_hip.h
FP16, SPLIT = 0, 1                       # ALADIN_PRECISION_*


def lib():
    from aladin_amd import _lib
    return _lib.load()


def _rescore(p, k=4, dim=1, x_max=10, y_max=10, D=64, precision=SPLIT, x_full=70, out=None, cand=None, rows=None):
    """aladin_align_rescore on HOST buffers: a call that got as far as a launch would fail differently (ALADIN_ERR_HIP)."""
    rows = p if rows is None else rows
    return lib().aladin_align_rescore(rows, p, p, None, 4, x_max, p, p, p, None, 4, y_max, D, precision, dim, x_full,
                                      p if cand is None else cand, k, p if out is None else out, None)


def test_rescore_checks_arguments_before_touching_a_device():
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    assert _rescore(p, out=null) == ERR_ARG                       # null output
    assert b'align_rescore' in lib().aladin_last_error()
    assert _rescore(p, cand=null) == ERR_ARG
    assert _rescore(p, rows=null) == ERR_ARG
    assert _rescore(p, dim=3) == ERR_ARG
    assert b'align_rescore' in lib().aladin_last_error()
    assert _rescore(p, precision=7) == ERR_ARG
    assert _rescore(p, x_full=0) == ERR_ARG
    for k in (0, 257):
        assert _rescore(p, k=k) == ERR_UNSUPPORTED
        msg = lib().aladin_last_error().decode()
        assert 'align_rescore' in msg and '256' in msg, msg
    for kw in ({'x_max': 97}, {'y_max': 97}):
        assert _rescore(p, **kw) == ERR_UNSUPPORTED
        msg = lib().aladin_last_error().decode()
        assert 'align_rescore' in msg and '96' in msg and '97' in msg, msg
    assert _rescore(p, D=0) == ERR_ARG


def test_rerank_order_checks_arguments_before_touching_a_device():
    fn = lib().aladin_rerank_order
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    for args in ((null, p, 2, 4, p, p), (p, null, 2, 4, p, p), (p, p, 2, 4, null, p), (p, p, 2, 4, p, null), (p, p, 0, 4, p, p)):
        assert fn(*args, None) == ERR_ARG
        assert b'rerank_order' in lib().aladin_last_error()
    for k in (0, 257):
        assert fn(p, p, 2, k, p, p, None) == ERR_UNSUPPORTED
        msg = lib().aladin_last_error().decode()
        assert 'rerank_order' in msg and '256' in msg, msg


def _host_store(D=64, tail=0, precision='split', counts=(3, 5)):
    """A store on the host with its tables filled in by hand: enough for every check that precedes the device."""
    from aladin_amd.store import PackedSetStore
    st = PackedSetStore(D, tail, 'cpu', capacity_rows=16, precision=precision)
    st.lengths = [c + 1 + tail for c in counts]
    st._counts = list(counts)
    st.n_rows = sum(counts)
    return st


def test_python_wrappers_raise_value_error():
    from aladin_amd import evaluation as E
    from aladin_amd.store import alignment_scores_for_pairs
    si, sc = _host_store(tail=0), _host_store(tail=2)
    cand = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match='precision'):
        alignment_scores_for_pairs(si, _host_store(tail=2, precision='fp16'), cand)
    with pytest.raises(ValueError, match='feature sizes'):
        alignment_scores_for_pairs(si, _host_store(D=128, tail=2), cand)
    with pytest.raises(ValueError, match='empty'):
        alignment_scores_for_pairs(si, _host_store(tail=2, counts=()), cand)
    with pytest.raises(ValueError, match='stores'):
        alignment_scores_for_pairs(torch.zeros((2, 5, 64)), torch.zeros((2, 5, 64)), cand)
    with pytest.raises(ValueError, match='stores'):
        E.search_rerank(torch.zeros((2, 64)), torch.zeros((2, 64)), k=1)
    with pytest.raises(ValueError, match='stores'):
        E.search_rerank(si, torch.zeros((2, 64)), k=1)
    with pytest.raises(ValueError):
        E.search_rerank(si, sc, k=1, direction='both')
    for bad in (torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.float32), torch.zeros((3, 3), dtype=torch.int32),
                torch.zeros((2,), dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 257), dtype=torch.int32),
                [[0, 1, 1], [0, 0, 1]]):
        with pytest.raises(ValueError, match='shortlist'):
            alignment_scores_for_pairs(si, sc, bad)
        with pytest.raises(ValueError, match='shortlist'):
            E.search_rerank(si, sc, k=3, shortlist=bad)
    with pytest.raises(ValueError, match='shortlist'):
        alignment_scores_for_pairs(si.view([0]), sc, cand, 'i2t')           # two rows for a one-image view
    with pytest.raises(ValueError, match='96'):
        alignment_scores_for_pairs(_host_store(counts=(3, 97)), sc, cand)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        alignment_scores_for_pairs(si, sc, cand)                            # inside the limits: refused for the device, never computed


def order_model(cand, val):
    """The rule of rerank_order_kernel (csrc/rescore.hip) in numpy: entry t goes to position #{j that precede t}; j precedes t
    when j is a candidate and t is none, or both are alike and val_j > val_t, or the values are equal and j < t."""
    cand, val = np.asarray(cand), np.asarray(val, np.float32)
    out_i, out_v = np.empty_like(cand), np.empty_like(val)
    for q in range(cand.shape[0]):
        none = cand[q] < 0
        v = np.where(none | np.isnan(val[q]), -np.inf, val[q]).astype(np.float32)
        for t in range(cand.shape[1]):
            j = np.arange(cand.shape[1])
            before = np.where(none != none[t], none[t], (v > v[t]) | ((v == v[t]) & (j < t)))
            rank = int(before.sum())
            out_i[q, rank] = -1 if none[t] else cand[q, t]
            out_v[q, rank] = v[t]
    return out_i, out_v


def stable_order(cand, val):
    """The specification: a stable descending sort of the scores (-inf where there is no candidate)."""
    cand, val = np.asarray(cand), np.asarray(val, np.float32)
    v = np.where(cand < 0, -np.inf, val).astype(np.float32)
    order = np.argsort(-v, axis=1, kind='stable')
    return np.take_along_axis(np.where(cand < 0, -1, cand), order, 1), np.take_along_axis(v, order, 1)


def test_ordering_model_is_a_stable_descending_sort():
    rng = np.random.RandomState(3)
    cases = []
    cases.append((rng.randint(0, 100, (5, 50)), np.full((5, 50), 0.25, np.float32)))                    # all-equal rows
    c, v = rng.randint(0, 100, (6, 50)), rng.standard_normal((6, 50)).astype(np.float32)
    c[:, 37:] = -1                                                                                      # -1 / -inf tails
    c[3] = -1
    cases.append((c, v))
    c, v = rng.randint(0, 7, (8, 256)), rng.standard_normal((8, 256)).astype(np.float32)                # duplicate candidates ...
    v = np.round(v * 2) / 2                                                                             # ... and many equal scores
    c[rng.random_sample(c.shape) < 0.1] = -1                                                            # holes anywhere in the row
    cases.append((c, v))
    cases.append((np.array([[4]]), np.array([[1.5]], np.float32)))
    for cand, val in cases:
        val = np.where(cand < 0, -np.inf, val).astype(np.float32)          # what aladin_align_rescore leaves at a -1
        got_i, got_v = order_model(cand, val)
        ref_i, ref_v = stable_order(cand, val)
        np.testing.assert_array_equal(got_i, ref_i)
        np.testing.assert_array_equal(got_v, ref_v)
        assert all((row[:(row >= 0).sum()] >= 0).all() for row in got_i)   # -1 last


def test_float64_order_of_the_gpu_check_is_decided():
    """tests/test_rerank_gpu.py::test_full_order_on_separated_data demands the float64 order int for int: its seed must leave
    every adjacent gap inside every query's shortlist >= 1e-4, in both directions, no query left out."""
    import test_rerank_gpu as G
    gaps = G.separated_gaps()
    assert set(gaps) == {'i2t', 't2i'} and min(gaps.values()) >= 1e-4, gaps
