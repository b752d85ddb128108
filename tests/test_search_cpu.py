"""CPU tier: the host side of the top-k gallery search (aladin_search_workspace_bytes, the argument and limit checks of
aladin_search_topk and of ops.search_topk) -- nothing here touches a device -- and the float64 side of the GPU tier's independent
check."""
import ctypes as C

import numpy as np
import pytest
import torch

ERR_ARG, ERR_UNSUPPORTED = 1, 2          # ALADIN_ERR_* of include/aladin_hip.h
MAX_GALLERY = 36864 * 16


def lib():
    from aladin_amd import _lib
    return _lib.load()


def test_workspace_is_zero_for_arguments_the_call_refuses():
    ws = lib().aladin_search_workspace_bytes
    assert ws(5000, 25000, 768, 50, 1) > 0 and ws(5000, 25000, 768, 50, 0) > 0
    for args in ((0, 25000, 768, 50, 1), (5000, 0, 768, 50, 1), (5000, 25000, 0, 50, 1), (-1, 25000, 768, 50, 0), (5000, -7, 768, 50, 0),
                 (5000, 25000, 768, 0, 1), (5000, 25000, 768, 257, 1), (5000, 25000, 768, 50, 2), (5000, 25000, 768, 50, -1),
                 (8, MAX_GALLERY + 1, 64, 50, 1), (MAX_GALLERY + 1, 8, 64, 50, 0)):
        assert ws(*args) == 0, args
    assert ws(8, MAX_GALLERY, 64, 50, 1) > 0 and ws(MAX_GALLERY, 8, 64, 50, 0) > 0
    assert ws(MAX_GALLERY + 1, 8, 64, 50, 1) > 0                        # the limit is on the gallery, not on the queries


def test_workspace_is_monotone_in_k():
    ws = lib().aladin_search_workspace_bytes
    for n_img, n_cap, D in ((5000, 25000, 768), (70, 40000, 64), (37, 53, 30)):
        for dim in (0, 1):
            sizes = [ws(n_img, n_cap, D, k, dim) for k in range(1, 257)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (n_img, n_cap, D, dim)
            assert all(s >= lib().aladin_sim_workspace_bytes(n_img, n_cap, D) for s in sizes)
    assert ws(25000, 25000, 768, 256, 1) > ws(25000, 25000, 768, 1, 1)


def test_workspace_stays_far_below_the_score_matrix():
    """5000 x 25000 x 768, k = 50: the stored path's matrix is 500 MB; the search adds group maxima, a slot table and the
    candidates of the selected groups to the packed operands -- at most a quarter of the matrix in either direction."""
    matrix = 5000 * 25000 * 4
    base = lib().aladin_sim_workspace_bytes(5000, 25000, 768)
    for dim in (0, 1):
        extra = lib().aladin_search_workspace_bytes(5000, 25000, 768, 50, dim) - base
        assert 0 < extra <= matrix // 4, (dim, extra)


def test_search_topk_checks_arguments_before_touching_a_device():
    fn = lib().aladin_search_topk
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)                    # host memory: a call that got as far as a launch would fail differently
    null = C.c_void_p(0)
    assert fn(null, 16, null, 16, 4, 4, 16, 2, 1, null, null, null, null) == ERR_ARG
    for img, cap, out, ws in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        assert fn(img, 16, cap, 16, 4, 4, 16, 2, 1, out, null, ws, null) == ERR_ARG
    assert b'search_topk' in lib().aladin_last_error()
    for k in (0, 257, -3):
        assert fn(p, 16, p, 16, 4, 4, 16, k, 1, p, null, p, null) == ERR_ARG
    assert fn(p, 16, p, 16, 4, 4, 16, 2, 2, p, null, p, null) == ERR_ARG           # dim
    assert fn(p, 8, p, 16, 4, 4, 16, 2, 1, p, null, p, null) == ERR_ARG            # row stride shorter than a row
    assert fn(p, 16, p, 16, 4, MAX_GALLERY + 1, 16, 2, 1, p, null, p, null) == ERR_UNSUPPORTED
    msg = lib().aladin_last_error().decode()
    assert str(MAX_GALLERY) in msg and '36864' in msg, msg
    assert fn(p, 16, p, 16, MAX_GALLERY + 1, 4, 16, 2, 0, p, null, p, null) == ERR_UNSUPPORTED


def test_python_wrapper_raises_value_error_for_the_limits():
    """The limits are checked on shapes alone, before the device check: reachable with CPU tensors."""
    from aladin_amd import ops
    small = torch.zeros((4, 1))
    big = torch.zeros((MAX_GALLERY + 1, 1))
    with pytest.raises(ValueError, match=str(MAX_GALLERY)):
        ops.search_topk(small, big, 5, dim=1)
    with pytest.raises(ValueError, match=str(MAX_GALLERY)):
        ops.search_topk(big, small, 5, dim=0)
    for k in (0, 257):
        with pytest.raises(ValueError, match='256'):
            ops.search_topk(small, small, k)
    with pytest.raises(ValueError):
        ops.search_topk(small, small, 5, dim=3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.search_topk(small, small, 1)                                # inside the limits: refused for the device, never computed


def test_float64_ranking_of_the_gpu_check_is_decided():
    """tests/test_search_gpu.py compares against a float64 ranking only where float64 decides it by more than 1e-5; the seed must
    leave out at most 5 % of the queries by float64 alone."""
    import test_search_gpu as G
    _, _, _, decided, ordered = G.separated_problem()
    assert len(decided) == 200
    assert (~decided).sum() <= 0.05 * len(decided), int((~decided).sum())
    assert (~ordered).sum() <= 0.05 * len(ordered), int((~ordered).sum())


def _model_search(scores, k):
    """numpy model of csrc/search.hip for one query: group maxima with padding as -inf, the min(k, n_groups) best groups by
    (maximum descending, index ascending), slots in index order, top-k of the slots' candidates by (score descending, position
    ascending), positions past the gallery excluded."""
    n_g = len(scores)
    n_groups = -(-n_g // 16)
    padded = np.full(n_groups * 16, -np.inf)
    padded[:n_g] = np.where(np.isnan(scores), -np.inf, scores)
    gmax = padded.reshape(n_groups, 16).max(axis=1)
    sel = np.argsort(-gmax, kind='stable')[:min(k, n_groups)]
    slots = np.sort(sel)
    pos = (slots[:, None] * 16 + np.arange(16)[None, :]).ravel()
    pos = pos[pos < n_g]
    best = pos[np.argsort(-padded[pos], kind='stable')][:k]
    return np.concatenate([best, np.full(k - len(best), -1, dtype=best.dtype)])


def test_group_selection_model_equals_a_stable_sort():
    """The argument of DESIGN.md section 4.4 (a query's k best scores lie in its k best groups), ties included: all-equal rows,
    three-valued rows, all-negative rows, partial last groups, k larger than the gallery."""
    rng = np.random.RandomState(7)
    for case in range(600):
        n_g = int(rng.choice([1, 9, 16, 17, 53, 200, 1003]))
        k = int(rng.choice([1, 2, 13, 50, 256]))
        kind = case % 4
        if kind == 0:
            s = rng.standard_normal(n_g)
        elif kind == 1:
            s = rng.choice([-1.0, 0.0, 2.5], size=n_g)
        elif kind == 2:
            s = np.full(n_g, -3.0)
        else:
            s = -np.abs(rng.standard_normal(n_g)) - 0.5
            s[rng.randint(0, n_g, size=max(1, n_g // 7))] = -0.25          # many equal maxima, all negative
        want = np.argsort(-s, kind='stable')[:k]
        want = np.concatenate([want, np.full(k - len(want), -1, dtype=want.dtype)])
        assert np.array_equal(_model_search(s, k), want), (case, n_g, k)
