"""CPU tier: the host side of the pair alignment maps (aladin_align_pair_map, ops.align_pair_map, store.alignment_map_for_pairs,
evaluation.search_explain) -- argument and limit checks that must hold before a device is touched -- a numpy model of the
(value, index) combine the kernel reduces with, and the float64 model the GPU tier compares against."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_rerank_cpu import ERR_ARG, ERR_UNSUPPORTED, SPLIT, _host_store, lib


def _pair_map(p, k=4, dim=1, x_max=10, y_max=10, D=64, precision=SPLIT, x_full=70, y_full=68, cand=None, rows=None, score=None,
              w_idx=None, w_cos=None, word_ld=10, r_idx=None, r_cos=None, region_ld=10):
    """aladin_align_pair_map on HOST buffers: a call that got as far as a launch would fail differently (ALADIN_ERR_HIP)."""
    pick = lambda v: p if v is None else v                                                   # noqa: E731
    return lib().aladin_align_pair_map(pick(rows), p, p, None, 4, x_max, p, p, p, None, 4, y_max, D, precision, dim, x_full, y_full,
                                       pick(cand), k, pick(score), pick(w_idx), pick(w_cos), word_ld, pick(r_idx), pick(r_cos),
                                       region_ld, None)


def test_pair_map_checks_arguments_before_touching_a_device():
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    assert _pair_map(p, score=null, w_idx=null, w_cos=null, r_idx=null, r_cos=null) == ERR_ARG      # nothing asked for
    assert b'align_pair_map' in lib().aladin_last_error()
    for kw in ({'w_idx': null}, {'w_cos': null}, {'r_idx': null}, {'r_cos': null}):                 # half of a pair of outputs
        assert _pair_map(p, **kw) == ERR_ARG
        assert b'align_pair_map' in lib().aladin_last_error()
    assert _pair_map(p, cand=null) == ERR_ARG
    assert _pair_map(p, rows=null) == ERR_ARG
    assert _pair_map(p, dim=3) == ERR_ARG
    assert _pair_map(p, precision=7) == ERR_ARG
    assert _pair_map(p, x_full=0) == ERR_ARG
    assert _pair_map(p, y_full=0) == ERR_ARG
    assert _pair_map(p, D=0) == ERR_ARG
    assert _pair_map(p, word_ld=9) == ERR_ARG                                                       # a row stride under the counts
    assert _pair_map(p, region_ld=9) == ERR_ARG
    assert b'align_pair_map' in lib().aladin_last_error()
    for k in (0, 257):
        assert _pair_map(p, k=k) == ERR_UNSUPPORTED
        msg = lib().aladin_last_error().decode()
        assert 'align_pair_map' in msg and '256' in msg, msg
    for kw in ({'x_max': 97, 'region_ld': 97}, {'y_max': 97, 'word_ld': 97}):
        assert _pair_map(p, **kw) == ERR_UNSUPPORTED
        msg = lib().aladin_last_error().decode()
        assert 'align_pair_map' in msg and '96' in msg and '97' in msg, msg
    # the limits hold for any subset of the outputs
    assert _pair_map(p, k=257, score=null, r_idx=null, r_cos=null) == ERR_UNSUPPORTED
    assert _pair_map(p, k=257, w_idx=null, w_cos=null, word_ld=0) == ERR_UNSUPPORTED


def test_python_wrappers_raise_before_a_device_is_touched():
    from aladin_amd import evaluation as E
    from aladin_amd import ops
    from aladin_amd.store import alignment_map_for_pairs
    si, sc = _host_store(tail=0), _host_store(tail=2)
    cand = torch.zeros((2, 3), dtype=torch.int32)
    for fn in (alignment_map_for_pairs, lambda a, b, c, *r: E.search_explain(a, b, k=3, shortlist=c)):
        with pytest.raises(ValueError, match='precision'):
            fn(si, _host_store(tail=2, precision='fp16'), cand)
        with pytest.raises(ValueError, match='feature sizes'):
            fn(si, _host_store(D=128, tail=2), cand)
        with pytest.raises(ValueError, match='empty'):
            fn(si, _host_store(tail=2, counts=()), cand)
        with pytest.raises(ValueError, match='stores'):
            fn(torch.zeros((2, 5, 64)), torch.zeros((2, 5, 64)), cand)
        with pytest.raises(ValueError, match='stores'):
            fn(si, torch.zeros((2, 64)), cand)
        for bad in (torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.float32), torch.zeros((3, 3), dtype=torch.int32),
                    torch.zeros((2,), dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 257), dtype=torch.int32),
                    [[0, 1, 1], [0, 0, 1]]):
            with pytest.raises(ValueError, match='shortlist'):
                fn(si, sc, bad)
        with pytest.raises(ValueError, match='96'):
            fn(_host_store(counts=(3, 97)), sc, cand)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(si, sc, cand)                                                # inside the limits: refused for the device, never computed
    with pytest.raises(ValueError, match='direction'):
        alignment_map_for_pairs(si, sc, cand, 'both')
    with pytest.raises(ValueError, match='shortlist'):
        alignment_map_for_pairs(si.view([0]), sc, cand, 'i2t')              # two rows for a one-image view
    with pytest.raises(ValueError, match='direction'):
        E.search_explain(si, sc, k=3, direction='both')
    for top in (0, -2):
        with pytest.raises(ValueError, match='top'):
            E.search_explain(si, sc, k=3, shortlist=cand, top=top)
        with pytest.raises(ValueError, match='top'):
            E.search_explain(torch.zeros((2, 64)), torch.zeros((2, 64)), k=3, top=top)       # before anything else is looked at
    # ops.align_pair_map on host tables
    oi, ci = torch.zeros(2, dtype=torch.int64), torch.tensor([3, 5], dtype=torch.int32)
    rows = torch.zeros((8, 128), dtype=torch.float16)
    x, y = (rows, oi, ci, None, 2, 5), (rows, oi, ci, None, 2, 5)
    with pytest.raises(ValueError, match='dim'):
        ops.align_pair_map(x, y, cand, 2, 64, 'split', 70, 68)
    with pytest.raises(ValueError, match='shortlist'):
        ops.align_pair_map(x, y, cand.to(torch.int64), 1, 64, 'split', 70, 68)
    with pytest.raises(ValueError, match='shortlist'):
        ops.align_pair_map(x, (rows, oi, ci, None, 3, 5), cand, 0, 64, 'split', 70, 68)      # dim = 0: one row per caption
    with pytest.raises(ValueError, match='96'):
        ops.align_pair_map((rows, oi, ci, None, 2, 97), y, cand, 1, 64, 'split', 70, 68)
    with pytest.raises(ValueError, match='96'):
        ops.align_pair_map(x, (rows, oi, ci, None, 2, 97), cand, 1, 64, 'split', 70, 68)
    for fulls in ((0, 68), (70, 0)):
        with pytest.raises(ValueError, match='x_full'):
            ops.align_pair_map(x, y, cand, 1, 64, 'split', *fulls)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.align_pair_map(x, y, cand, 1, 64, 'split', 70, 68)


# ------------------------------------------------------------------------------------------------
# The combine of the kernel's reductions (ALADIN_ARGMAX_STEP, csrc/common.hpp) in numpy
# ------------------------------------------------------------------------------------------------
FILL = 0x7fffffff          # the index the zero fill carries through the reduction (RESCORE_FILL): it loses every tie


def combine(a, b):
    """Greater value, or equal value and lower index."""
    (va, ia), (vb, ib) = a, b
    return b if (vb > va or (vb == va and ib < ia)) else a


def reduce_in_order(items, rng):
    """Reduce by combining two random elements at a time: a random order AND a random association (a tree, as the lanes do)."""
    items = list(items)
    while len(items) > 1:
        i, j = rng.choice(len(items), 2, replace=False)
        a, b = items[i], items[j]
        items = [v for n, v in enumerate(items) if n not in (i, j)] + [combine(a, b) if rng.random_sample() < 0.5 else combine(b, a)]
    return items[0]


def kernel_model(values, fill, rng):
    """One output entry as the kernel forms it: the real candidates with their indices, the fill as (0.0, FILL) for a side
    shorter than its padded set, (-inf, FILL) for the masked rows of the tiles; written as -1 / 0.0 where the fill is left."""
    items = [(np.float32(v), i) for i, v in enumerate(values)]
    items += [(np.float32(-np.inf), FILL)] * int(rng.randint(0, 5))           # rows of the 16-row tile past the count
    items.append((np.float32(0.0), FILL) if fill else (np.float32(-np.inf), FILL))
    v, i = reduce_in_order(items, rng)
    return (-1, np.float32(0.0) if fill else v) if i == FILL else (i, v)


def specification(values, fill):
    """Max, lowest index attaining it; the fill only if it is strictly greater than every real value."""
    values = np.asarray(values, np.float32)
    if values.size == 0 or (fill and values.max() < 0):
        assert fill, 'a side that fills its set has a position'
        return -1, np.float32(0.0)
    return int(np.flatnonzero(values == values.max())[0]), values.max()


def test_combine_model_is_order_independent():
    rng = np.random.RandomState(9)
    rows = [
        [0.5, 0.25, 0.5, -1.0, 0.5],                         # equal maxima: the first
        [0.25] * 40,                                         # all equal
        [-0.5, -0.25, -0.75],                                # all negative: the fill, or the best of them for a full side
        [-0.5, 0.0, -0.25, 0.0],                             # a real zero ties with the fill and wins
        [0.0],
        [-0.0, 0.0],                                         # signed zeros compare equal: the lower index
        [-3.0],
        [],                                                  # no candidate at all: only a shorter-than-padded side has none
        list(np.round(rng.standard_normal(96) * 2) / 2),     # many ties over the 96-position limit
        list(-np.abs(np.round(rng.standard_normal(70) * 2) / 2) - 0.5),
    ]
    for values in rows:
        for fill in (True, False):
            if not values and not fill:
                continue
            want = specification(values, fill)
            for _ in range(25):
                got = kernel_model(values, fill, rng)
                assert got[0] == want[0] and got[1] == want[1], (values, fill, got, want)
    assert kernel_model([-0.5, -0.25], True, rng) == (-1, 0.0) and kernel_model([-0.5, -0.25], False, rng)[0] == 1
    assert kernel_model([-0.5, 0.0, 0.0], True, rng)[0] == 1


def test_combine_is_commutative_and_associative():
    rng = np.random.RandomState(10)
    vals = [np.float32(v) for v in (-np.inf, -1.0, -0.0, 0.0, 0.5, 0.5, 2.0)]
    items = [(v, int(i)) for v in vals for i in (0, 3, 3, 17, FILL)]
    eq = lambda a, b: a[0] == b[0] and a[1] == b[1]                                          # noqa: E731
    for _ in range(2000):
        a, b, c = (items[k] for k in rng.randint(0, len(items), 3))
        assert eq(combine(a, b), combine(b, a))
        assert eq(combine(combine(a, b), c), combine(a, combine(b, c)))


# ------------------------------------------------------------------------------------------------
# The float64 model of tests/test_align_map_gpu.py, without a device
# ------------------------------------------------------------------------------------------------
def test_float64_model_is_the_oracles_score_and_its_band_shares_are_under_the_caps():
    """The GPU tier's weak index check (inside the band) is capped at 5 % (fp16, D = 64 / 100), 12 % (fp16, D = 768) and 0.2 %
    (split) of the entries: the float64 model alone must be under those caps on the whole grid of its inputs, and its column maxima
    with the fill must sum to the oracle's score."""
    import alad_oracle as O
    import test_align_map_gpu as G
    for D, n_img, n_cap in ((64, 23, 27), (100, 23, 27), (768, 12, 20)):
        images, il, captions, cl = G.edge_sets(D, n_img, n_cap)
        m = G.Model(images, il, captions, cl)
        ref = O.alignment_scores(images, captions, il, cl, dtype=np.float64)
        pairs = [(i, j) for i in range(n_img) for j in range(n_cap)]
        assert max(abs(m.score(i, j) - ref[i, j]) for i, j in pairs) <= 1e-12
        for precision in ('fp16', 'split'):
            shares = G.model_shares(m, pairs, precision)
            print('D=%d %s: %.2f %% word->region, %.2f %% region->word inside the band' % (D, precision, 100 * shares[0], 100 * shares[1]))
            assert max(shares) <= G.share_cap(precision, D), (D, precision, shares)


def test_float64_model_of_the_constructed_cases():
    """The fill construction of the GPU tier: the word / region built as minus the sum of the other side's unit rows has only
    negative cosines, clear of zero."""
    import test_align_map_gpu as G
    *_, m = G.fill_sets()
    assert m.cos(0, 1)[:, 2].max() < -0.05 and m.cos(1, 0)[4].max() < -0.05
    best, arg, gap = G.best_and_gap(m.cos(0, 1), True)
    assert arg[2] == -1 and best[2] == 0.0 and gap[2] > 0.05
    best, arg, gap = G.best_and_gap(m.cos(0, 1), False)
    assert arg[2] >= 0 and best[2] < -0.05
