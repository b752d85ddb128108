"""GPU tier (-m gpu): the gallery index (ops.build_search_index / search_index_topk, evaluation.GalleryIndex; csrc/search.hip) --
held int for int and bit for bit to ops.search_topk on the same tensors on both routes, to the stored path (ops.sim_matrix +
aladin_topk) on the small galleries, and to a float64 ranking on separated data."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_search_gpu import T, bits, dev, randn, stored_topk          # noqa: E402  (plain helpers of the search suite)


def sides(queries, gallery, dim):
    """(img, cap) of ops.search_topk for queries against a gallery."""
    return (queries, gallery) if dim == 1 else (gallery, queries)


def assert_equals_search_topk(index, queries, gallery, k, dim):
    from aladin_amd import ops
    ref_idx, ref_val = ops.search_topk(*sides(queries, gallery, dim), k, dim=dim, return_scores=True)
    idx, val = ops.search_index_topk(index, queries, k, dim=dim, return_scores=True)
    n_q = queries.shape[0]
    assert idx.shape == (n_q, k) and idx.dtype == torch.int32 and val.shape == (n_q, k) and val.dtype == torch.float32
    assert torch.equal(idx, ref_idx), (idx != ref_idx).nonzero()[:8].tolist()
    assert torch.equal(bits(val), bits(ref_val))
    assert torch.equal(ops.search_index_topk(index, queries, k, dim=dim), ref_idx)        # the call without scores: the same indices
    return idx, val


@functools.lru_cache(maxsize=None)
def gallery_and_index(n_g, D):
    from aladin_amd import ops
    g = T(randn((n_g, D), 12 + n_g))
    return g, ops.build_search_index(g)


# small-batch route: a gallery smaller than one group, one with a partial last group, one of many slabs; D = 30 is not
# float4-addressable and pads to 64.  k = 50 and 256 exceed the small galleries: the -1 / -inf tail.
@pytest.mark.parametrize('dim', [1, 0])
@pytest.mark.parametrize('D', [30, 100, 768])
@pytest.mark.parametrize('n_g', [9, 53, 1003])
def test_small_batch_route_equals_search_topk(n_g, D, dim):
    from aladin_amd import ops
    gallery, index = gallery_and_index(n_g, D)
    assert len(index) == n_g
    for n_q in (1, 5, 16, 17, 32):
        queries = T(randn((n_q, D), 100 + n_q))
        for k in (1, 50, 256):
            idx, val = assert_equals_search_topk(index, queries, gallery, k, dim)
            live = min(k, n_g)
            assert bool((idx[:, live:] == -1).all()) and bool((val[:, live:] == float('-inf')).all())
            assert bool((idx[:, :live] >= 0).all()) and bool((idx[:, :live] < n_g).all()) and bool(torch.isfinite(val[:, :live]).all())
    if n_g < 1003:                                                      # the stored path, where aladin_topk pins the same bits
        queries = T(randn((17, D), 117))
        sim = ops.sim_matrix(*sides(queries, gallery, dim))
        for k in (1, 50, 256):
            ref_idx, ref_val = stored_topk(sim, k, dim)
            idx, val = ops.search_index_topk(index, queries, k, dim=dim, return_scores=True)
            assert torch.equal(idx, ref_idx) and torch.equal(bits(val), bits(ref_val))


@pytest.mark.parametrize('dim', [1, 0])
def test_tile_route_and_the_routing_edge(dim):
    from aladin_amd import ops
    gallery, index = gallery_and_index(1003, 100)
    limit = ops.SEARCH_INDEX_STREAM_MAX_Q
    assert limit == 32
    for n_q in (300, limit, limit + 1):
        queries = T(randn((n_q, 100), 200 + n_q))
        for k in (1, 50, 256):
            assert_equals_search_topk(index, queries, gallery, k, dim)
    # a D the one-pass route cannot hold takes the tile route at any n_q
    D = ops.SEARCH_INDEX_STREAM_MAX_D + 64
    g = T(randn((53, D), 7))
    assert_equals_search_topk(ops.build_search_index(g), T(randn((5, D), 8)), g, 50, dim)


@pytest.mark.parametrize('dim', [1, 0])
def test_one_index_many_calls(dim):
    from aladin_amd import ops
    D, n_g, k = 100, 1003, 50
    gallery = T(randn((n_g, D), 61))
    keep = gallery.clone()
    index = ops.build_search_index(gallery)
    batches = [T(randn((5, D), 62)), T(3.0 * randn((32, D), 63)), T(0.01 * randn((300, D), 64))]     # three scales, both routes
    want = [ops.search_topk(*sides(q, keep, dim), k, dim=dim, return_scores=True) for q in batches]
    for q, (ri, rv) in zip(batches, want):
        idx, val = ops.search_index_topk(index, q, k, dim=dim, return_scores=True)
        assert torch.equal(idx, ri) and torch.equal(bits(val), bits(rv))
    gallery.fill_(float('nan'))                                         # the fp32 gallery is not needed after the build
    gallery[::2] = 1e30
    torch.cuda.synchronize()
    for q, (ri, rv) in zip(batches, want):
        idx, val = ops.search_index_topk(index, q, k, dim=dim, return_scores=True)
        assert torch.equal(idx, ri) and torch.equal(bits(val), bits(rv))
    # two streams at once against the one index
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = [ops.search_index_topk(index, batches[0], k, dim=dim, return_scores=True) for _ in range(3)]
    with torch.cuda.stream(s2):
        b = [ops.search_index_topk(index, batches[1], k, dim=dim, return_scores=True) for _ in range(3)]
    torch.cuda.synchronize()
    for idx, val in a:
        assert torch.equal(idx, want[0][0]) and torch.equal(bits(val), bits(want[0][1]))
    for idx, val in b:
        assert torch.equal(idx, want[1][0]) and torch.equal(bits(val), bits(want[1][1]))


@pytest.mark.parametrize('dim', [1, 0])
@pytest.mark.parametrize('n_g', [53, 1003])
def test_padding_never_beats_negative_scores(n_g, dim):
    """Every real score is negative; a padded gallery position scores 0 in the accumulators (zero rows of the index).  It must
    count as -inf and never reach the output before the gallery is exhausted."""
    from aladin_amd import ops
    D, n_q = 32, 5
    neg, pos = T(-1.0 + 0.1 * randn((n_q if dim == 1 else n_g, D), 3)), T(1.0 + 0.1 * randn((n_g if dim == 1 else n_q, D), 4))
    queries, gallery = (neg, pos) if dim == 1 else (pos, neg)
    assert bool((ops.sim_matrix(*sides(queries, gallery, dim)) < 0).all())
    index = ops.build_search_index(gallery)
    for k in (50, 60, 256):
        idx, val = assert_equals_search_topk(index, queries, gallery, k, dim)
        live = min(k, n_g)
        assert bool((idx[:, :live] >= 0).all()) and bool((idx[:, :live] < n_g).all()) and bool((val[:, :live] < 0).all())
        assert bool((idx[:, live:] == -1).all())
        srt = torch.sort(idx[:, :live].long(), dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all())                  # no gallery item twice


@pytest.mark.parametrize('dim', [1, 0])
def test_ties_go_to_the_lower_index(dim):
    """800 gallery rows drawn from 40 vectors: duplicates inside a group of 16, across groups and across the slabs a workgroup
    owns (8 groups = 128 rows at this D: rows 127 / 128, 255 / 256, and far apart).  Then a gallery of identical rows."""
    from aladin_amd import ops
    n_g, D, k = 800, 64, 50
    base = randn((40, D), 21)
    which = np.random.RandomState(22).randint(0, 40, size=n_g)
    which[[3, 5, 40, 127, 128, 255, 256, 130, 700, 383, 384]] = [7, 7, 7, 9, 9, 11, 11, 13, 13, 15, 15]
    gallery = T(base[which])
    index = ops.build_search_index(gallery)
    for n_q in (5, 32):
        queries = T(randn((n_q, D), 23))
        idx, val = assert_equals_search_topk(index, queries, gallery, k, dim)
        ties = val[:, 1:] == val[:, :-1]
        assert int(ties.sum()) > n_q * k // 2                           # the case really is about ties
        assert bool((idx[:, 1:][ties] > idx[:, :-1][ties]).all())       # equal scores: ascending index
        sim = ops.sim_matrix(*sides(queries, gallery, dim))
        ref = torch.sort(sim if dim == 1 else sim.t().contiguous(), dim=1, descending=True, stable=True)
        assert torch.equal(idx.long(), ref.indices[:, :k])
    same = T(np.repeat(base[:1], n_g, axis=0))
    index = ops.build_search_index(same)
    queries = T(randn((5, D), 23))
    for kk in (50, 256):
        idx, val = assert_equals_search_topk(index, queries, same, kk, dim)
        assert torch.equal(idx, torch.arange(kk, dtype=torch.int32, device=idx.device).expand(5, kk))
        assert bool((val == val[:, :1]).all())


@pytest.mark.parametrize('dim', [1, 0])
@pytest.mark.parametrize('n_q', [5, 40])
def test_nan_rows(n_q, dim):
    """A NaN gallery row scores NaN against every query and sorts last; a NaN query row scores NaN everywhere."""
    D, n_g = 64, 203
    g, q = randn((n_g, D), 71), randn((n_q, D), 72)
    g[17, 3] = np.nan
    g[200] = np.nan
    q[2, 0] = np.nan
    gallery, queries = T(g), T(q)
    from aladin_amd import ops
    index = ops.build_search_index(gallery)
    for k in (10, 256):
        assert_equals_search_topk(index, queries, gallery, k, dim)


@pytest.mark.parametrize('dim', [1, 0])
def test_strided_inputs(dim):
    """Gallery and queries as column slices of wider tensors: a row stride greater than D (and, at offset 3, rows that are not
    16-byte aligned)."""
    from aladin_amd import ops
    D = 100
    wide_g, wide_q, wide_q2 = T(randn((203, D + 28), 81)), T(randn((17, D + 12), 82)), T(randn((40, D + 12), 83))
    for off in (0, 3):
        gallery, queries, many = wide_g[:, off:off + D], wide_q[:, off:off + D], wide_q2[:, off:off + D]
        assert gallery.stride(0) > D and not gallery.is_contiguous()
        index = ops.build_search_index(gallery)
        assert_equals_search_topk(index, queries, gallery, 50, dim)
        assert_equals_search_topk(index, many, gallery, 50, dim)
        same = ops.build_search_index(gallery.contiguous())             # the index does not depend on how its gallery was laid out
        a, b = (ops.search_index_topk(ix, queries, 50, dim=dim, return_scores=True) for ix in (index, same))
        assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize('dim', [1, 0])
@pytest.mark.parametrize('n_q,seed_q,seed_g', [(16, 101, 102), (5, 103, 104)])
def test_float64_anchor(n_q, seed_q, seed_g, dim):
    """An independent check: numpy float64, no kernel of this library.  The split-fp16 chain carries ~2^-21 relative operand
    error per side, so against |q||g| a score is off by far less than 2^-17 |q||g|; the test first makes sure, on the host, that
    every query's top 11 float64 scores are 2^-16 max|q| max|g| apart (measured without a GPU: 3.4x and 15x that bound), then
    the indices must be the float64 ranking."""
    from aladin_amd import ops
    k = 10
    q, g = randn((n_q, 64), seed_q), randn((1003, 64), seed_g)
    S = q.astype(np.float64) @ g.astype(np.float64).T
    order = np.argsort(-S, axis=1, kind='stable')
    top = np.take_along_axis(S, order[:, :k + 1], axis=1)
    gap = float((top[:, :-1] - top[:, 1:]).min())
    bound = 2.0 ** -16 * np.linalg.norm(q.astype(np.float64), axis=1).max() * np.linalg.norm(g.astype(np.float64), axis=1).max()
    print('smallest gap among the top %d: %.3g = %.2f x the bound %.3g' % (k + 1, gap, gap / bound, bound))
    assert gap >= bound
    idx, val = ops.search_index_topk(ops.build_search_index(T(g)), T(q), k, dim=dim, return_scores=True)
    assert np.array_equal(idx.cpu().numpy(), order[:, :k])
    np.testing.assert_allclose(val.cpu().numpy(), top[:, :k], rtol=0, atol=bound)


@pytest.mark.parametrize('dim', [1, 0])
def test_index_search_under_graph_capture(dim):
    """No allocation, no synchronisation, no host-side decision in the call: captured once, replayed twice on new queries of the
    same shape, equal to the eager result."""
    from aladin_amd import ops
    n_q, n_g, D, k = 5, 1003, 100, 50
    gallery, index = gallery_and_index(n_g, D)
    queries = T(randn((n_q, D), 91))
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        ops.search_index_topk(index, queries, k, dim=dim, return_scores=True)          # warm-up outside the capture (one-time kernel attributes)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_idx, g_val = ops.search_index_topk(index, queries, k, dim=dim, return_scores=True)
    for seed, mag in ((92, 1.0), (93, 5.0)):                            # another magnitude: another power-of-two scale
        queries.copy_(T(mag * randn((n_q, D), seed)))
        graph.replay()
        torch.cuda.synchronize()
        idx, val = ops.search_index_topk(index, queries, k, dim=dim, return_scores=True)
        assert torch.equal(g_idx, idx) and torch.equal(bits(g_val), bits(val))
        assert_equals_search_topk(index, queries, gallery, k, dim)


@functools.lru_cache(maxsize=None)
def two_stores():
    import test_rerank_gpu as R
    D = 64
    images, il = R.make_sets([R.IMG_COUNTS[k % 10] for k in range(13)], 0, D, 41)
    captions, cl = R.make_sets([R.CAP_COUNTS[k % 10] for k in range(21)], 2, D, 42)
    return R.fill_store(images, il, 0, 'split'), R.fill_store(captions, cl, 2, 'split')


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y) if y.dtype == torch.float32 else y)
        else:                                                           # the PairAlignment of search_explain: a tuple of tensors
            assert len(x) == 5
            same_results(x, y)


@pytest.mark.parametrize('direction', ['i2t', 't2i'])
def test_stores_and_views_through_a_gallery_index(direction):
    """search_topk / search_rerank / search_explain with GalleryIndex(store, side) in the gallery position: exactly what the same
    calls return with the store itself.  The gallery is a whole store, then a StoreView."""
    from aladin_amd import evaluation as E
    si, sc = two_stores()
    for img, cap in ((si, sc), (si.view(slice(0, None, 2)), sc.view(slice(1, None, 2)))):
        side = 'captions' if direction == 'i2t' else 'images'
        gi = E.GalleryIndex(cap if direction == 'i2t' else img, side)
        assert len(gi) == (cap if direction == 'i2t' else img).glob.shape[0]
        with_index = (img, gi) if direction == 'i2t' else (gi, cap)
        for k in (5, 50):
            same_results(E.search_topk(*with_index, k, direction), E.search_topk(img, cap, k, direction))
            same_results(E.search_rerank(*with_index, k, direction), E.search_rerank(img, cap, k, direction))
            same_results(E.search_explain(*with_index, k, direction, top=3), E.search_explain(img, cap, k, direction, top=3))
        same_results(gi.search((img if direction == 'i2t' else cap).glob, 5), E.search_topk(img, cap, 5, direction))
    # an index of plain embeddings: search_topk takes it, the two-stage calls refuse it
    gi = E.GalleryIndex((sc if direction == 'i2t' else si).glob.cpu().numpy(), 'captions' if direction == 'i2t' else 'images')
    with_index = (si, gi) if direction == 'i2t' else (gi, sc)
    same_results(E.search_topk(*with_index, 5, direction), E.search_topk(si, sc, 5, direction))
    with pytest.raises(ValueError, match='built from a store'):
        E.search_rerank(*with_index, 5, direction)
