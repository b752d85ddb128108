"""GPU tier (-m gpu): nDCG evaluation -- aladin_ndcg (csrc/ndcg.hip) through ops.ndcg_from_ranking, the aladin_amd.dcg scorer,
evaluation.search_ndcg and i2t / t2i with a scorer.

Tolerance, derived rather than chosen (tests/helpers/ndcg_numpy.py: ndcg_bound): device exp2f and glibc's float32 power are each
within 1 ulp of 2^rel in [1, 2], so two gains differ by at most 2 * 2^-23; everything else is double.  For a query with ideal DCG
`best` at k counted positions   |d ndcg| <= 2 * (2 * 2^-23) * sum_{r<k} 1 / log2(r + 2) / best   -- 3.9e-6 for k = 25, best >= 1.
The bound is computed per query from the restatement's own `best`, with no extra factor; queries whose relevances are all zero
must give exactly 0.0.  Every comparison prints its worst |error| / bound ratio (DESIGN section 4.4.4 records it)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import ndcg_numpy as N                   # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ['image', 'sentence']
METHODS = ['rougeL', 'spice']


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())


def I(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev())


def bits(v):
    return v.contiguous().view(torch.int64)


def assert_within_bound(got, want, best, k, what):
    """|got - want| <= ndcg_bound(best, k) per query, exactly 0 where best == 0."""
    got, want, best = (np.asarray(v, np.float64).reshape(-1) for v in (got, want, best))
    bound = N.ndcg_bound(best, k)
    err = np.abs(got - want)
    assert (got[best == 0] == 0).all(), what
    ratio = float((err[best > 0] / bound[best > 0]).max()) if (best > 0).any() else 0.0
    print('ndcg %-44s worst |err| %.3g  worst err / bound %.4f' % (what, err.max(), ratio))
    assert (err <= bound).all(), (what, float(err.max()), ratio)
    return ratio


def relevance_rows(n_q, n_c, seed, sparse=False):
    """float32 relevances in [0, 0.6] with one exact 1.0 per row (ideal DCG >= 1); sparse: ~70 % zeros, values in steps of 1/50."""
    rng = np.random.RandomState(seed)
    r = 0.6 * rng.random_sample((n_q, n_c))
    if sparse:
        r = np.round(r * 50) / 50
        r[rng.random_sample((n_q, n_c)) < 0.7] = 0
    r = r.astype(np.float32)
    r[np.arange(n_q), rng.randint(0, n_c, n_q)] = 1.0
    return r


def random_lists(n_q, n_c, rank, seed):
    """(n_q, rank) int32: the head of a random permutation of the gallery per query, -1 past the gallery size."""
    rng = np.random.RandomState(seed)
    out = np.full((n_q, rank), -1, np.int32)
    for q in range(n_q):
        out[q, :min(rank, n_c)] = rng.permutation(n_c)[:rank]
    return out


def fixture_cases(g):
    return [(ci, int(npts), int(fold), KINDS[int(kind)], int(rank), g['list_%d' % ci], g['expect_%d' % ci])
            for ci, (npts, fold, kind, rank) in enumerate(g['cases'])]


def fixture_block(r, npts, fold):
    return r[5 * npts * fold:5 * npts * (fold + 1), npts * fold:npts * (fold + 1)]


# ------------------------------------------------------------------------------------------------
# the reference's recorded values
# ------------------------------------------------------------------------------------------------
def test_fixture_windows_through_the_op_on_the_whole_matrix():
    """Every window of tests/golden/ndcg_small.npz against the reference's values: the window is a view of the whole (300 x 60)
    device matrix (padded leading dimension, offset base), queries along its rows ('image', dim=1) or its columns ('sentence',
    dim=0, read in place)."""
    from aladin_amd import ops
    g = load_golden('ndcg_small')
    whole = {m: T(g['rel_' + m]) for m in METHODS}
    for ci, npts, fold, kind, rank, lists, expect in fixture_cases(g):
        for mi, m in enumerate(METHODS):
            view = fixture_block(whole[m], npts, fold)
            assert not view.is_contiguous() or npts == 60
            got = ops.ndcg_from_ranking(view, I(lists), dim=1 if kind == 'image' else 0, rank=rank)
            assert got.dtype == torch.float64 and got.shape == (lists.shape[0],)
            win = fixture_block(g['rel_' + m], npts, fold)
            _, _, best = N.ndcg_table(win, lists, dim=1 if kind == 'image' else 0, rank=rank)
            assert_within_bound(got.cpu().numpy(), expect[:, mi], best, min(rank, view.shape[1 if kind == 'image' else 0]),
                                'fixture case %d %s %s' % (ci, kind, m))


def test_fixture_windows_through_the_scorer():
    """DCG.compute_ndcg_batch on every window, DCG.compute_ndcg on a handful of single queries, against the reference's values; the
    scorer's second call (kept ideal DCG, IDEAL_GIVEN path) against its first: bit-equal."""
    from aladin_amd import dcg as D
    g = load_golden('ndcg_small')
    scorers = {}
    for ci, npts, fold, kind, rank, lists, expect in fixture_cases(g):
        sc = scorers.setdefault(rank, D.DCG(None, 300, 'test', rank=rank, relevance_methods=METHODS,
                                            relevances=[g['rel_' + m] for m in METHODS]))
        first = sc.compute_ndcg_batch(npts, I(lists), fold_index=fold, retrieval=kind)
        assert (0, npts, fold, kind) in sc._ideals and (1, npts, fold, kind) in sc._ideals
        second = sc.compute_ndcg_batch(npts, lists, fold_index=fold, retrieval=kind)          # a numpy table: uploaded by the scorer
        dim = 1 if kind == 'image' else 0
        for mi, m in enumerate(METHODS):
            win = fixture_block(g['rel_' + m], npts, fold)
            _, _, best = N.ndcg_table(win, lists, dim=dim, rank=rank)
            k = min(rank, win.shape[dim])
            assert_within_bound(first[m].cpu().numpy(), expect[:, mi], best, k, 'scorer case %d %s %s' % (ci, kind, m))
            assert torch.equal(bits(first[m]), bits(second[m])), (ci, m)
        for q in (0, 7 if kind == 'sentence' else 37, lists.shape[0] - 1):                    # 7 / 35..39: the zeroed image and its captions
            single = sc.compute_ndcg(npts, q, [int(v) for v in lists[q] if v >= 0], fold_index=fold, retrieval=kind)
            for mi, m in enumerate(METHODS):
                win = fixture_block(g['rel_' + m], npts, fold)
                row = win[q] if kind == 'image' else win[:, q]
                best = N.ndcg_parts(row, lists[q], rank)[2]
                assert_within_bound([single[m]], [expect[q, mi]], [best], min(rank, len(row)), 'single case %d q %d %s' % (ci, q, m))
                assert single[m] == float(first[m][q].item())                                 # one query or all: the same bits
    scorers[25].clear()
    assert not scorers[25]._windows and not scorers[25]._ideals


def test_module_level_functions():
    from aladin_amd import dcg as D
    rel = relevance_rows(1, 40, 5)[0]
    lst = random_lists(1, 40, 25, 6)[0]
    nd, dc, best = N.ndcg_parts(rel, lst)
    assert_within_bound([D.ndcg_from_ranking(rel, lst)], [nd], [best], 25, 'module ndcg_from_ranking')
    assert abs(D.dcg_from_ranking(list(rel), list(lst)) - dc) <= 2 * N.GAIN_ULP * float(np.sum(1 / np.log2(np.arange(25) + 2)))
    assert D.ndcg_from_ranking([5, 3, 2], [0, 1, 2]) == 1.0 and D.ndcg_from_ranking([0, 0, 0], [0, 1]) == 0.0


# ------------------------------------------------------------------------------------------------
# layouts and paths: bit-equal
# ------------------------------------------------------------------------------------------------
def test_layouts_and_the_ideal_given_path_are_bit_equal():
    """dim=0 on a matrix against dim=1 on its contiguous transpose, a padded leading dimension against a compact one (relevances
    and ranking table), the IDEAL_GIVEN path against the fused one, and run to run: all outputs bit-equal."""
    from aladin_amd import ops
    n_q, n_c, rank = 37, 300, 25
    rel = relevance_rows(n_q, n_c, 11, sparse=True)
    lists = random_lists(n_q, n_c, rank, 12)
    base = ops.ndcg_from_ranking(T(rel), I(lists), return_parts=True)
    want = N.ndcg_table(rel, lists)
    assert_within_bound(base[0].cpu().numpy(), want[0], want[2], rank, 'compact rows')
    padded = torch.zeros((n_q, n_c + 13), device=dev())
    padded[:, :n_c] = T(rel)
    padded_t = torch.zeros((n_c, n_q + 5), device=dev())
    padded_t[:, :n_q] = T(rel.T)
    wide = torch.full((n_q, rank + 7), 3, dtype=torch.int32, device=dev())
    wide[:, :rank] = I(lists)
    variants = {'transposed, dim=0': ops.ndcg_from_ranking(T(rel.T), I(lists), dim=0, return_parts=True),
                'padded rows': ops.ndcg_from_ranking(padded[:, :n_c], I(lists), return_parts=True),
                'padded columns, dim=0': ops.ndcg_from_ranking(padded_t[:, :n_q], I(lists), dim=0, return_parts=True),
                'wide table': ops.ndcg_from_ranking(T(rel), wide, rank=rank, return_parts=True),
                'table column view': ops.ndcg_from_ranking(T(rel), wide[:, :rank], return_parts=True),
                'again': ops.ndcg_from_ranking(T(rel), I(lists), return_parts=True)}
    for name, got in variants.items():
        for a, b, part in zip(got, base, ('ndcg', 'dcg', 'ideal')):
            assert torch.equal(bits(a), bits(b)), (name, part)
    for dim, r in ((1, T(rel)), (0, T(rel.T))):
        given = ops.ndcg_from_ranking(r, I(lists), dim=dim, ideal=base[2], return_parts=True)
        assert torch.equal(bits(given[0]), bits(base[0])) and torch.equal(bits(given[1]), bits(base[1])), dim
        assert given[2].data_ptr() == base[2].data_ptr()
        alone = ops.ndcg_from_ranking(r, I(lists), dim=dim, ideal=base[2].clone())
        assert torch.equal(bits(alone), bits(base[0]))


def test_the_ideal_order_scores_exactly_one():
    """A ranking that lists the k largest relevances in descending order: ndcg == 1.0 exactly (both sums add the same terms in the
    same order), whatever the ties; dcg and ideal are the same bits."""
    from aladin_amd import ops
    for n_c, rank, sparse in ((30, 25, False), (30, 40, True), (300, 25, True), (1000, 100, True), (257, 257, False)):
        rel = relevance_rows(9, n_c, 100 + n_c, sparse)
        order = np.argsort(-rel, axis=1, kind='stable')[:, :rank]
        lists = np.full((9, rank), -1, np.int32)
        lists[:, :order.shape[1]] = order
        nd, dc, best = ops.ndcg_from_ranking(T(rel), I(lists), return_parts=True)
        assert (nd == 1.0).all(), (n_c, rank, nd.tolist())
        assert torch.equal(bits(dc), bits(best))
        want = N.ndcg_table(rel, lists)
        assert (want[0] == 1.0).all()
        s = float(np.sum(1 / np.log2(np.arange(min(rank, n_c)) + 2)))
        assert np.abs(best.cpu().numpy() - want[2]).max() <= 2 * N.GAIN_ULP * s


# ------------------------------------------------------------------------------------------------
# edges against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_c', [1, 255, 256, 257, 36864])
def test_gallery_sizes_around_the_ownership_stride_and_at_the_limit(n_c):
    """A thread owns the positions c = tid mod 256: 255 / 256 / 257 bracket that edge; 36864 fills the LDS (one query)."""
    from aladin_amd import ops
    n_q = 1 if n_c == 36864 else 5
    rel = relevance_rows(n_q, n_c, 200 + n_c, sparse=n_c == 257)
    for rank in (1, 25):
        lists = random_lists(n_q, n_c, rank, 300 + n_c)
        for dim, r in ((1, T(rel)), (0, T(rel.T))):
            got = ops.ndcg_from_ranking(r, I(lists), dim=dim, return_parts=True)
            want = N.ndcg_table(rel, lists)
            k = min(rank, n_c)
            assert_within_bound(got[0].cpu().numpy(), want[0], want[2], k, 'n_c %d rank %d dim %d' % (n_c, rank, dim))
            s = float(np.sum(1 / np.log2(np.arange(k) + 2)))
            assert np.abs(got[1].cpu().numpy() - want[1]).max() <= 2 * N.GAIN_ULP * s                # dcg, ideal: 2 ulp per gain
            assert np.abs(got[2].cpu().numpy() - want[2]).max() <= 2 * N.GAIN_ULP * s


def test_the_gallery_limit_is_gone_with_the_ideal_given():
    from aladin_amd import ops
    n_c = 40000
    rel = relevance_rows(2, n_c, 17)
    lists = random_lists(2, n_c, 25, 18)
    with pytest.raises(ValueError, match='36864'):
        ops.ndcg_from_ranking(T(rel), I(lists))
    want = N.ndcg_table(rel, lists)
    for dim, r in ((1, T(rel)), (0, T(rel.T))):
        got = ops.ndcg_from_ranking(r, I(lists), dim=dim, ideal=torch.from_numpy(want[2]).to(dev()), return_parts=True)
        assert_within_bound(got[0].cpu().numpy(), want[0], want[2], 25, 'ideal given, 40000 items, dim %d' % dim)


def test_rank_past_the_gallery_and_entries_that_are_no_item():
    """rank > n_c counts min(rank, n_c) positions; -1, an all -1 row, entries >= n_c and < -1 add nothing, keep their position's
    discount and are not read: the result is bit-equal to the row with them replaced by -1 (the relevance buffer ends with the
    matrix, so an entry that were dereferenced would read past it)."""
    from aladin_amd import ops
    n_q, n_c, rank = 6, 30, 40
    rel = relevance_rows(n_q, n_c, 21)
    lists = random_lists(n_q, n_c, rank, 22)
    assert (lists[:, 30:] == -1).all()
    lists[2] = -1                                                          # nothing retrieved: dcg 0, ndcg 0, ideal > 0
    lists[3, [0, 5, 9]] = -1
    clean = lists.copy()
    lists[4, [1, 2, 3, 4]] = [n_c, n_c + 1000, -2, np.iinfo(np.int32).min]
    lists[5, [0, 29]] = [np.iinfo(np.int32).max, 2 ** 20]
    clean[4, [1, 2, 3, 4]] = -1
    clean[5, [0, 29]] = -1
    for dim, r in ((1, T(rel)), (0, T(rel.T))):
        got = ops.ndcg_from_ranking(r, I(lists), dim=dim, return_parts=True)
        ref = ops.ndcg_from_ranking(r, I(clean), dim=dim, return_parts=True)
        given = ops.ndcg_from_ranking(r, I(lists), dim=dim, ideal=ref[2], return_parts=True)
        for a, b, c in zip(got, ref, given):
            assert torch.equal(bits(a), bits(b)) and torch.equal(bits(c), bits(b))
        want = N.ndcg_table(rel, lists)
        assert_within_bound(got[0].cpu().numpy(), want[0], want[2], n_c, 'no-item entries dim %d' % dim)
        assert got[0][2].item() == 0.0 and got[1][2].item() == 0.0 and got[2][2].item() >= 1.0
    short = ops.ndcg_from_ranking(T(rel), I(lists[:, :30]), return_parts=True)             # rank 30 == gallery: the same k
    full = ops.ndcg_from_ranking(T(rel), I(lists), return_parts=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(short, full))


def test_thirty_maximal_relevances_retire_and_rescan():
    """30 relevances equal to the maximum, rank 25: every selection round retires one of them and its owner rescans (several
    share an owner: positions 256 apart); the ideal is sum gain(max) / discount."""
    from aladin_amd import ops
    n_c, rank = 700, 25
    rel = relevance_rows(3, n_c, 31, sparse=True)
    rel[rel >= 0.9] = 0.5
    top = np.float32(0.9)
    pos = np.concatenate([np.arange(3, 700, 256), np.arange(10, 37)])     # 3, 259, 515 share thread 3
    assert len(pos) == 30
    rel[:, pos] = top
    lists = random_lists(3, n_c, rank, 32)
    got = ops.ndcg_from_ranking(T(rel), I(lists), return_parts=True)
    want = N.ndcg_table(rel, lists)
    s = float(np.sum(1 / np.log2(np.arange(rank) + 2)))
    ideal = float(np.sum(np.float64(2 ** top - 1) / np.log2(np.arange(rank) + 2)))
    assert np.abs(got[2].cpu().numpy() - ideal).max() <= 2 * N.GAIN_ULP * s
    assert_within_bound(got[0].cpu().numpy(), want[0], want[2], rank, '30 maximal relevances')
    assert torch.equal(bits(got[2][0]), bits(got[2][1])) and torch.equal(bits(got[2][0]), bits(got[2][2]))


def test_graph_capture_and_replay_on_new_data():
    from aladin_amd import ops
    n_q, n_c, rank = 20, 300, 25
    rel_t, list_t = T(relevance_rows(n_q, n_c, 41)), I(random_lists(n_q, n_c, rank, 42))
    rel_tt = rel_t.t().contiguous()                                       # the same relevances, queries along the columns
    ideal_t = torch.zeros(n_q, dtype=torch.float64, device=dev())
    out = {}

    def run():
        out['fused'] = ops.ndcg_from_ranking(rel_t, list_t, return_parts=True)
        out['cols'] = ops.ndcg_from_ranking(rel_tt, list_t, dim=0)
        out['given'] = ops.ndcg_from_ranking(rel_t, list_t, ideal=ideal_t)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run()                                                             # warm-up outside the capture (one-time kernel attributes)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    rel2, list2 = relevance_rows(n_q, n_c, 43, sparse=True), random_lists(n_q, n_c, rank, 44)
    rel_t.copy_(T(rel2))
    rel_tt.copy_(T(rel2.T))
    list_t.copy_(I(list2))
    want = N.ndcg_table(rel2, list2)
    ideal_t.copy_(torch.from_numpy(want[2]).to(dev()))
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: ([t.clone() for t in v] if isinstance(v, tuple) else v.clone()) for k, v in out.items()}
    run()
    torch.cuda.synchronize()
    for a, b in zip(replayed['fused'], out['fused']):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(replayed['cols']), bits(out['cols'])) and torch.equal(bits(replayed['given']), bits(out['given']))
    assert_within_bound(replayed['fused'][0].cpu().numpy(), want[0], want[2], rank, 'graph replay, fused')
    assert_within_bound(replayed['given'].cpu().numpy(), want[0], want[2], rank, 'graph replay, ideal given')
    assert torch.equal(bits(replayed['cols']), bits(replayed['fused'][0]))


# ------------------------------------------------------------------------------------------------
# evaluation surface
# ------------------------------------------------------------------------------------------------
def _eval_relevances(n_img, seed):
    """(5 n_img, n_img) rows = captions, columns = images; 1.0 for own pairs."""
    a, b = relevance_rows(5 * n_img, n_img, seed), relevance_rows(5 * n_img, n_img, seed + 1, sparse=True)
    for r in (a, b):
        r[r == 1.0] = 0.5
        r[np.arange(5 * n_img), np.arange(5 * n_img) // 5] = 1.0
    return [a, b]


@pytest.mark.parametrize('sim_function', [None, 'alignment'])
def test_i2t_t2i_with_a_scorer(sim_function):
    """40 images x 200 captions: the two means equal the restatement applied to ops.topk_indices of the same grid, within the
    bound (a mean of per-query values within their bounds is within the mean bound); the first five entries of the tuple and
    return_ranks are unchanged from the call without a scorer; one method leaves the second entry 0."""
    from aladin_amd import dcg as D
    from aladin_amd import evaluation as E
    from aladin_amd import ops, synth
    n_img = 40
    images, captions, il, cl = synth.eval_sets(n_img, 64, 57)
    images, captions = T(images), T(captions)
    rels = _eval_relevances(n_img, 58)
    sc = D.DCG(None, 5 * n_img, 'test', rank=25, relevance_methods=METHODS, relevances=rels)
    sim = E._eval_scores(images, captions, il, cl, 'dot', sim_function)
    assert tuple(sim.shape) == (n_img, 5 * n_img)
    for fn, direction, dim in ((E.i2t, 'i2t', 1), (E.t2i, 't2i', 0)):
        plain, (r0, t0) = fn(images, captions, il, cl, return_ranks=True, sim_function=sim_function)
        for _ in range(2):                                                # the second call runs on the kept ideal DCG: the same numbers
            m, (r1, t1) = fn(images, captions, il, cl, return_ranks=True, ndcg_scorer=sc, sim_function=sim_function)
            assert plain[5:] == (0, 0) and m[:5] == plain[:5]
            np.testing.assert_array_equal(r1, r0)
            np.testing.assert_array_equal(t1, t0)
            top = ops.topk_indices(sim, 25, dim=dim).cpu().numpy()
            for mi in range(2):
                nd, _, best = N.ndcg_table(rels[mi], top, dim=1 - dim)       # 'i2t': the images are the COLUMNS of the relevances
                assert best.min() >= 1.0
                assert abs(m[5 + mi] - nd.mean()) <= N.ndcg_bound(best, 25).mean(), (direction, mi, m[5 + mi], nd.mean())
                assert 0.05 < m[5 + mi] < 1.0
        assert fn(images, captions, il, cl, ndcg_scorer=sc, sim_function=sim_function) == m
        one = D.DCG(None, 5 * n_img, 'test', relevance_methods=['spice'], relevances=rels[1:])
        m1 = fn(images, captions, il, cl, ndcg_scorer=one, sim_function=sim_function)
        assert m1[5] == m[6] and m1[6] == 0 and m1[:5] == plain[:5]
    E.clear_eval_cache()


def test_search_ndcg_grades_search_topk_and_search_rerank():
    """search_ndcg on the tables search_topk and search_rerank return (8 images x 40 captions in stores, k past the gallery in one
    direction) against the restatement on those same lists."""
    import test_rerank_gpu as G
    from aladin_amd import dcg as D
    from aladin_amd import evaluation as E
    n_img = 8
    images, il = G.make_sets([G.IMG_COUNTS[k % 10] for k in range(n_img)], 0, 64, 61)
    captions, cl = G.make_sets([G.CAP_COUNTS[k % 10] for k in range(5 * n_img)], 2, 64, 62)
    si, sc = G.fill_store(images, il, 0, 'split'), G.fill_store(captions, cl, 2, 'split')
    rels = _eval_relevances(n_img, 63)
    scorer = D.DCG(None, 5 * n_img, 'test', rank=25, relevance_methods=METHODS, relevances=rels)
    for direction, k, dim in (('i2t', 10, 0), ('i2t', 30, 0), ('t2i', 5, 1), ('t2i', 12, 1)):
        for name, (idx, _) in (('search_topk', E.search_topk(si, sc, k, direction)), ('search_rerank', E.search_rerank(si, sc, k, direction))):
            got = E.search_ndcg(idx, scorer, direction)
            assert list(got) == METHODS
            lists = idx.cpu().numpy()
            counted = min(k, 25)
            for mi, m in enumerate(METHODS):
                want = N.ndcg_table(rels[mi], lists, dim=dim, rank=counted)
                assert got[m].shape == (lists.shape[0],) and got[m].dtype == torch.float64
                assert_within_bound(got[m].cpu().numpy(), want[0], want[2], min(counted, rels[mi].shape[dim]),
                                    '%s %s k %d %s' % (name, direction, k, m))
    assert len(scorer._windows) == 2
