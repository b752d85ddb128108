"""GPU tier (-m gpu): top-k gallery search straight from the embeddings (ops.search_topk, csrc/search.hip) -- held int for int
and bit for bit to the stored path (ops.sim_matrix + aladin_topk with values) wherever that path can run, to a stable sort of
the stored matrix past aladin_topk's 36864-candidate limit, and to a float64 ranking on well-separated data."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())


def randn(shape, seed):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def stored_topk(sim, k, dim):
    """aladin_topk with values on a stored (n_img, n_cap) matrix: the reference ops.search_topk is held to."""
    from aladin_amd import _lib
    from aladin_amd._ops_common import _ld, _ptr, _stream
    n_q, n_c = (sim.shape[0], sim.shape[1]) if dim == 1 else (sim.shape[1], sim.shape[0])
    q_stride, c_stride = (_ld(sim), 1) if dim == 1 else (1, _ld(sim))
    idx = torch.empty((n_q, k), dtype=torch.int32, device=sim.device)
    val = torch.empty((n_q, k), dtype=torch.float32, device=sim.device)
    _lib.check(_lib.load().aladin_topk(_ptr(sim), q_stride, c_stride, n_q, n_c, k, _ptr(idx), _ptr(val), _stream()), 'topk')
    return idx, val


def bits(v):
    return v.contiguous().view(torch.int32)


def assert_equals_stored(img, cap, k, dim, sim=None):
    from aladin_amd import ops
    sim = ops.sim_matrix(img, cap) if sim is None else sim
    ref_idx, ref_val = stored_topk(sim, k, dim)
    idx, val = ops.search_topk(img, cap, k, dim=dim, return_scores=True)
    n_q = img.shape[0] if dim == 1 else cap.shape[0]
    assert idx.shape == (n_q, k) and idx.dtype == torch.int32 and val.shape == (n_q, k) and val.dtype == torch.float32
    assert torch.equal(idx, ref_idx), (idx != ref_idx).nonzero()[:8].tolist()
    assert torch.equal(bits(val), bits(ref_val))
    assert torch.equal(ops.search_topk(img, cap, k, dim=dim), ref_idx)          # the call without scores: the same indices
    return idx, val, sim


# (n_img, n_cap, D, ks): one tile with ragged edges; 2 x 3 tiles with partial last tiles and a partial last group, at a short and
# at the shipped depth; a gallery smaller than one group (9 items, either direction); fewer groups than k (200 items = 13 groups
# at k = 50, either direction).  k = 256 and k = 50 exceed several of the galleries: the -1 / -inf tail.
STORED_CASES = [
    (37, 53, 30, (1, 50, 256)),
    (300, 1003, 100, (1, 50, 256)),
    (300, 1000, 768, (1, 50)),
    (40, 9, 30, (1, 50)),
    (9, 40, 30, (1, 50)),
    (60, 200, 64, (50, 256)),
    (200, 60, 64, (50, 256)),
]


@pytest.mark.parametrize('dim', [1, 0])
@pytest.mark.parametrize('n_img,n_cap,D,ks', STORED_CASES)
def test_search_equals_the_stored_path_int_for_int(n_img, n_cap, D, ks, dim):
    from aladin_amd import ops
    img, cap = T(randn((n_img, D), 11 + n_img)), T(randn((n_cap, D), 12 + n_cap))
    sim = ops.sim_matrix(img, cap)
    n_g = n_cap if dim == 1 else n_img
    for k in ks:
        idx, val, _ = assert_equals_stored(img, cap, k, dim, sim)
        if k > n_g:                                                     # past the gallery: -1 / -inf, and only there
            assert bool((idx[:, n_g:] == -1).all()) and bool((val[:, n_g:] == float('-inf')).all())
        assert bool((idx[:, :min(k, n_g)] >= 0).all()) and bool((idx[:, :min(k, n_g)] < n_g).all())
        assert bool(torch.isfinite(val[:, :min(k, n_g)]).all())


@pytest.mark.parametrize('dim', [1, 0])
@pytest.mark.parametrize('n_img,n_cap', [(37, 53), (300, 1003)])
def test_padding_never_beats_negative_scores(n_img, n_cap, dim):
    """Every real score is negative; a padded gallery position scores 0 in the accumulators (zero operand rows).  It must count
    as -inf in the group maxima and never reach the output before the gallery is exhausted."""
    from aladin_amd import ops
    D = 32
    img = T(-1.0 + 0.1 * randn((n_img, D), 3))
    cap = T(1.0 + 0.1 * randn((n_cap, D), 4))
    sim = ops.sim_matrix(img, cap)
    assert bool((sim < 0).all())
    n_g = n_cap if dim == 1 else n_img
    for k in (50, 60):
        idx, val, _ = assert_equals_stored(img, cap, k, dim, sim)
        live = min(k, n_g)
        assert bool((idx[:, :live] >= 0).all()) and bool((idx[:, :live] < n_g).all()) and bool((val[:, :live] < 0).all())
        assert bool((idx[:, live:] == -1).all())
        srt = torch.sort(idx[:, :live].long(), dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all())                  # no gallery item twice


@pytest.mark.parametrize('dim', [1, 0])
def test_ties_go_to_the_lower_index(dim):
    """Duplicated gallery rows give bit-equal scores: inside one group of 16, across groups, across the tile boundary (column 384 /
    row 256).  800 gallery rows drawn from 40 distinct vectors: every score of a query occurs ~20 times, all over the gallery.
    Then a gallery of identical rows: every score equal, the answer is 0 .. k-1."""
    from aladin_amd import ops
    n_q, n_g, D, k = 70, 800, 64, 50
    base = randn((40, D), 21)
    which = np.random.RandomState(22).randint(0, 40, size=n_g)
    which[[3, 5, 40, 380, 390, 383, 384, 250, 260, 255, 256]] = [7, 7, 7, 9, 9, 11, 11, 13, 13, 15, 15]
    gallery, queries = base[which], randn((n_q, D), 23)
    img, cap = (T(queries), T(gallery)) if dim == 1 else (T(gallery), T(queries))
    idx, val, sim = assert_equals_stored(img, cap, k, dim)
    ties = val[:, 1:] == val[:, :-1]
    assert int(ties.sum()) > n_q * k // 2                               # the case really is about ties
    assert bool((idx[:, 1:][ties] > idx[:, :-1][ties]).all())           # equal scores: ascending index
    # the final pass's rule alone: equal scores in groups whose selection order is not their index order
    ref = torch.sort(sim if dim == 1 else sim.t().contiguous(), dim=1, descending=True, stable=True)
    assert torch.equal(idx.long(), ref.indices[:, :k])
    gallery = np.repeat(base[:1], n_g, axis=0)
    img, cap = (T(queries), T(gallery)) if dim == 1 else (T(gallery), T(queries))
    for kk in (50, 256):
        idx, val, _ = assert_equals_stored(img, cap, kk, dim)
        assert torch.equal(idx, torch.arange(kk, dtype=torch.int32, device=idx.device).expand(n_q, kk))
        assert bool((val == val[:, :1]).all())


@pytest.mark.parametrize('dim', [1, 0])
def test_gallery_past_the_stored_limit(dim):
    """40000 gallery items: aladin_topk stages a query's scores in LDS and refuses more than 36864, so the reference is a stable
    descending sort of the stored matrix (equal scores keep their index order, as in the top-k kernels)."""
    from aladin_amd import ops
    n_q, n_g, D, k = 70, 40000, 64, 50
    queries, gallery = T(randn((n_q, D), 31)), T(randn((n_g, D), 32))
    img, cap = (queries, gallery) if dim == 1 else (gallery, queries)
    sim = ops.sim_matrix(img, cap)
    with pytest.raises(RuntimeError, match='36864'):
        ops.topk_indices(sim, k, dim=dim)                               # what the stored path cannot do
    idx, val = ops.search_topk(img, cap, k, dim=dim, return_scores=True)
    ref = torch.sort(sim if dim == 1 else sim.t().contiguous(), dim=1, descending=True, stable=True)
    assert torch.equal(idx.long(), ref.indices[:, :k])
    assert torch.equal(bits(val), bits(ref.values[:, :k]))


SEPARATED = dict(n_img=200, D=64, seed=2024, sigma=2.0, k=10)


def separated_problem():
    """COCO-protocol rows at a small size and their float64 ranking: 200 distinct images query 1000 captions.
    Returns (img, cap, order, decided, ordered): order = float64 descending stable ranking; decided = queries whose k-th and
    (k+1)-th float64 scores differ by more than 1e-5; ordered = those whose first k + 1 scores all differ by more than that."""
    from aladin_amd import synth
    p = SEPARATED
    img_rows, cap = synth.retrieval_embeddings(p['n_img'], p['D'], p['seed'], sigma=p['sigma'])
    img = img_rows[0::5]
    S = img.astype(np.float64) @ cap.astype(np.float64).T
    order = np.argsort(-S, axis=1, kind='stable')
    top = np.take_along_axis(S, order[:, :p['k'] + 1], axis=1)
    gaps = top[:, :-1] - top[:, 1:]
    return img, cap, order, gaps[:, -1] > 1e-5, (gaps > 1e-5).all(axis=1)


def test_search_equals_a_float64_ranking_on_separated_data():
    """An independent check: numpy float64, no kernel of this library.  The split-fp16 chain carries ~2^-21 relative operand
    error, ~1e-6 absolute on unit-norm rows, so a ranking decided by more than 1e-5 in float64 must come out the same.
    Queries left out (k-th and (k+1)-th float64 scores within 1e-5): 0 of 200 at this seed (computed without a GPU by
    tests/test_search_cpu.py, which holds the cap of 5 %)."""
    from aladin_amd import ops
    k = SEPARATED['k']
    img, cap, order, decided, ordered = separated_problem()
    left_out = int((~decided).sum())
    print('float64 ranking: %d of %d queries left out (gap <= 1e-5), %d more not order-checked' % (left_out, len(decided), int((decided & ~ordered).sum())))
    assert left_out <= 0.05 * len(decided)
    idx = ops.search_topk(T(img), T(cap), k, dim=1).cpu().numpy()
    want = order[:, :k]
    assert np.array_equal(np.sort(idx[decided], axis=1), np.sort(want[decided], axis=1))        # the k best, as a set
    assert np.array_equal(idx[ordered], want[ordered])                                           # and in order where float64 decides the order
    # captions query the images (dim = 0): the transposed problem on the same rows
    S = cap.astype(np.float64) @ img.astype(np.float64).T
    order0 = np.argsort(-S, axis=1, kind='stable')
    top = np.take_along_axis(S, order0[:, :k + 1], axis=1)
    ok0 = ((top[:, :-1] - top[:, 1:]) > 1e-5).all(axis=1)
    assert (~ok0).sum() <= 0.05 * len(ok0)
    idx0 = ops.search_topk(T(img), T(cap), k, dim=0).cpu().numpy()
    assert np.array_equal(idx0[ok0], order0[:, :k][ok0])


def test_evaluation_search_topk_directions():
    """evaluation.search_topk: 'i2t' = images query captions, 't2i' = captions query images; numpy inputs are accepted."""
    from aladin_amd import evaluation, ops
    img, cap = randn((37, 30), 41), randn((53, 30), 42)
    for direction, dim in (('i2t', 1), ('t2i', 0)):
        idx, val = evaluation.search_topk(img, cap, k=5, direction=direction)
        ref_idx, ref_val = ops.search_topk(T(img), T(cap), 5, dim=dim, return_scores=True)
        assert torch.equal(idx, ref_idx) and torch.equal(bits(val), bits(ref_val))
    with pytest.raises(ValueError):
        evaluation.search_topk(img, cap, direction='both')


def test_python_limits_raise_value_error():
    from aladin_amd import ops
    img, cap = T(randn((8, 16), 1)), T(randn((9, 16), 2))
    for bad_k in (0, 257):
        with pytest.raises(ValueError):
            ops.search_topk(img, cap, bad_k)
    with pytest.raises(ValueError):
        ops.search_topk(img, cap, 5, dim=2)
    with pytest.raises(ValueError):
        ops.search_topk(img, cap[:, :8], 5)


@pytest.mark.parametrize('dim', [1, 0])
def test_search_under_graph_capture(dim):
    """No allocation, no synchronisation, no host-side decision in the call: captured once, replayed on new data of the same
    shape, equal to the eager result."""
    from aladin_amd import ops
    n_img, n_cap, D, k = 300, 1003, 100, 50
    img, cap = T(randn((n_img, D), 51)), T(randn((n_cap, D), 52))
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        ops.search_topk(img, cap, k, dim=dim, return_scores=True)       # warm-up outside the capture (one-time kernel attributes)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_idx, g_val = ops.search_topk(img, cap, k, dim=dim, return_scores=True)
    img.copy_(T(randn((n_img, D), 53)))
    cap.copy_(T(3.0 * randn((n_cap, D), 54)))                           # another magnitude: another power-of-two scale
    graph.replay()
    torch.cuda.synchronize()
    idx, val = ops.search_topk(img, cap, k, dim=dim, return_scores=True)
    assert torch.equal(g_idx, idx) and torch.equal(bits(g_val), bits(val))
    assert_equals_stored(img, cap, k, dim)
