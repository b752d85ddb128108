"""GPU tier (-m gpu): two-stage retrieval -- alignment-head scores of listed pairs straight from two stores
(store.alignment_scores_for_pairs, csrc/rescore.hip) and the ordered re-scored shortlist (evaluation.search_rerank).
Values are held to the float64 oracle on the padded-71 sets with the project's tolerances (split: rtol 2e-6, atol 3e-6,
tests/test_gpu_parity.py; fp16: 1e-3 |ref| + 3e-4 max |ref| for D >= 64; atol 2e-3 at toy widths), orders to
stable sorts, and a pair's bits to the pair alone."""
import functools

import numpy as np
import pytest
import torch

import alad_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

L = 71
IMG_COUNTS = [1, 15, 16, 17, 32, 33, 48, 49, 50, 70]          # the edges of the 16-row region tiles; 70 fills the padded set
CAP_COUNTS = [0, 1, 8, 9, 16, 17, 35, 40, 41, 68]             # ... of the 8-row pieces and 16-word tiles; 0: no scored word


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())


def bits(v):
    return v.contiguous().view(torch.int32)


def make_sets(counts, tail, D, seed):
    """(N, 71, D) zero-padded sets whose samples have the given scored-position counts (length = count + 1 + tail)."""
    rng = np.random.RandomState(seed)
    lens = [int(c) + 1 + tail for c in counts]
    sets = np.zeros((len(counts), L, D), np.float32)
    for k, n in enumerate(lens):
        sets[k, :n] = rng.standard_normal((n, D))
    return sets, lens


def fill_store(sets, lens, tail, precision, batch=7, capacity_rows=64):
    from aladin_amd.store import PackedSetStore
    st = PackedSetStore(sets.shape[2], tail, dev(), capacity_rows=capacity_rows, precision=precision)
    for k0 in range(0, sets.shape[0], batch):
        k1 = min(sets.shape[0], k0 + batch)
        st.append(T(sets[k0:k1, :max(lens[k0:k1])]), lens[k0:k1])
    return st


def assert_close(got, ref, precision, D, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if precision == 'split':
        err, tol = np.abs(got - ref), 3e-6 + 2e-6 * np.abs(ref)
    elif D >= 64:
        err, tol = np.abs(got - ref), 1e-3 * np.abs(ref) + 3e-4 * (np.abs(ref).max() if scale is None else scale)
    else:
        err, tol = np.abs(got - ref), np.full(ref.shape, 2e-3)
    print('max err %.3g, max err / tol %.3g (%s, D=%d)' % (err.max(initial=0), (err / tol).max(initial=0), precision, D))
    assert (err <= tol).all(), (float(err.max()), np.argwhere(err > tol)[:8].tolist())


def pair_reference(ref_grid, cand, direction):
    """The oracle grid's entries of the listed pairs, -inf where there is no candidate."""
    cand = np.asarray(cand)
    q = np.arange(cand.shape[0])[:, None]
    c = np.where(cand < 0, 0, cand)
    vals = ref_grid[q, c] if direction == 'i2t' else ref_grid[c, q]
    return np.where(cand < 0, -np.inf, vals)


def random_shortlist(n_q, n_g, k, seed):
    """Random candidates with repeats inside a row, some -1 entries and one row of nothing but -1."""
    rng = np.random.RandomState(seed)
    cand = rng.randint(0, n_g, (n_q, k)).astype(np.int32)
    cand[rng.random_sample(cand.shape) < 0.08] = -1
    cand[n_q // 2] = -1
    if k > 1:
        cand[0, 1] = cand[0, 0] = abs(int(cand[0, 0]))        # a repeat for certain
    return cand


@functools.lru_cache(maxsize=None)
def edge_problem(precision, D, n_img=23, n_cap=27):
    """Stores whose samples sit on the tile edges + the float64 oracle grid, built once per (precision, D)."""
    rng = np.random.RandomState(D)
    ic = [IMG_COUNTS[k % len(IMG_COUNTS)] for k in range(n_img)]
    cc = [CAP_COUNTS[k % len(CAP_COUNTS)] for k in rng.permutation(n_cap)]
    images, il = make_sets(ic, 0, D, 100 + D)
    captions, cl = make_sets(cc, 2, D, 200 + D)
    ref = O.alignment_scores(images, captions, il, cl, dtype=np.float64)          # on the padded-71 sets, like the reference
    ref.setflags(write=False)
    return fill_store(images, il, 0, precision), fill_store(captions, cl, 2, precision), ref, cc


@pytest.mark.parametrize('k', [1, 7, 50, 256])
@pytest.mark.parametrize('D', [64, 100])
@pytest.mark.parametrize('direction', ['i2t', 't2i'])
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_pair_scores_vs_oracle(precision, direction, D, k):
    from aladin_amd.store import alignment_scores_for_pairs
    si, sc, ref, cc = edge_problem(precision, D)
    n_q, n_g = (len(si), len(sc)) if direction == 'i2t' else (len(sc), len(si))
    cand = random_shortlist(n_q, n_g, k, 7 * k + D)
    got = alignment_scores_for_pairs(si, sc, torch.from_numpy(cand).to(dev()), direction)
    assert got.shape == (n_q, k) and got.dtype == torch.float32
    got = got.cpu().numpy()
    want = pair_reference(ref, cand, direction)
    assert np.array_equal(np.isneginf(got), cand < 0)                     # -inf exactly at the -1 slots
    assert_close(got[cand >= 0], want[cand >= 0], precision, D, scale=np.abs(ref).max())
    empty = np.array(cc) == 0                                             # the caption without a scored word: exactly 0.0
    if direction == 'i2t':
        hit = (cand >= 0) & empty[np.where(cand < 0, 0, cand)]
    else:
        hit = (cand >= 0) & empty[:, None]
    assert (got[hit] == 0.0).all() and (k < 50 or hit.any())


@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_pair_scores_vs_oracle_at_the_shipped_depth(precision):
    """D = 768: twelve (fp16) / thirty-six (split) K steps through the double buffer, on a 12 x 20 sub-case."""
    from aladin_amd.store import alignment_scores_for_pairs
    si, sc, ref, _ = edge_problem(precision, 768, 12, 20)
    for direction, n_q, n_g in (('i2t', 12, 20), ('t2i', 20, 12)):
        cand = random_shortlist(n_q, n_g, 7, 5)
        got = alignment_scores_for_pairs(si, sc, torch.from_numpy(cand).to(dev()), direction).cpu().numpy()
        want = pair_reference(ref, cand, direction)
        assert np.array_equal(np.isneginf(got), cand < 0)
        assert_close(got[cand >= 0], want[cand >= 0], precision, 768, scale=np.abs(ref).max())


@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_zero_fill_of_short_images_only(precision):
    """The construction of test_trimmed_grid_keeps_the_zero_fill_of_the_longest_image: every region points to -e0 and one word is
    +e0.  An image shorter than the padded set takes the zero fill into that word's max (contribution 0); one that fills the
    set (70 regions) keeps its negative maximum."""
    from aladin_amd.store import alignment_scores_for_pairs
    D = 16
    rng = np.random.default_rng(5)
    il, cl = [33, L, 20], [12, 9, 7]
    images, captions = np.zeros((3, L, D), np.float32), np.zeros((3, L, D), np.float32)
    for i, n in enumerate(il):
        images[i, :n] = rng.standard_normal((n, D))
    for j, n in enumerate(cl):
        captions[j, :n] = rng.standard_normal((n, D))
    images[1, 1:33] = images[0, 1:33]                              # the same regions, then more of them
    images[1, 33:] = images[0, 1:39]
    images[0, :, 0] = np.where(np.arange(L) < 33, -np.abs(images[0, :, 0]) - 3.0, 0)
    images[1, :, 0] = -np.abs(images[1, :, 0]) - 3.0
    captions[0, 2] = 0
    captions[0, 2, 0] = 5.0                                        # word 1 of caption 0 is +e0: every cosine with images 0, 1 < 0
    ref = O.alignment_scores(images, captions, il, cl, dtype=np.float64)
    assert ref[0, 0] > ref[1, 0] + 0.1
    si, sc = fill_store(images, il, 0, precision), fill_store(captions, cl, 2, precision)
    cand = torch.tensor([[0, 1, 2]] * 3, dtype=torch.int32, device=dev())
    got = alignment_scores_for_pairs(si, sc, cand, 'i2t').cpu().numpy()
    assert_close(got, ref, precision, D)
    assert got[0, 0] > got[1, 0] + 0.1
    got_t = alignment_scores_for_pairs(si, sc, cand, 't2i').cpu().numpy()
    assert_close(got_t, ref.T, precision, D)


@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_a_pairs_bits_depend_on_the_pair_only(precision):
    from aladin_amd.store import alignment_scores_for_pairs
    D = 64
    si, sc, ref, _ = edge_problem(precision, D)
    n_img, n_cap = len(si), len(sc)
    rng = np.random.RandomState(11)
    cand = random_shortlist(n_img, n_cap, 50, 3)
    d_cand = torch.from_numpy(cand).to(dev())
    base = alignment_scores_for_pairs(si, sc, d_cand, 'i2t')
    # two runs of the same call
    assert torch.equal(bits(alignment_scores_for_pairs(si, sc, d_cand, 'i2t')), bits(base))
    # permuted columns -> permuted values
    perm = rng.permutation(50)
    got = alignment_scores_for_pairs(si, sc, torch.from_numpy(np.ascontiguousarray(cand[:, perm])).to(dev()), 'i2t')
    assert torch.equal(bits(got), bits(base[:, torch.from_numpy(perm).to(dev())]))
    # k = 1 against the same pair inside the k = 50 row
    for col in (0, 13, 49):
        got = alignment_scores_for_pairs(si, sc, d_cand[:, col:col + 1].contiguous(), 'i2t')
        assert torch.equal(bits(got), bits(base[:, col:col + 1]))
    # i2t against t2i: the full grid listed from either side
    grid_i = torch.arange(n_cap, dtype=torch.int32, device=dev()).repeat(n_img, 1)
    grid_c = torch.arange(n_img, dtype=torch.int32, device=dev()).repeat(n_cap, 1)
    from_i = alignment_scores_for_pairs(si, sc, grid_i, 'i2t')
    from_c = alignment_scores_for_pairs(si, sc, grid_c, 't2i')
    assert torch.equal(bits(from_i), bits(from_c.t()))
    assert_close(from_i.cpu().numpy(), ref, precision, D)
    # views against the same samples in freshly filled stores
    ic = [IMG_COUNTS[k % len(IMG_COUNTS)] for k in range(n_img)]
    images, il = make_sets(ic, 0, D, 100 + D)
    for ids in (list(range(n_img))[0:None:5], [int(v) for v in rng.permutation(n_img)[:9]]):
        view = si.view(slice(0, None, 5)) if ids[:2] == [0, 5] else si.view(ids)
        fresh = fill_store(images[ids], [il[v] for v in ids], 0, precision, batch=4)
        sub = torch.arange(n_cap, dtype=torch.int32, device=dev()).repeat(len(ids), 1)
        want = alignment_scores_for_pairs(fresh, sc, sub, 'i2t')
        assert torch.equal(bits(alignment_scores_for_pairs(view, sc, sub, 'i2t')), bits(want))
        assert torch.equal(bits(want), bits(from_i[torch.tensor(ids, device=dev())]))
        # ... and as the gallery of the captions
        gal = torch.arange(len(ids), dtype=torch.int32, device=dev()).repeat(n_cap, 1)
        assert torch.equal(bits(alignment_scores_for_pairs(view, sc, gal, 't2i')), bits(alignment_scores_for_pairs(fresh, sc, gal, 't2i')))


@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_last_sample_of_an_exactly_full_store(precision):
    """The queried / listed sample is the last one of a store whose allocation ends with its last row, and its count (13 regions,
    11 words) is no multiple of 8 or 16: the rows its 8-row pieces and 16-row tiles would read past it do not exist.  The kernel
    clamps every source row into the sample (rescore_stage), so this reads nothing outside the allocation."""
    from aladin_amd.store import alignment_scores_for_pairs
    D = 64
    ic, cc = [16, 5, 13], [9, 20, 11]
    images, il = make_sets(ic, 0, D, 31)
    captions, cl = make_sets(cc, 2, D, 32)
    ref = O.alignment_scores(images, captions, il, cl, dtype=np.float64)
    si = fill_store(images, il, 0, precision, batch=3, capacity_rows=sum(ic))
    sc = fill_store(captions, cl, 2, precision, batch=3, capacity_rows=sum(cc))
    assert si.rows.shape[0] == si.n_rows == sum(ic) and sc.rows.shape[0] == sc.n_rows == sum(cc)
    cand = torch.tensor([[2, 0, 1, 2]] * 3, dtype=torch.int32, device=dev())
    got = alignment_scores_for_pairs(si, sc, cand, 'i2t').cpu().numpy()
    assert_close(got, ref[:, [2, 0, 1, 2]], precision, D)
    got = alignment_scores_for_pairs(si, sc, cand, 't2i').cpu().numpy()
    assert_close(got, ref.T[:, [2, 0, 1, 2]], precision, D)


def np_stable(cand, val):
    order = np.argsort(-val, axis=1, kind='stable')
    return np.take_along_axis(cand, order, 1), np.take_along_axis(val, order, 1)


def test_search_rerank_is_the_stable_sort_of_the_pair_scores():
    from aladin_amd import evaluation as E
    from aladin_amd.store import alignment_scores_for_pairs
    D, precision = 64, 'split'
    images, il = make_sets([IMG_COUNTS[k % 10] for k in range(13)], 0, D, 41)
    captions, cl = make_sets([CAP_COUNTS[k % 10] for k in range(21)], 2, D, 42)
    si = fill_store(images, il, 0, precision)
    sc = fill_store(np.concatenate([captions, captions]), cl + cl, 2, precision)         # every caption twice: equal scores
    for direction, n_q, n_g in (('i2t', 13, 42), ('t2i', 42, 13)):
        for k in (5, 42, 50):                                                            # k past the gallery: -1 / -inf last
            short, _ = E.search_topk(si, sc, k, direction)
            pair = alignment_scores_for_pairs(si, sc, short, direction)
            idx, val = E.search_rerank(si, sc, k, direction)
            assert idx.shape == (n_q, k) and idx.dtype == torch.int32 and val.dtype == torch.float32
            want_i, want_v = np_stable(short.cpu().numpy(), pair.cpu().numpy())
            np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
            np.testing.assert_array_equal(val.cpu().numpy().view(np.int32), want_v.view(np.int32))
            n_real = min(k, n_g)
            assert (idx[:, :n_real] >= 0).all() and (idx[:, n_real:] == -1).all() and torch.isneginf(val[:, n_real:]).all()
            idx2, val2 = E.search_rerank(si, sc, k, direction, shortlist=short)           # the caller's shortlist: the same
            assert torch.equal(idx2, idx) and torch.equal(bits(val2), bits(val))
    # equal scores: the twin captions j and j + 21 score the same bits; the one in the earlier shortlist slot comes first
    short, _ = E.search_topk(si, sc, 42, 'i2t')
    idx, val = E.search_rerank(si, sc, 42, 'i2t')
    short, idx, val = short.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()
    twins = 0
    for q in range(13):
        slot = {int(c): s for s, c in enumerate(short[q])}
        pos = {int(c): s for s, c in enumerate(idx[q])}
        for j in range(21):
            assert val[q, pos[j]] == val[q, pos[j + 21]]
            first, second = (j, j + 21) if slot[j] < slot[j + 21] else (j + 21, j)
            assert pos[first] < pos[second]
            twins += pos[second] == pos[first] + 1
    assert twins > 13 * 10


def test_search_rerank_reproduces_the_reference_ranks():
    """tests/golden/eval_pipeline.npz (the reference's own i2t / t2i with its alignment head, 50 images x 250 captions): with a
    shortlist that covers the whole gallery the re-ranked order puts every query's ground truth where the reference ranks it, and
    starts with the reference's top-1 -- all queries, exactly (the float64 oracle separates these scores by >= 3.3e-5)."""
    from aladin_amd import synth
    from aladin_amd import evaluation as E
    g = load_golden('eval_pipeline')
    batches = synth.encoder_batches()
    N = int(g['N'])

    class FakeModel:
        logger = None

        def eval(self):
            pass

        def forward_emb(self, example_imgs, example_txts):
            b = batches[int(example_txts[0][0])]
            return (T(b['img_glob']), T(b['cap_glob']), T(b['img_set']), T(b['cap_seq']), list(b['img_len']), list(b['cap_len']), 0)

    class Loader(list):
        dataset = list(range(N))
    loader = Loader([((torch.zeros((len(b['img_len']), 1)),), (torch.full((len(b['img_len']),), k),)) for k, b in enumerate(batches)])
    si, sc, il, cl = E.encode_data_packed(FakeModel(), loader, logging=None, precision='split')
    imgs = si.view(slice(0, None, 5))
    idx, _ = E.search_rerank(imgs, sc, k=250, direction='i2t')
    idx = idx.cpu().numpy()
    assert idx.shape == (50, 250) and all(sorted(row) == list(range(250)) for row in idx.tolist())
    ranks = np.array([min(int(np.where(idx[i] == c)[0][0]) for c in range(5 * i, 5 * i + 5)) for i in range(50)], np.float64)
    np.testing.assert_array_equal(ranks, g['i2t_align_ranks'])
    np.testing.assert_array_equal(idx[:, 0].astype(np.float64), g['i2t_align_top1'])
    idx, _ = E.search_rerank(imgs, sc, k=50, direction='t2i')
    idx = idx.cpu().numpy()
    assert idx.shape == (250, 50) and all(sorted(row) == list(range(50)) for row in idx.tolist())
    ranks = np.array([int(np.where(idx[c] == c // 5)[0][0]) for c in range(250)], np.float64)
    np.testing.assert_array_equal(ranks, g['t2i_align_ranks'])
    np.testing.assert_array_equal(idx[:, 0].astype(np.float64), g['t2i_align_top1'])


SEPARATED_SEED = 31          # chosen on the CPU: every adjacent float64 gap inside every shortlist below is >= 1e-4 (asserted)


@functools.lru_cache(maxsize=None)
def separated_problem():
    """40 queries, a gallery of 300, k = 10 in either direction from synth.eval_sets(300): 300 distinct images (every fifth row)
    and the first 300 captions; the shortlists are the float64 matching-head top-10 (computed here, so the test's pairs do not
    depend on the device) and the float64 oracle scores of their pairs."""
    from aladin_amd import synth
    images, captions, il, cl = synth.eval_sets(300, D=64, seed=SEPARATED_SEED)
    images, il = images[::5], il[::5]
    captions, cl = captions[:300], cl[:300]
    out = {}
    for direction in ('i2t', 't2i'):
        qs, gs = (images[:40, 0], captions[:, 0]) if direction == 'i2t' else (captions[:40, 0], images[:, 0])
        m = qs.astype(np.float64) @ gs.astype(np.float64).T
        short = np.argsort(-m, axis=1, kind='stable')[:, :10].astype(np.int32)
        ref = np.empty((40, 10))
        for q in range(40):
            c = short[q]
            if direction == 'i2t':
                ref[q] = O.alignment_scores(images[q:q + 1], captions[c], il[q:q + 1], [cl[v] for v in c], dtype=np.float64)[0]
            else:
                ref[q] = O.alignment_scores(images[c], captions[q:q + 1], [il[v] for v in c], cl[q:q + 1], dtype=np.float64)[:, 0]
        out[direction] = (short, ref)
    return images, il, captions, cl, out


def separated_gaps():
    *_, out = separated_problem()
    return {d: float(np.min(-np.diff(-np.sort(-ref, axis=1), axis=1))) for d, (short, ref) in out.items()}


@pytest.mark.parametrize('direction', ['i2t', 't2i'])
def test_full_order_on_separated_data(direction):
    from aladin_amd import evaluation as E
    images, il, captions, cl, out = separated_problem()
    short, ref = out[direction]
    gap = np.min(-np.diff(-np.sort(-ref, axis=1), axis=1))
    assert gap >= 1e-4, gap                                               # every query, every adjacent pair of its shortlist
    if direction == 'i2t':
        si, sc = fill_store(images[:40], il[:40], 0, 'split', batch=37), fill_store(captions, cl, 2, 'split', batch=37)
    else:
        si, sc = fill_store(images, il, 0, 'split', batch=37), fill_store(captions[:40], cl[:40], 2, 'split', batch=37)
    idx, val = E.search_rerank(si, sc, 10, direction, shortlist=torch.from_numpy(short).to(dev()))
    want = np.take_along_axis(short, np.argsort(-ref, axis=1, kind='stable'), 1)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert_close(val.cpu().numpy(), -np.sort(-ref, axis=1), 'split', 64)


def test_no_grid_is_allocated():
    """1000 queries x 40 000 gallery items (fp16 stores, 3-6 scored positions per set), k = 50: the grid would be 160 MB and
    ops.topk_indices refuses that gallery; the two-stage call must stay under a quarter of it."""
    from aladin_amd import evaluation as E
    from aladin_amd.store import PackedSetStore
    D, n_q, n_g, k = 64, 1000, 40000, 50
    rng = np.random.RandomState(8)

    def store(n, tail, seed):
        r = np.random.RandomState(seed)
        counts = r.randint(3, 7, n)
        lens = [int(c) + 1 + tail for c in counts]
        Lb = 7 + tail
        sets = r.standard_normal((n, Lb, D)).astype(np.float32)
        sets *= (np.arange(Lb)[None, :] < np.array(lens)[:, None])[:, :, None]
        st = PackedSetStore(D, tail, dev(), capacity_rows=int(counts.sum()), precision='fp16')
        st.append(T(sets), lens)
        return st, sets, lens
    si, images, il = store(n_q, 0, 81)
    sc, captions, cl = store(n_g, 2, 82)
    si.glob, sc.glob                                                      # the stores are built: their embeddings are in place
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    idx, val = E.search_rerank(si, sc, k, 'i2t')
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    print('peak allocation of search_rerank: %.1f MB (the grid: %.1f MB)' % (delta / 1e6, n_q * n_g * 4 / 1e6))
    assert delta < n_q * n_g * 4 // 4, delta
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert (idx >= 0).all() and (idx < n_g).all() and (np.diff(val, axis=1) <= 0).all()

    def pad(sets):
        out = np.zeros((sets.shape[0], L, D), np.float32)
        out[:, :sets.shape[1]] = sets
        return out
    for q in rng.choice(n_q, 20, replace=False):
        c = idx[q]
        ref = O.alignment_scores(pad(images[q:q + 1]), pad(captions[c]), il[q:q + 1], [cl[v] for v in c], dtype=np.float64)[0]
        assert_close(val[q], ref, 'fp16', D)


def test_rescore_and_order_under_graph_capture():
    """The ops-level calls with preallocated outputs: captured once on one stream, replayed after the shortlist was overwritten,
    equal to the eager calls bit for bit."""
    from aladin_amd import ops
    si, sc, _, _ = edge_problem('split', 64)
    n_img, n_cap, k = len(si), len(sc), 50
    oi, ci = si._tables()
    oc, cc = sc._tables()
    x = (si.rows, oi, ci, None, n_img, si.max_count())
    y = (sc.rows, oc, cc, None, n_cap, sc.max_count())
    cand = torch.from_numpy(random_shortlist(n_img, n_cap, k, 61)).to(dev())
    out = torch.empty((n_img, k), dtype=torch.float32, device=dev())
    o_idx = torch.empty((n_img, k), dtype=torch.int32, device=dev())
    o_val = torch.empty((n_img, k), dtype=torch.float32, device=dev())

    def run():
        ops.align_rescore(x, y, cand, 1, si.D, si.precision, si.padded_len - 1, out=out)
        ops.rerank_order(cand, out, out_idx=o_idx, out_val=o_val)
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
    cand.copy_(torch.from_numpy(random_shortlist(n_img, n_cap, k, 62)).to(dev()))
    graph.replay()
    torch.cuda.synchronize()
    g_out, g_idx, g_val = out.clone(), o_idx.clone(), o_val.clone()
    e_out = ops.align_rescore(x, y, cand, 1, si.D, si.precision, si.padded_len - 1)
    e_idx, e_val = ops.rerank_order(cand, e_out)
    assert torch.equal(bits(g_out), bits(e_out)) and torch.equal(g_idx, e_idx) and torch.equal(bits(g_val), bits(e_val))
    assert not torch.equal(g_idx[:, 0], cand[:, 0])                       # the order did something
