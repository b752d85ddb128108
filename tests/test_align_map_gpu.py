"""GPU tier (-m gpu): pair alignment maps -- for the listed pairs of two stores, per word the region that carried the max over
regions and per region its best word (store.alignment_map_for_pairs, evaluation.search_explain, csrc/rescore.hip).
The reference is each pair's cosine matrix in float64 numpy from the normalised scored rows, tied to the oracle's score first.
Values are held to the tolerances of tests/test_rerank_gpu.py (split 3e-6 + 2e-6 |ref|; fp16 1e-3 |ref| + 3e-4), indices to
equality wherever float64 separates the best from the second-best candidate by a band of twice that tolerance, and to a
candidate within the band of the maximum elsewhere; a cap on the share of such entries keeps the weak check from carrying the test."""
import functools

import numpy as np
import pytest
import torch

import alad_oracle as O
from test_rerank_gpu import CAP_COUNTS, IMG_COUNTS, L, T, bits, dev, edge_problem, fill_store, make_sets, random_shortlist

pytestmark = pytest.mark.gpu

X_FULL, Y_FULL = L - 1, L - 3                  # counts at which an image / a caption fills the padded-71 set


# ------------------------------------------------------------------------------------------------
# the float64 model (numpy only: tests/test_align_map_cpu.py checks its band shares without a device)
# ------------------------------------------------------------------------------------------------
def edge_sets(D, n_img=23, n_cap=27):
    """The sets behind test_rerank_gpu.edge_problem(precision, D, n_img, n_cap): (images, img_lens, captions, cap_lens)."""
    rng = np.random.RandomState(D)
    ic = [IMG_COUNTS[k % len(IMG_COUNTS)] for k in range(n_img)]
    cc = [CAP_COUNTS[k % len(CAP_COUNTS)] for k in rng.permutation(n_cap)]
    images, il = make_sets(ic, 0, D, 100 + D)
    captions, cl = make_sets(cc, 2, D, 200 + D)
    return images, il, captions, cl


def unit_rows(sets, lens, tail):
    """Per sample the float64 unit vectors of its scored rows: positions [1, len - tail)."""
    out = []
    for s, n in zip(np.asarray(sets, np.float64), lens):
        r = s[1:max(n - tail, 1)]
        out.append(r / np.sqrt((r * r).sum(1, keepdims=True)))
    return out


class Model:
    """cos(i, c): the (regions x words) float64 cosine matrix of image i and caption c."""

    def __init__(self, images, il, captions, cl, x_full=X_FULL, y_full=Y_FULL):
        self.x, self.y = unit_rows(images, il, 0), unit_rows(captions, cl, 2)
        self.x_full, self.y_full = x_full, y_full
        self._cos = {}

    def cos(self, i, c):
        if (i, c) not in self._cos:
            self._cos[(i, c)] = self.x[i] @ self.y[c].T
        return self._cos[(i, c)]

    def score(self, i, c):
        """Column maxima with the zero fill, summed: what the oracle's MrSw entry is."""
        A = self.cos(i, c)
        if A.shape[1] == 0:
            return 0.0
        m = A.max(0) if A.shape[0] else np.full(A.shape[1], -np.inf)
        return float((np.maximum(m, 0.0) if A.shape[0] < self.x_full else m).sum())


@functools.lru_cache(maxsize=None)
def edge_model(D, n_img=23, n_cap=27):
    return Model(*edge_sets(D, n_img, n_cap))


def value_tol(ref, precision):
    ref = np.abs(np.asarray(ref, np.float64))
    return 3e-6 + 2e-6 * ref if precision == 'split' else 1e-3 * ref + 3e-4


def best_and_gap(A, fill):
    """Over axis 0 of A (candidates x entries), with the zero fill as one more candidate when `fill`: the maximum, the lowest
    index attaining it (-1: the fill, which loses a tie with a real candidate), and the gap to the second-best candidate."""
    n, m = A.shape
    cands = np.concatenate([A, np.zeros((1, m))]) if fill else A
    if cands.shape[0] == 0:
        raise AssertionError('a side that fills its set has at least one position')
    order = np.sort(cands, axis=0)
    best = order[-1]
    gap = best - order[-2] if cands.shape[0] > 1 else np.full(m, np.inf)
    arg = cands.argmax(0)                                  # the lowest index; the fill is last, so it loses ties
    return best, np.where(arg >= n, -1, arg), gap


def check_entries(A, fill, got_idx, got_val, precision, stats, share_band):
    """One direction of one pair: A is (candidates x entries); got_idx / got_val the device's entries."""
    best, arg, gap = best_and_gap(A, fill)
    n = A.shape[0]
    tol = value_tol(best, precision)
    err = np.abs(got_val.astype(np.float64) - best)
    assert (err <= tol).all(), ('value', float(err.max()), float(tol.min()))
    band = 2.0 * tol
    clear = gap >= band
    assert np.array_equal(got_idx[clear], arg[clear]), ('index', got_idx[clear].tolist(), arg[clear].tolist())
    for e in np.nonzero(~clear)[0]:                        # inside the band: still a candidate within the band of the maximum
        g = int(got_idx[e])
        assert (fill and g == -1) or 0 <= g < n, g
        assert best[e] - (0.0 if g < 0 else A[g, e]) <= band[e], (int(e), g, float(best[e]), float(band[e]))
    assert ((got_idx >= 0) | (got_val == 0.0)).all()       # the fill's value is exactly 0.0
    stats['entries'] += gap.size
    stats['in_band'] += int((gap < share_band).sum())
    stats['max_err_over_tol'] = max(stats['max_err_over_tol'], float((err / tol).max(initial=0)))


SHARE_BAND = {'fp16': 2e-3, 'split': 2e-5}


def share_cap(precision, D):
    return 0.002 if precision == 'split' else (0.12 if D >= 768 else 0.05)


def new_stats():
    return {'entries': 0, 'in_band': 0, 'max_err_over_tol': 0.0}


def check_map(pa, cand, direction, model, precision, ref_grid=None):
    """Every entry of a PairAlignment (host arrays) against the float64 model; returns the band statistics of the two maps."""
    cand = np.asarray(cand)
    score, w_idx, w_cos, r_idx, r_cos = pa
    sw, sr = new_stats(), new_stats()
    for q in range(cand.shape[0]):
        for s in range(cand.shape[1]):
            c = int(cand[q, s])
            if c < 0:
                assert np.isneginf(score[q, s])
                assert (w_idx[q, s] == -1).all() and (w_cos[q, s] == 0.0).all()
                assert (r_idx[q, s] == -1).all() and (r_cos[q, s] == 0.0).all()
                continue
            i, j = (q, c) if direction == 'i2t' else (c, q)
            A = model.cos(i, j)
            nr, nw = A.shape
            if ref_grid is not None:                       # the model's column maxima, with the fill, are the oracle's score
                assert abs(model.score(i, j) - ref_grid[i, j]) <= 1e-12, (i, j, model.score(i, j), ref_grid[i, j])
            # entries past the sample's count: -1 / 0.0
            assert (w_idx[q, s, nw:] == -1).all() and (w_cos[q, s, nw:] == 0.0).all()
            assert (r_idx[q, s, nr:] == -1).all() and (r_cos[q, s, nr:] == 0.0).all()
            if nw == 0:                                    # the caption without words: score 0.0, nothing but fill
                assert score[q, s] == 0.0 and (r_idx[q, s] == -1).all() and (r_cos[q, s] == 0.0).all()
                continue
            check_entries(A, nr < model.x_full, w_idx[q, s, :nw], w_cos[q, s, :nw], precision, sw, SHARE_BAND[precision])
            check_entries(A.T, nw < model.y_full, r_idx[q, s, :nr], r_cos[q, s, :nr], precision, sr, SHARE_BAND[precision])
    return sw, sr


def model_shares(model, pairs, precision):
    """Band shares (word -> region, region -> word) of the float64 model alone over the given (image, caption) pairs."""
    out = []
    for transpose in (False, True):
        n = hit = 0
        for i, j in pairs:
            A = model.cos(i, j)
            if A.shape[1] == 0:
                continue
            fill = (A.shape[1] < model.y_full) if transpose else (A.shape[0] < model.x_full)
            _, _, gap = best_and_gap(A.T if transpose else A, fill)
            n += gap.size
            hit += int((gap < SHARE_BAND[precision]).sum())
        out.append(hit / max(n, 1))
    return out


def host(pa):
    return tuple(None if v is None else v.cpu().numpy() for v in pa)


def equal_bits(a, b):
    return all((u is None and v is None) or torch.equal(bits(u), bits(v)) for u, v in zip(a, b))


def run_case(precision, direction, D, ks, n_img=23, n_cap=27):
    """Every entry of the maps of random shortlists of k candidates, for each k of `ks`, against the float64 model; then the cap on
    the share of the entries of the case that only had the weak (inside the band) index check."""
    from aladin_amd.store import alignment_map_for_pairs
    si, sc, ref, _ = edge_problem(precision, D, n_img, n_cap)
    model = edge_model(D, n_img, n_cap)
    n_q, n_g = (n_img, n_cap) if direction == 'i2t' else (n_cap, n_img)
    total = {'word->region': new_stats(), 'region->word': new_stats()}
    for k in ks:
        cand = random_shortlist(n_q, n_g, k, 7 * k + D)
        assert (cand < 0).any() and (cand[n_q // 2] == -1).all()                       # -1 slots and an all -1 row
        pa = alignment_map_for_pairs(si, sc, torch.from_numpy(cand).to(dev()), direction)
        assert pa.score.shape == (n_q, k) and pa.score.dtype == torch.float32
        assert pa.word_region.shape == pa.word_cos.shape == (n_q, k, sc.max_count()) and pa.word_region.dtype == torch.int32
        assert pa.region_word.shape == pa.region_cos.shape == (n_q, k, si.max_count()) and pa.region_word.dtype == torch.int32
        assert pa.word_cos.dtype == pa.region_cos.dtype == torch.float32
        for name, st in zip(total, check_map(host(pa), cand, direction, model, precision, ref)):
            total[name]['entries'] += st['entries']
            total[name]['in_band'] += st['in_band']
            total[name]['max_err_over_tol'] = max(total[name]['max_err_over_tol'], st['max_err_over_tol'])
    for name, st in total.items():
        share = st['in_band'] / max(st['entries'], 1)
        print('%s: %d entries, %.2f %% inside the %g band, max err / tol %.3g (%s, %s, D=%d, k=%s)'
              % (name, st['entries'], 100 * share, SHARE_BAND[precision], st['max_err_over_tol'], precision, direction, D, list(ks)))
        assert st['entries'] > 0 and share <= share_cap(precision, D), (name, share)


# ------------------------------------------------------------------------------------------------
# 1. against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [64, 100])
@pytest.mark.parametrize('direction', ['i2t', 't2i'])
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_maps_vs_float64(precision, direction, D):
    """k = 1, 7 and 50 in one case: the cap on the band share is a statement about the case's inputs, and the 22 pairs of a k = 1
    shortlist alone are too few entries to measure a share of 0.2 % (split) or 5 % (fp16) on."""
    run_case(precision, direction, D, (1, 7, 50))


@pytest.mark.parametrize('direction', ['i2t', 't2i'])
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_maps_vs_float64_at_the_shipped_depth(precision, direction):
    """D = 768: twelve (fp16) / thirty-six (split) K steps, on the 12 x 20 sub-case of test_rerank_gpu."""
    run_case(precision, direction, 768, (1, 7, 50), 12, 20)


# ------------------------------------------------------------------------------------------------
# 2. score bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('direction', ['i2t', 't2i'])
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_score_is_the_rescore_calls_bits(precision, direction):
    from aladin_amd.store import alignment_map_for_pairs, alignment_scores_for_pairs
    for D in (64, 100):
        si, sc, _, _ = edge_problem(precision, D)
        n_q, n_g = (len(si), len(sc)) if direction == 'i2t' else (len(sc), len(si))
        cand = torch.from_numpy(random_shortlist(n_q, n_g, 50, 19 + D)).to(dev())
        want = alignment_scores_for_pairs(si, sc, cand, direction)
        for kw in ({}, {'regions': False}, {'words': False}):
            got = alignment_map_for_pairs(si, sc, cand, direction, **kw)
            assert torch.equal(bits(got.score), bits(want)), kw


# ------------------------------------------------------------------------------------------------
# 3. exact ties
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_exact_ties_go_to_the_lowest_index(precision):
    """Image 0: region 3 points along three words of caption 0 and is copied to region 5 (same 16-row tile) and region 35
    (another tile), scaled by powers of two (the unit vectors, and so the operands, are the same bits).  Caption 0: word 4 is
    copied to word 9 and region 10 of the image points along it."""
    from aladin_amd.store import alignment_map_for_pairs
    D = 64
    images, il = make_sets([50, 20], 0, D, 71)
    captions, cl = make_sets([12, 9], 2, D, 72)
    captions[0, 1 + 9] = 2.0 * captions[0, 1 + 4]
    images[0, 1 + 3] = captions[0, 1 + 2] + captions[0, 1 + 6] + captions[0, 1 + 7]
    images[0, 1 + 5] = 2.0 * images[0, 1 + 3]
    images[0, 1 + 35] = 0.5 * images[0, 1 + 3]
    images[0, 1 + 10] = 3.0 * captions[0, 1 + 4] + 0.25 * images[0, 1 + 10]
    A = Model(images, il, captions, cl).cos(0, 0)
    tied = [w for w in range(12) if A[:, w].argmax() == 3]
    assert set(tied) >= {2, 6, 7} and A[:, 4].argmax() == 10 and A[10].argmax() == 4          # float64 agrees on the construction
    si, sc = fill_store(images, il, 0, precision), fill_store(captions, cl, 2, precision)
    for direction, cand in (('i2t', [[0, 1], [0, 1]]), ('t2i', [[0, 1], [1, 0]])):
        pa = alignment_map_for_pairs(si, sc, torch.tensor(cand, dtype=torch.int32, device=dev()), direction)
        q, s = 0, 0                                                                            # pair (image 0, caption 0) either way
        w_idx, w_cos = pa.word_region[q, s].cpu().numpy(), pa.word_cos[q, s].cpu().numpy()
        r_idx, r_cos = pa.region_word[q, s].cpu().numpy(), pa.region_cos[q, s].cpu().numpy()
        assert (w_idx[tied] == 3).all(), w_idx.tolist()                                        # never 5 or 35
        assert w_idx[4] == w_idx[9] == 10 and w_cos[4:5].view(np.int32) == w_cos[9:10].view(np.int32)
        assert r_idx[10] == 4 and not (r_idx[:50] == 9).any(), r_idx.tolist()                  # the lower of the twin words
        for twin in (5, 35):                                                                   # the copies: the same row of cosines
            assert r_idx[twin] == r_idx[3] and r_cos[twin:twin + 1].view(np.int32) == r_cos[3:4].view(np.int32)


# ------------------------------------------------------------------------------------------------
# 4. fill
# ------------------------------------------------------------------------------------------------
def store_of(sets, lens, tail, precision, padded_len):
    from aladin_amd.store import PackedSetStore
    st = PackedSetStore(sets.shape[2], tail, dev(), capacity_rows=64, precision=precision, padded_len=padded_len)
    st.append(T(sets[:, :max(lens)]), lens)
    return st


def fill_sets(D=64):
    """Image 0 (10 regions) and caption 0 (8 words); word 2 of caption 1 is minus the sum of image 0's unit regions, region 4 of
    image 1 minus the sum of caption 0's unit words: every cosine of that word with image 0 / that region with caption 0 < 0."""
    images, il = make_sets([10, 10], 0, D, 82)          # seeds chosen on the CPU: every such cosine < -0.15 in float64
    captions, cl = make_sets([8, 8], 2, D, 83)
    captions[1, 1 + 2] = -unit_rows(images[:1], il[:1], 0)[0].sum(0)
    images[1, 1 + 4] = -unit_rows(captions[:1], cl[:1], 2)[0].sum(0)
    m = Model(images, il, captions, cl)
    return images, il, captions, cl, m


@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_zero_fill_wins_only_against_a_shorter_side(precision):
    from aladin_amd.store import alignment_map_for_pairs
    images, il, captions, cl, m = fill_sets()
    word_col, region_row = m.cos(0, 1)[:, 2], m.cos(1, 0)[4]
    assert word_col.max() < -0.05 and region_row.max() < -0.05                                 # float64: all negative, clear of zero
    cand = torch.tensor([[0, 1], [0, 1]], dtype=torch.int32, device=dev())
    # both sides shorter than the padded set (71): the fill wins
    si, sc = store_of(images, il, 0, precision, L), store_of(captions, cl, 2, precision, L)
    for direction in ('i2t', 't2i'):
        pa = alignment_map_for_pairs(si, sc, cand, direction)
        wq, ws = (0, 1) if direction == 'i2t' else (1, 0)                                      # pair (image 0, caption 1)
        assert int(pa.word_region[wq, ws, 2]) == -1 and float(pa.word_cos[wq, ws, 2]) == 0.0
        rq, rs = (1, 0) if direction == 'i2t' else (0, 1)                                      # pair (image 1, caption 0)
        assert int(pa.region_word[rq, rs, 4]) == -1 and float(pa.region_cos[rq, rs, 4]) == 0.0
        check_map(host(pa), cand.cpu().numpy(), direction, m, precision)
    # the same rows in stores whose padded_len the samples fill (10 regions of 11 positions, 8 words of 11): a real index, < 0
    full = Model(images, il, captions, cl, x_full=10, y_full=8)
    si, sc = store_of(images, il, 0, precision, 11), store_of(captions, cl, 2, precision, 11)
    for direction in ('i2t', 't2i'):
        pa = alignment_map_for_pairs(si, sc, cand, direction)
        wq, ws = (0, 1) if direction == 'i2t' else (1, 0)
        assert int(pa.word_region[wq, ws, 2]) == int(word_col.argmax())
        np.testing.assert_allclose(float(pa.word_cos[wq, ws, 2]), word_col.max(), atol=float(value_tol(word_col.max(), precision)), rtol=0)
        rq, rs = (1, 0) if direction == 'i2t' else (0, 1)
        assert int(pa.region_word[rq, rs, 4]) == int(region_row.argmax())
        np.testing.assert_allclose(float(pa.region_cos[rq, rs, 4]), region_row.max(), atol=float(value_tol(region_row.max(), precision)),
                                   rtol=0)
        check_map(host(pa), cand.cpu().numpy(), direction, full, precision)
    # one side full, the other short: each fill follows its own side
    si, sc = store_of(images, il, 0, precision, 11), store_of(captions, cl, 2, precision, L)
    pa = alignment_map_for_pairs(si, sc, cand, 'i2t')
    assert int(pa.word_region[0, 1, 2]) == int(word_col.argmax()) and int(pa.region_word[1, 0, 4]) == -1
    check_map(host(pa), cand.cpu().numpy(), 'i2t', Model(images, il, captions, cl, x_full=10, y_full=Y_FULL), precision)


# ------------------------------------------------------------------------------------------------
# 5. a pair's bits depend on the pair alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_all_outputs_depend_on_the_pair_only(precision):
    from aladin_amd.store import alignment_map_for_pairs
    D = 64
    si, sc, _, _ = edge_problem(precision, D)
    n_img, n_cap = len(si), len(sc)
    rng = np.random.RandomState(12)
    cand = random_shortlist(n_img, n_cap, 50, 4)
    d_cand = torch.from_numpy(cand).to(dev())
    base = alignment_map_for_pairs(si, sc, d_cand, 'i2t')
    assert equal_bits(alignment_map_for_pairs(si, sc, d_cand, 'i2t'), base)                    # run to run
    perm = rng.permutation(50)                                                                 # a changed slot
    got = alignment_map_for_pairs(si, sc, torch.from_numpy(np.ascontiguousarray(cand[:, perm])).to(dev()), 'i2t')
    d_perm = torch.from_numpy(perm).to(dev())
    assert equal_bits(got, [v[:, d_perm] for v in base])
    for col in (0, 13, 49):                                                                    # k = 1 against k = 50
        got = alignment_map_for_pairs(si, sc, d_cand[:, col:col + 1].contiguous(), 'i2t')
        assert equal_bits(got, [v[:, col:col + 1] for v in base])
    grid_i = torch.arange(n_cap, dtype=torch.int32, device=dev()).repeat(n_img, 1)             # i2t against t2i: the full grid
    grid_c = torch.arange(n_img, dtype=torch.int32, device=dev()).repeat(n_cap, 1)
    from_i = alignment_map_for_pairs(si, sc, grid_i, 'i2t')
    from_c = alignment_map_for_pairs(si, sc, grid_c, 't2i')
    assert equal_bits(from_i, [v.transpose(0, 1) for v in from_c])
    ic = [IMG_COUNTS[k % len(IMG_COUNTS)] for k in range(n_img)]                               # a view against a fresh store
    images, il = make_sets(ic, 0, D, 100 + D)
    for ids in (list(range(n_img))[0:None:5], [int(v) for v in rng.permutation(n_img)[:9]]):
        view = si.view(slice(0, None, 5)) if ids[:2] == [0, 5] else si.view(ids)
        fresh = fill_store(images[ids], [il[v] for v in ids], 0, precision, batch=4)
        sub = torch.arange(n_cap, dtype=torch.int32, device=dev()).repeat(len(ids), 1)
        want = alignment_map_for_pairs(fresh, sc, sub, 'i2t')
        assert equal_bits(alignment_map_for_pairs(view, sc, sub, 'i2t'), want)
        nr = fresh.max_count()                                                                 # the view's stride: its own largest count
        d_ids = torch.tensor(ids, device=dev())
        assert equal_bits(want, [v[d_ids] if v.dim() == 2 or v.shape[2] == sc.max_count() else v[d_ids][:, :, :nr] for v in from_i])
        gal = torch.arange(len(ids), dtype=torch.int32, device=dev()).repeat(n_cap, 1)
        assert equal_bits(alignment_map_for_pairs(view, sc, gal, 't2i'), alignment_map_for_pairs(fresh, sc, gal, 't2i'))


# ------------------------------------------------------------------------------------------------
# 6. edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_last_sample_of_an_exactly_full_store(precision):
    """The stores of test_rerank_gpu's test of the same name: the allocation ends with the last sample's last row, whose count
    (13 regions, 11 words) is no multiple of 8 or 16."""
    from aladin_amd.store import alignment_map_for_pairs
    D = 64
    ic, cc = [16, 5, 13], [9, 20, 11]
    images, il = make_sets(ic, 0, D, 31)
    captions, cl = make_sets(cc, 2, D, 32)
    ref = O.alignment_scores(images, captions, il, cl, dtype=np.float64)
    si = fill_store(images, il, 0, precision, batch=3, capacity_rows=sum(ic))
    sc = fill_store(captions, cl, 2, precision, batch=3, capacity_rows=sum(cc))
    assert si.rows.shape[0] == si.n_rows == sum(ic) and sc.rows.shape[0] == sc.n_rows == sum(cc)
    m = Model(images, il, captions, cl)
    cand = np.array([[2, 0, 1, 2]] * 3, np.int32)
    for direction in ('i2t', 't2i'):
        pa = alignment_map_for_pairs(si, sc, torch.from_numpy(cand).to(dev()), direction)
        assert pa.word_region.shape == (3, 4, 20) and pa.region_word.shape == (3, 4, 16)
        check_map(host(pa), cand, direction, m, precision, ref)


@pytest.mark.parametrize('direction', ['i2t', 't2i'])
@pytest.mark.parametrize('precision', ['split', 'fp16'])
def test_caption_without_words_and_unrequested_outputs(precision, direction):
    from aladin_amd.store import alignment_map_for_pairs
    D = 100
    si, sc, _, cc = edge_problem(precision, D)
    empty = [j for j, c in enumerate(cc) if c == 0]
    assert empty
    n_q, n_g = (len(si), len(sc)) if direction == 'i2t' else (len(sc), len(si))
    cand = random_shortlist(n_q, n_g, 7, 23)
    if direction == 'i2t':
        cand[:, 3] = empty[0]                                                                  # every image against the empty caption
    d_cand = torch.from_numpy(cand).to(dev())
    full = alignment_map_for_pairs(si, sc, d_cand, direction)
    q, s = (slice(None), 3) if direction == 'i2t' else (empty[0], slice(None))
    live = torch.from_numpy(cand >= 0).to(dev())[q, s]
    assert live.any()
    assert (full.score[q, s][live] == 0.0).all() and (full.word_region[q, s] == -1).all() and (full.word_cos[q, s] == 0.0).all()
    assert (full.region_word[q, s] == -1).all() and (full.region_cos[q, s] == 0.0).all()
    only_w = alignment_map_for_pairs(si, sc, d_cand, direction, regions=False)
    only_r = alignment_map_for_pairs(si, sc, d_cand, direction, words=False)
    assert only_w.region_word is None and only_w.region_cos is None and only_r.word_region is None and only_r.word_cos is None
    assert equal_bits(only_w[:3], full[:3]) and equal_bits(only_r[3:], full[3:]) and equal_bits(only_r[:1], full[:1])
    neither = alignment_map_for_pairs(si, sc, d_cand, direction, words=False, regions=False)
    assert equal_bits(neither[:1], full[:1]) and all(v is None for v in neither[1:])


# ------------------------------------------------------------------------------------------------
# 7. search_explain
# ------------------------------------------------------------------------------------------------
def test_search_explain_is_search_rerank_plus_the_map_of_its_head():
    from aladin_amd import evaluation as E
    from aladin_amd.store import PairAlignment, alignment_map_for_pairs
    si, sc, _, _ = edge_problem('split', 64)
    for direction, n_q, n_g in (('i2t', 23, 27), ('t2i', 27, 23)):
        for k, top in ((10, 5), (10, 1), (3, 5), (50, 30)):                                   # top past k; k past the gallery
            want_i, want_v = E.search_rerank(si, sc, k, direction)
            idx, val, pa = E.search_explain(si, sc, k, direction, top=top)
            assert torch.equal(idx, want_i) and torch.equal(bits(val), bits(want_v)) and isinstance(pa, PairAlignment)
            t = min(top, k)
            assert pa.score.shape == (n_q, t)
            assert equal_bits(pa, alignment_map_for_pairs(si, sc, idx[:, :t].contiguous(), direction))
            assert torch.equal(bits(pa.score), bits(val[:, :t]))
            if t > n_g:                                                                        # -1 slots: -inf, nothing but fill
                assert (idx[:, n_g:t] == -1).all() and torch.isneginf(pa.score[:, n_g:]).all()
                assert (pa.word_region[:, n_g:] == -1).all() and (pa.region_cos[:, n_g:] == 0.0).all()
    short = torch.full((23, 4), -1, dtype=torch.int32, device=dev())                          # a shortlist shorter than top
    short[:, 0] = torch.arange(23, device=dev()) % 27
    short[:, 1] = 5
    idx, val, pa = E.search_explain(si, sc, 4, 'i2t', shortlist=short, top=3)
    want_i, want_v = E.search_rerank(si, sc, 4, 'i2t', shortlist=short)
    assert torch.equal(idx, want_i) and torch.equal(bits(val), bits(want_v))
    assert pa.score.shape == (23, 3) and (idx[:, 2] == -1).all() and torch.isneginf(pa.score[:, 2]).all()
    assert (pa.word_region[:, 2] == -1).all() and (pa.word_cos[:, 2] == 0.0).all() and (pa.region_word[:, 2] == -1).all()
    assert (pa.score[:, :2] > -np.inf).all()


# ------------------------------------------------------------------------------------------------
# 8. graph capture
# ------------------------------------------------------------------------------------------------
def test_pair_map_under_graph_capture():
    """ops.align_pair_map with preallocated outputs: captured once, replayed after the shortlist was overwritten, equal to the
    eager call bit for bit."""
    from aladin_amd import ops
    si, sc, _, _ = edge_problem('split', 64)
    n_img, n_cap, k = len(si), len(sc), 7
    oi, ci = si._tables()
    oc, cc = sc._tables()
    x = (si.rows, oi, ci, None, n_img, si.max_count())
    y = (sc.rows, oc, cc, None, n_cap, sc.max_count())
    cand = torch.from_numpy(random_shortlist(n_img, n_cap, k, 61)).to(dev())
    out = (torch.empty((n_img, k), dtype=torch.float32, device=dev()),
           torch.empty((n_img, k, sc.max_count()), dtype=torch.int32, device=dev()),
           torch.empty((n_img, k, sc.max_count()), dtype=torch.float32, device=dev()),
           torch.empty((n_img, k, si.max_count()), dtype=torch.int32, device=dev()),
           torch.empty((n_img, k, si.max_count()), dtype=torch.float32, device=dev()))

    def run():
        ops.align_pair_map(x, y, cand, 1, si.D, si.precision, X_FULL, Y_FULL, out=out)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run()                                                             # warm-up outside the capture (one-time kernel attributes)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    first = [v.clone() for v in out]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    cand.copy_(torch.from_numpy(random_shortlist(n_img, n_cap, k, 62)).to(dev()))
    for v in out:
        v.fill_(7)                                                        # every entry is written again by the replay
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.align_pair_map(x, y, cand, 1, si.D, si.precision, X_FULL, Y_FULL)
    assert equal_bits(out, eager) and not equal_bits(out, first)
