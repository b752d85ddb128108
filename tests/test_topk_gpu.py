"""GPU tier (-m gpu): the top-k selection rounds and the stored-matrix rank kernels against numpy alone.  ops.topk_indices and
ops.search_topk run the same rounds (topk_rounds, csrc/sim_common.hpp), so comparing one with the other cannot see a bug in them;
here the expected integers come from a stable argsort / plain counting, exactly: no tolerance.  Scores are small integers, so every
shape is full of ties across threads, waves and ownership strides (a thread owns the positions c = tid mod 256: 255, 256 and 257
candidates bracket that edge), and k > n_c is covered."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def int_scores(shape, seed):
    return np.random.RandomState(seed).randint(-3, 4, size=shape).astype(np.float32)


def topk_reference(q_major, k):
    """(n_q, k) from the query-major (n_q, n_c) scores: stable descending argsort, NaN as -inf, -1 past n_c."""
    x = np.where(np.isnan(q_major), -np.inf, q_major)
    order = np.argsort(-x, axis=1, kind='stable')[:, :k].astype(np.int32)
    out = np.full((x.shape[0], k), -1, np.int32)
    out[:, :order.shape[1]] = order
    return out


def check_topk(scores_t, q_major, k, dim):
    from aladin_amd import ops
    got = ops.topk_indices(scores_t, k, dim=dim).cpu().numpy()
    np.testing.assert_array_equal(got, topk_reference(q_major, k))


@pytest.mark.parametrize('dim', [1, 0])
@pytest.mark.parametrize('n_q,n_c,k', [(3, 1, 1), (5, 7, 10), (4, 255, 50), (4, 256, 50), (4, 257, 50), (2, 1000, 300)])
def test_topk_indices_equals_stable_argsort(n_q, n_c, k, dim):
    q_major = int_scores((n_q, n_c), 1000 * n_c + k)
    stored = q_major if dim == 1 else np.ascontiguousarray(q_major.T)       # dim 0: the queries are the columns
    check_topk(torch.from_numpy(stored).to(dev()), q_major, k, dim)


@pytest.mark.parametrize('dim', [1, 0])
def test_topk_indices_nan_and_minus_inf_sort_last_by_index(dim):
    n_q, n_c, k = 4, 257, 50
    rng = np.random.RandomState(77)
    q_major = int_scores((n_q, n_c), 78)
    q_major[rng.random_sample((n_q, n_c)) < 0.1] = np.nan
    for q in range(n_q):
        q_major[q, rng.choice(n_c, 3, replace=False)] = -np.inf
    q_major[3, 20:] = np.nan                                                # fewer than k finite scores: NaN and -inf fill the list by index
    q_major[3, 25] = -np.inf
    stored = q_major if dim == 1 else np.ascontiguousarray(q_major.T)
    check_topk(torch.from_numpy(stored).to(dev()), q_major, k, dim)


@pytest.mark.parametrize('dim', [1, 0])
def test_topk_indices_strided_views(dim):
    """x[:, ::2] is copied by the wrapper; the row slice x[::2] is read in place with its leading dimension."""
    n_q, n_c, k = 4, 257, 50
    rows, cols = (n_q, n_c) if dim == 1 else (n_c, n_q)
    big = int_scores((2 * rows, 2 * cols), 5)
    t = torch.from_numpy(big).to(dev())
    for view_t, view in ((t[:, ::2], big[:, ::2]), (t[::2], big[::2])):
        view_t, view = view_t[:rows, :cols], view[:rows, :cols]
        assert not view_t.is_contiguous()
        check_topk(view_t, view if dim == 1 else view.T, k, dim)


@pytest.mark.parametrize('n_img,cpi', [(3, 2), (300, 2), (2050, 1)])
def test_recall_ranks_equal_counting(n_img, cpi):
    """rank = #(scores strictly above the row's largest ground truth (i2t) / the column's ground truth (t2i)), top-1 = the first
    maximal index; the three sizes are the three row splits of the column kernel (below 256 images, from 256, from 2048)."""
    from aladin_amd import ops
    n_cap = n_img * cpi
    sim = int_scores((n_img, n_cap), 31 * n_img + cpi)
    cols = np.arange(n_cap)
    gt_t2i = sim[cols // cpi, cols]
    gt_i2t = gt_t2i.reshape(n_img, cpi).max(axis=1)
    want = ((sim > gt_i2t[:, None]).sum(axis=1), sim.argmax(axis=1), (sim > gt_t2i[None, :]).sum(axis=0), sim.argmax(axis=0))
    got = ops.recall_ranks(torch.from_numpy(sim).to(dev()), caps_per_img=cpi)
    for g, w, name in zip(got, want, ('rank_i2t', 'top1_i2t', 'rank_t2i', 'top1_t2i')):
        np.testing.assert_array_equal(g.cpu().numpy(), w.astype(np.int32), err_msg=name)
