"""GPU tier: aladin_rouge_l (csrc/rouge.hip) through ops.rouge_l_relevance / rouge_l_launch, aladin_amd.rouge and
DCG.from_captions.  Every comparison is bit-equality of the float32 words: with the reference's recorded matrix
(tests/golden/rouge_small.npz) or with the restatement tests/helpers/rouge_numpy.py, which the CPU tier pins to that matrix."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import rouge_numpy as R                  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CLASS_LENGTHS = {1: [1, 2, 9, 31, 32, 33, 63, 64], 2: [65, 66, 100, 127, 128], 4: [129, 130, 191, 192, 193, 255, 256]}


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, '%d of %d entries differ, first at %s: %r vs %r' % (
        len(bad), g.size, tuple(bad[0]), float(np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got)[tuple(bad[0])]),
        float(np.asarray(want)[tuple(bad[0])]))


def dev_csr(seqs):
    tok, off = R.csr(seqs)
    return torch.from_numpy(tok).to(DEV), torch.from_numpy(off).to(DEV)


def dev_groups(groups):
    return torch.tensor(list(groups), dtype=torch.int64, device=DEV)


def random_seqs(rng, lengths, vocab):
    return [[int(v) for v in rng.randint(0, vocab, size=n)] for n in lengths]


def ragged_groups(rng, n_img, lo=1, hi=7):
    return [0] + [int(v) for v in np.cumsum(rng.randint(lo, hi + 1, size=n_img))]


def relevance(queries, gallery, groups, **kw):
    from aladin_amd import ops
    qt, qo = dev_csr(queries)
    gt, go = dev_csr(gallery)
    return ops.rouge_l_relevance(qt, qo, gt, go, dev_groups(groups), **kw)


@pytest.fixture(scope='module')
def golden_rouge():
    g = load_golden('rouge_small')
    return [str(c) for c in g['captions']], g['relevance']


def test_golden_captions_give_the_reference_matrix(golden_rouge):
    from aladin_amd import rouge
    caps, rel = golden_rouge
    got = rouge.relevance_matrix(caps)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == rel.shape
    same_bits(got, rel)
    some = [119, 0, 57, 58, 3]
    same_bits(rouge.relevance_matrix(caps, 5, queries=some), rel[some])


@pytest.mark.parametrize('W', [1, 2, 4])
@pytest.mark.parametrize('n_q,n_img', [(1, 65), (7, 1), (9, 63)])
def test_word_classes_with_listed_rows_and_a_padded_output(W, n_q, n_img):
    """One length class per launch: queries not a multiple of the workgroup's 8 / 4 / 2, images not a multiple of 64, the rows
    of the output listed in any order (q_rows), ld_out > n_img with the padding and the unlisted rows left as they were."""
    from aladin_amd import ops
    rng = np.random.RandomState(100 * W + n_q)
    pool = CLASS_LENGTHS[W]
    lens = [pool[-1 - i % len(pool)] for i in range(n_q)]                # the class's longest first: one query = a full last word
    vocab = 5 if W > 1 else 9
    queries = random_seqs(rng, lens, vocab)
    groups = ragged_groups(rng, n_img, 1, 3)
    gallery = random_seqs(rng, rng.choice([3, 17, 64, 65, 130, 256], size=groups[-1]), vocab)
    want = R.relevance(queries, gallery, groups)
    same_bits(relevance(queries, gallery, groups), want)
    rows = rng.permutation(n_q + 3)[:n_q]
    out = torch.full((n_q + 3, n_img + 5), -7.0, device=DEV)
    qt, qo = dev_csr(queries)
    gt, go = dev_csr(gallery)
    ret = ops.rouge_l_relevance(qt, qo, gt, go, dev_groups(groups), out=out[:, 2:2 + n_img],
                                q_rows=torch.from_numpy(rows.astype(np.int32)).to(DEV))
    assert ret.data_ptr() == out[:, 2:].data_ptr()
    full = np.full((n_q + 3, n_img + 5), -7.0, np.float32)
    full[rows, 2:2 + n_img] = want
    same_bits(out, full)
    # the same through the single launch, the class's maximum stated exactly
    out2 = torch.full((n_q, n_img + 1), -7.0, device=DEV)
    ops.rouge_l_launch(qt, qo, max(lens), gt, go, 256, dev_groups(groups), out2[:, :n_img])
    same_bits(out2[:, :n_img], want)
    assert (out2[:, n_img] == -7.0).all()


def test_mixed_classes_split_into_launches_and_truncate_past_256():
    rng = np.random.RandomState(7)
    lens = [3, 200, 64, 65, 128, 129, 256, 1, 90, 300, 12]
    queries = random_seqs(rng, lens, 6)
    groups = ragged_groups(rng, 20, 1, 7)
    gallery = random_seqs(rng, rng.choice([1, 5, 11, 70, 140, 256, 280], size=groups[-1]), 6)
    want = R.relevance([q[:256] for q in queries], [g[:256] for g in gallery], groups)
    same_bits(relevance(queries, gallery, groups), want)
    lcs = R.relevance([q[:256] for q in queries], [g[:256] for g in gallery], groups, fn=R.max_lcs)
    same_bits(relevance(queries, gallery, groups, lcs=True), lcs)


def test_ragged_groups_and_the_extreme_length_pairs():
    rng = np.random.RandomState(11)
    groups = ragged_groups(rng, 70, 1, 7)
    assert set(np.diff(groups)) == set(range(1, 8))
    gallery = random_seqs(rng, rng.randint(4, 21, size=groups[-1]), 12)
    queries = random_seqs(rng, rng.randint(4, 21, size=13), 12)
    same_bits(relevance(queries, gallery, groups), R.relevance(queries, gallery, groups))
    long_gallery = random_seqs(rng, [256] * 9, 4)
    one = [[2], [3], [99]]
    g3 = [0, 1, 4, 9]
    same_bits(relevance(one, long_gallery, g3), R.relevance(one, long_gallery, g3))
    same_bits(relevance(long_gallery, one, [0, 1, 3]), R.relevance(long_gallery, one, [0, 1, 3]))


def test_hostile_ids():
    """No vocabulary limit: ids up to 2^31 - 1; ids that meet in the query's hash table -- differing by multiples of its size, and
    ids chosen to share a slot of the kernel's multiplicative hash (top 8 / 9 bits of id * 0x9E3779B1); a query of 64 distinct
    tokens and one of 64 equal tokens."""
    rng = np.random.RandomState(13)
    big = [2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30, 2 ** 31 - 257, 0, 1]
    step256 = [5 + 256 * k for k in range(64)]
    step512 = [7 + 512 * k for k in range(130)]
    ids = np.arange(1, 400000, dtype=np.uint64)
    mixed = (ids * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    slot256 = [int(v) for v in ids[(mixed >> np.uint64(24)) == 77][:64]]
    slot512 = [int(v) for v in ids[(mixed >> np.uint64(23)) == 301][:200]]
    assert len(slot256) == 64 and len(slot512) == 200
    pools = [big, step256, step512, slot256, slot512]
    queries = [big * 3, step256, step512, step512[:128], slot256, slot512, slot512[:65], list(range(1000, 1064)), [4] * 64, [4] * 200,
               step256[::-1], slot256[::2] + big]
    gallery = []
    for pool in pools:
        for n in (3, 40, 64, 150):
            gallery.append([pool[i] for i in rng.randint(0, len(pool), size=n)])
    gallery += [list(range(1000, 1064)), list(range(1063, 999, -1)), [4] * 64, [4] * 3, step256, slot256, slot512, step512[:100] + [4] * 50]
    groups = list(range(0, len(gallery) + 1, 2))
    same_bits(relevance(queries, gallery, groups), R.relevance(queries, gallery, groups))


@pytest.fixture(scope='module')
def coco_like():
    """2000 captions of 8..20 tokens (Zipf ids over 3000 words), 400 images: (captions as id lists, the device matrix)."""
    rng = np.random.RandomState(17)
    lens = np.clip(rng.poisson(2.5, size=2000) + 8, 8, 20)
    caps = [[int(v) for v in np.minimum(rng.zipf(1.3, size=n), 3000)] for n in lens]
    groups = list(range(0, 2001, 5))
    return caps, groups, relevance(caps, caps, groups)


def test_coco_like_matrix_sampled_against_the_restatement(coco_like):
    caps, groups, got = coco_like
    got = got.cpu().numpy()
    assert got.shape == (2000, 400)
    assert (got[np.arange(2000), np.arange(2000) // 5] == 1.0).all()
    assert (got >= 0).all() and (got <= 1).all()
    rng = np.random.RandomState(19)
    qs, js = rng.randint(0, 2000, size=20000), rng.randint(0, 400, size=20000)
    want = np.array([R.score(caps[q], caps[5 * j:5 * j + 5]) for q, j in zip(qs, js)], dtype=np.float32)
    same_bits(got[qs, js], want)


def test_runs_repeat_and_a_graph_replay_gives_the_same_bits(coco_like):
    from aladin_amd import ops
    caps, groups, first = coco_like
    qt, qo = dev_csr(caps[:501])
    gt, go = dev_csr(caps)
    grp = dev_groups(groups)
    again = ops.rouge_l_relevance(qt, qo, gt, go, grp)
    same_bits(again, first[:501])
    out = torch.zeros((501, 400), device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.rouge_l_launch(qt, qo, 20, gt, go, 20, grp, out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same_bits(out, first[:501])


def test_scorer_from_captions_equals_the_scorer_over_the_golden_matrix(golden_rouge):
    from aladin_amd import dcg
    caps, rel = golden_rouge
    made = dcg.DCG.from_captions(caps)
    kept = dcg.DCG(None, 120, 'test', relevances=[rel])
    assert made.relevance_methods == ['rougeL'] and made.rank == 25
    rng = np.random.RandomState(23)
    for kind, n_q, gallery in (('image', 120, 24), ('sentence', 24, 120)):
        table = np.stack([rng.permutation(gallery)[:min(25, gallery)] for _ in range(n_q)]).astype(np.int32)
        a = made.compute_ndcg_batch(24, table, retrieval=kind)['rougeL']
        b = kept.compute_ndcg_batch(24, table, retrieval=kind)['rougeL']
        assert a.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64)) and float(a.max()) > 0


def test_relevance_file_round_trip_and_the_single_score(golden_rouge, tmp_path):
    from aladin_amd import dcg, rouge
    caps, rel = golden_rouge
    config = {'dataset': {'data': str(tmp_path), 'name': 'toy'}}
    path = rouge.write_relevance_file(config, 'test', caps, chunk=50)
    assert path == str(tmp_path / 'toy' / 'relevances' / 'toy-test-rougeL.npy')
    assert open(path, 'rb').read() == rel.tobytes()
    sc = dcg.DCG(config, 120, 'test')
    assert sc.relevances[0].shape == (120, 24) and np.array_equal(bits(np.array(sc.relevances[0])), bits(rel))
    got = rouge.Rouge().score(["a  b"], ["a b"])
    assert isinstance(got, float) and np.float32(got) == np.float32(0.8299319727891156)
    assert rouge.Rouge().score([caps[3]], caps[0:5]) == 1.0 and rouge.Rouge().score(['zebra'], ['a b', 'c']) == 0.0
    assert rouge.my_lcs('the dog runs on the grass'.split(), 'a dog on grass'.split()) == 3
    assert rouge.my_lcs(['x'], ['y', 'z']) == 0
