"""Generate tests/golden/ndcg_small.npz and tests/golden/signatures_ndcg.json by running the REFERENCE (mesnico/ALADIN) nDCG scorer.

Like make_golden.py this runs ONLY where the reference is importable (read-only) and copies none of it: it writes two raw float32
relevance files (300 captions x 60 images, two methods) to a temporary directory, builds the reference's
alad.evaluate_utils.dcg.DCG over them and records, for every query of a few fold windows, a top-`rank` list from a seeded tie-free
random score row and the reference's two nDCG values.  The CPU tier pins the tests' numpy restatement to these values; the GPU tier
holds aladin_ndcg to them within the derived bound.

    relevances   'rougeL': dense in [0, 0.6];  'spice': about 70 % zeros, values rounded to 1/50 (equal relevances abound);
                 both: exactly 1.0 for own pairs (caption c, image c // 5), image column ZERO_IMAGE and caption row ZERO_CAPTION all
                 zero; the five captions of ZERO_IMAGE get their 1.0 at image ZERO_IMAGE + 1 instead.
    windows      npts = 30 folds 0 and 1, npts = 60 fold 0, both retrieval kinds: galleries of 30, 60, 150 and 300 items (300 is
                 past the 256 positions a selection round's first sweep covers; 30 and 60 images have k = 25 < gallery), and
                 npts = 30 with rank = 40 > 30 images (k = gallery).
    condition    every query's window is all zero (expected value exactly 0.0) or holds a relevance of exactly 1.0, so the ideal
                 DCG is >= 1 -- asserted below.

    python tests/golden/make_golden_ndcg.py
"""
import inspect
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('ALADIN_REFERENCE', '/root/reference'))

import numpy as np

import alad.evaluate_utils.dcg as ref_dcg          # noqa: E402

NAME = 'ndcg_small'
N_CAP, N_IMG, SEED = 300, 60, 1407
METHODS = ['rougeL', 'spice']
ZERO_IMAGE, ZERO_CAPTION = 7, 203
# (npts, fold_index, retrieval: 0 = 'image' / 1 = 'sentence', rank)
CASES = [(30, 0, 0, 25), (30, 0, 1, 25), (30, 1, 0, 25), (30, 1, 1, 25), (60, 0, 0, 25), (60, 0, 1, 25), (30, 1, 0, 40)]
KINDS = ['image', 'sentence']


def relevance_matrices():
    rng = np.random.RandomState(SEED)
    dense = (0.6 * rng.random_sample((N_CAP, N_IMG))).astype(np.float32)
    sparse = (np.round(0.6 * rng.random_sample((N_CAP, N_IMG)) * 50) / 50).astype(np.float32)
    sparse[rng.random_sample((N_CAP, N_IMG)) < 0.7] = 0
    out = []
    for r in (dense, sparse):
        r[np.arange(N_CAP), np.arange(N_CAP) // 5] = 1.0
        r[:, ZERO_IMAGE] = 0
        r[5 * ZERO_IMAGE:5 * ZERO_IMAGE + 5, ZERO_IMAGE + 1] = 1.0
        r[ZERO_CAPTION, :] = 0
        out.append(r)
    return out


def window(r, npts, fold, kind):
    """(queries, gallery) view of a fold window, the reference's arithmetic (dcg.py:22-29) restated for the data check only."""
    blk = r[5 * npts * fold:5 * npts * (fold + 1), npts * fold:npts * (fold + 1)]
    return blk if kind == 'image' else blk.T


def signature_record(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def main():
    rels = relevance_matrices()
    out = dict(n_cap=N_CAP, n_img=N_IMG, seed=SEED, zero_image=ZERO_IMAGE, zero_caption=ZERO_CAPTION,
               cases=np.array(CASES, dtype=np.int32), methods=np.array(METHODS))
    for m, r in zip(METHODS, rels):
        out['rel_' + m] = r
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'toy', 'relevances'))
        for m, r in zip(METHODS, rels):
            r.tofile(os.path.join(tmp, 'toy', 'relevances', 'toy-test-%s.npy' % m))
        config = {'dataset': {'data': tmp, 'name': 'toy'}}
        rng = np.random.RandomState(SEED + 1)
        scorers = {}
        for ci, (npts, fold, kind_i, rank) in enumerate(CASES):
            kind = KINDS[kind_i]
            if rank not in scorers:
                scorers[rank] = ref_dcg.DCG(config, N_CAP, 'test', rank=rank, relevance_methods=METHODS)
            wins = [window(r, npts, fold, kind) for r in rels]
            n_q, gallery = wins[0].shape
            lists = np.full((n_q, rank), -1, dtype=np.int32)
            expect = np.zeros((n_q, len(METHODS)), dtype=np.float64)
            n_zero = 0
            for q in range(n_q):
                for w in wins:
                    assert not w[q].any() or (w[q] == 1.0).any(), (ci, q)
                n_zero += not wins[0][q].any()
                scores = rng.random_sample(gallery)
                assert len(np.unique(scores)) == gallery
                full = np.argsort(scores)[::-1]
                got = scorers[rank].compute_ndcg(npts, q, full, fold_index=fold, retrieval=kind)
                lists[q, :min(rank, gallery)] = full[:rank]
                expect[q] = [float(got[m]) for m in METHODS]
            out['list_%d' % ci] = lists
            out['expect_%d' % ci] = expect
            print('case %d: npts %3d fold %d %-8s rank %2d  queries %3d gallery %3d  all-zero queries %d  mean nDCG %s'
                  % (ci, npts, fold, kind, rank, n_q, gallery, n_zero, expect.mean(0).round(4)))
        del scorers
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print('%s %.1f KB' % (NAME, os.path.getsize(path) / 1024))
    rec = {'DCG.__init__': signature_record(ref_dcg.DCG.__init__), 'DCG.compute_ndcg': signature_record(ref_dcg.DCG.compute_ndcg),
           'ndcg_from_ranking': signature_record(ref_dcg.ndcg_from_ranking), 'dcg_from_ranking': signature_record(ref_dcg.dcg_from_ranking)}
    with open(os.path.join(HERE, 'signatures_ndcg.json'), 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('signatures_ndcg.json: %d callables' % len(rec))


if __name__ == '__main__':
    main()
