"""Generate tests/golden/rouge_small.npz and tests/golden/signatures_rouge.json by running the REFERENCE (mesnico/ALADIN) ROUGE-L.

Like make_golden_ndcg.py this runs ONLY where the reference is importable (read-only) and copies none of it: it builds 120 caption
strings (24 images x 5), calls alad.evaluate_utils.rouge.Rouge().score for every (caption, image) pair as
alad/evaluate_utils/compute_relevance.py does, and stores the strings with the float32 matrix.  The CPU tier pins the tests' two
restatements to the matrix bit for bit; the GPU tier holds aladin_rouge_l to the same bits.

    lengths      drawn from {1, 2, 3, 5, 8, 12, 13, 20, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 256} (every one at least
                 once: both sides of the kernel's 64- and 128-position word boundaries) mixed with COCO-like 6..15
    vocabulary   6 words for every third image (long common subsequences, many repeated tokens), 40 for the others
    specials     two identical captions in different images; mixed case; a doubled space (an empty token); the empty caption; one
                 caption of words nothing else uses (its row is 0.0 outside its own image)

    python tests/golden/make_golden_rouge.py
"""
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('ALADIN_REFERENCE', '/root/reference'))

import numpy as np

import alad.evaluate_utils.rouge as ref_rouge          # noqa: E402

NAME = 'rouge_small'
N_IMG, CAPS, SEED = 24, 5, 2207
EDGE_LENGTHS = [1, 2, 3, 5, 8, 12, 13, 20, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 256]
SMALL = ['a', 'the', 'dog', 'on', 'grass', 'runs']
LARGE = SMALL + ['w%02d' % i for i in range(34)]          # shares the small vocabulary: few pairs without a common token
LONER, TWIN_A, TWIN_B, CASED, DOUBLED, EMPTY = 17, 22, 58, 31, 44, 73


def captions():
    rng = np.random.RandomState(SEED)
    n = N_IMG * CAPS
    lengths = [int(v) for v in rng.randint(6, 16, size=n)]
    for k, slot in enumerate(rng.permutation(n)[:2 * len(EDGE_LENGTHS)]):           # every edge length twice, anywhere
        lengths[slot] = EDGE_LENGTHS[k % len(EDGE_LENGTHS)]
    caps = []
    for c in range(n):
        words = SMALL if (c // CAPS) % 3 == 0 else LARGE
        caps.append(' '.join(words[i] for i in rng.randint(0, len(words), size=lengths[c])))
    caps[LONER] = 'zebra quagga okapi tapir'
    caps[TWIN_B] = caps[TWIN_A]
    caps[CASED] = ' '.join(w.upper() if i % 2 else w.capitalize() for i, w in enumerate(caps[CASED].split(' ')))
    head = caps[DOUBLED].split(' ')
    caps[DOUBLED] = ' '.join(head[:2]) + '  ' + ' '.join(head[2:]) + ' '              # a doubled and a trailing space
    caps[EMPTY] = ''
    return caps


def signature_record(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def main():
    caps = captions()
    scorer = ref_rouge.Rouge()
    n = len(caps)
    rel = np.zeros((n, N_IMG), dtype=np.float32)
    for c in range(n):
        for j in range(N_IMG):
            rel[c, j] = scorer.score([caps[c]], caps[CAPS * j:CAPS * j + CAPS])
    own = rel[np.arange(n), np.arange(n) // CAPS]
    assert (own == 1.0).all(), 'a caption against its own image must score exactly 1.0'
    zeros = float((rel == 0.0).mean())
    assert zeros > 0.01, zeros
    loner = np.delete(rel[LONER], LONER // CAPS)
    assert (loner == 0.0).all()
    assert (rel >= 0).all() and (rel <= 1).all()
    lens = sorted({len(c.lower().split(' ')) for c in caps})
    assert set(EDGE_LENGTHS) <= set(lens), set(EDGE_LENGTHS) - set(lens)
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, captions=np.array(caps), relevance=rel, caps_per_img=CAPS, seed=SEED,
                        specials=np.array([LONER, TWIN_A, TWIN_B, CASED, DOUBLED, EMPTY], dtype=np.int32))
    print('%s %.1f KB: %d captions x %d images, %.1f %% zeros, lengths %s' % (NAME, os.path.getsize(path) / 1024, n, N_IMG, 100 * zeros, lens))
    rec = {'Rouge.score': signature_record(ref_rouge.Rouge.score), 'my_lcs': signature_record(ref_rouge.my_lcs)}
    with open(os.path.join(HERE, 'signatures_rouge.json'), 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('signatures_rouge.json: %d callables' % len(rec))
    print('Rouge().score(["a  b"], ["a b"]) = %r' % scorer.score(['a  b'], ['a b']))


if __name__ == '__main__':
    main()
