"""Two restatements of the ROUGE-L relevance that aladin_rouge_l computes (include/aladin_hip.h), i.e. of Rouge.score of reference
alad/evaluate_utils/rouge.py:46-76, on token sequences of any hashable kind (strings or ids):

    lcs_bits      the bit-parallel LCS (Allison-Dix / Hyyro) on Python's unbounded integers -- no word boundary, no carry chain
    lcs_dp        the plain dynamic programme, a numpy row at a time -- the reference's procedure

and the F-measure in the reference's double arithmetic and association.  tests/test_rouge_cpu.py pins both to the reference's
recorded float32 matrix bit for bit; the GPU tests compare the kernel with them."""
import numpy as np

BETA = 1.2
BETA2 = 1.2 * 1.2                    # == 1.2 ** 2 bit for bit (asserted in the CPU tier)


def tokens(caption):
    """The reference's tokens of a caption string (rouge.py:59,63)."""
    return caption.lower().split(" ")


def lcs_bits(query, ref):
    m = len(query)
    masks = {}
    for p, t in enumerate(query):
        masks[t] = masks.get(t, 0) | (1 << p)
    full = (1 << m) - 1
    v = full
    for t in ref:
        mt = masks.get(t, 0)
        u = v & mt
        v = ((v + u) | (v & ~mt)) & full
    return m - bin(v).count('1')


def lcs_dp(query, ref):
    vocab = {}
    a = np.asarray([vocab.setdefault(t, len(vocab)) for t in query], dtype=np.int64)
    row = np.zeros(len(a) + 1, dtype=np.int64)
    for t in ref:
        hit = a == vocab.get(t, -1)
        diag = row[:-1] + hit                            # lengths[i-1][j-1] + 1 where the tokens match
        new = np.maximum(row[1:], diag)                  # a match's diagonal + 1 is never below the two neighbours
        row = np.concatenate(([0], np.maximum.accumulate(new)))           # lengths[i][j-1] carried along the row
    return int(row[-1])


def f_measure(lcs, m, lens):
    """lcs[i], lens[i]: LCS with and length of reference i; m: the query's length."""
    prec_max = max(l / float(m) for l in lcs)
    rec_max = max(l / float(n) for l, n in zip(lcs, lens))
    if prec_max != 0 and rec_max != 0:
        return ((1 + BETA2) * prec_max * rec_max) / float(rec_max + BETA2 * prec_max)
    return 0.0


def score(query, refs, lcs=lcs_bits):
    """Rouge.score on token sequences: a Python float (double)."""
    return f_measure([lcs(query, r) for r in refs], len(query), [len(r) for r in refs])


def max_lcs(query, refs, lcs=lcs_bits):
    return max(lcs(query, r) for r in refs)


def relevance(queries, gallery, groups, lcs=lcs_bits, fn=score):
    """(len(queries), len(groups) - 1) float32: query token sequences against images, image j holding gallery[groups[j]:groups[j + 1]];
    rounded to float32 on the store, as the reference's assignment into its float32 memmap does."""
    out = np.zeros((len(queries), len(groups) - 1), dtype=np.float32)
    for i, q in enumerate(queries):
        for j in range(len(groups) - 1):
            out[i, j] = fn(q, gallery[groups[j]:groups[j + 1]], lcs)
    return out


def caption_relevance(captions, caps_per_img=5, lcs=lcs_bits):
    """The reference's relevance file of a caption list: rows = captions, columns = images."""
    toks = [tokens(c) for c in captions]
    return relevance(toks, toks, list(range(0, len(toks) + 1, caps_per_img)), lcs)


def csr(seqs):
    """Token-id sequences -> (int32 tokens, int64 offsets)."""
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    tok = np.concatenate([np.asarray(s, dtype=np.int64) for s in seqs]).astype(np.int32) if len(seqs) else np.zeros(0, np.int32)
    return tok, off
