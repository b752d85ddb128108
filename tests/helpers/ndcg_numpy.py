"""A numpy restatement of the nDCG that aladin_ndcg computes (include/aladin_hip.h): the arithmetic of reference
alad/evaluate_utils/dcg.py:169-216 -- float32 gains 2 ** rel - 1, double discounts log2(r + 2), double sums -- with the two rules
the reference leaves open stated: k = min(rank, gallery), and an entry outside [0, gallery) is "no item" (adds nothing, keeps its
position's discount).  tests/test_ndcg_cpu.py pins it to the reference's recorded values; the GPU tests compare with it."""
import numpy as np

GAIN_ULP = 2.0 ** -23                # one ulp of a float32 in [1, 2): the accuracy assumed of exp2f and of glibc's float32 power


def ndcg_parts(rel, ranking, rank=None):
    """(ndcg, dcg, ideal) of one query: rel (gallery,) float32 relevances, ranking the listed gallery positions, best first."""
    rel = np.asarray(rel, dtype=np.float32).reshape(-1)
    ranking = np.asarray(ranking).reshape(-1).astype(np.int64)
    k = min(len(ranking) if rank is None else int(rank), len(rel))
    lst = ranking[:k]
    ok = (lst >= 0) & (lst < len(rel))
    gains = np.zeros(k, dtype=np.float32)
    gains[ok] = 2 ** rel[lst[ok]] - 1                    # float32, as on the reference's float32 memmap
    disc = np.log2(np.arange(k) + 2)
    dcg = float(np.sum(gains / disc))
    top = rel[np.argsort(rel)[::-1][:k]]                 # gathered (contiguous) like the reference's: numpy's float32 power is
    best = float(np.sum((2 ** top - 1) / disc))          # not bit-identical between its contiguous and its strided loop
    return (0.0 if best == 0 else dcg / best), dcg, best


def ndcg_table(rel, rankings, dim=1, rank=None):
    """ndcg_parts for every query of a relevance matrix: its rows (dim=1) or its columns (dim=0) -> three float64 (n_q,) arrays."""
    rel = np.asarray(rel, dtype=np.float32)
    rows = rel if dim == 1 else rel.T
    out = np.array([ndcg_parts(rows[q], rankings[q], rank) for q in range(len(rankings))], dtype=np.float64).reshape(-1, 3)
    return out[:, 0], out[:, 1], out[:, 2]


def ndcg_bound(best, k):
    """The derived tolerance on nDCG for a query with ideal DCG `best` at k counted positions: two implementations whose float32
    2^rel are each within 1 ulp differ by at most 2 ulp per gain, in the numerator and in the denominator, everything else being
    double:  2 * (2 * 2^-23) * sum_{r<k} 1 / log2(r + 2) / best.  0 where best == 0 (both sides give exactly 0)."""
    best = np.asarray(best, dtype=np.float64)
    s = float(np.sum(1.0 / np.log2(np.arange(int(k)) + 2)))
    return np.where(best > 0, 2 * (2 * GAIN_ULP) * s / np.where(best > 0, best, 1.0), 0.0)
