"""nDCG scorer with the reference's call surface, computed on the GPU: the drop-in for alad/evaluate_utils/dcg.py.

    DCG                                      <- alad/evaluate_utils/dcg.py:7-33 (same relevance files, same window arithmetic)
    DCG.compute_ndcg_batch                   new: every query of a fold window in one launch
    DCG.from_captions                        new: the 'rougeL' scorer of a split's captions, its relevance matrix computed on the device
                                             (aladin_amd/rouge.py) instead of read from a precomputed file
    ndcg_from_ranking / dcg_from_ranking     <- alad/evaluate_utils/dcg.py:169-216

The reference takes two numpy.argsorts per query and relevance method on the host; here a fold window of the relevance matrix is
uploaded once and ops.ndcg_from_ranking (csrc/ndcg.hip) grades every ranked list of the window in one launch.  The ideal DCG
depends on the data set and the rank only, so the scorer keeps it: the first call on a window runs the fused kernel, later calls
skip the selection (same bits).  The precision / average-precision helpers of the reference file are not mirrored.

One deviation: an entry of a ranking that is -1 or outside the window is "no item" and adds nothing; numpy would wrap a negative
index or raise on a large one.
"""
import os

import numpy as np
import torch

from . import ops

CAPS_PER_IMG = 5


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('aladin_amd: nDCG is computed by a HIP kernel on an MI355X only (no GPU visible, no CPU fallback exists)')
    return torch.device('cuda', torch.cuda.current_device())


def _ranking_table(rankings, dev):
    """-> (n_q, width) int32 device tensor from a tensor, an array or nested lists of gallery positions."""
    if isinstance(rankings, torch.Tensor):
        t = rankings
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(rankings)).astype(np.int64, copy=False))
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError('aladin_amd: rankings must be an (n_q, k >= 1) table of gallery positions')
    return t.to(dev, torch.int32)


def _as_row(ranking):
    """One query's ranking (list, array or tensor) as a (1, k) table."""
    return ranking.reshape(1, -1) if isinstance(ranking, torch.Tensor) else np.asarray(ranking).reshape(1, -1)


class DCG:
    """reference alad/evaluate_utils/dcg.py:7-33.  The relevance matrices are the reference's raw float32 files
    <data>/<name>/relevances/<name>-<split>-<method>.npy (memory maps shaped (n_queries, -1): rows = captions, columns = images),
    or, with the trailing relevances=, a list of 2-D arrays / tensors in the order of relevance_methods."""

    def __init__(self, config, n_queries, split, rank=25, relevance_methods=['rougeL'], relevances=None):
        self.rank = int(rank)
        self.relevance_methods = list(relevance_methods)
        if self.rank < 1:
            raise ValueError('DCG: rank must be >= 1 (got %d)' % self.rank)
        if relevances is None:
            name = config['dataset']['name']
            relevance_dir = os.path.join(config['dataset']['data'], name, 'relevances')
            files = [os.path.join(relevance_dir, '{}-{}-{}.npy'.format(name, split, m)) for m in self.relevance_methods]
            self.relevances = [np.memmap(f, dtype=np.float32, mode='r') for f in files]
            for r in self.relevances:
                r.shape = (n_queries, -1)
        else:
            relevances = list(relevances)
            if len(relevances) != len(self.relevance_methods):
                raise ValueError('DCG: %d relevance matrices for %d methods' % (len(relevances), len(self.relevance_methods)))
            self.relevances = relevances
            for r in self.relevances:
                if len(r.shape) != 2 or r.shape[0] != n_queries or r.shape[1] < 1:
                    raise ValueError('DCG: a relevance matrix must be (n_queries=%d, n_images), got %s' % (n_queries, tuple(r.shape)))
        self._windows = {}           # (method index, npts, fold_index) -> (5*npts, npts) float32 device tensor, both retrieval kinds
        self._ideals = {}            # (method index, npts, fold_index, retrieval) -> (rank, float64 (n_q,) ideal DCG)

    @classmethod
    def from_captions(cls, captions, rank=25, caps_per_img=5):
        """A 'rougeL' scorer straight from the captions of a split (image j owns captions 5j .. 5j + 4): the relevance matrix is
        computed on the device (aladin_amd.rouge.relevance_matrix) instead of being read from the reference's precomputed file."""
        if int(caps_per_img) != CAPS_PER_IMG:
            raise ValueError('DCG: the fold windows hold %d captions per image (got caps_per_img=%d)' % (CAPS_PER_IMG, caps_per_img))
        from .rouge import relevance_matrix
        rel = relevance_matrix(captions, caps_per_img)
        return cls(None, rel.shape[0], None, rank=rank, relevance_methods=['rougeL'], relevances=[rel])

    def clear(self):
        """Drop the uploaded fold windows and their ideal DCGs."""
        self._windows.clear()
        self._ideals.clear()

    @staticmethod
    def _window_shape(npts, retrieval):
        """(queries, gallery) of a fold window, reference dcg.py:22-29."""
        if retrieval == 'image':
            return CAPS_PER_IMG * npts, npts
        if retrieval == 'sentence':
            return npts, CAPS_PER_IMG * npts
        raise ValueError("DCG: retrieval must be 'image' or 'sentence'")

    def _check_window(self, npts, fold_index, retrieval):
        npts, fold_index = int(npts), int(fold_index)
        self._window_shape(npts, retrieval)
        rows, cols = self.relevances[0].shape
        if npts < 1 or fold_index < 0 or CAPS_PER_IMG * npts * (fold_index + 1) > rows or npts * (fold_index + 1) > cols:
            raise ValueError('DCG: fold %d of %d images (captions %d..%d, images %d..%d) lies outside the %d x %d relevance matrix'
                             % (fold_index, npts, CAPS_PER_IMG * npts * fold_index, CAPS_PER_IMG * npts * (fold_index + 1),
                                npts * fold_index, npts * (fold_index + 1), rows, cols))
        return npts, fold_index

    def _window(self, m, npts, fold_index):
        """The fold's block of relevance matrix m on the device: rows = the fold's captions, columns = its images.  retrieval='image'
        reads its rows as queries, 'sentence' its columns (in place)."""
        key = (m, npts, fold_index)
        win = self._windows.get(key)
        if win is None:
            r = self.relevances[m]
            blk = r[CAPS_PER_IMG * npts * fold_index:CAPS_PER_IMG * npts * (fold_index + 1), npts * fold_index:npts * (fold_index + 1)]
            if isinstance(blk, torch.Tensor):
                win = blk.to(_device(), torch.float32).contiguous()
            else:
                win = torch.from_numpy(np.array(blk, dtype=np.float32, order='C')).to(_device())      # a copy: the memory map is read-only
            self._windows[key] = win
        return win

    def _grade(self, m, npts, fold_index, retrieval, table, rank, first=0):
        """nDCG of the table's rows = queries first .. first + rows of the window, by method m."""
        win = self._window(m, npts, fold_index)
        n_q, _ = self._window_shape(npts, retrieval)
        rows = table.shape[0]
        dim = 1 if retrieval == 'image' else 0
        rel = win[first:first + rows] if dim == 1 else win[:, first:first + rows]
        key = (m, npts, fold_index, retrieval)
        kept = self._ideals.get(key)
        if kept is not None and kept[0] == rank:
            return ops.ndcg_from_ranking(rel, table, dim=dim, rank=rank, ideal=kept[1][first:first + rows])
        ndcg, _, ideal = ops.ndcg_from_ranking(rel, table, dim=dim, rank=rank, return_parts=True)
        if rows == n_q:
            self._ideals[key] = (rank, ideal)
        return ndcg

    def compute_ndcg(self, npts, query_id, sorted_indexes, fold_index=0, retrieval='image'):
        """reference dcg.py:19-33: {method: nDCG} of one query's ranking (its first `rank` entries) inside fold `fold_index` of
        `npts` images.  Python floats; the same device op as compute_ndcg_batch with one query."""
        npts, fold_index = self._check_window(npts, fold_index, retrieval)
        n_q, _ = self._window_shape(npts, retrieval)
        query_id = int(query_id)
        if not 0 <= query_id < n_q:
            raise ValueError('DCG: query %d outside the fold\'s %d queries' % (query_id, n_q))
        table = _ranking_table(_as_row(sorted_indexes)[:, :self.rank], _device())
        return {name: float(self._grade(m, npts, fold_index, retrieval, table, table.shape[1], first=query_id).item())
                for m, name in enumerate(self.relevance_methods)}

    def compute_ndcg_batch(self, npts, rankings, fold_index=0, retrieval='image'):
        """{method: float64 (n_q,) device tensor}: row i of `rankings` (an (n_q, k) table of gallery positions inside the fold, best
        first; its first min(k, rank) entries count) is query i of the fold -- caption 5*npts*fold_index + i ('image') or image
        npts*fold_index + i ('sentence')."""
        npts, fold_index = self._check_window(npts, fold_index, retrieval)
        n_q, _ = self._window_shape(npts, retrieval)
        table = _ranking_table(rankings, _device())
        if table.shape[0] > n_q:
            raise ValueError('DCG: %d rankings for the fold\'s %d queries' % (table.shape[0], n_q))
        rank = min(self.rank, table.shape[1])
        return {name: self._grade(m, npts, fold_index, retrieval, table, rank) for m, name in enumerate(self.relevance_methods)}


def _single(y_true, ranking):
    dev = _device()
    y = torch.as_tensor(np.asarray(y_true, dtype=np.float32) if not isinstance(y_true, torch.Tensor) else y_true)
    if y.dim() != 1 or y.shape[0] < 1:
        raise ValueError('aladin_amd: y_true must be a non-empty 1-D array of relevances')
    table = _ranking_table(_as_row(ranking), dev)
    return ops.ndcg_from_ranking(y.to(dev, torch.float32).reshape(1, -1), table, return_parts=True)


def dcg_from_ranking(y_true, ranking):
    """reference dcg.py:169-191: the DCG of one ranking against the relevance vector y_true, a Python float."""
    return float(_single(y_true, ranking)[1].item())


def ndcg_from_ranking(y_true, ranking):
    """reference dcg.py:194-216: DCG / ideal DCG at k = len(ranking), 0 where the ideal is 0; a Python float."""
    return float(_single(y_true, ranking)[0].item())
