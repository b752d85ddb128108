"""Device-resident, length-packed fp16 embedding store for evaluation.

The reference's encode_data (alad/evaluation.py:80-155) copies every batch to the host into
(N, 71, D) fp32 buffers and i2t / t2i copy slices back per query.  A PackedSetStore keeps what the
two retrieval heads read and nothing else:

    rows   fp16 (total_rows, Dp)  the positions [1, len - tail) of every set, L2-normalised exactly
                                  as the alignment pack kernels do, contiguous by TRUE length
    glob   fp32 (N, D)            the slot-0 global embedding (matching head, alad/evaluation.py:127-128)
    lengths                       the raw length list the reference returns

COCO-5k captions (25 000 x ~12 scored words x 768) take 0.46 GB instead of 5.4 GB; alignment scores
computed from a store are bit-identical to those computed from the fp32 sets (same fp16 operands).
"""
import collections

import torch

from . import _lib, eval_grid, ops


class PackedSetStore:
    def __init__(self, feat_dim, tail, device, capacity_rows=4096, precision='split', padded_len=71):
        """tail = trailing positions the alignment head drops: 0 for image sets, 2 for captions
        (reference alad/loss.py:87-90).  precision: 'split' keeps every unit vector as an fp16 hi/lo pair
        (rows twice as wide) so that alignment scores are rank-exact (ops.set_eval_precision); 'fp16' keeps
        the single-rounding training operand.  padded_len: the length the reference's encode_data pads every
        set to (max_len = 71, alad/evaluation.py:98-99): a sample shorter than that competes with the zero
        fill in the max over regions (alad/loss.py:116,124), one that fills it does not."""
        lib = _lib.load()
        self.D = int(feat_dim)
        self.precision = precision
        self.padded_len = int(padded_len)
        self.Dp = int(lib.aladin_store_row_width(self.D, ops._precision_code(precision)))
        if self.Dp < self.D:
            raise ValueError('aladin_amd: bad feature size %r' % (feat_dim,))
        self.tail = int(tail)
        self.device = torch.device(device)
        self.rows = torch.empty((max(int(capacity_rows), 1), self.Dp), dtype=torch.float16, device=self.device)
        self.n_rows = 0
        self.lengths = []                     # raw lengths, as the reference's encode_data returns them
        self._counts = []                     # usable positions per sample (host copy)
        self._glob, self._offsets_t, self._counts_t = [], None, None

    # ------------------------------------------------------------------------------------------ filling
    def _reserve(self, extra):
        need = self.n_rows + extra
        if need > self.rows.shape[0]:
            grown = torch.empty((max(need, 2 * self.rows.shape[0]), self.Dp), dtype=torch.float16, device=self.device)
            grown[:self.n_rows] = self.rows[:self.n_rows]
            self.rows = grown

    def append(self, sets, lengths, glob=None):
        """sets: (B, L, D) fp32 on the device (any strides with a unit inner stride); lengths: B ints;
        glob: (B, D) global embeddings for the matching head (defaults to slot 0 of the sets)."""
        ops._require_gpu(sets)
        B, L, D = sets.shape
        if D != self.D or len(lengths) != B:
            raise ValueError('aladin_amd: store.append got a (%d,%d,%d) batch with %d lengths (store D=%d)'
                             % (B, L, D, len(lengths), self.D))
        lengths = [int(v) for v in lengths]
        if L > self.padded_len:
            raise ValueError('aladin_amd: store.append got sets of %d positions, more than padded_len=%d' % (L, self.padded_len))
        counts = [min(max(v - 1 - self.tail, 0), L - 1) for v in lengths]
        offs, run = [], self.n_rows
        for c in counts:
            offs.append(run)
            run += c
        self._reserve(run - self.n_rows)
        sets = ops._rows_inner_contig(sets)
        lens_t = torch.tensor(lengths, dtype=torch.int32, device=self.device)
        offs_t = torch.tensor(offs, dtype=torch.int64, device=self.device)
        if L >= 2:
            _lib.check(_lib.load().aladin_store_append(ops._ptr(sets), sets.stride(0), sets.stride(1), ops._ptr(lens_t), B, L,
                                                            D, self.tail, ops._ptr(offs_t), ops._ptr(self.rows),
                                                            ops._precision_code(self.precision), ops._stream()),
                       'store_append')
        self._glob.append((sets[:, 0, :] if glob is None else glob).to(torch.float32).clone())
        self.n_rows = run
        self.lengths.extend(lengths)
        self._counts.extend(counts)
        self._offsets_t = self._counts_t = None

    # ------------------------------------------------------------------------------------------ reading
    def __len__(self):
        return len(self.lengths)

    @property
    def glob(self):
        if len(self._glob) != 1:
            self._glob = [torch.cat(self._glob)] if self._glob else [torch.empty((0, self.D), device=self.device)]
        return self._glob[0]

    def nbytes(self):
        return self.n_rows * self.Dp * 2 + len(self) * (self.D * 4 + 12)      # Dp already counts hi and lo for split stores

    def _tables(self):
        if self._offsets_t is None:
            offs, run = [], 0
            for c in self._counts:
                offs.append(run)
                run += c
            self._offsets_t = torch.tensor(offs, dtype=torch.int64, device=self.device)
            self._counts_t = torch.tensor(self._counts, dtype=torch.int32, device=self.device)
        return self._offsets_t, self._counts_t

    def view(self, index):
        """A selection (slice or index list) sharing this store's rows, e.g. store.view(slice(0, None, 5))
        for the de-duplicated images of alad/evaluation.py:171."""
        ids = list(range(len(self)))[index] if isinstance(index, slice) else [int(v) for v in index]
        return StoreView(self, ids)

    def max_count(self, ids=None):
        cs = self._counts if ids is None else [self._counts[k] for k in ids]
        return max(cs) if cs else 0


class StoreView:
    def __init__(self, store, ids):
        self.store, self.ids = store, ids
        self._ids_t = None

    def __len__(self):
        return len(self.ids)

    @property
    def lengths(self):
        return [self.store.lengths[k] for k in self.ids]

    @property
    def glob(self):
        return self.store.glob.index_select(0, self.ids_t.to(torch.int64))

    @property
    def ids_t(self):
        if self._ids_t is None:
            self._ids_t = torch.tensor(self.ids, dtype=torch.int32, device=self.store.device)
        return self._ids_t


def _unwrap(x):
    return (x.store, x.ids, x.ids_t) if isinstance(x, StoreView) else (x, None, None)


def _check_pair(img, cap):
    """What every score of two stores / views needs: samples on both sides, one feature size, one precision."""
    si, sc = getattr(img, 'store', img), getattr(cap, 'store', cap)
    if len(img) < 1 or len(cap) < 1:
        raise ValueError('aladin_amd: empty store')
    if si.D != sc.D:
        raise ValueError('aladin_amd: feature sizes differ (%d vs %d)' % (si.D, sc.D))
    if si.precision != sc.precision:
        raise ValueError('aladin_amd: the two stores hold different precisions (%s vs %s)' % (si.precision, sc.precision))


def alignment_scores_from_stores(img, cap):
    """(N_img, N_cap) 'MrSw' scores (reference alad/loss.py:80-125) between two stores / views: operands are row copies of the
    stores (no fp32 read, no normalisation).  The grid is eval_grid.score_grid's, as for tensors: length classes for large
    ragged grids, caption chunks under eval_grid's scratch limit, and the zero fill of every image shorter than padded_len."""
    _check_pair(img, cap)
    return eval_grid.score_grid(eval_grid.StoreSide(img), eval_grid.StoreSide(cap), getattr(img, 'store', img).precision)


def _pair_sides(img, cap, cand, direction, who):
    """The checks of every call on LISTED pairs of two stores / views, and the two sides as ops.align_rescore takes them."""
    from .evaluation import _is_packed_store
    if not (_is_packed_store(img) and _is_packed_store(cap)):
        raise ValueError('aladin_amd: %s takes two stores / views, not tensors' % who)
    if direction not in ('i2t', 't2i'):
        raise ValueError("direction must be 'i2t' or 't2i'")
    _check_pair(img, cap)
    si, ids_i, idt_i = _unwrap(img)
    sc, ids_c, idt_c = _unwrap(cap)
    ops._check_shortlist(cand, len(img) if direction == 'i2t' else len(cap))
    oi, ci = si._tables()
    oc, cc = sc._tables()
    x = (si.rows, oi, ci, idt_i, len(img), si.max_count(ids_i))
    y = (sc.rows, oc, cc, idt_c, len(cap), sc.max_count(ids_c))
    return si, sc, x, y


def alignment_scores_for_pairs(img, cap, cand, direction='i2t'):
    """(n_q, k) float32 'MrSw' scores of LISTED pairs between two stores / views: direction='i2t' scores image q against the
    captions cand[q, :], 't2i' caption q against the images cand[q, :].  cand: (n_q, k) int32 device tensor of positions in the
    gallery view (a search_topk shortlist), -1 = no candidate (-inf in the result).  The rows are read where they lie in the
    stores (ops.align_rescore): work and memory follow n_q * k, not the grid, and a pair's bits do not depend on where it is
    listed.  Semantics are those of alignment_scores_from_stores (zero fill for images shorter than the padded set included)."""
    si, sc, x, y = _pair_sides(img, cap, cand, direction, 'alignment_scores_for_pairs')
    return ops.align_rescore(x, y, cand, 1 if direction == 'i2t' else 0, si.D, si.precision, si.padded_len - 1 - si.tail)


PairAlignment = collections.namedtuple('PairAlignment', 'score word_region word_cos region_word region_cos')


def alignment_map_for_pairs(img, cap, cand, direction='i2t', words=True, regions=True):
    """The alignment behind alignment_scores_for_pairs, for the same LISTED pairs of two stores / views: a PairAlignment of
    score (n_q, k) float32 -- alignment_scores_for_pairs' bits; word_region int32 / word_cos float32 (n_q, k, max words of the
    caption view): for every word the region that carried the max over regions, and that cosine; region_word / region_cos
    (n_q, k, max regions of the image view): for every region the word it matches best.  An index is the position among the
    sample's scored rows, i.e. position index + 1 of the padded set.  Ties -> the lowest index.  -1 / 0.0: the zero fill of a
    side shorter than its padded set won (every real cosine < 0), the entry lies past the sample's count, or the slot holds no
    candidate (score -inf).  words=False / regions=False: that pair of outputs is None (and is not computed)."""
    si, sc, x, y = _pair_sides(img, cap, cand, direction, 'alignment_map_for_pairs')
    return PairAlignment(*ops.align_pair_map(x, y, cand, 1 if direction == 'i2t' else 0, si.D, si.precision, si.padded_len - 1 - si.tail,
                                             sc.padded_len - 1 - sc.tail, words=words, regions=regions))
