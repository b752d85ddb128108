"""Matching-head retrieval over the C ABI: the stored similarity matrix, rank kernels, the fused screened retrieval, top-k lists
(reference alad/recall_auxiliary.py:30-56, alad/evaluation.py:196-223,285-309)."""
import ctypes as C

import torch

from . import _lib
from ._ops_common import _RAW_STREAM, _stream, _ptr, _require_gpu, _rows_inner_contig, _LEN_CACHE, lengths_tensor, _ld, _workspace


# ------------------------------------------------------------------------------------------------
# retrieval
# ------------------------------------------------------------------------------------------------
def sim_matrix(img, cap):
    """(n_img, n_cap) = img @ cap.T on the split-fp16 MFMA path (no autograd); replaces
    ims.mm(caps.t()), reference alad/recall_auxiliary.py:30 and alad/evaluation.py:196,285."""
    _require_gpu(img, cap)
    lib = _lib.load()
    img = img if img.stride(1) == 1 else img.contiguous()
    cap = cap if cap.stride(1) == 1 else cap.contiguous()
    n_img, D = img.shape
    n_cap = cap.shape[0]
    sim = torch.empty((n_img, n_cap), dtype=torch.float32, device=img.device)
    ws = _workspace(lib.aladin_sim_workspace_bytes(n_img, n_cap, D), img.device)
    _lib.check(lib.aladin_sim_matrix(_ptr(img), _ld(img), _ptr(cap), _ld(cap), n_img, n_cap, D, _ptr(sim),
                                     _ld(sim), _ptr(ws), _stream()), 'sim_matrix')
    return sim


def _rank_outputs(n_img, n_cap, dev):
    """(rank_i2t, top1_i2t, rank_t2i, top1_t2i): uninitialised int32 outputs of the two rank entry points."""
    return tuple(torch.empty(n, dtype=torch.int32, device=dev) for n in (n_img, n_img, n_cap, n_cap))


def recall_ranks(sim, caps_per_img=5):
    """(rank_i2t, top1_i2t, rank_t2i, top1_t2i) int32 device tensors from a (n_img, 5*n_img) score
    matrix; replaces the argsort/where loops of reference alad/recall_auxiliary.py:34-56."""
    _require_gpu(sim)
    lib = _lib.load()
    sim = sim if sim.stride(1) == 1 else sim.contiguous()
    n_img, n_cap = sim.shape
    dev = sim.device
    r_i2t, t_i2t, r_t2i, t_t2i = _rank_outputs(n_img, n_cap, dev)
    ws = _workspace(lib.aladin_recall_workspace_bytes(n_cap), dev)
    _lib.check(lib.aladin_recall_ranks(_ptr(sim), _ld(sim), n_img, n_cap, caps_per_img, _ptr(r_i2t), _ptr(t_i2t),
                                       _ptr(r_t2i), _ptr(t_t2i), _ptr(ws), _stream()), 'recall_ranks')
    return r_i2t, t_i2t, r_t2i, t_t2i


def retrieval_ranks(img, cap, caps_per_img=5, exact=False, return_stats=False):
    """(rank_i2t, top1_i2t, rank_t2i, top1_t2i) straight from the (n_img, D) / (n_cap, D) embeddings:
    sim_matrix + recall_ranks fused, the (n_img, n_cap) score matrix is never written.  Same bits as
    the two-step path; replaces reference alad/recall_auxiliary.py:30-56 in one pass.
    The kernel screens with the hi.hi third of the split product and continues to the exact score only the pairs a
    rigorous per-pair bound leaves undecided (include/aladin_hip.h); exact=True forces the three-product path on
    every tile (same outputs).  return_stats=True appends {'exact_tiles', 'listed_pairs', 'rescored_pairs', 'skipped_tiles', 'tiles'}
    (one D2H copy): tiles continued in place, pairs listed, listed pairs whose chains were continued, tiles that skipped the screen.
    The four outputs are deterministic; these statistics (and the call's duration) are NOT -- a tile decides whether to skip its
    analysis from what earlier tiles of the same launch have reported so far, which depends on scheduling.  Only
    rescored_pairs <= listed_pairs and skipped_tiles <= exact_tiles <= tiles hold run to run."""
    _require_gpu(img, cap)
    if img.dim() != 2 or cap.dim() != 2 or img.shape[1] != cap.shape[1]:
        raise ValueError('aladin_amd: (n_img,D) and (n_cap,D) embeddings expected')
    lib = _lib.load()
    img = img if img.stride(1) == 1 else img.contiguous()
    cap = cap if cap.stride(1) == 1 else cap.contiguous()
    n_img, n_cap, D = img.shape[0], cap.shape[0], img.shape[1]
    dev = img.device
    r_i2t, t_i2t, r_t2i, t_t2i = _rank_outputs(n_img, n_cap, dev)
    ws = _workspace(lib.aladin_retrieval_workspace_bytes(n_img, n_cap, D), dev)
    fn = lib.aladin_retrieval_ranks_exact if exact else lib.aladin_retrieval_ranks
    _lib.check(fn(_ptr(img), img.stride(0), _ptr(cap), cap.stride(0), n_img, n_cap, D, caps_per_img,
                  _ptr(r_i2t), _ptr(t_i2t), _ptr(r_t2i), _ptr(t_t2i), _ptr(ws), _stream()), 'retrieval_ranks')
    if return_stats:
        off = lib.aladin_retrieval_stats_offset(n_img, n_cap, D)
        st = ws[off:off + 36].view(torch.int32).cpu().tolist()
        tiles = -(-n_img // 256) * -(-n_cap // 384)
        return r_i2t, t_i2t, r_t2i, t_t2i, {'exact_tiles': st[0], 'listed_pairs': st[1], 'rescored_pairs': st[5], 'skipped_tiles': st[8],
                                            'tiles': tiles}
    return r_i2t, t_i2t, r_t2i, t_t2i


def topk_indices(scores, k, dim=1):
    """(n_q, k) int32 indices of each query's k best candidates, best first, ties -> lower index; queries are
    the rows of `scores` (dim=1) or its columns (dim=0, read in place: no transpose).  Replaces the
    `inds[i][0:50]` slices of the descending argsorts in reference alad/evaluation.py:303-309 (-1 past the
    number of candidates)."""
    _require_gpu(scores)
    if scores.dim() != 2 or dim not in (0, 1):
        raise ValueError('aladin_amd: topk_indices expects a 2-D score matrix and dim 0 or 1')
    sc = scores if scores.stride(1) == 1 else scores.contiguous()
    n_q, n_c = (sc.shape[0], sc.shape[1]) if dim == 1 else (sc.shape[1], sc.shape[0])
    q_stride, c_stride = (_ld(sc), 1) if dim == 1 else (1, _ld(sc))
    out = torch.empty((n_q, int(k)), dtype=torch.int32, device=sc.device)
    _lib.check(_lib.load().aladin_topk(_ptr(sc), q_stride, c_stride, n_q, n_c, int(k), _ptr(out), _ptr(None), _stream()),
               'topk')
    return out


SEARCH_MAX_K = 256
SEARCH_MAX_GALLERY = 36864 * 16      # groups of 16 gallery items, at most topk's 36864 candidates of them


def search_topk(img, cap, k, dim=1, return_scores=False):
    """(n_q, k) int32 indices of each query's k best gallery items straight from the (n_img, D) / (n_cap, D) embeddings:
    sim_matrix + topk_indices fused, the (n_img, n_cap) score matrix is never written and the gallery may hold up to
    589824 items.  dim=1: images query the captions; dim=0: captions query the images (the operands keep their roles, as in
    topk_indices(sim_matrix(img, cap), k, dim)).  Best first, ties -> lower index, -1 past the gallery size; the same ints as
    the two-step path.  return_scores=True: (indices, scores), the scores bit-equal to sim_matrix's entries (-inf past the
    gallery size)."""
    if img.dim() != 2 or cap.dim() != 2 or img.shape[1] != cap.shape[1] or dim not in (0, 1):
        raise ValueError('aladin_amd: search_topk expects (n_img,D) and (n_cap,D) embeddings and dim 0 or 1')
    k = int(k)
    if not 1 <= k <= SEARCH_MAX_K:
        raise ValueError('aladin_amd: search_topk needs 1 <= k <= %d (got %d)' % (SEARCH_MAX_K, k))
    n_img, n_cap, D = img.shape[0], cap.shape[0], img.shape[1]
    n_q, n_g = (n_img, n_cap) if dim == 1 else (n_cap, n_img)
    if n_g > SEARCH_MAX_GALLERY:
        raise ValueError('aladin_amd: search_topk searches at most %d gallery items (got %d)' % (SEARCH_MAX_GALLERY, n_g))
    if n_img < 1 or n_cap < 1 or D < 1:
        raise ValueError('aladin_amd: search_topk needs non-empty embeddings')
    _require_gpu(img, cap)                               # after the limits: they hold whatever the device
    lib = _lib.load()
    img = img if img.stride(1) == 1 else img.contiguous()
    cap = cap if cap.stride(1) == 1 else cap.contiguous()
    dev = img.device
    idx = torch.empty((n_q, k), dtype=torch.int32, device=dev)
    val = torch.empty((n_q, k), dtype=torch.float32, device=dev) if return_scores else None
    ws = _workspace(lib.aladin_search_workspace_bytes(n_img, n_cap, D, k, dim), dev)
    _lib.check(lib.aladin_search_topk(_ptr(img), _ld(img), _ptr(cap), _ld(cap), n_img, n_cap, D, k, dim, _ptr(idx), _ptr(val),
                                      _ptr(ws), _stream()), 'search_topk')
    return (idx, val) if return_scores else idx


SEARCH_INDEX_STREAM_MAX_Q = 32       # queries of D <= 768 that take the one-pass route of an index search (STREAM_MAX_Q, csrc/search.hip)
SEARCH_INDEX_STREAM_MAX_D = 768


class SearchIndex:
    """A gallery packed once for search_index_topk: the device buffer of aladin_search_index_build, the gallery's n and D.
    Immutable; it cannot be appended to (a new absmax would rescale the rows already packed) -- build a new one."""

    __slots__ = ('buf', 'n', 'D')

    def __init__(self, buf, n, D):
        self.buf, self.n, self.D = buf, n, D

    def __len__(self):
        return self.n

    @property
    def device(self):
        return self.buf.device


def build_search_index(gallery):
    """SearchIndex of an (n, D) float32 device tensor of matching-head embeddings, images or captions alike: the rows packed
    [hi | lo] with one power-of-two scale (the operand format of sim_matrix), up to 589824 of them.  The gallery tensor is not
    needed afterwards."""
    if not isinstance(gallery, torch.Tensor) or gallery.dim() != 2:
        raise ValueError('aladin_amd: build_search_index expects an (n,D) embedding tensor')
    n, D = gallery.shape
    if n > SEARCH_MAX_GALLERY:
        raise ValueError('aladin_amd: build_search_index indexes at most %d gallery items (got %d)' % (SEARCH_MAX_GALLERY, n))
    if n < 1 or D < 1:
        raise ValueError('aladin_amd: build_search_index needs non-empty embeddings')
    _require_gpu(gallery)
    lib = _lib.load()
    gallery = gallery if gallery.stride(1) == 1 else gallery.contiguous()
    buf = torch.empty(int(lib.aladin_search_index_bytes(n, D)), dtype=torch.uint8, device=gallery.device)
    _lib.check(lib.aladin_search_index_build(_ptr(gallery), _ld(gallery), n, D, _ptr(buf), _stream()), 'search_index_build')
    return SearchIndex(buf, n, D)


def search_index_topk(index, queries, k, dim=1, return_scores=False):
    """search_topk with the gallery taken from a SearchIndex: (n_q, k) int32 indices of each query's k best gallery items, the same
    ints (and, with return_scores=True, the same score bits) as search_topk on the fp32 gallery.  dim=1: the (n_q, D) queries are
    images and the index holds captions; dim=0: the queries are captions and the index holds images.  Only the queries are
    packed per call; up to 32 queries of D <= 768 read the gallery once."""
    if not isinstance(index, SearchIndex) or queries.dim() != 2 or queries.shape[1] != index.D or dim not in (0, 1):
        raise ValueError('aladin_amd: search_index_topk expects a SearchIndex, (n_q,D) embeddings of its D and dim 0 or 1')
    k = int(k)
    if not 1 <= k <= SEARCH_MAX_K:
        raise ValueError('aladin_amd: search_index_topk needs 1 <= k <= %d (got %d)' % (SEARCH_MAX_K, k))
    n_q, D = queries.shape
    if n_q < 1:
        raise ValueError('aladin_amd: search_index_topk needs non-empty embeddings')
    _require_gpu(queries)
    if queries.device != index.device:
        raise RuntimeError('aladin_amd: the queries are on %s, the index on %s' % (queries.device, index.device))
    lib = _lib.load()
    queries = queries if queries.stride(1) == 1 else queries.contiguous()
    dev = queries.device
    idx = torch.empty((n_q, k), dtype=torch.int32, device=dev)
    val = torch.empty((n_q, k), dtype=torch.float32, device=dev) if return_scores else None
    ws = _workspace(lib.aladin_search_index_workspace_bytes(n_q, index.n, D, k, dim), dev)
    _lib.check(lib.aladin_search_index_topk(_ptr(index.buf), index.n, D, _ptr(queries), _ld(queries), n_q, k, dim, _ptr(idx), _ptr(val),
                                            _ptr(ws), _stream()), 'search_index_topk')
    return (idx, val) if return_scores else idx


RESCORE_MAX_K = 256
RESCORE_MAX_COUNT = 96               # scored positions per set: the tile classes' limit


def _check_shortlist(cand, n_q=None):
    if not isinstance(cand, torch.Tensor) or cand.dim() != 2 or cand.dtype != torch.int32:
        raise ValueError('aladin_amd: the shortlist must be an (n_q, k) int32 tensor')
    if n_q is not None and cand.shape[0] != n_q:
        raise ValueError('aladin_amd: the shortlist has %d rows for %d queries' % (cand.shape[0], n_q))
    if not 1 <= cand.shape[1] <= RESCORE_MAX_K:
        raise ValueError('aladin_amd: a shortlist holds 1 <= k <= %d candidates per query (got %d)' % (RESCORE_MAX_K, cand.shape[1]))


def align_rescore(x, y, cand, dim, D, precision, x_full, out=None):
    """(n_q, k) float32 alignment-head (MrSw) scores of the listed pairs straight from two embedding stores -- no repacking,
    nothing of the size of the (n_q, gallery) grid.  x / y: the image / caption side as (rows, offsets, counts, ids or None,
    samples in the view, largest count); cand: (n_q, k) int32 gallery-view positions, -1 = none (-inf in the output);
    dim=1: images query captions, dim=0: captions query images.  out: a preallocated result (graph capture).
    aladin_amd.store.alignment_scores_for_pairs is the front end."""
    if dim not in (0, 1):
        raise ValueError('aladin_amd: align_rescore takes dim 0 or 1')
    n_q = x[4] if dim == 1 else y[4]
    _check_shortlist(cand, n_q)
    if x[5] > RESCORE_MAX_COUNT or y[5] > RESCORE_MAX_COUNT:
        raise ValueError('aladin_amd: align_rescore scores sets of at most %d positions (got %d regions, %d words)'
                         % (RESCORE_MAX_COUNT, x[5], y[5]))
    if not cand.is_cuda:
        raise RuntimeError('aladin_amd: the shortlist must live on the GPU (no CPU fallback exists)')
    cand = cand.contiguous()
    if out is None:
        out = torch.empty(cand.shape, dtype=torch.float32, device=cand.device)
    elif out.shape != cand.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError('aladin_amd: align_rescore needs a contiguous float32 output of the shortlist\'s shape')
    from .ops import _precision_code
    _lib.check(_lib.load().aladin_align_rescore(_ptr(x[0]), _ptr(x[1]), _ptr(x[2]), _ptr(x[3]), int(x[4]), int(x[5]),
                                                _ptr(y[0]), _ptr(y[1]), _ptr(y[2]), _ptr(y[3]), int(y[4]), int(y[5]),
                                                int(D), _precision_code(precision), int(dim), int(x_full), _ptr(cand),
                                                cand.shape[1], _ptr(out), _stream()), 'align_rescore')
    return out


def align_pair_map(x, y, cand, dim, D, precision, x_full, y_full, words=True, regions=True, out=None):
    """The alignment behind align_rescore's scores: (score, word_region, word_cos, region_word, region_cos) of the listed pairs.
    x, y, cand, dim, D, precision, x_full: as align_rescore takes them; y_full: the count at which a caption fills its padded set.
    score (n_q, k) float32: align_rescore's bits.  word_region int32 / word_cos float32, (n_q, k, y[5]): per word the best region
    (position among the image's scored rows) and its cosine; region_word / region_cos, (n_q, k, x[5]): per region the best word.
    Ties -> the lowest index; -1 / 0.0 where the zero fill of a shorter-than-padded side wins, past a sample's count and at -1
    slots (score -inf).  words=False / regions=False: that pair of outputs is None and is not computed.
    out: a preallocated 5-tuple of contiguous results (None where not requested; graph capture)."""
    if dim not in (0, 1):
        raise ValueError('aladin_amd: align_pair_map takes dim 0 or 1')
    n_q = x[4] if dim == 1 else y[4]
    _check_shortlist(cand, n_q)
    if x[5] > RESCORE_MAX_COUNT or y[5] > RESCORE_MAX_COUNT:
        raise ValueError('aladin_amd: align_pair_map maps sets of at most %d positions (got %d regions, %d words)'
                         % (RESCORE_MAX_COUNT, x[5], y[5]))
    if int(x_full) < 1 or int(y_full) < 1:
        raise ValueError('aladin_amd: align_pair_map needs x_full >= 1 and y_full >= 1 (got %d, %d)' % (x_full, y_full))
    if not cand.is_cuda:
        raise RuntimeError('aladin_amd: the shortlist must live on the GPU (no CPU fallback exists)')
    cand = cand.contiguous()
    n_q, k = cand.shape
    shapes = [((n_q, k), torch.float32), ((n_q, k, int(y[5])), torch.int32), ((n_q, k, int(y[5])), torch.float32),
              ((n_q, k, int(x[5])), torch.int32), ((n_q, k, int(x[5])), torch.float32)]
    wanted = [True, words, words, regions, regions]
    if out is None:
        out = tuple(torch.empty(sh, dtype=dt, device=cand.device) if w else None for (sh, dt), w in zip(shapes, wanted))
    elif len(out) != 5 or any((o is None) == w or (w and (tuple(o.shape) != sh or o.dtype != dt or not o.is_contiguous()))
                              for o, (sh, dt), w in zip(out, shapes, wanted)):
        raise ValueError('aladin_amd: align_pair_map needs contiguous (score, word_region, word_cos, region_word, region_cos) outputs of '
                         'the shortlist\'s shape x the views\' largest counts, None where not requested')
    from .ops import _precision_code
    _lib.check(_lib.load().aladin_align_pair_map(_ptr(x[0]), _ptr(x[1]), _ptr(x[2]), _ptr(x[3]), int(x[4]), int(x[5]),
                                                 _ptr(y[0]), _ptr(y[1]), _ptr(y[2]), _ptr(y[3]), int(y[4]), int(y[5]),
                                                 int(D), _precision_code(precision), int(dim), int(x_full), int(y_full), _ptr(cand), k,
                                                 _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), int(y[5]), _ptr(out[3]), _ptr(out[4]),
                                                 int(x[5]), _stream()), 'align_pair_map')
    return tuple(out)


def rerank_order(cand, scores, out_idx=None, out_val=None):
    """(indices, scores): every row of the shortlist `cand` and of its scores in descending score order -- a stable sort, ties go
    to the earlier shortlist slot; -1 entries last, as -1 / -inf.  out_idx / out_val: preallocated results (graph capture)."""
    _check_shortlist(cand)
    if not isinstance(scores, torch.Tensor) or scores.shape != cand.shape or scores.dtype != torch.float32:
        raise ValueError('aladin_amd: rerank_order needs float32 scores of the shortlist\'s shape')
    _require_gpu(scores)
    cand, scores = cand.contiguous(), scores.contiguous()
    if out_idx is None:
        out_idx = torch.empty_like(cand)
    if out_val is None:
        out_val = torch.empty_like(scores)
    _lib.check(_lib.load().aladin_rerank_order(_ptr(cand), _ptr(scores), cand.shape[0], cand.shape[1], _ptr(out_idx), _ptr(out_val),
                                               _stream()), 'rerank_order')
    return out_idx, out_val


NDCG_MAX_GALLERY = 36864             # relevances per query among which the ideal DCG is selected (topk's candidate limit)
NDCG_IDEAL_GIVEN = 1                 # ALADIN_NDCG_IDEAL_GIVEN of include/aladin_hip.h


def ndcg_from_ranking(rel, ranking, dim=1, rank=None, ideal=None, return_parts=False):
    """nDCG of n_q ranked lists, a float64 (n_q,) device tensor: dcg_from_ranking / ndcg_from_ranking of reference
    alad/evaluate_utils/dcg.py:169-216 for every query at once (exponential gain 2 ** rel - 1 in float32, discount log2(r + 2) and
    both sums in double; 0 where the ideal DCG is 0).
    rel: 2-D float32 device tensor of relevances; the queries are its rows (dim=1) or its columns (dim=0, read in place: no
    transpose), the other axis is the gallery.  ranking: (n_q, >= rank) int32, entry r of row q = the gallery position ranked r-th,
    -1 (or anything outside the gallery) = no item: it adds nothing and keeps its position's discount.  rank: how many entries
    count (default: the table's width); past the gallery size min(rank, gallery) counts.
    ideal: the float64 (n_q,) ideal DCG of the same relevances AT THE SAME rank, from an earlier call with return_parts -- the
    selection is skipped (the result's bits do not change) and the gallery limit of 36864 items does not apply.
    return_parts=True: (ndcg, dcg, ideal).  Relevances are expected finite: a NaN's effect is unspecified."""
    if not isinstance(rel, torch.Tensor) or rel.dim() != 2 or rel.dtype != torch.float32 or dim not in (0, 1):
        raise ValueError('aladin_amd: ndcg_from_ranking expects a 2-D float32 relevance tensor and dim 0 or 1')
    n_q, n_c = (rel.shape[0], rel.shape[1]) if dim == 1 else (rel.shape[1], rel.shape[0])
    if n_q < 1 or n_c < 1:
        raise ValueError('aladin_amd: ndcg_from_ranking needs a non-empty relevance matrix')
    if not isinstance(ranking, torch.Tensor) or ranking.dim() != 2 or ranking.dtype != torch.int32 or ranking.shape[0] != n_q:
        raise ValueError('aladin_amd: the ranking must be an (n_q, k) int32 tensor with one row per query (%d queries)' % n_q)
    rank = ranking.shape[1] if rank is None else int(rank)
    if not 1 <= rank <= ranking.shape[1]:
        raise ValueError('aladin_amd: ndcg_from_ranking needs 1 <= rank <= the ranking\'s width %d (got %d)' % (ranking.shape[1], rank))
    if ideal is None and n_c > NDCG_MAX_GALLERY:
        raise ValueError('aladin_amd: ndcg_from_ranking selects the ideal DCG among at most %d gallery items (got %d); pass ideal='
                         % (NDCG_MAX_GALLERY, n_c))
    if ideal is not None and (not isinstance(ideal, torch.Tensor) or ideal.dtype != torch.float64 or tuple(ideal.shape) != (n_q,)):
        raise ValueError('aladin_amd: ideal must be a float64 tensor of %d entries' % n_q)
    _require_gpu(rel)                                    # after the limits: they hold whatever the device
    if not ranking.is_cuda or (ideal is not None and not ideal.is_cuda):
        raise RuntimeError('aladin_amd: the ranking and the ideal DCG must live on the GPU (no CPU fallback exists)')
    sc = rel if rel.stride(1) == 1 else rel.contiguous()
    ranking = ranking if ranking.stride(1) == 1 else ranking.contiguous()
    q_stride, c_stride = (_ld(sc), 1) if dim == 1 else (1, _ld(sc))
    out = torch.empty((3 if ideal is None else 2, n_q), dtype=torch.float64, device=sc.device)
    best = out[2] if ideal is None else ideal.contiguous()
    _lib.check(_lib.load().aladin_ndcg(_ptr(sc), q_stride, c_stride, n_q, n_c, _ptr(ranking), _ld(ranking), rank,
                                       0 if ideal is None else NDCG_IDEAL_GIVEN, _ptr(out[0]), _ptr(out[1]), _ptr(best), _stream()),
               'ndcg')
    return (out[0], out[1], best) if return_parts else out[0]


ROUGE_MAX_LEN = 256                  # tokens of a caption the LCS kernel scores (4 words of 64 query positions); longer ones are truncated
ROUGE_CLASSES = (64, 128, 256)       # query length classes: 1, 2 or 4 words per query, one launch each
ROUGE_LCS = 1                        # ALADIN_ROUGE_LCS of include/aladin_hip.h


def _check_captions(q_tok, q_off, g_tok, g_off, grp_off):
    """The CSR operands of rouge_l: -> (n_q, n_g, n_img)."""
    for tok, off, what in ((q_tok, q_off, 'query'), (g_tok, g_off, 'gallery')):
        if not isinstance(tok, torch.Tensor) or tok.dim() != 1 or tok.dtype != torch.int32:
            raise ValueError('aladin_amd: rouge_l: the %s tokens must be a 1-D int32 tensor of ids' % what)
        if not isinstance(off, torch.Tensor) or off.dim() != 1 or off.dtype != torch.int64 or off.shape[0] < 2:
            raise ValueError('aladin_amd: rouge_l: the %s offsets must be a 1-D int64 tensor of count + 1 >= 2 entries' % what)
    if not isinstance(grp_off, torch.Tensor) or grp_off.dim() != 1 or grp_off.dtype != torch.int64 or grp_off.shape[0] < 2:
        raise ValueError('aladin_amd: rouge_l: the group offsets must be a 1-D int64 tensor of n_img + 1 >= 2 entries')
    return q_off.shape[0] - 1, g_off.shape[0] - 1, grp_off.shape[0] - 1


def _require_gpu_ints(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('aladin_amd: ROUGE-L is computed by a HIP kernel on an MI355X only; got a %s tensor '
                               '(no CPU fallback exists)' % t.device)


def rouge_l_launch(q_tok, q_off, q_max_len, g_tok, g_off, g_max_len, grp_off, out, q_rows=None, lcs=False):
    """ONE aladin_rouge_l launch into `out`, nothing read back from the device (graph-capturable): the queries are scored with
    1, 2 or 4 words by q_max_len <= 64 / 128 / 256, captions longer than q_max_len / g_max_len are truncated to it.
    out: float32, rows with a unit inner stride and n_img columns (a column slice of a wider matrix keeps its other columns);
    q_rows (int32, one per query): the row of `out` each query is written to (None: its own index).  lcs=True: the largest LCS
    length instead of the F-measure.  rouge_l_relevance is the front end that finds the lengths and splits the classes."""
    n_q, n_g, n_img = _check_captions(q_tok, q_off, g_tok, g_off, grp_off)
    q_max_len, g_max_len = int(q_max_len), int(g_max_len)
    if not (1 <= q_max_len <= ROUGE_MAX_LEN and 1 <= g_max_len <= ROUGE_MAX_LEN):
        raise ValueError('aladin_amd: rouge_l scores captions of 1 to %d tokens (got maximum lengths %d and %d)'
                         % (ROUGE_MAX_LEN, q_max_len, g_max_len))
    if q_rows is not None and (not isinstance(q_rows, torch.Tensor) or q_rows.dtype != torch.int32 or tuple(q_rows.shape) != (n_q,)):
        raise ValueError('aladin_amd: rouge_l: q_rows must be an int32 tensor with one output row per query (%d)' % n_q)
    if not isinstance(out, torch.Tensor) or out.dim() != 2 or out.dtype != torch.float32 or out.shape[1] != n_img or \
            (out.shape[1] > 1 and out.stride(1) != 1) or (q_rows is None and out.shape[0] != n_q):
        raise ValueError('aladin_amd: rouge_l needs a float32 output of %s rows x %d images with a unit inner stride'
                         % ('one row per query (%d)' % n_q if q_rows is None else 'the listed', n_img))
    _require_gpu_ints(q_tok, q_off, g_tok, g_off, grp_off, out, q_rows)
    q_tok, q_off, g_tok, g_off, grp_off = (t.contiguous() for t in (q_tok, q_off, g_tok, g_off, grp_off))
    q_rows = q_rows.contiguous() if q_rows is not None else None
    ld = out.stride(0) if out.shape[0] > 1 else max(out.stride(0), n_img)
    _lib.check(_lib.load().aladin_rouge_l(_ptr(q_tok), _ptr(q_off), _ptr(q_rows), n_q, q_max_len, _ptr(g_tok), _ptr(g_off), n_g, g_max_len,
                                          _ptr(grp_off), n_img, _ptr(out), ld, ROUGE_LCS if lcs else 0, _stream()), 'rouge_l')
    return out


def rouge_l_relevance(q_tok, q_off, g_tok, g_off, grp_off, out=None, q_rows=None, lcs=False):
    """(n_q, n_img) float32 device tensor of ROUGE-L relevances: Rouge.score of reference alad/evaluate_utils/rouge.py:46-76 for
    every (query caption, image) pair, the bits of the float32 file alad/evaluate_utils/compute_relevance.py writes.
    q_tok / g_tok: int32 token ids of the query / gallery captions, one after another (any non-negative ids: no vocabulary limit);
    q_off / g_off: int64 offsets, count + 1 entries; grp_off: int64, n_img + 1 entries -- image j owns gallery captions
    grp_off[j] .. grp_off[j + 1] - 1.  Captions longer than 256 tokens are truncated to 256.
    The maximum lengths are found on the host (one copy of the offsets); the queries go in one launch per non-empty length class
    (<= 64, <= 128, <= 256 tokens: 1, 2 or 4 words of query positions).
    out: a preallocated result (rows with a unit inner stride; other columns of a wider matrix are left alone).  q_rows (int32,
    needs out): the row of `out` each query is written to.  lcs=True: the largest LCS length instead of the F-measure."""
    n_q, _, n_img = _check_captions(q_tok, q_off, g_tok, g_off, grp_off)
    if q_rows is not None and out is None:
        raise ValueError('aladin_amd: rouge_l: q_rows names rows of a preallocated out=')
    _require_gpu_ints(q_tok, q_off, g_tok, g_off, grp_off, out, q_rows)
    if out is None:
        out = torch.empty((n_q, n_img), dtype=torch.float32, device=q_tok.device)
    q_len = (q_off[1:] - q_off[:-1]).cpu()
    g_len = g_off[1:] - g_off[:-1]
    if int(q_len.min()) < 1 or int(g_len.min()) < 1:
        raise ValueError('aladin_amd: rouge_l: every caption holds at least one token (the empty caption is the one token \'\')')
    g_max = min(int(g_len.max()), ROUGE_MAX_LEN)
    if int(q_len.max()) <= ROUGE_CLASSES[0]:                 # COCO: every query in the one-word class, nothing to regroup
        return rouge_l_launch(q_tok, q_off, int(q_len.max()), g_tok, g_off, g_max, grp_off, out, q_rows, lcs)
    lo = 0
    for hi in ROUGE_CLASSES:
        pick = (q_len > lo) & (q_len <= hi) if hi < ROUGE_MAX_LEN else q_len > lo
        lo = hi
        idx = torch.nonzero(pick).flatten()
        if idx.numel() == 0:
            continue
        # the class as a CSR of its own: its captions' tokens gathered in order
        lens = q_len[idx]
        off_c = torch.zeros(idx.numel() + 1, dtype=torch.int64)
        off_c[1:] = torch.cumsum(lens, 0)
        dev = q_tok.device
        idx_d, off_d = idx.to(dev), off_c.to(dev)
        seg = torch.repeat_interleave(torch.arange(idx.numel(), device=dev), lens.to(dev))
        src = q_off[idx_d][seg] + (torch.arange(int(off_c[-1]), device=dev) - off_d[seg])
        rows = idx_d.to(torch.int32) if q_rows is None else q_rows[idx_d].contiguous()
        rouge_l_launch(q_tok[src], off_d, min(int(lens.max()), hi), g_tok, g_off, g_max, grp_off, out, rows, lcs)
    return out
