"""Retrieval evaluation with the reference's call surface, scored and ranked on the GPU.

    compute_sim_matrix                       new name for the sites
                                             recall_auxiliary.py:30,51, evaluation.py:196,285 and
                                             the alignment_sim_fn closures train.py:495-498 / test.py:260-263
    recall / recall_test / compute_recall    <- alad/recall_auxiliary.py:8-149
    i2t / t2i                                <- alad/evaluation.py:158-327
    search_topk                              new: the k best gallery items of every query from matching-head embeddings,
                                             without the score matrix (ops.search_topk)
    search_ndcg                              new: the nDCG of any ranking table by an aladin_amd.dcg.DCG scorer (ops.ndcg_from_ranking);
                                             i2t / t2i with ndcg_scorer= report its means
    AverageMeter / LogCollector              <- alad/evaluation.py:22-77 (host bookkeeping)

The per-query Python loops, per-iteration host->device copies and numpy argsort of the reference
are replaced by one score-matrix launch plus one rank launch per direction; only the rank vectors
come back to the host.  Rank = number of strictly larger scores, which equals the reference's
argsort position except on exact ties (whose order numpy leaves unspecified).
"""
from collections import OrderedDict

import numpy as np
import torch

from . import ops

CAPS_PER_IMG = 5


class AverageMeter:
    """Last value and running weighted mean of one logged quantity (same fields and printing as the
    meter of reference alad/evaluation.py:22-47: val, avg, sum, count; weight 0 records without averaging)."""

    __slots__ = ('val', 'avg', 'sum', 'count')

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=0):
        self.val = val
        self.count += n
        self.sum += n * val
        self.avg = self.sum / (self.count + 1e-4)          # the reference's guard against an empty meter

    def __str__(self):
        return str(self.val) if not self.count else '{:.4f} ({:.4f})'.format(self.val, self.avg)


class LogCollector:
    """Named AverageMeters in insertion order (reference alad/evaluation.py:50-77), incl. the
    TensorBoard hook `tb_log` the training driver calls."""

    def __init__(self):
        self.meters = OrderedDict()

    def update(self, k, v, n=0):
        self.meters.setdefault(k, AverageMeter()).update(v, n)

    def __str__(self):
        return '  '.join('%s %s' % (name, meter) for name, meter in self.meters.items())

    def tb_log(self, tb_logger, prefix='', step=None):
        for name, meter in self.meters.items():
            tb_logger.add_scalar(prefix + name, meter.val, global_step=step)


def encode_data(model, data_loader, log_step=10, logging=print, max_len=71):
    """reference alad/evaluation.py:80-155 with the embedding store kept ON THE DEVICE.

    Same protocol (model.forward_emb per batch under no_grad, sets zero-padded to `max_len` positions,
    slot 0 overwritten with the global matching-head embedding, length lists) and same return
    signature, but `img_embs` / `cap_embs` are float32 CUDA tensors: the reference's per-batch
    device->host copy (:124-128) and the per-query host->device copies of i2t / t2i
    (:179,202,267,291) disappear, and compute_sim_matrix() consumes the buffers in place."""
    import time
    clear_eval_cache()                               # a new embedding store is coming: the last grid is stale
    batch_time = AverageMeter()
    val_logger = LogCollector()
    model.eval()
    end = time.time()
    img_embs = cap_embs = None
    img_lengths, cap_lengths = [], []
    ids_pointer = 0
    n_total = len(data_loader.dataset)
    for i, (example_imgs, example_txts) in enumerate(data_loader):
        model.logger = val_logger
        with torch.no_grad():
            img_glob, cap_glob, img_emb, cap_emb, img_length, cap_length, _ = model.forward_emb(example_imgs, example_txts)
            bs = img_glob.shape[0]
            if img_embs is None:
                dev = img_emb.device
                img_embs = torch.zeros((n_total, max_len, img_emb.size(2)), dtype=torch.float32, device=dev)
                cap_embs = torch.zeros((n_total, max_len, cap_emb.size(2)), dtype=torch.float32, device=dev)
            sl = slice(ids_pointer, ids_pointer + bs)
            img_embs[sl, :img_emb.size(0), :] = img_emb.permute(1, 0, 2)          # (S,B,D) -> (B,S,D)
            cap_embs[sl, :cap_emb.size(0), :] = cap_emb.permute(1, 0, 2)
            img_embs[sl, 0, :] = img_glob                                         # I-CLS / T-CLS slots (:127-128)
            cap_embs[sl, 0, :] = cap_glob
            img_lengths.extend(img_length)
            cap_lengths.extend(cap_length)
            ids_pointer += bs
        batch_time.update(time.time() - end)
        end = time.time()
        if logging is not None and i % log_step == 0:
            logging('Test: [{0}/{1}]\t{e_log}\tTime {bt.val:.3f} ({bt.avg:.3f})\t'.format(
                i, len(data_loader), bt=batch_time, e_log=str(model.logger)))
    return img_embs, cap_embs, img_lengths, cap_lengths


def encode_data_packed(model, data_loader, log_step=10, logging=print, precision='split', max_len=71):
    """encode_data with the embedding store kept on the device in packed 16-bit form (SURVEY.md
    section 8(f) row 2): returns (img_store, cap_store, img_lengths, cap_lengths) where the stores are
    aladin_amd.store.PackedSetStore objects that compute_sim_matrix / i2t / t2i accept in place of the
    (N, 71, D) tensors -- same protocol as alad/evaluation.py:80-155 otherwise.  precision 'split' (default:
    rank-exact alignment retrieval, fp16 hi/lo pair per value) or 'fp16' (half the bytes, ~1e-4 score error)."""
    import time
    from .store import PackedSetStore
    clear_eval_cache()
    batch_time = AverageMeter()
    val_logger = LogCollector()
    model.eval()
    end = time.time()
    img_store = cap_store = None
    for i, (example_imgs, example_txts) in enumerate(data_loader):
        model.logger = val_logger
        with torch.no_grad():
            img_glob, cap_glob, img_emb, cap_emb, img_length, cap_length, _ = model.forward_emb(example_imgs, example_txts)
            if img_store is None:
                img_store = PackedSetStore(img_emb.size(2), 0, img_emb.device, precision=precision, padded_len=max_len)
                cap_store = PackedSetStore(cap_emb.size(2), 2, cap_emb.device, precision=precision, padded_len=max_len)
            img_store.append(img_emb.permute(1, 0, 2), img_length, img_glob)      # (S,B,D) -> (B,S,D) view
            cap_store.append(cap_emb.permute(1, 0, 2), cap_length, cap_glob)
        batch_time.update(time.time() - end)
        end = time.time()
        if logging is not None and i % log_step == 0:
            logging('Test: [{0}/{1}]\t{e_log}\tTime {bt.val:.3f} ({bt.avg:.3f})\t'.format(
                i, len(data_loader), bt=batch_time, e_log=str(model.logger)))
    return img_store, cap_store, list(img_store.lengths), list(cap_store.lengths)


def _is_packed_store(x):
    from .store import PackedSetStore, StoreView
    return isinstance(x, (PackedSetStore, StoreView))


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('aladin_amd: retrieval scoring runs in HIP kernels on an MI355X only (no GPU visible)')
    return torch.device('cuda', torch.cuda.current_device())


def compute_sim_matrix(img, cap, img_len=None, cap_len=None, mode='matching', precision=None):
    """(N_img, N_cap) score matrix on the GPU.

    mode='matching'  : img (N_img, D), cap (N_cap, D) global embeddings -> img @ cap.T
    mode='alignment' : img (N_img, R, D), cap (N_cap, T, D) sets with length lists -> MrSw scores
                       (trimmed to the real lengths, chunked, in the evaluation precision: eval_grid.score_grid;
                       precision='fp16' | 'split' overrides ops.set_eval_precision())
    Both arguments may instead be PackedSetStore / StoreView objects (encode_data_packed).
    """
    dev = _device()
    if _is_packed_store(img) != _is_packed_store(cap):
        raise ValueError('compute_sim_matrix: pass two stores or two tensors')
    if _is_packed_store(img):                            # packed 16-bit stores (encode_data_packed): lengths travel with them
        from .store import alignment_scores_from_stores
        with torch.no_grad():
            if mode == 'matching':
                return ops.sim_matrix(img.glob, cap.glob)
            if mode == 'alignment':
                return alignment_scores_from_stores(img, cap)
        raise ValueError("mode must be 'matching' or 'alignment'")
    img = torch.as_tensor(img).to(dev, torch.float32)
    cap = torch.as_tensor(cap).to(dev, torch.float32)
    with torch.no_grad():
        if mode == 'matching':
            return ops.sim_matrix(img, cap)
        if mode == 'alignment':
            if img_len is None or cap_len is None:
                raise ValueError("compute_sim_matrix(mode='alignment') needs img_len and cap_len")
            return ops.alignment_scores(img, cap, list(img_len), list(cap_len), 'MrSw', precision=precision)
    raise ValueError("mode must be 'matching' or 'alignment'")


class GalleryIndex:
    """A matching-head gallery prepared once and searched many times (ops.build_search_index): GalleryIndex(gallery, side) with
    side = 'captions' (image queries, direction 'i2t') or 'images' (caption queries, 't2i').  gallery: an (n, D) array or tensor
    of embeddings, or a PackedSetStore / StoreView -- then its .glob rows are indexed and the store is kept (.store) for the
    re-scoring of search_rerank / search_explain.  .search(queries, k) -> (indices, scores), search_topk's; len() = the gallery
    size.  search_topk / search_rerank / search_explain take it in the gallery position.  The index is a snapshot: it does not
    follow a store that is appended to afterwards, and it cannot be extended -- build a new one."""

    SIDES = {'captions': ('i2t', 1), 'images': ('t2i', 0)}

    def __init__(self, gallery, side):
        if side not in self.SIDES:
            raise ValueError("GalleryIndex: side must be 'captions' or 'images'")
        self.side = side
        self.direction, self.dim = self.SIDES[side]
        self.store = gallery if _is_packed_store(gallery) else None
        dev = _device()
        rows = gallery.glob if self.store is not None else gallery
        with torch.no_grad():
            self.index = ops.build_search_index(torch.as_tensor(rows).to(dev, torch.float32))

    def __len__(self):
        return len(self.index)

    def search(self, queries, k=50):
        """(indices, scores) of the k best gallery items of every query: (n_q, D) embeddings, or a store / view (its .glob rows)."""
        dev = _device()
        if _is_packed_store(queries):
            queries = queries.glob
        with torch.no_grad():
            return ops.search_index_topk(self.index, torch.as_tensor(queries).to(dev, torch.float32), k, dim=self.dim,
                                         return_scores=True)


def _gallery_index(images, captions, direction, who):
    """The GalleryIndex among a search's two sides, checked against the direction: (index or None, queries)."""
    if isinstance(images, GalleryIndex) and isinstance(captions, GalleryIndex):
        raise ValueError('%s: one side is the gallery index, the other the queries' % who)
    for side, gallery, queries in (('captions', captions, images), ('images', images, captions)):
        if isinstance(gallery, GalleryIndex):
            if gallery.side != side or gallery.direction != direction:
                want = 'captions' if direction == 'i2t' else 'images'
                raise ValueError("%s: direction %r searches a gallery of %s, passed in the %s position; got an index of %s in the %s position"
                                 % (who, direction, want, want, gallery.side, side))
            return gallery, queries
    return None, None


def search_topk(images, captions, k=50, direction='i2t'):
    """The k best gallery items of every query from matching-head embeddings, best first: (indices, scores) as an (n_q, k) int32
    and an (n_q, k) float32 device tensor.  direction='i2t': the (n_img, D) images query the (n_cap, D) captions; 't2i': the
    captions query the images.  The same entries as the first k of a stable descending sort of compute_sim_matrix(images,
    captions) along the gallery axis (ties -> lower index; -1 / -inf past the gallery size), without the score matrix:
    ops.search_topk, up to 589824 gallery items.  The gallery side (captions for 'i2t', images for 't2i') may be a GalleryIndex:
    the same result without packing the gallery again."""
    if direction not in ('i2t', 't2i'):
        raise ValueError("direction must be 'i2t' or 't2i'")
    index, queries = _gallery_index(images, captions, direction, 'search_topk')
    if index is not None:
        return index.search(queries, k)
    dev = _device()
    if _is_packed_store(images) != _is_packed_store(captions):
        raise ValueError('search_topk: pass two stores or two tensors')
    if _is_packed_store(images):
        images, captions = images.glob, captions.glob
    img = torch.as_tensor(images).to(dev, torch.float32)
    cap = torch.as_tensor(captions).to(dev, torch.float32)
    with torch.no_grad():
        return ops.search_topk(img, cap, k, dim=1 if direction == 'i2t' else 0, return_scores=True)


def search_rerank(images, captions, k=50, direction='i2t', shortlist=None):
    """Two-stage retrieval over two PackedSetStore / StoreView objects: (indices, scores) as an (n_q, k) int32 and an (n_q, k)
    float32 device tensor, best first by the ALIGNMENT head.  The shortlist of every query is search_topk(images, captions, k,
    direction) on the stores' matching-head embeddings (shortlist=None) or the caller's (n_q, k) int32 table of gallery
    positions (-1 = none); its pairs are scored straight from the stores (store.alignment_scores_for_pairs) and ordered by
    score, ties -> the earlier shortlist slot, -1 / -inf last.  Nothing of the size of the (n_q, gallery) grid is computed.
    The gallery side may be a GalleryIndex built from a store / view: the shortlist comes from the index, the re-scoring from its
    store -- the same result."""
    if direction not in ('i2t', 't2i'):
        raise ValueError("direction must be 'i2t' or 't2i'")
    index, queries = _gallery_index(images, captions, direction, 'search_rerank')
    if index is not None:
        if index.store is None:
            raise ValueError('search_rerank: the gallery index must be built from a store / view (its sets are re-scored), not from a tensor')
        if not _is_packed_store(queries):
            raise ValueError('search_rerank: pass two stores / views (encode_data_packed), not tensors')
        if shortlist is None:
            shortlist, _ = index.search(queries, k)
        images, captions = (queries, index.store) if direction == 'i2t' else (index.store, queries)
    if not (_is_packed_store(images) and _is_packed_store(captions)):
        raise ValueError('search_rerank: pass two stores / views (encode_data_packed), not tensors')
    from .store import alignment_scores_for_pairs
    with torch.no_grad():
        if shortlist is None:
            shortlist, _ = search_topk(images, captions, k, direction)
        scores = alignment_scores_for_pairs(images, captions, shortlist, direction)
        return ops.rerank_order(shortlist, scores)


def search_explain(images, captions, k=50, direction='i2t', shortlist=None, top=5):
    """search_rerank plus the alignment behind its best results: (indices, scores, PairAlignment).  indices / scores are exactly
    search_rerank(images, captions, k, direction, shortlist)'s; the PairAlignment (store.alignment_map_for_pairs) covers every
    query's first min(top, k) re-ranked candidates -- for each word the region that carried its max and the cosine, for each
    region its best word; -1 slots of a short shortlist stay -1 / -inf there."""
    top = int(top)
    if top < 1:
        raise ValueError('search_explain: top must be >= 1 (got %d)' % top)
    idx, val = search_rerank(images, captions, k, direction, shortlist)
    if isinstance(images, GalleryIndex):                 # search_rerank has checked it: built from a store, on the direction's side
        images = images.store
    if isinstance(captions, GalleryIndex):
        captions = captions.store
    from .store import alignment_map_for_pairs
    with torch.no_grad():
        return idx, val, alignment_map_for_pairs(images, captions, idx[:, :min(top, idx.shape[1])].contiguous(), direction)


def _metrics(ranks):
    ranks = np.asarray(ranks, dtype=np.float64)
    r1 = 100.0 * len(np.where(ranks < 1)[0]) / len(ranks)
    r5 = 100.0 * len(np.where(ranks < 5)[0]) / len(ranks)
    r10 = 100.0 * len(np.where(ranks < 10)[0]) / len(ranks)
    medr = np.floor(np.median(ranks)) + 1
    meanr = ranks.mean() + 1
    return r1, r5, r10, medr, meanr


def _to_host(ranks4, n_img, n_cap):
    """(rank_i2t, top1_i2t, rank_t2i, top1_t2i) device vectors -> float64 numpy arrays with ONE device-to-host copy."""
    both = torch.cat(list(ranks4)).cpu().numpy().astype(np.float64)
    return both[:n_img], both[n_img:2 * n_img], both[2 * n_img:2 * n_img + n_cap], both[2 * n_img + n_cap:]


def _ranks(sim):
    return _to_host(ops.recall_ranks(sim, CAPS_PER_IMG), *sim.shape)


def _fused_ranks(img, cap):
    """Ranks of both directions straight from the global embeddings (ops.retrieval_ranks: the score
    matrix is never materialised); same numbers as _ranks(compute_sim_matrix(img, cap))."""
    dev = _device()
    img = torch.as_tensor(img).to(dev, torch.float32)
    cap = torch.as_tensor(cap).to(dev, torch.float32)
    with torch.no_grad():
        return _to_host(ops.retrieval_ranks(img, cap, CAPS_PER_IMG), img.shape[0], cap.shape[0])


def recall(images, captions, model, mode='i2t', lenghts=None, return_ranks=False):
    """reference alad/recall_auxiliary.py:8-69: rows 0::5 of `images` are the distinct images."""
    if mode not in ('i2t', 't2i'):
        raise ValueError('mode not correct')
    r_i2t, t_i2t, r_t2i, t_t2i = _fused_ranks(torch.as_tensor(images)[0::CAPS_PER_IMG], captions)
    ranks, top1 = (r_i2t, t_i2t) if mode == 'i2t' else (r_t2i, t_t2i)
    m = _metrics(ranks)
    return (m, (ranks, top1)) if return_ranks else m


def recall_test(img_embs, cap_embs, tot_lengths, model):
    """reference alad/recall_auxiliary.py:72-86; both directions from one fused GEMM + rank pass."""
    r_i2t, _, r_t2i, _ = _fused_ranks(torch.as_tensor(img_embs)[0::CAPS_PER_IMG], cap_embs)
    r1, r5, r10, _, _ = _metrics(r_i2t)
    r1i, r5i, r10i, _, _ = _metrics(r_t2i)
    return r1, r5, r10, r1i, r5i, r10i, r1 + r5 + r10 + r1i + r5i + r10i


def compute_recall(img_embs, cap_embs, tot_lengths=None, model=None, verbose=True):
    """reference alad/recall_auxiliary.py:133-149."""
    r1, r5, r10, r1i, r5i, r10i, _ = recall_test(img_embs, cap_embs, tot_lengths, model)
    rsum = r1 + r5 + r10 + r1i + r5i + r10i
    if verbose:
        print("Recall Image to text: %.2f, %.2f, %.2f" % (r1, r5, r10))
        print("Recall Text to image: %.2f, %.2f, %.2f" % (r1i, r5i, r10i))
        print('Sum score: %.2f' % rsum)
    return r1, r5, r10, r1i, r5i, r10i, rsum


def recall_1k_5fold_test(img_embs, cap_embs, tot_lengths=None, model=None, verbose=True):
    """reference alad/recall_auxiliary.py:90-130: mean over five 5000-row folds (torch.split(.., 5000))."""
    img_folds = torch.split(torch.as_tensor(img_embs), 5000, dim=0)
    cap_folds = torch.split(torch.as_tensor(cap_embs), 5000, dim=0)
    res = []
    for i in range(5):
        if verbose:
            print('Computing Test recall... chunk %s of 5' % (i + 1))
        res.append(recall_test(img_folds[i], cap_folds[i], tot_lengths, model)[:6])
    r1, r5, r10, r1i, r5i, r10i = (float(v) for v in np.mean(np.array(res, dtype=np.float64), axis=0))
    rsum = r1 + r5 + r10 + r1i + r5i + r10i
    if verbose:
        print("Test 1K 5Folds - Recall Image to text: %.2f, %.2f, %.2f" % (r1, r5, r10))
        print("Test 1K 5Folds - Recall Text to image: %.2f, %.2f, %.2f" % (r1i, r5i, r10i))
        print('Test 1K 5Folds - Sum score: %.2f' % rsum)
    return r1, r5, r10, r1i, r5i, r10i, rsum


# The score grid of the last i2t / t2i call: validate() / test() call the two back to back on the same
# embeddings (reference train.py:504-509, test.py:271-276), so the second call re-uses the first one's grid.
# A hit needs the SAME input objects, still alive (weak references compared with `is`: an address alone says
# nothing -- the caching allocator hands the next validation's buffers the block the previous ones freed, with
# the same shape and the same number of in-place fills), unchanged (tensor version counter / store row count).
# The memo never keeps its inputs alive, and encode_data / encode_data_packed drop it before they start.
_GRID_MEMO = {'key': None, 'refs': None, 'sim': None}


def clear_eval_cache():
    """Drop the memoised score grid (it holds N_img x N_cap floats on the device: 500 MB at COCO-5k)."""
    _GRID_MEMO['key'] = _GRID_MEMO['refs'] = _GRID_MEMO['sim'] = None


def _memo_key(images, captions, img_lenghts, cap_lenghts, measure, sim_function):
    """-> (key, objects the key is only valid for) or (None, None) when an input cannot be tracked (then nothing
    is memoised)."""
    import weakref
    objs = []

    def ident(x):
        if isinstance(x, torch.Tensor):
            objs.append(x)
            return ('t', x.data_ptr(), tuple(x.shape), tuple(x.stride()), x._version, str(x.device))
        if _is_packed_store(x):
            st = getattr(x, 'store', x)
            objs.extend([x, st])
            return ('s', st.n_rows, len(st), hash(tuple(getattr(x, 'ids', ()))), len(x))
        if isinstance(x, np.ndarray):
            return None                              # no version counter: an in-place refill would go unnoticed
        return None
    ki, kc = ident(images), ident(captions)
    if ki is None or kc is None:
        return None, None
    if sim_function is None or isinstance(sim_function, str):
        fn = sim_function
    else:
        objs.append(sim_function)
        fn = 'callable'
    try:
        refs = [weakref.ref(o) for o in objs]
    except TypeError:                                # e.g. a bound method: a new object per access, not trackable
        return None, None
    key = (ki, kc, tuple(int(v) for v in img_lenghts) if img_lenghts is not None else None,
           tuple(int(v) for v in cap_lenghts) if cap_lenghts is not None else None, measure, fn, ops._EVAL_PRECISION[0])
    return key, (refs, objs)


def _eval_scores(images, captions, img_lenghts, cap_lenghts, measure, sim_function):
    """(n_img, n_cap) scores of the de-duplicated images (rows 0::5, alad/evaluation.py:171,252) against every
    caption -- ONE grid instead of the reference's per-query loops."""
    key, tracked = _memo_key(images, captions, img_lenghts, cap_lenghts, measure, sim_function)
    if key is not None and _GRID_MEMO['key'] == key and _GRID_MEMO['refs'] is not None \
            and len(_GRID_MEMO['refs']) == len(tracked[1]) \
            and all(r() is o for r, o in zip(_GRID_MEMO['refs'], tracked[1])):
        return _GRID_MEMO['sim']
    clear_eval_cache()                               # release the old grid before the new one is allocated
    sim = _eval_scores_uncached(images, captions, img_lenghts, cap_lenghts, measure, sim_function)
    if key is not None:
        _GRID_MEMO['key'], _GRID_MEMO['refs'], _GRID_MEMO['sim'] = key, tracked[0], sim
    return sim


def _eval_scores_uncached(images, captions, img_lenghts, cap_lenghts, measure, sim_function):
    if _is_packed_store(images):
        ims = images.view(slice(0, None, CAPS_PER_IMG))
        if measure == 'order':
            with torch.no_grad():
                return ops.order_scores(ims.glob, captions.glob)
        if sim_function is None:
            return compute_sim_matrix(ims, captions)
        if sim_function == 'alignment':
            return compute_sim_matrix(ims, captions, mode='alignment')
        raise ValueError("aladin_amd: with packed stores sim_function must be None or 'alignment'")
    images = torch.as_tensor(images)
    captions = torch.as_tensor(captions)
    ims = images[0::CAPS_PER_IMG]
    if measure == 'order':
        # alad/evaluation.py:184-192,272-281 score order embeddings with order_sim (alad/loss.py:20-26) in blocks
        # of 100 queries.  That branch predates the (N, 71, D) sets -- order_sim's expand() takes (n, D) matrices
        # and fails on 3-D input -- so here it scores the slot-0 global embeddings, which is what the same call
        # sites use for 'dot' (:196, :285); 2-D embedding matrices are taken as they are.
        dev = _device()
        a = (ims[:, 0, :] if ims.dim() == 3 else ims).to(dev, torch.float32)
        b = (captions[:, 0, :] if captions.dim() == 3 else captions).to(dev, torch.float32)
        with torch.no_grad():
            return ops.order_scores(a, b)
    if sim_function is None:                      # matching head on the slot-0 global embeddings (:196, :285)
        return compute_sim_matrix(ims[:, 0, :], captions[:, 0, :])
    ims_len = list(img_lenghts[0::CAPS_PER_IMG])
    if sim_function == 'alignment':
        return compute_sim_matrix(ims, captions, ims_len, list(cap_lenghts), mode='alignment')
    # a reference-style closure (train.py:495-498: AlignmentContrastiveLoss(...)(..., return_loss=False) under
    # no_grad): called ONCE on the whole grid; with aladin_amd's loss module inside, that call lands on the same
    # trimmed / chunked / split-precision path as sim_function='alignment'
    dev = _device()
    with torch.no_grad():
        return sim_function(ims.to(dev, torch.float32), captions.to(dev, torch.float32), ims_len,
                            list(cap_lenghts)).to(torch.float32)


def _npts(images, npts):
    n_img = len(images) // CAPS_PER_IMG
    return n_img if npts is None else min(int(npts), n_img)


def search_ndcg(indices, ndcg_scorer, direction='i2t', fold_index=0, npts=None):
    """nDCG of any (n_q, k) ranking table -- search_topk's, search_rerank's, a caller's -- as {method: float64 (n_q,) device
    tensor}: row i is query i of fold `fold_index` of the scorer (aladin_amd.dcg.DCG), its entries gallery positions inside the
    fold, best first (-1 = none); the first min(k, scorer.rank) count.  direction='i2t': images query captions (the scorer's
    retrieval='sentence'); 't2i': captions query images ('image').  npts: the fold's images, default n_q ('i2t') or n_q // 5."""
    if direction not in ('i2t', 't2i'):
        raise ValueError("direction must be 'i2t' or 't2i'")
    if ndcg_scorer is None or not hasattr(ndcg_scorer, 'compute_ndcg_batch'):
        raise ValueError('search_ndcg: pass an aladin_amd.dcg.DCG scorer')
    if not hasattr(indices, 'shape') or len(indices.shape) != 2 or indices.shape[0] < 1 or indices.shape[1] < 1:
        raise ValueError('search_ndcg: the ranking must be an (n_q, k) table')
    n_q = indices.shape[0]
    if npts is None:
        npts = n_q if direction == 'i2t' else n_q // CAPS_PER_IMG
    return ndcg_scorer.compute_ndcg_batch(int(npts), indices, fold_index, 'sentence' if direction == 'i2t' else 'image')


def _ndcg_means(sim, npts, direction, ndcg_scorer, fold_index):
    """The last two entries of the i2t / t2i tuple: (0, 0) without a scorer, else the mean nDCG of the first npts images' (or their
    captions') top-`rank` lists by the scorer's first two relevance methods."""
    if ndcg_scorer is None:
        return (0, 0)
    n_img, n_cap = sim.shape
    gallery, window, what = (n_cap, CAPS_PER_IMG * npts, 'captions') if direction == 'i2t' else (n_img, npts, 'images')
    if gallery != window:
        # the reference indexes the fold window with positions of the FULL ranking (dcg.py:25,29): an IndexError or silently wrong
        # relevances when the two differ
        raise ValueError('aladin_amd: nDCG needs the ranked gallery to be the fold window: %d %s ranked, %d in the window of npts=%d'
                         % (gallery, what, window, npts))
    with torch.no_grad():
        if direction == 'i2t':
            top = ops.topk_indices(sim[:npts], ndcg_scorer.rank, dim=1)
        else:
            top = ops.topk_indices(sim[:, :CAPS_PER_IMG * npts], ndcg_scorer.rank, dim=0)
        per_query = search_ndcg(top, ndcg_scorer, direction, fold_index, npts)
    means = [float(per_query[m].mean().item()) for m in list(ndcg_scorer.relevance_methods)[:2]]
    return tuple(means + [0] * (2 - len(means)))


def i2t(images, captions, img_lenghts, cap_lenghts, npts=None, return_ranks=False, ndcg_scorer=None, fold_index=0,
        measure='dot', sim_function=None, cap_batches=1):
    """reference alad/evaluation.py:158-241.  sim_function may be None (matching head), the string
    'alignment' (HIP alignment scores) or a callable (img, cap, img_len, cap_len) -> scores; it is
    called ONCE on the whole (n_img x n_cap) grid instead of once per query and caption chunk
    (cap_batches is accepted and ignored).  npts: only the first npts images are queries (:164-165); they are
    still ranked against every caption.  Returns the 7-tuple, plus (ranks, top1) with return_ranks.
    ndcg_scorer: an aladin_amd.dcg.DCG; the last two entries of the tuple are then the MEAN nDCG over the queries by the scorer's
    first and second relevance method (0 for a method it does not have), from every query's top-`scorer.rank` list
    (ops.topk_indices on the grid) inside fold `fold_index`.  A deviation: the reference computes the per-query values and then
    returns literal zeros (:236-237); the means are what its call sites print.  The ranked gallery must be exactly the fold's
    window (5 * npts captions), ValueError otherwise.  Without a scorer the two entries stay 0."""
    sim = _eval_scores(images, captions, img_lenghts, cap_lenghts, measure, sim_function)
    n = _npts(images, npts)
    ndcg = _ndcg_means(sim, n, 'i2t', ndcg_scorer, fold_index)
    ranks, top1, _, _ = _ranks(sim)
    ranks, top1 = ranks[:n], top1[:n]
    m = _metrics(ranks) + ndcg
    return (m, (ranks, top1)) if return_ranks else m


def t2i(images, captions, img_lenghts, cap_lenghts, npts=None, return_ranks=False, ndcg_scorer=None, fold_index=0,
        measure='dot', sim_function=None, im_batches=1):
    """reference alad/evaluation.py:244-327.  With return_ranks the second element is (ranks, top50) as in the
    reference (:262,309,324-325): top50[c] = the 50 best images of caption c, best first (HIP top-k kernel; -1
    where there are fewer than 50 images).  npts: only the captions of the first npts images are queries
    (:250-251), ranked against every image.
    ndcg_scorer / fold_index: as in i2t -- the last two entries become the mean nDCG over the caption queries (the reference
    returns literal zeros, :321-322); the ranked gallery must be exactly the fold's npts images, ValueError otherwise."""
    sim = _eval_scores(images, captions, img_lenghts, cap_lenghts, measure, sim_function)
    n_img = _npts(images, npts)
    ndcg = _ndcg_means(sim, n_img, 't2i', ndcg_scorer, fold_index)
    _, _, ranks, _ = _ranks(sim)
    n = CAPS_PER_IMG * n_img
    ranks = ranks[:n]
    m = _metrics(ranks) + ndcg
    if not return_ranks:
        return m
    top50 = ops.topk_indices(sim[:, :n], 50, dim=0).cpu().numpy().astype(np.float64)     # float table like numpy.zeros((5*npts, 50))
    return m, (ranks, top50)
