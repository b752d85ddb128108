"""The loss heads of a training step as single autograd nodes (reference alad/alad_model.py:371-454 calling alad/loss.py): the
matching hinge, the alignment hinge and ListNet distillation with their weighted sum -- the small-batch kernels at B <= 64 (every
shipped YAML trains with bs 32), the general kernels above."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from ._ops_common import (_stream, _ptr, _require_gpu, _require_tensors, _rows_inner_contig, _ld, _workspace, _unit_cols, _set_view,
                          _sets_for_node, _upstream)
from .ops import (AlignSaved, _align_forward, _align_head_forward, _caption_fill, _check_backward_supported, _check_sets,
                  _pair_kernel_covers, is_long)
from .ops_losses import (_grad_combine, _hinge_raw, _listnet_raw, _product, _product_backward, _xent_limit, _xent_raw, _xent_scale,
                         _xent_temperature, dot_scores)


# ------------------------------------------------------------------------------------------------
# small-batch matching + distillation (B <= 64: the batch size of every shipped YAML is 32)
# ------------------------------------------------------------------------------------------------
SMALL_BATCH_MAX = 64
HEAD_MATCH_HINGE, HEAD_ALIGN_HINGE, HEAD_LISTNET = 1, 2, 4      # ALADIN_HEAD_* of include/aladin_hip.h


def _small_rows(x):
    """Embedding rows as the small-batch kernels read them through _ld: _unit_cols, and -- where D is a multiple of 4 -- rows on
    16-byte boundaries: heads_small_stats_kernel sums a misaligned row lane by lane and an aligned one four features per lane, in
    another order, and the result must not depend on the memory layout."""
    x = _unit_cols(x)
    if x.shape[1] % 4 == 0 and (x.data_ptr() % 16 or (x.shape[0] > 1 and x.stride(0) % 4)):
        return x.contiguous()
    return x


def _square(want, B, dev):
    return torch.empty((B, B), dtype=torch.float32, device=dev) if want else None


SmallHeadsOut = namedtuple('SmallHeadsOut', 'M terms total dMh dMl dS pairs table_ws sets', defaults=(None, None, None))


def _heads_small_fwd(im, s, S, margin, max_violation, flags, temperature, eps, weights, want_grads, want_pairs, align=None):
    """Launch aladin_heads_small_fwd -> SmallHeadsOut of its outputs (include/aladin_hip.h; terms = [matching, alignment, listnet];
    what was not asked for is None); pairs: the alignment hinge's pair list for _align_backward (want_pairs).
    align = (im_set, s_seq, im_len_t, s_len_t, packed): with the hardest-negative alignment hinge and the fp16 pair
    kernel's shapes the element-wise pass shares its launch with the backward's pair recompute (aladin_heads_small_fwd_argmax);
    table_ws then holds the arg-max table and sets the sets in the row layout the kernels were given."""
    lib = _lib.load()
    B = (im if im is not None else S).shape[0]
    dev = (im if im is not None else S).device
    D = im.shape[1] if im is not None else 1
    M = _square(flags & (HEAD_MATCH_HINGE | HEAD_LISTNET), B, dev)
    terms = torch.empty(3, dtype=torch.float32, device=dev)
    total = torch.empty((), dtype=torch.float32, device=dev)
    # a head with weight 0 is computed for its logged value only (the distillation term before distill_epoch,
    # alad_model.py:442-444): no gradient matrix is produced for it, and the kernels keep it out of the total
    dMh = _square(want_grads and flags & HEAD_MATCH_HINGE and weights[0] != 0, B, dev)
    dMl = _square(want_grads and flags & HEAD_LISTNET and weights[2] != 0, B, dev)
    dS = _square(want_grads and flags & HEAD_ALIGN_HINGE, B, dev)
    ws = _workspace(lib.aladin_heads_small_workspace_bytes(B), dev)
    # the argument run the two entry points share, img .. dS, around their own dimensions and hinge mode
    head = (_ptr(im), _ld(im) if im is not None else 0, _ptr(s), _ld(s) if s is not None else 0, _ptr(S), _ld(S) if S is not None else 0)
    outs = (int(flags), float(temperature), float(eps), float(weights[0]), float(weights[1]), float(weights[2]), _ptr(M), _ptr(terms),
            _ptr(total), _ptr(dMh), _ptr(dMl), _ptr(dS))
    im_set, s_seq, im_len_t, s_len_t, packed = align if align is not None else (None,) * 5
    if packed is not None and dS is not None and max_violation and _pair_kernel_covers(packed.geom) and not packed.geom.split:
        geom = packed.geom
        sets = im_c, s_c = _rows_inner_contig(im_set), _rows_inner_contig(s_seq)
        table_ws = torch.empty(lib.aladin_align_bwd_workspace_bytes(C.byref(geom), 0), dtype=torch.uint8, device=dev)
        vi, vs, pk = _set_view(im_c, im_len_t), _set_view(s_c, s_len_t), packed.struct()
        _lib.check(lib.aladin_heads_small_fwd_argmax(*head, D, float(margin), *outs, _ptr(ws), C.byref(vi), C.byref(vs), C.byref(geom),
                                                     C.byref(pk), _ptr(table_ws), _stream()), 'heads_small_fwd_argmax')
        return SmallHeadsOut(M, terms, total, dMh, dMl, dS, None, table_ws, sets)
    pairs = None
    if want_pairs and dS is not None:
        pairs = (torch.empty(B * B, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    _lib.check(lib.aladin_heads_small_fwd(*head, B, D, float(margin), int(bool(max_violation)), *outs, _ptr(pairs[0] if pairs else None),
                                          _ptr(pairs[1] if pairs else None), _ptr(ws), _stream()), 'heads_small_fwd')
    return SmallHeadsOut(M, terms, total, dMh, dMl, dS, pairs)


def _heads_small_bwd(ctx, a, b, dMh, g_h, w_h, dMl, g_l, w_l, g_M=None, g_a=None, w_a=0.0, scale=None):
    """Launch aladin_heads_small_bwd -> (d_a, d_b), each for an input that needs it: (g_h w_h dMh + g_l w_l dMl + g_M) times the
    other side's rows; scale (one float32, or None) receives g_a * w_a for the alignment backward."""
    B, D = a.shape
    d_a = torch.empty((B, D), dtype=torch.float32, device=a.device) if ctx.needs_input_grad[0] else None
    d_b = torch.empty((B, D), dtype=torch.float32, device=a.device) if ctx.needs_input_grad[1] else None
    _lib.check(_lib.load().aladin_heads_small_bwd(_ptr(a), _ld(a), _ptr(b), _ld(b), B, D, _ptr(dMh), _ptr(g_h), w_h, _ptr(dMl), _ptr(g_l),
                                                  w_l, _ptr(g_M), _ld(g_M) if g_M is not None else 0, _ptr(g_a), w_a, _ptr(scale),
                                                  _ptr(d_a), _ptr(d_b), _stream()), 'heads_small_bwd')
    return d_a, d_b


class _SmallMatchDistill(torch.autograd.Function):
    """(hinge loss on M, listnet loss of M against the teacher, M) with M = im @ s.T, in two forward launches and
    one backward launch (csrc/small_batch.hip).  Either loss may be switched off (returns a zero scalar)."""

    @staticmethod
    def forward(ctx, im, s, teacher, margin, max_violation, want_hinge, temperature, eps):
        im, s = _small_rows(im), _small_rows(s)
        t = _unit_cols(teacher) if teacher is not None else None
        flags = (HEAD_MATCH_HINGE if want_hinge else 0) | (HEAD_LISTNET if t is not None else 0)
        need = any(ctx.needs_input_grad[:2])
        o = _heads_small_fwd(im, s, t, margin, max_violation, flags, temperature, eps, (1.0, 1.0, 1.0), need, False)
        ctx.save_for_backward(im, s, o.dMh, o.dMl)
        ctx.set_materialize_grads(False)
        return o.terms[0], o.terms[2], o.M

    @staticmethod
    def backward(ctx, g_h, g_l, g_M):
        im, s, dMh, dMl = ctx.saved_tensors
        if (g_h is None or dMh is None) and (g_l is None or dMl is None) and g_M is None:
            return (None,) * 8
        gh = _upstream(g_h) if (g_h is not None and dMh is not None) else None
        gl = _upstream(g_l) if (g_l is not None and dMl is not None) else None
        gM = _unit_cols(g_M) if g_M is not None else None          # autograd hands over (0, 1)- and (0, 0)-strided gradients
        return _heads_small_bwd(ctx, im, s, dMh if gh is not None else None, gh, 1.0, dMl if gl is not None else None, gl, 1.0, gM) \
            + (None,) * 6


def _heads_save(ctx, weights, align, a, b, im_len_t, s_len_t, dMh, dMl, terms, S, M):
    """What the forward of _SmallHeads / _BigHeads leaves on ctx: the weights, the alignment head's AlignSaved (None: no such
    head) and one save_for_backward layout; only the total is differentiable."""
    ctx.weights, ctx.align = weights, align
    ctx.save_for_backward(a, b, im_len_t, s_len_t, dMh, dMl, *(align.tensors() if align else ()))
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(*[t for t in (terms, S, M) if t is not None])       # one call: it replaces the set


def _heads_grads(ctx, d_a=None, d_b=None, saved=None, im_len_t=None, s_len_t=None, scale=None):
    """The return of the two backwards (called bare: no gradient arrived on the total): the embeddings' gradients, the sets'
    through ctx.align -- scale: upstream gradient x alignment weight on the device, None without a live alignment head -- and None
    for every other argument of the forward."""
    d_im = d_s = None
    if scale is not None and any(ctx.needs_input_grad[2:4]):
        d_im, d_s = ctx.align.backward(saved, im_len_t, s_len_t, scale)
    return (d_a, d_b, d_im, d_s) + (None,) * (len(ctx.needs_input_grad) - 4)


class _SmallHeads(torch.autograd.Function):
    """The whole loss-head step at B <= 64 as ONE autograd node: alignment scores (pack, side GEMM, score kernel),
    then the three heads and their fixed-weight sum (alad_model.py:450-453) in two launches; backward = one launch for
    the matching side + the two alignment backward kernels.  No element-wise glue kernels at all.
    Returns (total, terms[3] = matching / alignment / distillation, S, M); only `total` is differentiable."""

    @staticmethod
    def forward(ctx, img_emb, cap_emb, im, s, im_len_t, s_len_t, margin, max_violation, flags, weights, temperature, eps):
        need_sets = any(ctx.needs_input_grad[2:4])
        need_embs = any(ctx.needs_input_grad[0:2])
        S, packed = None, None
        if flags & (HEAD_ALIGN_HINGE | HEAD_LISTNET):
            if need_sets and flags & HEAD_ALIGN_HINGE:
                _check_backward_supported(im, s, 0, 2)
            S, packed = _align_forward(im, s, im_len_t, s_len_t)
        a = b = None
        if flags & (HEAD_MATCH_HINGE | HEAD_LISTNET):
            a, b = _small_rows(img_emb), _small_rows(cap_emb)
        align = (im, s, im_len_t, s_len_t, packed) if (packed is not None and need_sets and flags & HEAD_ALIGN_HINGE) else None
        o = _heads_small_fwd(a, b, S, margin, max_violation, flags, temperature, eps, weights, need_sets or need_embs, True, align)
        if o.sets is not None:
            im, s = o.sets
        saved = None if packed is None else AlignSaved(packed.geom, im, s, o.dS, o.table_ws, packed.operands(),
                                                       table=o.table_ws is not None, base_ws=True, pairs=o.pairs)
        _heads_save(ctx, weights, saved, a, b, im_len_t, s_len_t, o.dMh, o.dMl, o.terms, S, o.M)
        return o.total, o.terms, S, o.M

    @staticmethod
    def backward(ctx, g_total, _g_terms, _g_S, _g_M):
        if g_total is None:
            return _heads_grads(ctx)
        a, b, im_len_t, s_len_t, dMh, dMl, *saved = ctx.saved_tensors
        w = ctx.weights
        g = _upstream(g_total)
        d_a = d_b = None
        scale = torch.empty(1, dtype=torch.float32, device=g.device) if (ctx.align is not None and ctx.align.live) else None
        if a is not None:
            d_a, d_b = _heads_small_bwd(ctx, a, b, dMh, g, float(w[0]), dMl, g, float(w[2]), None, g, float(w[1]), scale)
        elif scale is not None:
            scale = g * float(w[1])
        return _heads_grads(ctx, d_a, d_b, saved, im_len_t, s_len_t, scale)


class _BigHeads(torch.autograd.Function):
    """_SmallHeads for B > 64: the same single autograd node over the general kernels -- alignment scores + fused hinge,
    exact-fp32 matching GEMM, hinge and ListNet on it, aladin_loss_total for the weighted sum; backward =
    aladin_grad_combine (upstream gradient x weights x dLoss/dM, and the alignment backward's scale) + two GEMMs + the
    alignment backward.  No element-wise torch kernels."""

    @staticmethod
    def forward(ctx, img_emb, cap_emb, im, s, im_len_t, s_len_t, margin, max_violation, flags, weights, temperature, eps, fill):
        need_sets = any(ctx.needs_input_grad[2:4])
        need_embs = any(ctx.needs_input_grad[0:2])
        dev = img_emb.device
        terms = torch.empty(3, dtype=torch.float32, device=dev)          # slots of absent heads are never read
        S = saved = None
        if flags & (HEAD_ALIGN_HINGE | HEAD_LISTNET):
            _, S, saved = _align_head_forward(im, s, im_len_t, s_len_t, margin, max_violation, need_sets, fill,
                                              hinge=bool(flags & HEAD_ALIGN_HINGE), loss_out=terms[1:2])
        a = b = M = dMh = dMl = None
        if flags & (HEAD_MATCH_HINGE | HEAD_LISTNET):
            a, b = _unit_cols(img_emb), _unit_cols(cap_emb)
            M = _product(a, b)
            if flags & HEAD_MATCH_HINGE:
                _, dMh, _ = _hinge_raw(M, margin, max_violation, need_embs, loss_out=terms[0:1])
            if flags & HEAD_LISTNET:            # weight 0: the logged value only, no gradient matrix
                _, dMl = _listnet_raw(S, M, temperature, eps, need_embs and weights[2] != 0, loss_out=terms[2:3])
        total = torch.empty((), dtype=torch.float32, device=dev)
        tp = terms.data_ptr()
        _lib.check(_lib.load().aladin_loss_total(C.c_void_p(tp) if flags & HEAD_MATCH_HINGE else C.c_void_p(0), float(weights[0]),
                                                 C.c_void_p(tp + 4) if flags & HEAD_ALIGN_HINGE else C.c_void_p(0), float(weights[1]),
                                                 C.c_void_p(tp + 8) if flags & HEAD_LISTNET else C.c_void_p(0), float(weights[2]),
                                                 _ptr(total), _stream()), 'loss_total')
        _heads_save(ctx, weights, saved, a, b, im_len_t, s_len_t, dMh, dMl, terms, S, M)
        return total, terms, S, M

    @staticmethod
    def backward(ctx, g_total, _g_terms, _g_S, _g_M):
        if g_total is None:
            return _heads_grads(ctx)
        a, b, im_len_t, s_len_t, dMh, dMl, *saved = ctx.saved_tensors
        w = ctx.weights
        g = _upstream(g_total)
        d_a = d_b = None
        want_m = (dMh is not None or dMl is not None) and any(ctx.needs_input_grad[0:2])
        want_a = ctx.align is not None and ctx.align.live and any(ctx.needs_input_grad[2:4])
        C_tot = torch.empty_like(dMh if dMh is not None else dMl) if want_m else None
        scale = torch.empty(1, dtype=torch.float32, device=g.device) if want_a else None
        if want_m or want_a:
            _grad_combine(g, float(w[0]), dMh, float(w[2]), dMl, C_tot, float(w[1]), scale)
        if want_m:
            d_a, d_b = _product_backward(C_tot, a, b, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return _heads_grads(ctx, d_a, d_b, saved, im_len_t, s_len_t, scale)


def loss_heads(img_emb, cap_emb, im_set, s_seq, im_len, s_len, margin, max_violation, heads, weights,
               temperature=6.0, eps=1e-10):
    """The loss heads of one training step in a single autograd node (three head launches at B <= SMALL_BATCH_MAX,
    the general kernels above it -- either way no element-wise glue).
    heads: subset of {'matching', 'alignment', 'distillation'}; weights: dict head -> fixed loss weight.
    -> (total = sum_k w_k L_k  [differentiable], terms (3,) = matching / alignment / distillation values, S, M).
    The slots of `terms` that belong to heads not selected are unspecified (uninitialised above SMALL_BATCH_MAX): read only the
    selected heads' slots."""
    flags = (HEAD_MATCH_HINGE if 'matching' in heads else 0) | (HEAD_ALIGN_HINGE if 'alignment' in heads else 0) | \
        (HEAD_LISTNET if 'distillation' in heads else 0)
    if not flags:
        raise ValueError('aladin_amd: no loss head selected')
    _require_gpu(img_emb, cap_emb)
    im_len_t = s_len_t = None
    if flags & (HEAD_ALIGN_HINGE | HEAD_LISTNET):
        im_len_t, s_len_t = _check_sets(im_set, s_seq, im_len, s_len)
        if not (im_set.shape[0] == s_seq.shape[0] == img_emb.shape[0]):
            raise ValueError('aladin_amd: the loss heads need one image set, one caption and one embedding pair per sample')
        im_set, s_seq = _sets_for_node(im_set, s_seq)
    w = (float(weights.get('matching', 0.0)), float(weights.get('alignment', 0.0)), float(weights.get('distillation', 0.0)))
    # long sets never reach the small-batch kernels (their tile classes stop at 96 scored positions): the general node
    long_sets = im_set is not None and s_seq is not None and flags & (HEAD_ALIGN_HINGE | HEAD_LISTNET) and \
        is_long(im_set.shape[1], s_seq.shape[1])
    args = (img_emb, cap_emb, im_set, s_seq, im_len_t, s_len_t, margin, max_violation, flags, w, temperature, eps)
    if img_emb.shape[0] <= SMALL_BATCH_MAX and not long_sets:
        return _SmallHeads.apply(*args)
    return _BigHeads.apply(*args, _caption_fill(s_len, s_seq.shape[1]) if (not max_violation and flags & HEAD_ALIGN_HINGE) else None)


small_batch_loss_heads = loss_heads            # its first name, from when it took B <= SMALL_BATCH_MAX only


class _MatchHinge(torch.autograd.Function):
    """(hinge loss on M, M) with M = im @ s.T (alad/loss.py:8-11 + :42-67) as ONE autograd node at any batch size: forward = the
    exact-fp32 GEMM + the fused hinge, backward = aladin_grad_combine (g_loss * dLoss/dM + g_M in one launch) + two GEMMs.  Both
    outputs are differentiable, as ContrastiveLoss(return_similarity_mat=True)'s are in the reference."""

    @staticmethod
    def forward(ctx, im, s, margin, max_violation):
        a, b = _unit_cols(im), _unit_cols(s)
        M = _product(a, b)
        loss, dM, _ = _hinge_raw(M, margin, max_violation, any(ctx.needs_input_grad[:2]))
        ctx.save_for_backward(a, b, dM)
        ctx.set_materialize_grads(False)
        return loss, M

    @staticmethod
    def backward(ctx, g_loss, g_M):
        a, b, dM = ctx.saved_tensors
        if (g_loss is None or dM is None) and g_M is None:
            return None, None, None, None
        C_tot = g_M
        if g_loss is not None and dM is not None:
            C_tot = _grad_combine(_upstream(g_loss), 1.0, dM, out=torch.empty_like(dM))
            if g_M is not None:         # g_M would need weight 1 / g in the second matrix slot -- not expressible: a separate add
                C_tot = C_tot + g_M.contiguous()
        return (*_product_backward(C_tot, a, b, ctx.needs_input_grad[0], ctx.needs_input_grad[1]), None, None)


def match_hinge(im, s, margin, max_violation):
    """(loss, M) of ContrastiveLoss(measure='dot') in one autograd node -- the matching head as alad_model.py:380 calls it
    every step.  B <= SMALL_BATCH_MAX: the small-batch kernels (two launches forward, one backward); above: GEMM + fused hinge."""
    _require_gpu(im, s)
    if im.dim() != 2 or s.dim() != 2 or im.shape != s.shape:
        raise ValueError('aladin_amd: the contrastive loss needs a square score matrix: two (B, D) embedding matrices of equal shape '
                         '(the reference fails in diag/expand_as, alad/loss.py:43-45); got %s and %s' % (tuple(im.shape), tuple(s.shape)))
    if im.shape[0] <= SMALL_BATCH_MAX:
        loss, _, M = _SmallMatchDistill.apply(im, s, None, margin, max_violation, True, 6.0, 1e-10)
        return loss, M
    return _MatchHinge.apply(im, s, margin, max_violation)


class _MatchCrossEntropy(torch.autograd.Function):
    """(cross-entropy loss on M, M) with M = im @ s.T (alad/loss.py:196-200) as ONE autograd node, built like _MatchHinge: forward = the
    exact-fp32 GEMM + aladin_xent_fwd_bwd, backward = aladin_grad_combine (the upstream gradient times the saved dM and
    d log_temperature, one launch) + two GEMMs.  Both outputs are differentiable."""

    @staticmethod
    def forward(ctx, im, s, log_t):
        a, b = _unit_cols(im), _unit_cols(s)
        M = _product(a, b)
        ctx.want_dt = ctx.needs_input_grad[2]
        loss, grads = _xent_raw(M, log_t, any(ctx.needs_input_grad), ctx.want_dt)
        ctx.save_for_backward(a, b, grads)
        ctx.t_shape = log_t.shape
        ctx.set_materialize_grads(False)
        return loss, M

    @staticmethod
    def backward(ctx, g_loss, g_M):
        a, b, grads = ctx.saved_tensors
        if (g_loss is None or grads is None) and g_M is None:
            return None, None, None
        C_tot, d_t = g_M, None
        if g_loss is not None and grads is not None:
            C_tot, d_t = _xent_scale(grads, g_loss, a.shape[0], ctx.want_dt, ctx.t_shape)
            if g_M is not None:
                C_tot = C_tot + g_M
        return (*_product_backward(C_tot, a, b, ctx.needs_input_grad[0], ctx.needs_input_grad[1]), d_t)


def match_cross_entropy(im, s, log_temperature, return_scores=False):
    """CrossEntropyCriterion (reference alad/loss.py:190-201) from the embeddings in one autograd node: M = im @ s.T in exact fp32,
    then the symmetric cross-entropy of M * exp(log_temperature).  log_temperature: a one-element float32 GPU tensor (the module's
    parameter; it gets a gradient) or a Python float.  -> loss, or (loss, M) with return_scores; both are differentiable."""
    _require_tensors(im, s)
    if im.dim() != 2 or s.dim() != 2 or im.shape != s.shape or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError('aladin_amd: the cross-entropy criterion needs a square score matrix: two (B, D) embedding matrices of equal '
                         'shape (the reference fails in F.cross_entropy, alad/loss.py:198-199); got %s and %s'
                         % (tuple(im.shape), tuple(s.shape)))
    _require_gpu(im, s)
    _xent_limit(im.shape[0])
    loss, M = _MatchCrossEntropy.apply(im, s, _xent_temperature(log_temperature, im.device))
    return (loss, M) if return_scores else loss


def small_batch_match_distill(im, s, teacher, margin, max_violation, want_hinge=True, temperature=6.0, eps=1e-10):
    """-> (hinge_loss, listnet_loss, M) for B <= SMALL_BATCH_MAX unit-norm global embeddings im, s (B, D):
    M = im @ s.T (alad/loss.py:8-11), the VSE++ hinge on it (:42-67, if want_hinge) and the ListNet distillation from
    `teacher` (:427-445, detached; None = no distillation) -- two launches per step instead of about twelve."""
    _require_gpu(im, s)
    if im.dim() != 2 or s.dim() != 2 or im.shape != s.shape:
        raise ValueError('aladin_amd: two (B, D) embedding matrices of equal shape expected')
    if im.shape[0] > SMALL_BATCH_MAX:
        raise ValueError('aladin_amd: small_batch_match_distill takes B <= %d' % SMALL_BATCH_MAX)
    if teacher is not None:
        _require_gpu(teacher)
        if tuple(teacher.shape) != (im.shape[0], im.shape[0]):
            raise ValueError('aladin_amd: teacher scores must be (B, B)')
        teacher = teacher.detach()
    if not want_hinge and teacher is None:                    # scores only: the plain differentiable dot-product node
        return im.new_zeros(()), im.new_zeros(()), dot_scores(im, s)
    return _SmallMatchDistill.apply(im, s, teacher, margin, max_violation, want_hinge, temperature, eps)
