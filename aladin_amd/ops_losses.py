"""Score-matrix losses and the exact-fp32 products over the C ABI: the VSE++ hinge, ListNet and the other distillation modes,
the symmetric cross-entropy criterion, the attention distillation, order / dot similarities, l2norm (reference alad/loss.py:8-67,
190-201, 273-334, 359-447, alad/utils.py:134-139).  Autograd plumbing only."""
import ctypes as C

import torch

from . import _lib
from ._ops_common import (_stream, _ptr, _require_gpu, _require_tensors, _require_square, _rows_inner_contig, _ld, _workspace, _unit_cols,
                          _set_view, _grad_view, _pad_features, _check_sets, _upstream)


def _loss_buffers(scores, want_grad, workspace_bytes, loss_out=None):
    """What a *_fwd_bwd call on a (B, B) score matrix writes: -> (B, loss scalar, its gradient matrix or None, workspace).
    loss_out: a one-element float32 view the kernel writes the loss into (instead of a fresh scalar)."""
    B, dev = scores.shape[0], scores.device
    loss = loss_out if loss_out is not None else torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty((B, B), dtype=torch.float32, device=dev) if want_grad else None
    return B, loss, grad, _workspace(workspace_bytes(B), dev)


def _hinge_raw(scores, margin, max_violation, want_grad, want_pairs=False, loss_out=None):
    """-> (loss, dS or None, pairs or None); pairs = (int32 list of non-zero i*B+j, int32 count); loss_out: see _loss_buffers."""
    lib = _lib.load()
    sc, dev = _unit_cols(scores), scores.device
    B, loss, dS, ws = _loss_buffers(scores, want_grad, lib.aladin_hinge_workspace_bytes, loss_out)
    pairs = None
    if want_grad and want_pairs:
        pairs = (torch.empty(B * B, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    _lib.check(lib.aladin_hinge_fused(_ptr(sc), _ld(sc), B, float(margin), int(bool(max_violation)), _ptr(loss),
                                      _ptr(dS), _ptr(pairs[0] if pairs else None), _ptr(pairs[1] if pairs else None),
                                      _ptr(ws), _stream()), 'hinge_fused')
    return loss, dS, pairs


def _listnet_raw(teacher, student, temperature, eps, want_grad, loss_out=None):
    """-> (loss, dM or None), dM the gradient on the student; loss_out: see _loss_buffers."""
    lib = _lib.load()
    t, m = _unit_cols(teacher), _unit_cols(student)
    B, loss, dM, ws = _loss_buffers(student, want_grad, lib.aladin_listnet_workspace_bytes, loss_out)
    _lib.check(lib.aladin_listnet_fwd_bwd(_ptr(t), _ld(t), _ptr(m), _ld(m), B, float(temperature), float(eps), _ptr(loss), _ptr(dM),
                                          _ptr(ws), _stream()), 'listnet_fwd_bwd')
    return loss, dM


def _grad_combine(g, w_a, A, w_b=0.0, B=None, out=None, w_scale=0.0, scale=None):
    """aladin_grad_combine, one launch: out = g * (w_a * A + w_b * B) over out's elements (A, B at least as long; None: not there)
    and scale = g * w_scale, g the _upstream scalar.  -> out"""
    _lib.check(_lib.load().aladin_grad_combine(out.numel() if out is not None else 0, _ptr(g), w_a, _ptr(A), w_b, _ptr(B), _ptr(out),
                                               w_scale, _ptr(scale), _stream()), 'grad_combine')
    return out


def _scaled(saved, g):
    return saved * g if saved is not None else None


# ------------------------------------------------------------------------------------------------
# hinge / listnet / distillation modes: ONE *_fwd_bwd call leaves the loss and its gradient for an upstream 1, which goes through
# save_for_backward (released by backward(); a second backward() without retain_graph raises); backward scales it
# ------------------------------------------------------------------------------------------------
class _Hinge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, margin, max_violation):
        loss, dS, _ = _hinge_raw(scores, margin, max_violation, ctx.needs_input_grad[0])
        ctx.save_for_backward(dS)
        return loss

    @staticmethod
    def backward(ctx, g):
        return _scaled(ctx.saved_tensors[0], g), None, None


def hinge_loss(scores, margin, max_violation):
    """VSE++ hinge on a square score matrix; replaces reference alad/loss.py:42-67."""
    _require_gpu(scores)
    _require_square(scores, 'the contrastive loss', ' (the reference fails in diag/expand_as, alad/loss.py:43-45)')
    return _Hinge.apply(scores, margin, max_violation)


class _ListNet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, teacher, student, temperature, eps):
        loss, dM = _listnet_raw(teacher, student, temperature, eps, ctx.needs_input_grad[1])
        ctx.save_for_backward(dM)
        return loss

    @staticmethod
    def backward(ctx, g):
        return None, _scaled(ctx.saved_tensors[0], g), None, None


def listnet_loss(teacher_scores, student_scores, temperature=6.0, eps=1e-10):
    """ListNet distillation; replaces reference alad/loss.py:427-445 (teacher detached, :370)."""
    _require_gpu(teacher_scores, student_scores)
    if teacher_scores.shape != student_scores.shape:
        raise ValueError('aladin_amd: listnet needs two square score matrices of equal shape')
    _require_square(student_scores, 'listnet')
    return _ListNet.apply(teacher_scores.detach(), student_scores, temperature, eps)


class _DistillMode(torch.autograd.Function):
    """mse / contrastive / ordinal distillation: forward computes loss and d student in one call."""

    @staticmethod
    def forward(ctx, teacher, student, wb, mode, margin, threshold, stride):
        lib = _lib.load()
        t, m = _unit_cols(teacher), _unit_cols(student)
        B, loss, dM, ws = _loss_buffers(student, ctx.needs_input_grad[1], lib.aladin_distill_workspace_bytes)
        mats = (_ptr(t), _ld(t), _ptr(m), _ld(m), B)
        dwb = None
        if mode == 'mse':
            w = wb.detach().to(torch.float32).contiguous()
            dwb = torch.empty(2, dtype=torch.float32, device=student.device) if ctx.needs_input_grad[2] else None
            _lib.check(lib.aladin_distill_mse_fwd_bwd(*mats, _ptr(w), _ptr(loss), _ptr(dM), _ptr(dwb), _ptr(ws), _stream()),
                       'distill_mse_fwd_bwd')
        elif mode == 'contrastive':
            _lib.check(lib.aladin_distill_contrastive_fwd_bwd(*mats, float(margin), _ptr(loss), _ptr(dM), _ptr(ws), _stream()),
                       'distill_contrastive_fwd_bwd')
        else:
            _lib.check(lib.aladin_distill_ordinal_fwd_bwd(*mats, float(margin), float(threshold), int(stride), _ptr(loss), _ptr(dM),
                                                          _ptr(ws), _stream()), 'distill_ordinal_fwd_bwd')
        ctx.save_for_backward(dM, dwb)
        return loss

    @staticmethod
    def backward(ctx, g):
        dM, dwb = ctx.saved_tensors
        return None, _scaled(dM, g), _scaled(dwb, g), None, None, None, None


def distillation_loss(teacher_scores, student_scores, mode, margin=0.2, threshold=0.1, stride=3, wb=None):
    """DistillationLoss modes 'mse' / 'contrastive' / 'ordinal'; replaces reference alad/loss.py:371-425
    (teacher detached, :370).  ``wb`` is the learnable (2,) pair of the 'mse' mode (:366)."""
    _require_gpu(teacher_scores, student_scores)
    if mode not in ('mse', 'contrastive', 'ordinal'):
        raise ValueError('aladin_amd: unknown distillation mode %r' % (mode,))
    if teacher_scores.shape != student_scores.shape:
        raise ValueError('aladin_amd: distillation needs two square score matrices of equal shape')
    _require_square(student_scores, 'distillation')
    if mode == 'mse':
        if wb is None or wb.numel() != 2:
            raise ValueError("aladin_amd: mode 'mse' needs the (2,) parameter wb")
        _require_gpu(wb)
    elif mode == 'ordinal' and not 1 <= int(stride) < student_scores.shape[0]:
        raise ValueError('aladin_amd: ordinal distillation needs 1 <= stride < B')
    return _DistillMode.apply(teacher_scores.detach(), student_scores, wb, mode, margin, threshold, stride)


ORDER_BWD_PARTNERS = 16384        # order_bwd_kernel keeps one weight per partner row in 64 KiB of LDS


class _OrderScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im, s):
        lib = _lib.load()
        a, b = _unit_cols(im), _unit_cols(s)
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
        _lib.check(lib.aladin_order_sim_fwd(_ptr(a), _ld(a), _ptr(b), _ld(b), a.shape[0], b.shape[0], a.shape[1],
                                            _ptr(out), out.stride(0), _stream()), 'order_sim_fwd')
        ctx.save_for_backward(a, b, out)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        a, b, out = ctx.saved_tensors
        g = g.contiguous()
        # fresh row-major outputs: empty_like would keep the arbitrary row stride a single-row view reports
        d_im = torch.empty(a.shape, dtype=torch.float32, device=a.device) if ctx.needs_input_grad[0] else None
        d_s = torch.empty(b.shape, dtype=torch.float32, device=b.device) if ctx.needs_input_grad[1] else None
        _lib.check(lib.aladin_order_sim_bwd(_ptr(a), _ld(a), _ptr(b), _ld(b), a.shape[0], b.shape[0], a.shape[1],
                                            _ptr(g), _ld(g), _ptr(out), out.stride(0), _ptr(d_im),
                                            d_im.stride(0) if d_im is not None else 0, _ptr(d_s),
                                            d_s.stride(0) if d_s is not None else 0, _stream()), 'order_sim_bwd')
        return d_im, d_s


def order_scores(im, s):
    """-||max(s_j - im_i, 0)||; replaces order_sim, reference alad/loss.py:20-26."""
    _require_gpu(im, s)
    if im.dim() != 2 or s.dim() != 2 or im.shape[1] != s.shape[1]:
        raise ValueError('aladin_amd: (Bi,D) and (Bc,D) embeddings expected')
    if torch.is_grad_enabled() and (im.requires_grad or s.requires_grad) and max(im.shape[0], s.shape[0]) > ORDER_BWD_PARTNERS:
        # the limit of aladin_order_sim_bwd (distill.hip), reported here and not inside loss.backward()
        raise ValueError('aladin_amd: differentiable order scores support at most %d rows per side (got %d x %d); score under '
                         'torch.no_grad()' % (ORDER_BWD_PARTNERS, im.shape[0], s.shape[0]))
    return _OrderScores.apply(im, s)


# ------------------------------------------------------------------------------------------------
# dot-product scores (matching head)
# ------------------------------------------------------------------------------------------------
def _sgemm(M, N, K, A, a_rs, a_cs, B, b_rs, b_cs, out):
    _lib.check(_lib.load().aladin_sgemm_strided(M, N, K, _ptr(A), a_rs, a_cs, _ptr(B), b_rs, b_cs, _ptr(out),
                                                out.stride(0), _stream()), 'sgemm_strided')
    return out


def _product(a, b, M=None):
    """M = a @ b.T, a (Bi, D) and b (Bc, D) read through their strides: M[m][n] = sum_k a[m,k] * b[n,k], into a fresh or the given M."""
    if M is None:
        M = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    return _sgemm(a.shape[0], b.shape[0], a.shape[1], a, a.stride(0), a.stride(1), b, b.stride(1), b.stride(0), M)


def _product_backward(C, a, b, want_a=True, want_b=True):
    """(d_a, d_b) = (C @ b, C.T @ a) of M = a @ b.T for the gradient C on M; None for a product that is not wanted.  C is made
    row-major here: autograd hands over (0, 1)- and (0, 0)-strided gradients."""
    C = C.contiguous()
    (Bi, D), Bc = a.shape, b.shape[0]
    d_a = d_b = None
    if want_a:
        d_a = _sgemm(Bi, D, Bc, C, C.stride(0), 1, b, b.stride(0), b.stride(1), torch.empty((Bi, D), dtype=torch.float32, device=a.device))
    if want_b:
        d_b = _sgemm(Bc, D, Bi, C, 1, C.stride(0), a, a.stride(0), a.stride(1), torch.empty((Bc, D), dtype=torch.float32, device=a.device))
    return d_a, d_b


class _DotScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im, s):
        ctx.save_for_backward(im, s)
        return _product(im, s)

    @staticmethod
    def backward(ctx, dM):
        return _product_backward(dM, *ctx.saved_tensors)


def dot_scores(im, s):
    """im @ s.T in exact fp32 on the MFMA; replaces dot_sim, reference alad/loss.py:8-11."""
    _require_gpu(im, s)
    if im.dim() != 2 or s.dim() != 2 or im.shape[1] != s.shape[1]:
        raise ValueError('aladin_amd: (Bi,D) and (Bc,D) embeddings expected')
    return _DotScores.apply(im, s)


# ------------------------------------------------------------------------------------------------
# nearest-neighbour entropy (uniformity) term
# ------------------------------------------------------------------------------------------------
def _nn_entropy_raw(img, cap, want_loss):
    """aladin_nn_entropy_fwd on img (B, D) and cap (B, D) or None -> (loss or None, nn int32 (N,), dist (N,))."""
    lib = _lib.load()
    B, D = img.shape
    N = B * (2 if cap is not None else 1)
    dev = img.device
    loss = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
    nn = torch.empty(N, dtype=torch.int32, device=dev)
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    ws = _workspace(lib.aladin_nn_entropy_workspace_bytes(N), dev)
    _lib.check(lib.aladin_nn_entropy_fwd(_ptr(img), _ld(img), _ptr(cap), _ld(cap) if cap is not None else 0, B, D, _ptr(loss),
                                         _ptr(nn), _ptr(dist), _ptr(ws), _stream()), 'nn_entropy_fwd')
    return loss, nn, dist


def _nn_entropy_limit(N):
    if N > _lib.NN_ENTROPY_MAX_N:
        raise ValueError('aladin_amd: the nearest-neighbour search covers N <= %d rows, got %d' % (_lib.NN_ENTROPY_MAX_N, N))


class _NNEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, cap):
        a, b = _unit_cols(img), _unit_cols(cap)
        loss, nn, dist = _nn_entropy_raw(a, b, True)
        ctx.save_for_backward(a, b, nn, dist)
        ctx.mark_non_differentiable(nn, dist)
        return loss, nn, dist

    @staticmethod
    def backward(ctx, g, _g_nn, _g_dist):
        a, b, nn, dist = ctx.saved_tensors
        g = _upstream(g)
        d_img, d_cap = torch.empty_like(a, memory_format=torch.contiguous_format), torch.empty_like(b, memory_format=torch.contiguous_format)
        _lib.check(_lib.load().aladin_nn_entropy_bwd(_ptr(a), _ld(a), _ptr(b), _ld(b), a.shape[0], a.shape[1], _ptr(nn), _ptr(dist),
                                                     _ptr(g), _ptr(d_img), _ptr(d_cap), _stream()), 'nn_entropy_bwd')
        return d_img, d_cap


def nn_entropy_loss(img_emb, cap_emb, return_neighbours=False):
    """-mean_i log(N * ||x_i - x_nn(i) + 1e-6||) over the N = 2 B rows of cat([img_emb, cap_emb]), nn(i) the other row of largest
    inner product; replaces the 'entropy' term, reference alad/alad_model.py:410-421.  Ties go to the lowest index; no gradient
    flows through the neighbour choice.  return_neighbours: also the neighbour indices, int64 (N,)."""
    _require_gpu(img_emb, cap_emb)
    if img_emb.dim() != 2 or img_emb.shape != cap_emb.shape or img_emb.shape[0] < 1 or img_emb.shape[1] < 1:
        raise ValueError('aladin_amd: two non-empty (B, D) embedding matrices of equal shape expected')
    _nn_entropy_limit(2 * img_emb.shape[0])
    loss, nn, _ = _NNEntropy.apply(img_emb, cap_emb)
    return (loss, nn.to(torch.int64)) if return_neighbours else loss


def pairwise_nns_inner(x):
    """Index of every row's nearest other row by inner product, int64 (N,); replaces pairwise_NNs_inner, reference
    alad/alad_model.py:17-27 (diagonal set to -1, not -inf).  Ties go to the lowest index."""
    _require_gpu(x)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError('aladin_amd: a non-empty (N, D) matrix expected')
    _nn_entropy_limit(x.shape[0])
    x = x.detach()
    return _nn_entropy_raw(_unit_cols(x), None, False)[1].to(torch.int64)


# ------------------------------------------------------------------------------------------------
# symmetric cross-entropy (InfoNCE) with a learnable temperature
# ------------------------------------------------------------------------------------------------
def _xent_limit(B):
    if B > _lib.XENT_MAX_B:
        raise ValueError('aladin_amd: the cross-entropy criterion covers B <= %d, got %d' % (_lib.XENT_MAX_B, B))


def _xent_temperature(log_temperature, device):
    """-> the one-element float32 device tensor the kernels read: the caller's (it gets the gradient) or a constant made here"""
    if isinstance(log_temperature, torch.Tensor):
        _require_gpu(log_temperature)
        if log_temperature.numel() != 1:
            raise ValueError('aladin_amd: log_temperature is one element, got shape %s' % (tuple(log_temperature.shape),))
        return log_temperature
    return torch.full((1,), float(log_temperature), dtype=torch.float32, device=device)       # a fill: no host wait


def _xent_raw(scores, log_t, want_grad, want_dt):
    """aladin_xent_fwd_bwd on a square matrix with unit column stride -> (loss, grads or None): grads is ONE (B * B + 1,) buffer,
    dS row-major followed by d log_temperature, so that the backward scales both in one aladin_grad_combine launch."""
    lib = _lib.load()
    B = scores.shape[0]
    dev = scores.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grads = torch.empty(B * B + 1, dtype=torch.float32, device=dev) if want_grad else None
    ws = _workspace(lib.aladin_xent_workspace_bytes(B), dev)
    dt = C.c_void_p(grads.data_ptr() + 4 * B * B) if (want_grad and want_dt) else C.c_void_p(0)
    _lib.check(lib.aladin_xent_fwd_bwd(_ptr(scores), _ld(scores), B, _ptr(log_t), _ptr(loss), _ptr(grads), dt, _ptr(ws), _stream()),
               'xent_fwd_bwd')
    return loss, grads


def _xent_scale(grads, g, B, want_dt, t_shape):
    """-> (g * dS as (B, B), g * d log_temperature in t_shape or None) from _xent_raw's buffer, in one launch"""
    n = B * B
    out = _grad_combine(_upstream(g), 1.0, grads, out=torch.empty(n + (1 if want_dt else 0), dtype=torch.float32, device=grads.device))
    return out[:n].view(B, B), (out[n:].view(t_shape) if want_dt else None)


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, log_t):
        B = scores.shape[0]
        sc = _unit_cols(scores)
        ctx.want_dt = ctx.needs_input_grad[1]
        loss, grads = _xent_raw(sc, log_t, ctx.needs_input_grad[0] or ctx.want_dt, ctx.want_dt)
        ctx.save_for_backward(grads)
        ctx.B, ctx.t_shape = B, log_t.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (grads,) = ctx.saved_tensors
        if grads is None:
            return None, None
        dS, d_t = _xent_scale(grads, g, ctx.B, ctx.want_dt, ctx.t_shape)
        return (dS if ctx.needs_input_grad[0] else None), d_t


def cross_entropy_scores(scores, log_temperature):
    """Symmetric cross-entropy (InfoNCE) of a square score matrix: with L = scores * exp(log_temperature), the mean of
    cross_entropy(L, arange) and cross_entropy(L.T, arange) -- what CrossEntropyCriterion (reference alad/loss.py:190-201) computes
    from its logits.  log_temperature: a one-element float32 GPU tensor (it gets a gradient) or a Python float (a constant).
    One autograd node, two launches forward; the backward scales the saved gradients by the upstream one in one launch."""
    _require_tensors(scores)
    _require_square(scores, 'the cross-entropy criterion', ' (the reference fails in F.cross_entropy, alad/loss.py:198-199)')
    _require_gpu(scores)
    _xent_limit(scores.shape[0])
    return _CrossEntropy.apply(scores, _xent_temperature(log_temperature, scores.device))


# ------------------------------------------------------------------------------------------------
# semantic contrastive loss (the hinge anchored at relevance-chosen positives)
# ------------------------------------------------------------------------------------------------
SEMANTIC_COLUMN_ORDERS = ('reference', 'aligned')


class _SemanticHinge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, rel, draws, margin, threshold, flags, want_positives):
        lib = _lib.load()
        sc = _unit_cols(scores)
        B, loss, dS, ws = _loss_buffers(scores, ctx.needs_input_grad[0], lib.aladin_semantic_hinge_workspace_bytes)
        pos = torch.empty(2 * B, dtype=torch.int32, device=scores.device) if want_positives else None
        _lib.check(lib.aladin_semantic_hinge_fwd_bwd(_ptr(sc), _ld(sc), _ptr(rel), rel.stride(0), rel.stride(1), B, float(margin),
                                                     float(threshold), int(flags), _ptr(draws), _ptr(loss), _ptr(dS), _ptr(pos),
                                                     _ptr(ws), _stream()), 'semantic_hinge_fwd_bwd')
        ctx.save_for_backward(dS)
        if pos is None:
            return loss
        ctx.mark_non_differentiable(pos)
        return loss, pos

    @staticmethod
    def backward(ctx, g, *_):
        return _scaled(ctx.saved_tensors[0], g), None, None, None, None, None, None


def semantic_hinge_loss(scores, relevances, margin, threshold=0.4, max_violation=False, *, draws=None, generator=None,
                        column_positives='reference', mask_positives=False, return_positives=False):
    """The hinge of a square score matrix (images x captions) anchored at relevance-chosen positives; replaces
    compute_semantic_contrastive_loss, reference alad/loss.py:216-261.  Per row and per column ONE positive is drawn among the
    pairs with relevances > threshold (the ``draws[v] mod n``-th of a line's n candidates, ascending; a line WITHOUT candidates
    falls back to its diagonal cell, where the reference raises); the costs are cleared on the diagonal, as the reference's.
    relevances: (B, B) float32 aligned with scores, read in place through its strides (a transposed or sliced view costs no copy);
    it gets no gradient.  draws: int32 (2B,) on the device, values in [0, 2^31 - 1): rows, then columns; None draws them there
    with torch.randint(0, 2**31 - 1, ...) from ``generator`` -- the reference's distribution up to a modulo bias below B / 2^31,
    not its host stream.  column_positives: 'reference' hands the column anchors out in the row-major order the reference reads
    them back in, 'aligned' gives column j its own.  mask_positives (not in the reference): the costs are also cleared wherever
    relevances > threshold.  return_positives: also the int32 (2B,) choice, every row's column then every column's row.
    One autograd node: four launches ('aligned': three), no host synchronisation."""
    _require_tensors(scores, relevances)
    _require_square(scores, 'the semantic contrastive loss')
    if tuple(relevances.shape) != tuple(scores.shape):
        raise ValueError('aladin_amd: relevances of shape %s expected (aligned with the scores), got %s'
                         % (tuple(scores.shape), tuple(relevances.shape)))
    B = scores.shape[0]
    if B > _lib.SEM_MAX_B:
        raise ValueError('aladin_amd: the semantic contrastive loss covers B <= %d, got %d' % (_lib.SEM_MAX_B, B))
    if column_positives not in SEMANTIC_COLUMN_ORDERS:
        raise ValueError("aladin_amd: column_positives is 'reference' or 'aligned', got %r" % (column_positives,))
    if draws is not None:
        if not isinstance(draws, torch.Tensor):
            raise TypeError('aladin_amd: draws is an int32 tensor, got %r' % type(draws))
        if draws.dtype != torch.int32 or tuple(draws.shape) != (2 * B,):
            raise ValueError('aladin_amd: draws is an int32 tensor of shape (%d,) (rows, then columns), got %s of shape %s'
                             % (2 * B, draws.dtype, tuple(draws.shape)))
    _require_gpu(scores, relevances)
    if relevances.device != scores.device:
        raise RuntimeError('aladin_amd: relevances on %s, scores on %s' % (relevances.device, scores.device))
    if draws is None:
        draws = torch.randint(0, 2 ** 31 - 1, (2 * B,), dtype=torch.int32, device=scores.device, generator=generator)
    elif draws.device != scores.device:
        raise RuntimeError('aladin_amd: draws must live on the device of the scores (%s), got %s; they are read by the kernel'
                           % (scores.device, draws.device))
    flags = (_lib.SEM_MAX_VIOLATION if max_violation else 0) | (_lib.SEM_COLUMNS_ALIGNED if column_positives == 'aligned' else 0) \
        | (_lib.SEM_MASK_POSITIVES if mask_positives else 0)
    return _SemanticHinge.apply(scores, relevances.detach(), draws.contiguous(), margin, threshold, flags, bool(return_positives))


# ------------------------------------------------------------------------------------------------
# attention distillation (softmax over regions against a teacher's attention, every pair)
# ------------------------------------------------------------------------------------------------
def _attdistill_args(im, s, im_len_t, s_len_t, teacher):
    """the argument run aladin_attdistill_fwd / _bwd share (the views must stay alive until the call returned)"""
    sv_im, sv_s = _set_view(im, im_len_t), _set_view(s, s_len_t)
    Bi, R, D = im.shape
    Bc, T, _ = s.shape
    return (sv_im, sv_s), [C.byref(sv_im), C.byref(sv_s), Bi, Bc, R, T, D, _ptr(teacher), teacher.stride(0), teacher.stride(1),
                           teacher.stride(2), teacher.shape[2], teacher.shape[3]]


class _AttDistill(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im, s, im_len_t, s_len_t, teacher):
        lib = _lib.load()
        Bi, R, D = im.shape
        Bc, T, _ = s.shape
        loss = torch.empty((), dtype=torch.float32, device=im.device)
        ws = _workspace(lib.aladin_attdistill_workspace_bytes(Bi, Bc, R, T, D), im.device)
        keep, args = _attdistill_args(im, s, im_len_t, s_len_t, teacher)
        _lib.check(lib.aladin_attdistill_fwd(*args, _ptr(loss), _ptr(ws), _stream()), 'attdistill_fwd')
        ctx.save_for_backward(im, s, im_len_t, s_len_t, teacher, ws)
        return loss

    @staticmethod
    def backward(ctx, g):
        im, s, im_len_t, s_len_t, teacher, ws = ctx.saved_tensors
        g = _upstream(g)
        # fresh row-major outputs; the kernels write every row (slot 0 and masked positions as zeros)
        d_im = torch.empty(im.shape, dtype=torch.float32, device=im.device) if ctx.needs_input_grad[0] else None
        d_s = torch.empty(s.shape, dtype=torch.float32, device=s.device) if ctx.needs_input_grad[1] else None
        if d_im is None and d_s is None:
            return None, None, None, None, None
        gv_im = _grad_view(d_im) if d_im is not None else None
        gv_s = _grad_view(d_s) if d_s is not None else None
        keep, args = _attdistill_args(im, s, im_len_t, s_len_t, teacher)
        _lib.check(_lib.load().aladin_attdistill_bwd(*args, _ptr(g), C.byref(gv_im) if gv_im is not None else None,
                                                     C.byref(gv_s) if gv_s is not None else None, _ptr(ws), _stream()), 'attdistill_bwd')
        return d_im, d_s, None, None, None


def attention_distillation_loss(im_set, s_seq, im_len, s_len, teacher):
    """KL(teacher attention || softmax over regions of <word, region> / sqrt(D)) over every (image, caption) pair and every word,
    'batchmean' over the Bi * sum_j (s_len[j] - 1) word rows; replaces AttentionDistillationLoss.forward, reference
    alad/loss.py:277-334.  teacher: (Bi, Bc, Wt, Rt) float32 with Wt >= T - 1, Rt >= R - 1 and a unit innermost stride, read in
    place through its strides (the reference's 69 x 70 tensor as it is); it gets no gradient.  One autograd node: three launches
    forward, one per wanted gradient backward; the (Bi, Bc, R - 1, T - 1) logits tensor is never formed.  Masked regions drop
    out of the loss (behavioural notes)."""
    im_len_t, s_len_t = _check_sets(im_set, s_seq, im_len, s_len)
    Bi, R, _ = im_set.shape
    Bc, T, _ = s_seq.shape
    if Bi < 1 or Bc < 1 or R < 2 or T < 2 or im_set.shape[2] < 1:
        raise ValueError('aladin_amd: attention distillation needs non-empty sets with at least one scored position, got %s and %s'
                         % (tuple(im_set.shape), tuple(s_seq.shape)))
    if R - 1 > _lib.TILE_MAX_SCORED or T - 1 > _lib.TILE_MAX_SCORED:
        raise ValueError('aladin_amd: attention distillation covers at most %d scored positions per set (got %d regions, %d words)'
                         % (_lib.TILE_MAX_SCORED, R - 1, T - 1))
    if not isinstance(teacher, torch.Tensor) or not teacher.is_cuda or teacher.dtype != torch.float32 or teacher.device != im_set.device:
        raise ValueError('aladin_amd: the teacher attentions must be a float32 tensor on the device of the sets')
    if teacher.dim() != 4 or teacher.shape[0] != Bi or teacher.shape[1] != Bc or teacher.shape[2] < T - 1 or teacher.shape[3] < R - 1:
        raise ValueError('aladin_amd: teacher attentions of shape (%d, %d, >= %d, >= %d) expected (images, captions, words, regions), '
                         'got %s' % (Bi, Bc, T - 1, R - 1, tuple(teacher.shape)))
    if (teacher.shape[3] > 1 and teacher.stride(3) != 1) or teacher.stride(2) < teacher.shape[3] or min(teacher.stride()) < 0:
        raise ValueError('aladin_amd: the teacher attentions are read in place and need a unit innermost stride and word rows that '
                         'do not overlap (got strides %s for shape %s)' % (tuple(teacher.stride()), tuple(teacher.shape)))
    im_set, s_seq = _pad_features(im_set, s_seq)
    return _AttDistill.apply(_rows_inner_contig(im_set), _rows_inner_contig(s_seq), im_len_t, s_len_t, teacher.detach())


class _L2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _unit_cols(x)
        out = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().aladin_l2norm_fwd(_ptr(x), _ld(x), x.shape[0], x.shape[1], _ptr(out), _stream()), 'l2norm_fwd')
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = _unit_cols(g)
        dx = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().aladin_l2norm_bwd(_ptr(x), _ld(x), _ptr(g), _ld(g), x.shape[0], x.shape[1], _ptr(dx), _stream()),
                   'l2norm_bwd')
        return dx


def l2norm_rows(x):
    """X / sqrt(sum_dim1 X^2) without eps; replaces l2norm, reference alad/utils.py:134-139 (zero rows -> NaN)."""
    _require_gpu(x)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError('aladin_amd: l2norm expects a non-empty (rows, D) matrix')
    return _L2Norm.apply(x)
