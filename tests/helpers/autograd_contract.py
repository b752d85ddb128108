"""The autograd contract of the differentiable entry points, shared by tests/test_autograd_contract_cpu.py and
tests/test_autograd_contract_gpu.py.  TEST INFRASTRUCTURE.

  REGISTRY        every differentiable entry point as an Entry: its inputs (built here from seeds, read-only), gpu_call(t, st) -> the
                  tuple of outputs on the device, ref_call(t, st) -> the same tuple from a float64 torch restatement of the
                  reference's dataflow that torch's own autograd differentiates (oracle/faithful_torch.py for the alignment poolings
                  and the hinge, the short restatements below for the rest; never the code under test), and the gates the project
                  already holds for the op, imported from where they live;
  SET_LAYOUTS / MATRIX_LAYOUTS / ...   numpy array -> Layout(leaf, view, back, values): the views ordinary torch code produces;
  m_composites / l_composites          the ways a caller consumes a matrix / scalar output, named for the stride of the gradient
                                       that then reaches the node.

SKIPPED (combinations that are undefined for the op, never ones that fail):
  * nn_entropy_loss x the expanded-row / expanded-column layouts: every row equals another, so each row's nearest neighbour is an
    exact tie at distance |eps| -- the input condition of entropy_numpy (MIN_GAP) cannot hold and the gradient is ~1/eps^2 noise;
  * nn_entropy_loss's neighbour indices and distances, semantic_hinge_loss's positives, loss_heads' terms / S / M: integer or
    non-differentiable outputs, no upstream gradient exists for them (only the scalar's composites run);
  * the 'single' (1, N, D) set layout outside the entries that take a rectangle (the triplet loss and the loss heads need one
    caption per image, so a single image is a different problem, covered by their B = 1 tests elsewhere);
  * log_temperature / wb: one- and two-element parameters have no matrix layouts; they get their own (0-dim, (1,), strided)."""
import collections
import functools
import math
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import alad_oracle as O                                          # noqa: E402
import faithful_torch as FT                                      # noqa: E402
import attdistill_numpy as A                                     # noqa: E402
import entropy_numpy as E                                        # noqa: E402
import matrix_losses_numpy as H                                  # noqa: E402
import secondary_numpy as S2                                     # noqa: E402
import semantic_numpy as SM                                      # noqa: E402
import xent_numpy as X                                           # noqa: E402
from test_long_sets_gpu import RTOL, assert_grads_close, assert_scores_close, ragged_batch      # noqa: E402  (the DESIGN section 2 bars)
from test_entropy_gpu import GRAD_TOL as ENTROPY_GRAD_TOL, LOSS_TOL as ENTROPY_LOSS_TOL          # noqa: E402

Layout = collections.namedtuple('Layout', 'leaf view back values stride')
FILL = 1e30                                                      # the surroundings of a view: a stray read would swamp every result


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _only(g, index):
    """g[index], after checking that g is exactly zero everywhere else"""
    rest = g.copy()
    rest[index] = 0
    assert not rest.any(), 'gradient outside the view'
    return g[index]


# ------------------------------------------------------------------------------------------------
# input layouts: f(x numpy, to) -> Layout; to(numpy) -> a fresh torch tensor on the wanted device in the wanted dtype
# ------------------------------------------------------------------------------------------------
def _set_contig(x, to):
    leaf = to(x)
    return Layout(leaf, leaf, lambda g: g, x, tuple(leaf.stride()))


def _set_permuted(x, to):
    B, N, D = x.shape
    leaf = to(x.transpose(1, 0, 2))
    return Layout(leaf, leaf.permute(1, 0, 2), lambda g: g.transpose(1, 0, 2), x, (D, B * D, 1))


def _set_misaligned(x, to):
    B, N, D = x.shape
    big = np.full((B, N, D + 4), FILL, x.dtype)
    big[:, :, 1:D + 1] = x
    leaf = to(big)
    return Layout(leaf, leaf[:, :, 1:D + 1], lambda g: _only(g, (slice(None), slice(None), slice(1, D + 1))), x, (N * (D + 4), D + 4, 1))


def _set_strided(x, to):
    B, N, D = x.shape
    big = np.full((B, 2 * N, D), FILL, x.dtype)
    big[:, ::2] = x
    leaf = to(big)
    return Layout(leaf, leaf[:, ::2], lambda g: _only(g, (slice(None), slice(None, None, 2))), x, (2 * N * D, 2 * D, 1))


def _set_offset(x, to):
    B, N, D = x.shape
    big = np.full((B + 2, N, D), FILL, x.dtype)
    big[1:B + 1] = x
    leaf = to(big)
    return Layout(leaf, leaf[1:B + 1], lambda g: _only(g, (slice(1, B + 1),)), x, (N * D, D, 1))


def _set_expanded(x, to):
    B, N, D = x.shape
    leaf = to(x[:1])
    return Layout(leaf, leaf.expand(B, N, D), lambda g: g, np.broadcast_to(x[:1], x.shape).copy(), (0, D, 1))


def _set_single(x, to):
    _, N, D = x.shape
    leaf = to(x[:1].transpose(1, 0, 2))                          # (N, 1, D): the model's (S, B, D) layout at B = 1
    return Layout(leaf, leaf.permute(1, 0, 2), lambda g: g.transpose(1, 0, 2), x[:1].copy(), (D, D, 1))


SET_LAYOUTS = collections.OrderedDict([('contig', _set_contig), ('permuted', _set_permuted), ('misaligned', _set_misaligned),
                                       ('strided', _set_strided), ('offset', _set_offset), ('expanded', _set_expanded),
                                       ('single', _set_single)])


def _mat_contig(x, to):
    leaf = to(x)
    return Layout(leaf, leaf, lambda g: g, x, (x.shape[1], 1))


def _mat_t(x, to):
    leaf = to(x.T)
    return Layout(leaf, leaf.t(), lambda g: g.T, x, (1, x.shape[0]))


def _mat_cols(x, to):
    rows, K = x.shape
    big = np.full((rows, K + 7), FILL, x.dtype)
    big[:, 3:3 + K] = x
    leaf = to(big)
    return Layout(leaf, leaf[:, 3:3 + K], lambda g: _only(g, (slice(None), slice(3, 3 + K))), x, (K + 7, 1))


def _mat_inner2(x, to):
    rows, K = x.shape
    big = np.full((rows, 2 * K), FILL, x.dtype)
    big[:, ::2] = x
    leaf = to(big)
    return Layout(leaf, leaf[:, ::2], lambda g: _only(g, (slice(None), slice(None, None, 2))), x, (2 * K, 2))


def _mat_row(x, to):
    leaf = to(x[0])
    return Layout(leaf, leaf.expand(*x.shape), lambda g: g.reshape(1, -1), np.broadcast_to(x[:1], x.shape).copy(), (0, 1))


def _mat_col(x, to):
    leaf = to(x[:, :1])
    return Layout(leaf, leaf.expand(*x.shape), lambda g: g, np.broadcast_to(x[:, :1], x.shape).copy(), (1, 0))


MATRIX_LAYOUTS = collections.OrderedDict([('contig', _mat_contig), ('t', _mat_t), ('cols', _mat_cols), ('inner2', _mat_inner2),
                                          ('row', _mat_row), ('col', _mat_col)])


def _scalar_dim1(x, to):
    leaf = to(np.asarray(x, np.float32).reshape(1))
    return Layout(leaf, leaf, lambda g: g.reshape(1), np.asarray(x).reshape(1), (1,))


def _scalar_dim0(x, to):
    leaf = to(np.asarray(x, np.float32).reshape(()))
    return Layout(leaf, leaf, lambda g: g.reshape(1), np.asarray(x).reshape(1), ())


def _vec_contig(x, to):
    leaf = to(x)
    return Layout(leaf, leaf, lambda g: g, x, (1,))


def _vec_strided(x, to):
    big = np.full(2 * len(x), FILL, x.dtype)
    big[::2] = x
    leaf = to(big)
    return Layout(leaf, leaf[::2], lambda g: _only(g, (slice(None, None, 2),)), x, (2,))


LAYOUTS = {'set': SET_LAYOUTS, 'mat': MATRIX_LAYOUTS,
           'scalar': collections.OrderedDict([('contig', _scalar_dim1), ('dim0', _scalar_dim0)]),
           'vec': collections.OrderedDict([('contig', _vec_contig), ('strided', _vec_strided)])}
SUMMED = ('expanded', 'single', 'row', 'col')                    # layouts whose values differ from the base array's
EXPANDED = ('expanded', 'row', 'col')                            # ... whose leaf gradient is a sum over the expanded axis


def to_leaf(kind, layout, full):
    """an array of the view's shape -> the leaf's gradient layout AFTER back(): the sum over what the leaf is expanded along"""
    if (kind, layout) == ('set', 'expanded'):
        return full.sum(0, keepdims=True)
    if (kind, layout) == ('mat', 'row'):
        return full.sum(0, keepdims=True)
    if (kind, layout) == ('mat', 'col'):
        return full.sum(1, keepdims=True)
    return full


# ------------------------------------------------------------------------------------------------
# upstream composites: f(outs, K) -> scalar; K(key, shape, like) -> a constant tensor like `like`; applied unchanged to both sides
# ------------------------------------------------------------------------------------------------
def constant(key, shape):
    rng = np.random.default_rng(zlib.crc32(repr(('autograd-contract', key, tuple(shape))).encode()))
    return rng.standard_normal(shape).astype(np.float32)


def K(key, shape, like):
    return torch.from_numpy(constant(key, tuple(shape))).to(device=like.device, dtype=like.dtype)


def m_composites(i):
    """name -> (f, stride(M) of the gradient that reaches output M = o[i] of shape (r, c))"""
    return collections.OrderedDict([
        ('dense', (lambda o: (o[i] * K('W', o[i].shape, o[i])).sum(), lambda M: (M.shape[1], 1))),
        ('sum', (lambda o: o[i].sum(), lambda M: (0, 0))),
        ('cols', (lambda o: (o[i].sum(0) * K('v0', o[i].shape[1:], o[i])).sum(), lambda M: (0, 1))),
        ('rows', (lambda o: (o[i].sum(1) * K('v1', o[i].shape[:1], o[i])).sum(), lambda M: (1, 0))),
        ('t', (lambda o: (o[i].t() * K('Wt', o[i].t().shape, o[i])).sum(), lambda M: (1, M.shape[0]))),
        ('onehot', (lambda o: o[i][min(1, o[i].shape[0] - 1), min(2, o[i].shape[1] - 1)] * 3, lambda M: (M.shape[1], 1))),
        ('zerocols', (lambda o: o[i][:, 1:3].sum(), lambda M: (M.shape[1], 1))),
        ('double', (lambda o: (o[i].double() ** 2).sum(), lambda M: tuple(M.stride())))])     # the cast keeps M's own layout


L_SCALES = collections.OrderedDict([('L', 1.0), ('quarter', 0.25), ('neg2', -2.0), ('zero', 0.0)])


def l_composites(i):
    out = collections.OrderedDict((name, (lambda o, c=c: c * o[i] if c != 1.0 else o[i])) for name, c in L_SCALES.items())
    out['double3'] = lambda o: o[i].double() * 3
    return out


class Drop(torch.autograd.Function):
    """keep(x) with the unused outputs `rest` tied into its graph: their nodes run in the backward and, giving their inputs no
    gradient here, receive None for every output (a sibling graph the caller differentiates instead)."""

    @staticmethod
    def forward(ctx, x, *rest):
        ctx.n = len(rest)
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return (g,) + (None,) * ctx.n


def composites(entry):
    """name -> (f(outs) -> scalar, {output index: expected stride function}) for every way this entry's outputs are consumed"""
    out = collections.OrderedDict()
    diff = [(i, k) for i, k in enumerate(entry.outputs) if k in 'ML']
    for i, k in diff:
        tag = '' if len(diff) == 1 else 'o%d.' % i
        if k == 'L':
            for name, f in l_composites(i).items():
                out[tag + name] = (f, {})
        else:
            for name, (f, stride) in m_composites(i).items():
                out[tag + name] = (f, {i: stride})
    if len(diff) > 1:
        ls = [i for i, k in diff if k == 'L']
        ms = [i for i, k in diff if k == 'M']
        dense = m_composites(ms[0])['dense']
        out['all'] = (lambda o: 0.5 * sum(o[i] for i in ls) + dense[0](o), {ms[0]: dense[1]})
    return out


def base_composite(entry):
    return next(iter(composites(entry)))                         # (M * W).sum() of the first matrix output, else L of the first scalar


# ------------------------------------------------------------------------------------------------
# short float64 restatements (torch, differentiated by torch's own autograd)
# ------------------------------------------------------------------------------------------------
def t_l2norm(x):
    return x / x.pow(2).sum(1, keepdim=True).sqrt()              # alad/utils.py:134-139, no eps


def t_order(im, s):
    return -(s.unsqueeze(0) - im.unsqueeze(1)).clamp(min=0).pow(2).sum(2).sqrt()         # alad/loss.py:20-26


def t_listnet(teacher, student, tau=6.0, eps=1e-10):
    loss = 0
    for dim in (1, 0):                                           # alad/loss.py:431-443
        p, q = torch.softmax(teacher.detach(), dim), torch.softmax(student * tau, dim)
        loss = loss + (-(p * torch.log(q + eps)).sum(dim)).mean()
    return loss


def t_mse(teacher, student, wb):
    return ((student * wb[0] + wb[1] - teacher.detach()) ** 2).mean()                    # alad/loss.py:371-373


def t_contrastive(teacher, student, margin):
    t0 = teacher.detach().clone()                                # alad/loss.py:401-425
    t0.fill_diagonal_(0)
    diag = student.diag().view(-1, 1)
    cost_s = (margin + student - diag).clamp(min=0)
    cost_im = (margin + student - diag.t()).clamp(min=0)
    return cost_s.index_select(1, t0.argmax(1)).sum() + cost_im.index_select(0, t0.argmax(0)).sum()


def t_ordinal(teacher, student, margin, threshold, stride):
    loss = 0
    for tt, mm in ((teacher.detach(), student), (teacher.detach().t(), student.t())):    # alad/loss.py:374-399
        ts, order = torch.sort(tt, dim=1, stable=True)
        so = torch.gather(mm, 1, order)
        diff = so[:, :-stride] - so[:, stride:]
        valid = ts[:, stride:] >= threshold
        loss = loss + (margin + diff).clamp(min=0)[valid].mean()
    return loss


def t_xent(scores, log_t):
    logits = scores * torch.exp(log_t.reshape(()))               # alad/loss.py:196-200
    target = torch.arange(scores.shape[0])
    ce = torch.nn.functional.cross_entropy
    return (ce(logits, target) + ce(logits.t(), target)) / 2


def t_entropy(img, cap):
    x = torch.cat([img, cap], 0)                                 # alad/alad_model.py:17-27, 410-421
    nn = torch.from_numpy(E.neighbours(x.detach().numpy()))      # the neighbour choice carries no gradient
    dist = (x - x[nn] + E.EPS).pow(2).sum(1).sqrt()
    return -torch.log(len(x) * dist).mean()


def t_semantic(scores, rel, draws, margin, threshold):
    B = scores.shape[0]                                          # alad/loss.py:216-261, sum of violations
    pos = SM.positives(rel.detach().numpy(), threshold, draws)
    a1 = scores[torch.arange(B), torch.from_numpy(pos[:B])]
    cells = sorted((int(pos[B + j]), j) for j in range(B))
    a2 = torch.stack([scores[r, c] for r, c in cells])
    eye = torch.eye(B, dtype=torch.bool)
    cs = (margin + scores - a1.view(-1, 1)).clamp(min=0).masked_fill(eye, 0)
    ci = (margin + scores - a2.view(1, -1)).clamp(min=0).masked_fill(eye, 0)
    return cs.sum() + ci.sum()


def t_attdistill(im, s, im_len, s_len, teacher):
    Bi, R, D = im.shape                                          # alad/loss.py:277-334 with masked regions dropped
    Bc, T, _ = s.shape
    n, m = A.counts(im_len, s_len, R - 1, T - 1)
    logits = torch.einsum('jwd,ird->ijwr', s[:, 1:], im[:, 1:]) / math.sqrt(D)
    rmask = (torch.arange(R - 1)[None, :] < torch.from_numpy(n)[:, None])[:, None, None, :]
    wmask = (torch.arange(T - 1)[None, :] < torch.from_numpy(m)[:, None])[None, :, :, None]
    logp = torch.log_softmax(logits.masked_fill(~rmask, float('-inf')), dim=-1)
    a = teacher.detach()[:, :, :T - 1, :R - 1]
    p = a / a.abs().sum(-1, keepdim=True).clamp(min=1e-12)
    live = rmask & wmask & (p > 0)
    terms = torch.where(live, p * (torch.log(torch.where(live, p, torch.ones_like(p))) - torch.where(live, logp, torch.zeros_like(logp))),
                        torch.zeros_like(p))
    return terms.sum() / (Bi * int(m.sum()))


def t_heads(img, cap, im, s, st):
    """(total, terms, S, M) of alad_model.py:371-454 for the heads in st['heads'] with the hardest-negative hinges"""
    heads, w = st['heads'], st['weights']
    S = M = None
    terms = [torch.zeros((), dtype=torch.float64)] * 3
    if 'alignment' in heads or 'distillation' in heads:
        S = FT.alignment_scores_faithful(im, s, st['im_len'], st['s_len'])
    if 'matching' in heads or 'distillation' in heads:
        M = img @ cap.t()
    if 'matching' in heads:
        terms[0] = FT.hinge_faithful(M, st['margin'], True)
    if 'alignment' in heads:
        terms[1] = FT.hinge_faithful(S, st['margin'], True)
    if 'distillation' in heads:
        terms[2] = t_listnet(S.detach(), M)
    total = sum(w[k] * terms[i] for i, k in enumerate(('matching', 'alignment', 'distillation')) if k in heads)
    return total, torch.stack([t.detach() for t in terms]), (S.detach() if S is not None else None), (M.detach() if M is not None else None)


# ------------------------------------------------------------------------------------------------
# gates: check_outs(got, ref) on numpy tuples; check_grads(got, ref, ctx) on dicts of leaf-layout numpy arrays (None: no gradient).
# ctx: mode (the backward precision), values (name -> the full float32 array each view held), leaf (name -> full -> leaf layout),
#      up (output index -> the float64 gradient that reached the reference's output, None if none), scale (d composite / d L_i).
# ------------------------------------------------------------------------------------------------
def _f(x):
    return float(np.asarray(x))


def _present(got, ref, name):
    """False when neither side has a gradient for `name` (a missing gradient may stand for an exactly zero one)"""
    g, r = got.get(name), ref.get(name)
    if g is None or r is None:
        other = r if g is None else g
        assert other is None or not np.asarray(other).any(), (name, 'one side has no gradient, the other a non-zero one')
        return False
    assert g.shape == r.shape, (name, g.shape, r.shape)
    return True


def _pow2(c):
    return c == 0 or math.frexp(abs(c))[0] == 0.5


def outs_align(got, ref):
    assert_scores_close(got[0], ref[0])


def grads_fp16(got, ref, ctx, names=('im', 's')):
    for n in names:
        if _present(got, ref, n):
            assert_grads_close(got[n], ref[n], ctx['mode'])


def outs_triplet(got, ref):
    np.testing.assert_allclose(_f(got[0]), _f(ref[0]), rtol=RTOL, atol=1e-4)
    assert_scores_close(got[1], ref[1])


def outs_scan(got, ref):
    np.testing.assert_allclose(got[0], ref[0], equal_nan=True, **S2.SCAN_SCORE_TOL)
    assert S2.floor_ratio(got[0], ref[0]) <= S2.SCAN_GATE['scores']


def grads_scan(got, ref, ctx):
    live = [n for n in ('im', 's') if _present(got, ref, n)]
    scale = max([1e-3] + [float(np.abs(ref[n]).max()) for n in live])
    for n in live:
        np.testing.assert_allclose(got[n], ref[n], rtol=S2.SCAN_GRAD_RTOL, atol=S2.SCAN_GRAD_ATOL * scale)
        assert S2.floor_ratio(got[n], ref[n]) <= S2.SCAN_GATE['grads'], (n, S2.floor_ratio(got[n], ref[n]))


def outs_sum(got, ref):
    assert S2.floor_ratio(got[0], ref[0]) <= S2.NORMSUM_GATE['scores']


def grads_sum(got, ref, ctx):
    v, st = ctx['values'], ctx['st']
    ups = S2.sum_scores(v['im'], v['s'], st['im_len'], st['s_len'], ctx['up'][0], st['mean'])[3]
    for n, lens, tail, u in (('im', st['im_len'], 0, ups[0]), ('s', st['s_len'], 2, ups[1])):
        if _present(got, ref, n):
            scale = ctx['leaf'][n](S2.normsum_scales(v[n], lens, tail, u)[1][..., None])[..., 0]
            err = S2.scaled_error(got[n], ref[n], scale)
            assert err <= S2.NORMSUM_GATE['grad'], (n, err)


def _gemm_bound(k, x, y):
    return k * H.U32 * (np.abs(x) @ np.abs(y))


def outs_dot(got, ref, ctx=None):
    pass                                                          # held with the inputs at hand in grads_dot (the bound needs them)


def grads_dot(got, ref, ctx):
    """the derived bounds of test_matrix_losses_gpu.py.  The backward products are held against the gradient that actually reached
    the node (a composite such as (M.double() ** 2).sum() makes it from the float32 M), and that gradient against the reference's
    within what M's own bound makes of it (|d g / d M| <= 2 for every composite here) plus its float32 rounding."""
    a, b, dS = ctx['values']['im'].astype(np.float64), ctx['values']['s'].astype(np.float64), ctx['up'][0]
    bound_c = _gemm_bound(a.shape[1], a, b.T)
    assert (np.abs(ctx['outs'][0] - a @ b.T) <= bound_c).all()
    if ctx.get('arrived', {}).get(0) is not None:
        assert (np.abs(ctx['arrived'][0] - dS) <= 2 * bound_c + H.U32 * np.abs(dS)).all()
        dS = ctx['arrived'][0]
        ref = {'im': ctx['leaf']['im'](dS @ b) if ref.get('im') is not None else None,
               's': ctx['leaf']['s'](dS.T @ a) if ref.get('s') is not None else None}
    for n, full, bound in (('im', dS @ b, _gemm_bound(b.shape[0], dS, b)), ('s', dS.T @ a, _gemm_bound(a.shape[0], dS.T, a))):
        if _present(got, ref, n):
            rows = full.shape[0] / ctx['leaf'][n](full).shape[0]          # an expanded leaf: a float32 sum of that many rows on top
            bound = ctx['leaf'][n](bound) + (rows - 1) * H.U32 * ctx['leaf'][n](np.abs(full))
            assert (np.abs(got[n] - ref[n]) <= bound).all(), (n, float((np.abs(got[n] - ref[n]) / np.maximum(bound, 1e-300)).max()))


def outs_order(got, ref):
    np.testing.assert_allclose(got[0], ref[0], **S2.ORDER_SCORE_TOL)
    assert S2.floor_ratio(got[0], ref[0]) <= S2.ORDER_GATE[0]


def grads_order(got, ref, ctx):
    live = [n for n in ('im', 's') if _present(got, ref, n)]
    scale = max(1.0, float(np.abs(ref['im']).max())) if ref.get('im') is not None else 1.0
    for n in live:
        np.testing.assert_allclose(got[n], ref[n], rtol=S2.ORDER_GRAD_RTOL, atol=S2.ORDER_GRAD_ATOL * scale)
        assert S2.floor_ratio(got[n], ref[n]) <= S2.ORDER_GATE[1], (n, S2.floor_ratio(got[n], ref[n]))


def outs_l2norm(got, ref):
    np.testing.assert_allclose(got[0], ref[0], **H.L2NORM_FWD_TOL)


def grads_l2norm(got, ref, ctx):
    if _present(got, ref, 'x'):
        full = H.l2norm_ref(ctx['values']['x'], ctx['up'][0])[1]
        rows = full.size / ctx['leaf']['x'](full).size           # an expanded leaf: a float32 sum of that many terms on top
        slack = (rows - 1) * H.U32 * ctx['leaf']['x'](np.abs(full))
        assert (np.abs(got['x'] - ref['x']) <= H.l2norm_bwd_tol(ref['x']) + slack).all()


def outs_hinge_loss(got, ref):
    assert abs(_f(got[0]) - _f(ref[0])) <= H.HINGE_LOSS_RTOL * abs(_f(ref[0]))


def grads_exact(name):
    def check(got, ref, ctx):
        if _present(got, ref, name):                              # small integers times the upstream scale: exact in float32
            assert np.array_equal(got[name], ref[name].astype(np.float32)), (name, int((got[name] != ref[name].astype(np.float32)).sum()))
    return check


def outs_listnet(got, ref):
    np.testing.assert_allclose(_f(got[0]), _f(ref[0]), **H.LISTNET_LOSS_TOL)


def grads_cancelling(names, family='mild'):
    def check(got, ref, ctx):
        for n in names:
            if _present(got, ref, n):
                H.assert_cancelling_grad_close(got[n], ref[n], n, family)
    return check


def outs_mse(got, ref, ctx=None):
    pass                                                          # held in grads_mse, where the inputs of the derived bound are at hand


def grads_mse(got, ref, ctx):
    v, c = ctx['values'], ctx['scale'][0]
    (loss, _, _), (bl, bM, bwb) = S2.mse_ref(v['teacher'], v['student'], v['wb'])
    assert abs(ctx['outs'][0] - loss) <= bl
    extra = 0.0 if _pow2(c) else H.U32                           # one more float32 rounding: the saved gradient times the upstream scalar
    if _present(got, ref, 'student'):
        leaf = ctx['leaf']['student']
        rows = bM.size / leaf(bM).size
        bound = abs(c) * leaf(bM) + extra * np.abs(ref['student']) + (rows - 1) * H.U32 * abs(c) * leaf(np.abs(S2.mse_ref(v['teacher'], v['student'], v['wb'])[0][1]))
        assert (np.abs(got['student'] - ref['student']) <= bound).all()
    if _present(got, ref, 'wb'):
        assert (np.abs(got['wb'] - ref['wb']) <= abs(c) * bwb + extra * np.abs(ref['wb'])).all()


def outs_ordinal(got, ref):
    np.testing.assert_allclose(_f(got[0]), _f(ref[0]), equal_nan=True, **S2.ORDINAL_LOSS_TOL)


def grads_ordinal(got, ref, ctx):
    """assert_ordinal of test_secondary_heads_gpu.py under an upstream scale c: a single part (+-1 / n rounded once) is exact while
    c is a power of two and takes one more rounding otherwise; two parts: 2 ulp of the larger; an expanded leaf sums rows in float32"""
    if not _present(got, ref, 'student'):
        return
    v, st, c, leaf = ctx['values'], ctx['st'], ctx['scale'][0], ctx['leaf']['student']
    _, gr, gc, _, _, _ = S2.ordinal_parts(v['teacher'], v['student'], st['margin'], st['threshold'], st['stride'])
    one = (gr == 0) | (gc == 0)
    ulp = np.spacing(np.maximum(np.abs(gr), np.abs(gc)).astype(np.float32)).astype(np.float64) * abs(c)
    once = 0.5 * np.spacing(np.abs(c * (gr + gc)).astype(np.float32)).astype(np.float64)          # the float32 nearest the float64 value
    tol = np.where(one, once, 2 * ulp) + (0.0 if _pow2(c) else ulp)
    rows = tol.size / leaf(tol).size
    tol = leaf(tol) + (rows - 1) * H.U32 * abs(c) * leaf(np.abs(gr + gc))
    assert (np.abs(got['student'] - ref['student']) <= tol).all()


def outs_xent(got, ref):
    np.testing.assert_allclose(_f(got[0]), _f(ref[0]), **X.LOSS_TOL)
    if len(got) > 1:
        np.testing.assert_allclose(got[1], ref[1], rtol=1e-5, atol=1e-6)


def grads_xent(names, family):
    def check(got, ref, ctx):
        for n in names:
            if _present(got, ref, n):
                X.assert_grad_close(got[n], ref[n], family, n)
        if _present(got, ref, 'log_t'):
            np.testing.assert_allclose(got['log_t'], ref['log_t'], **X.LOSS_TOL)
    return check


def outs_semantic(got, ref):
    np.testing.assert_allclose(_f(got[0]), _f(ref[0]), rtol=H.HINGE_LOSS_RTOL, atol=0)


def outs_entropy(got, ref):
    np.testing.assert_allclose(_f(got[0]), _f(ref[0]), **ENTROPY_LOSS_TOL)


def grads_entropy(got, ref, ctx):
    for n in ('img', 'cap'):
        if _present(got, ref, n):
            np.testing.assert_allclose(got[n], ref[n], **ENTROPY_GRAD_TOL)


def outs_attdistill(got, ref, ctx=None):
    pass                                                          # held in grads_attdistill against the split-operand restatement


def grads_attdistill(got, ref, ctx):
    """the gates of test_attdistill_gpu.py: against the float64 restatement on the kernels' split operands"""
    v, st, c = ctx['values'], ctx['st'], ctx['scale'][0]
    loss, d_im, d_s = A.attdistill(v['im'], v['s'], st['im_len'], st['s_len'], v['teacher'], rounded='split')
    assert abs(ctx['outs'][0] - loss) <= A.GATE_LOSS_REL * abs(loss)
    for n, full in (('im', d_im), ('s', d_s)):
        if _present(got, ref, n):
            want = c * ctx['leaf'][n](full)
            top = float(np.abs(want).max())
            assert np.abs(got[n] - want).max() <= A.GATE_GRAD_MAXNORM * top, (n, float(np.abs(got[n] - want).max()) / max(top, 1e-300))


def outs_match(got, ref):
    assert abs(_f(got[0]) - _f(ref[0])) <= H.HINGE_LOSS_RTOL * abs(_f(ref[0]))
    assert np.array_equal(got[1], ref[1].astype(np.float32))     # quantised embeddings: exact products


def grads_match(got, ref, ctx):
    """d_im = C cap, d_s = C^T im with C the whole gradient on M: the derived GEMM bound of the dot_scores tests (two more roundings:
    C = g dM + g_M is formed in float32); exact (quantised embeddings, integer C) when only the loss is back-propagated"""
    a, b, C = ctx['values']['im'].astype(np.float64), ctx['values']['s'].astype(np.float64), ctx['up'][1]
    for n, full, bound in (('im', C @ b, _gemm_bound(b.shape[0] + 2, C, b)), ('s', C.T @ a, _gemm_bound(a.shape[0] + 2, C.T, a))):
        if _present(got, ref, n):
            rows = full.shape[0] / ctx['leaf'][n](full).shape[0]
            bound = ctx['leaf'][n](bound) + (rows - 1) * H.U32 * ctx['leaf'][n](np.abs(full))
            assert (np.abs(got[n] - ref[n]) <= bound).all(), n
            if ctx['loss_only']:
                assert np.array_equal(got[n], ref[n].astype(np.float32)), n


def outs_small(got, ref):
    assert abs(_f(got[0]) - _f(ref[0])) <= H.HINGE_LOSS_RTOL * abs(_f(ref[0]))
    np.testing.assert_allclose(_f(got[1]), _f(ref[1]), **H.LISTNET_LOSS_TOL)
    assert np.array_equal(got[2], ref[2].astype(np.float32))


def outs_heads(got, ref):
    np.testing.assert_allclose(_f(got[0]), _f(ref[0]), rtol=RTOL, atol=1e-4)
    np.testing.assert_allclose(got[1], ref[1], rtol=RTOL, atol=1e-4)
    if ref[2] is not None:
        assert_scores_close(got[2], ref[2])
    if ref[3] is not None:
        np.testing.assert_allclose(got[3], ref[3], rtol=1e-5, atol=1e-6)


def grads_heads(got, ref, ctx):
    """sets: the fp16 bars; embeddings: the cancelling-gradient gate, and the fp16 bars once the distillation head is there (its
    teacher is the fp16-operand score matrix)"""
    grads_fp16(got, ref, ctx, ('im', 's'))
    if 'distillation' in ctx['st']['heads']:
        grads_fp16(got, ref, dict(ctx, mode='fp16'), ('img', 'cap'))      # whatever the backward precision: the TEACHER is fp16-made
    else:
        grads_cancelling(('img', 'cap'))(got, ref, ctx)


# ------------------------------------------------------------------------------------------------
# the registry
# ------------------------------------------------------------------------------------------------
class Entry:
    """name/case of one differentiable entry point.  build(variant) -> (diff, aux, st): OrderedDicts name -> read-only numpy array of
    the tensor inputs that take / do not take a gradient and the remaining (python) arguments; variant 0: the base data, 1: other
    data of the same shapes, 2: another shape.  kinds: input name -> 'set' | 'mat' | 'scalar' | 'vec' | None (no layouts: draws).
    lens: set input -> the key of its lengths in st.  outputs: per output 'M' | 'L' | 'N' (not differentiable)."""

    def __init__(self, name, build, kinds, outputs, gpu_call, ref_call, check_outs, check_grads, lens=None, rect=False, align=False,
                 skip_layouts=(), single=None):
        self.name, self._build, self.kinds, self.outputs = name, build, kinds, outputs
        self.gpu_call, self.ref_call, self.check_outs, self.check_grads = gpu_call, ref_call, check_outs, check_grads
        self.lens, self.rect, self.align, self.skip_layouts, self.single = lens or {}, rect, align, tuple(skip_layouts), single

    @functools.lru_cache(maxsize=None)
    def build(self, variant=0):
        diff, aux, st = self._build(variant)
        return (collections.OrderedDict((k, frozen(v)) for k, v in diff.items()),
                collections.OrderedDict((k, frozen(v)) for k, v in aux.items()), st)

    def layouts(self, name):
        """the layouts of tensor input `name` that are defined for this entry"""
        kind = self.kinds.get(name)
        if kind is None:
            return []
        return [l for l in LAYOUTS[kind] if (name, l) not in self.skip_layouts and (l != 'single' or self.rect)]

    def with_layout(self, data, name, layout):
        """-> (the data the call with this layout takes, the data whose `name` holds the values the layout's view holds): they
        differ in `name` alone, and from `data` only for the layouts that change the values ('single': a batch of one)"""
        diff, aux, st = data
        pool = diff if name in diff else aux
        values = LAYOUTS[self.kinds[name]][layout](pool[name], lambda a: torch.from_numpy(np.array(a))).values
        diff, aux, st = collections.OrderedDict(diff), collections.OrderedDict(aux), dict(st)
        if layout == 'single':
            st[self.lens[name]] = st[self.lens[name]][:1]
            if self.single:
                self.single(name, aux)
        vdiff, vaux = collections.OrderedDict(diff), collections.OrderedDict(aux)
        (vdiff if name in vdiff else vaux)[name] = frozen(values)
        return (diff, aux, st), (vdiff, vaux, st)


SETS = {'base': (5, 4, 12, 9, 64), 'r35': (5, 4, 35, 9, 64), 'd30': (5, 4, 12, 9, 30), 'long': (3, 3, 101, 9, 32)}
SETS_OTHER = (5, 4, 13, 10, 64)                                  # variant 2: another shape


def _sets(shape, variant, square=False, seed=11):
    Bi, Bc, R, T, D = SETS_OTHER if variant == 2 else SETS[shape]
    if square:
        Bc = Bi
    im, s, il, sl = ragged_batch(Bi, Bc, R, T, D, seed + 100 * variant + R)
    return im, s, il, sl


def _align_entry(aggregation, shape):
    def build(variant):
        im, s, il, sl = _sets(shape, variant)
        return {'im': im, 's': s}, {}, {'im_len': il, 's_len': sl}

    def gpu(t, st):
        from aladin_amd import ops
        return (ops.alignment_scores(t['im'], t['s'], st['im_len'], st['s_len'], aggregation),)

    def ref(t, st):
        return (FT.alignment_scores_faithful(t['im'], t['s'], st['im_len'], st['s_len'], aggregation),)
    return Entry('alignment_scores[%s,%s]' % (aggregation, shape), build, {'im': 'set', 's': 'set'}, 'M', gpu, ref, outs_align,
                 grads_fp16, lens={'im': 'im_len', 's': 's_len'}, rect=True, align=True)


def _triplet_entry(mv, shape):
    def build(variant):
        im, s, il, sl = _sets(shape, variant, square=True)
        return {'im': im, 's': s}, {}, {'im_len': il, 's_len': sl}

    def gpu(t, st):
        from aladin_amd import ops
        return ops.alignment_triplet_loss(t['im'], t['s'], st['im_len'], st['s_len'], 0.2, mv)

    def ref(t, st):
        S = FT.alignment_scores_faithful(t['im'], t['s'], st['im_len'], st['s_len'])
        return FT.hinge_faithful(S, 0.2, mv), S
    return Entry('alignment_triplet_loss[mv=%d,%s]' % (mv, shape), build, {'im': 'set', 's': 'set'}, 'LM', gpu, ref, outs_triplet,
                 grads_fp16, lens={'im': 'im_len', 's': 's_len'}, align=True)


def _scan_entry():
    def build(variant):
        im, s, il, sl = _sets('base', variant)
        return {'im': im, 's': s}, {}, {'im_len': il, 's_len': sl}

    def gpu(t, st):
        from aladin_amd import ops
        return (ops.alignment_scan_scores(t['im'], t['s'], st['im_len'], st['s_len']),)
    return Entry('alignment_scan_scores', build, {'im': 'set', 's': 'set'}, 'M', gpu,
                 lambda t, st: (FT.alignment_scores_faithful(t['im'], t['s'], st['im_len'], st['s_len'], 'scan-sentences'),),
                 outs_scan, grads_scan, lens={'im': 'im_len', 's': 's_len'}, rect=True)


def _sum_entry(mean):
    def build(variant):
        im, s, il, sl = _sets('base', variant)
        return {'im': im, 's': s}, {}, {'im_len': il, 's_len': sl, 'mean': mean}

    def gpu(t, st):
        from aladin_amd import ops
        return (ops.alignment_sum_scores(t['im'], t['s'], st['im_len'], st['s_len'], mean=mean),)
    return Entry('alignment_sum_scores[mean=%d]' % mean, build, {'im': 'set', 's': 'set'}, 'M', gpu,
                 lambda t, st: (FT.alignment_scores_faithful(t['im'], t['s'], st['im_len'], st['s_len'], 'mean' if mean else 'sum'),),
                 outs_sum, grads_sum, lens={'im': 'im_len', 's': 's_len'}, rect=True)


def _emb_pair(variant, Bi=5, Bc=4, D=64):
    if variant == 2:
        Bi, Bc = Bi + 1, Bc + 1
    im, s, _ = S2.order_inputs(Bi, Bc, D + variant % 2)          # variant 1: other data (D + 1 keys another stream), cut back to D
    return im[:, :D].copy(), s[:, :D].copy()


def _dot_entry():
    def gpu(t, st):
        from aladin_amd import ops
        return (ops.dot_scores(t['im'], t['s']),)
    return Entry('dot_scores', lambda v: (dict(zip(('im', 's'), _emb_pair(v))), {}, {}), {'im': 'mat', 's': 'mat'}, 'M', gpu,
                 lambda t, st: (t['im'] @ t['s'].t(),), outs_dot, grads_dot)


def _order_entry():
    def gpu(t, st):
        from aladin_amd import ops
        return (ops.order_scores(t['im'], t['s']),)
    return Entry('order_scores', lambda v: (dict(zip(('im', 's'), _emb_pair(v))), {}, {}), {'im': 'mat', 's': 'mat'}, 'M', gpu,
                 lambda t, st: (t_order(t['im'], t['s']),), outs_order, grads_order)


def _l2norm_entry():
    def gpu(t, st):
        from aladin_amd import ops
        return (ops.l2norm_rows(t['x']),)
    return Entry('l2norm_rows', lambda v: ({'x': H.l2norm_inputs(5 + (v == 2), 64 + (v == 1))[0][:, :64].copy()}, {}, {}), {'x': 'mat'}, 'M', gpu,
                 lambda t, st: (t_l2norm(t['x']),), outs_l2norm, grads_l2norm)


def _B(variant, B=5):
    return B + 1 if variant == 2 else B


def _quant(variant, B, key):
    return S2.quantised(_B(variant, B), key, variant % 2)


def _hinge_entry(mv):
    def gpu(t, st):
        from aladin_amd import ops
        return (ops.hinge_loss(t['scores'], H.HINGE_MARGIN_Q, mv),)
    return Entry('hinge_loss[mv=%d]' % mv, lambda v: ({'scores': _quant(v, 5, 'hinge')}, {}, {}), {'scores': 'mat'}, 'L', gpu,
                 lambda t, st: (FT.hinge_faithful(t['scores'], H.HINGE_MARGIN_Q, mv),), outs_hinge_loss, grads_exact('scores'))


def _teacher_student(variant, family='mild'):
    B = _B(variant)
    t, m = H.listnet_inputs(B + 20 * (variant % 2), family)      # variant 1: the corner of a larger draw
    return t[:B, :B].copy(), m[:B, :B].copy()


def _listnet_entry():
    def gpu(t, st):
        from aladin_amd import ops
        return (ops.listnet_loss(t['teacher'], t['student']),)

    def build(v):
        t, m = _teacher_student(v)
        return {'student': m}, {'teacher': t}, {}
    return Entry('listnet_loss', build, {'student': 'mat', 'teacher': 'mat'}, 'L', gpu,
                 lambda t, st: (t_listnet(t['teacher'], t['student']),), outs_listnet, grads_cancelling(('student',)))


def _distill_entry(mode):
    st0 = {'margin': S2.MARGIN_Q, 'threshold': 0.1, 'stride': 3}

    def build(v):
        B = _B(v)
        teacher = S2.teacher(B + 20 * (v % 2), 'normal')[:B, :B].copy()
        student = S2.student_normal(B + 20 * (v % 2))[:B, :B].copy() if mode == 'mse' else _quant(v, 5, 'student')
        diff = {'student': student}
        if mode == 'mse':
            diff['wb'] = np.asarray(S2.WB, np.float32)
        return diff, {'teacher': teacher}, dict(st0)

    def gpu(t, st):
        from aladin_amd import ops
        return (ops.distillation_loss(t['teacher'], t['student'], mode, st['margin'], st['threshold'], st['stride'], wb=t.get('wb')),)

    def ref(t, st):
        if mode == 'mse':
            return (t_mse(t['teacher'], t['student'], t['wb']),)
        if mode == 'contrastive':
            return (t_contrastive(t['teacher'], t['student'], st['margin']),)
        return (t_ordinal(t['teacher'], t['student'], st['margin'], st['threshold'], st['stride']),)
    kinds = {'student': 'mat', 'teacher': 'mat', 'wb': 'vec'}
    checks = {'mse': (outs_mse, grads_mse), 'contrastive': (outs_hinge_loss, grads_exact('student')), 'ordinal': (outs_ordinal, grads_ordinal)}
    return Entry('distillation_loss[%s]' % mode, build, kinds, 'L', gpu, ref, *checks[mode])


def _xent_entry():
    def build(v):
        B = _B(v)
        S, t = X.matrix_inputs(B + 20 * (v % 2), 'mild')           # variant 1: another corner of a larger draw
        o = 20 * (v % 2)
        return {'scores': S[o:o + B, o:o + B].copy(), 'log_t': np.asarray([t], np.float32)}, {}, {}

    def gpu(t, st):
        from aladin_amd import ops
        return (ops.cross_entropy_scores(t['scores'], t['log_t']),)
    return Entry('cross_entropy_scores', build, {'scores': 'mat', 'log_t': 'scalar'}, 'L', gpu,
                 lambda t, st: (t_xent(t['scores'], t['log_t']),), outs_xent, grads_xent(('scores',), 'mild'))


def _match_xent_entry():
    def build(v):
        B = _B(v)
        im, s = X.case_inputs('independent', B, 64, 51 + v, 61 + v)
        return {'im': im, 's': s, 'log_t': np.asarray([1.5], np.float32)}, {}, {}

    def gpu(t, st):
        from aladin_amd import ops
        return ops.match_cross_entropy(t['im'], t['s'], t['log_t'], return_scores=True)

    def ref(t, st):
        M = t['im'] @ t['s'].t()
        return t_xent(M, t['log_t']), M
    return Entry('match_cross_entropy', build, {'im': 'mat', 's': 'mat', 'log_t': 'scalar'}, 'LM', gpu, ref, outs_xent,
                 grads_xent(('im', 's'), 'independent'))


SEM_MARGIN, SEM_THRESHOLD = SM.MARGIN, SM.THRESHOLD


def _semantic_entry():
    def build(v):
        B = _B(v)
        good = [sd for sd in range(64) if SM.condition_figures(*SM.matrix_inputs(B, 'dense', sd)[:2], SEM_MARGIN, SEM_THRESHOLD,
                                                               SM.matrix_inputs(B, 'dense', sd)[2], False)[2]]
        S, rel, draws = SM.matrix_inputs(B, 'dense', good[v % 2])             # seeds that meet semantic_numpy's input condition
        return {'scores': S}, {'rel': rel, 'draws': draws}, {}

    def gpu(t, st):
        from aladin_amd import ops
        return (ops.semantic_hinge_loss(t['scores'], t['rel'], SEM_MARGIN, SEM_THRESHOLD, False, draws=t['draws']),)
    return Entry('semantic_hinge_loss', build, {'scores': 'mat', 'rel': 'mat'}, 'L', gpu,
                 lambda t, st: (t_semantic(t['scores'], t['rel'], t['draws'].numpy(), SEM_MARGIN, SEM_THRESHOLD),), outs_semantic,
                 grads_exact('scores'))


def _entropy_entry():
    def build(v):
        img, cap = E.case_inputs('a', _B(v), 64, 71 + v)
        return {'img': img, 'cap': cap}, {}, {}

    def gpu(t, st):
        from aladin_amd import ops
        return (ops.nn_entropy_loss(t['img'], t['cap']),)
    skip = [(n, l) for n in ('img', 'cap') for l in ('row', 'col')]
    return Entry('nn_entropy_loss', build, {'img': 'mat', 'cap': 'mat'}, 'L', gpu, lambda t, st: (t_entropy(t['img'], t['cap']),),
                 outs_entropy, grads_entropy, skip_layouts=skip)


def _attdistill_entry():
    def build(v):
        Bi, Bc, R, T, D = SETS_OTHER if v == 2 else SETS['base']
        x = A.make_inputs(Bi, Bc, R, T, D, seed=41 + v)
        return {'im': x['im'], 's': x['s']}, {'teacher': x['teacher']}, {'im_len': x['im_len'], 's_len': x['s_len']}

    def gpu(t, st):
        from aladin_amd import ops
        return (ops.attention_distillation_loss(t['im'], t['s'], st['im_len'], st['s_len'], t['teacher']),)

    def single(name, aux):
        aux['teacher'] = frozen(aux['teacher'][:1] if name == 'im' else aux['teacher'][:, :1])
    return Entry('attention_distillation_loss', build, {'im': 'set', 's': 'set'}, 'L', gpu,
                 lambda t, st: (t_attdistill(t['im'], t['s'], st['im_len'], st['s_len'], t['teacher']),), outs_attdistill,
                 grads_attdistill, lens={'im': 'im_len', 's': 's_len'}, rect=True, single=single)


def _small_inputs(variant, B, D):
    B = _B(variant, B)
    img, cap, teacher = H.small_batch_inputs(B, D + 4 * (variant % 2))
    return img[:, :D].copy(), cap[:, :D].copy(), teacher


def _match_hinge_entry(B, D, mv=True):
    def build(v):
        img, cap, _ = _small_inputs(v, B, D)
        return {'im': img, 's': cap}, {}, {}

    def gpu(t, st):
        from aladin_amd import ops
        return ops.match_hinge(t['im'], t['s'], H.HINGE_MARGIN_Q, mv)

    def ref(t, st):
        M = t['im'] @ t['s'].t()
        return FT.hinge_faithful(M, H.HINGE_MARGIN_Q, mv), M
    return Entry('match_hinge[B=%d]' % B, build, {'im': 'mat', 's': 'mat'}, 'LM', gpu, ref, outs_match, grads_match)


def _small_distill_entry():
    def build(v):
        img, cap, teacher = _small_inputs(v, 5, 64)
        return {'im': img, 's': cap}, {'teacher': teacher}, {}

    def gpu(t, st):
        from aladin_amd import ops
        return ops.small_batch_match_distill(t['im'], t['s'], t['teacher'], H.HINGE_MARGIN_Q, True)

    def ref(t, st):
        M = t['im'] @ t['s'].t()
        return FT.hinge_faithful(M, H.HINGE_MARGIN_Q, True), t_listnet(t['teacher'], M), M
    return Entry('small_batch_match_distill', build, {'im': 'mat', 's': 'mat', 'teacher': 'mat'}, 'LLM', gpu, ref, outs_small,
                 grads_cancelling(('im', 's')))


HEAD_SETS = (('matching', 'alignment', 'distillation'), ('alignment', 'distillation'), ('alignment',), ('matching',), ('distillation',),
             ('matching', 'distillation'))
HEAD_WEIGHTS = {'matching': 0.1, 'alignment': 1.0, 'distillation': 0.75}


def _heads_entry(B, D, heads):
    def build(v):
        from aladin_amd import synth
        b = _B(v, B)
        im, s, il, sl = ragged_batch(b, b, 12, 9, D, 23 + v)
        img, cap = synth.global_embeddings(b, D, seed=322 + v, noise=1.0)
        return {'img': img, 'cap': cap, 'im': im, 's': s}, {}, {'im_len': il, 's_len': sl, 'heads': heads, 'weights': HEAD_WEIGHTS,
                                                                  'margin': 0.2}

    def gpu(t, st):
        from aladin_amd import ops
        total, terms, S, M = ops.loss_heads(t['img'], t['cap'], t['im'], t['s'], st['im_len'], st['s_len'], st['margin'], True, heads,
                                            HEAD_WEIGHTS)
        live = torch.tensor([k in heads for k in ('matching', 'alignment', 'distillation')], device=terms.device)
        return total, torch.where(live, terms, torch.zeros_like(terms)), S, M       # the slots of absent heads are unspecified
    return Entry('loss_heads[B=%d,%s]' % (B, '+'.join(h[0] for h in heads)), build, {'img': 'mat', 'cap': 'mat', 'im': 'set', 's': 'set'},
                 'LNNN', gpu, lambda t, st: t_heads(t['img'], t['cap'], t['im'], t['s'], st), outs_heads, grads_heads,
                 lens={'im': 'im_len', 's': 's_len'}, align=True)


def _registry():
    out = []
    for shape in SETS:
        out += [_align_entry(a, shape) for a in ('MrSw', 'MwSr', 'symm')]
        out += [_triplet_entry(mv, shape) for mv in (True, False)]
    out += [_scan_entry(), _sum_entry(False), _sum_entry(True), _dot_entry(), _order_entry(), _l2norm_entry(), _hinge_entry(True),
            _hinge_entry(False), _listnet_entry()]
    out += [_distill_entry(m) for m in ('mse', 'contrastive', 'ordinal')]
    out += [_xent_entry(), _match_xent_entry(), _semantic_entry(), _entropy_entry(), _attdistill_entry(), _match_hinge_entry(5, 64),
            _match_hinge_entry(65, 32), _small_distill_entry()]
    out += [_heads_entry(B, D, h) for B, D in ((5, 64), (65, 32)) for h in HEAD_SETS]
    return collections.OrderedDict((e.name, e) for e in out)


REGISTRY = _registry()
BASE = [n for n in REGISTRY if not any(tag in n for tag in (',r35]', ',d30]', ',long]'))]       # the base shapes (the CPU tier's closed forms)
EXTRA = [n for n in REGISTRY if n not in BASE]


# ------------------------------------------------------------------------------------------------
# running an entry: the same code drives the device run and the float64 reference
# ------------------------------------------------------------------------------------------------
def to_device(device, dtype):
    def to(a):
        t = torch.from_numpy(np.array(a, order='C'))               # a copy (np.ascontiguousarray would make a 0-dim array 1-dim)
        return t.to(device=device, dtype=dtype if t.is_floating_point() else t.dtype)
    return to


class Prepared:
    """leaves and views of one call: layouts = {input: layout name} (default 'contig'), requires = the inputs that take a gradient
    (default: every differentiable one)"""

    def __init__(self, entry, data, to, layouts=None, requires=None):
        diff, aux, st = data
        self.entry, self.st, self.names = entry, st, list(diff)
        self.lay, self.t = {}, {}
        requires = self.names if requires is None else requires
        for pool in (diff, aux):
            for n, x in pool.items():
                kind = entry.kinds.get(n)
                if kind is None:
                    self.t[n] = to(x)
                    continue
                need = n in diff and n in requires
                self.lay[n] = LAYOUTS[kind][(layouts or {}).get(n, 'contig')](x, lambda a: to(a).requires_grad_(need))
                self.t[n] = self.lay[n].view

    def grads(self):
        """name -> back(leaf.grad) as numpy (None without a gradient); the leaf's gradient must have the leaf's shape"""
        out = {}
        for n in self.names:
            leaf = self.lay[n].leaf
            if leaf.grad is None:
                out[n] = None
                continue
            assert leaf.grad.shape == leaf.shape, (n, leaf.grad.shape, leaf.shape)
            out[n] = self.lay[n].back(leaf.grad.detach().cpu().numpy().copy())
        return out

    def clear(self):
        for n in self.names:
            self.lay[n].leaf.grad = None


def np_outs(outs):
    return tuple(None if o is None else o.detach().cpu().numpy() for o in outs)


def reference(entry, data, composite, layouts=None, requires=None):
    """float64 on the CPU -> (outs, grads, up, scale): up[i] the gradient that reached output i (None: none), scale[i] = d composite
    / d output i for the scalar outputs"""
    p = Prepared(entry, data, to_device('cpu', torch.float64), layouts, requires)
    outs = entry.ref_call(p.t, p.st)
    kept = {}
    for i, k in enumerate(entry.outputs):
        if k in 'ML' and outs[i] is not None and outs[i].requires_grad:
            outs[i].retain_grad()
            kept[i] = outs[i]
    loss = composite(outs)
    if loss.requires_grad:
        loss.backward()
    up = {i: (o.grad.numpy() if o.grad is not None else None) for i, o in kept.items()}
    scale = {i: (float(up[i]) if up.get(i) is not None else 0.0) for i, k in enumerate(entry.outputs) if k == 'L'}
    return np_outs(outs), p.grads(), up, scale


def context(entry, values_data, layouts, mode, ref, outs, loss_only=False):
    """values_data: the (diff, aux, st) holding the values the views held (entry.with_layout for the layouts that change them)"""
    diff, aux, st = values_data
    values = dict(diff, **aux)
    leaf = {n: functools.partial(to_leaf, entry.kinds.get(n), (layouts or {}).get(n, 'contig')) for n in values}
    return {'mode': mode, 'values': values, 'leaf': leaf, 'st': st, 'up': ref[2], 'scale': ref[3], 'outs': outs, 'loss_only': loss_only}
