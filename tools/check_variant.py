#!/usr/bin/env python3
"""Scores and gradients of seeded problems from the library ALADIN_LIB selects, saved for a bit-for-bit comparison between two
builds (an old library built from another checkout against the new one):

    ALADIN_LIB=/path/to/old/libaladin_hip.so python tools/check_variant.py save old.pt
    python tools/check_variant.py save new.pt
    python tools/check_variant.py cmp old.pt new.pt

`save FILE retrieval` saves the retrieval group instead (`save FILE all`: every group): the stored similarity matrix with its ranks and
top-k lists, the fused retrieval (screened and exact=True; its four outputs, not its scheduling-dependent statistics) on clean
data and on the 'bulk' / 'exact_ties' recipes of tests/test_gpu_parity.py, and the top-k gallery search with its scores.
`save FILE eval` saves the no-grad evaluation grids: a ragged 90 x 450 grid scored in length classes, and in length classes with
the sum side chunked, from tensors ('MrSw', 'MwSr', 'symm') and from packed stores, and a 1000 x 5000 grid at the default
thresholds, all in fp16 and split precision.  Only host code decides these, so the file may be copied into a checkout of
another commit and run there: the planner's knobs are taken from whichever module has them.

Scores: the bench batch (B = 256, full lengths) and a ragged batch; one small ragged problem per body and epilogue variant of the
score kernels (SCORE_CASES: the geometry and the grid rule that select the body are asserted), in fp16 and split precision.
Arg-max table: the sum-of-violations step with the dense table forced, one problem per variant of the arg-max kernels
(ARGMAX_CASES).  Gradients (exact backward precision unless the name says
otherwise), one case per stage of the alignment backward: the fused triplet step in the three precision modes; the
sum-of-violations step with the GEMM and with the gather row step; a sparse gradient on the score matrix (fp16 pair kernel at
R = 65, fp32 fallback at R = 71); a long problem; the small-batch loss heads.
`save FILE pack` saves the packed operands themselves (PACK_CASES, the shapes of tests/test_pack_gpu.py, ragged with lengths 0, 1
and past the maximum; fp16, and split where the table says): xm, xe and y as raw 16-bit patterns and rnorm as 32-bit patterns,
packed jointly, as images alone + captions alone and -- where the fused triplet forward covers the shape -- through its prologue;
the rows of evaluation stores of the same sets and the operands built from them under a shuffled ids.
Long sets (LONG_CASES): scores past the tile classes on either side and at the 512-position limit in fp16 and split precision,
'MwSr' (the roles swapped), the long kernels forced onto a tile-class shape (ops.LONG_PATH_FORCE: scores and gradients), and
the hinge step of AlignmentContrastiveLoss with the hardest negative and the sum of violations in two backward precisions.
`save FILE losses` saves the loss heads on the score matrices at the smallest sizes where a kernel's structure changes: the hinge in
both modes at B = 1, 63, 64, 65, 257 (loss, dS, the pair count and the sorted pair list of the fused call) and the loss bits of a
B = 65 matrix with a NaN off the diagonal (dS is unspecified there); ListNet at B = 1, 63, 257; the small-batch heads
(ops.small_batch_match_distill) in both modes at (B, D) = (1, 8), (33, 30), (64, 768); the contrastive distillation mode at B = 2,
257; the weighted total and the gradient combine through the B > 64 loss heads at B = 65.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


# (Bi, Bc, R, T, D) -> (mrows, rem, tp16, trows), body, small-grid variant: what csrc/align_fwd.hip's select_scores picks
SCORE_CASES = (
    ((6, 5, 34, 50, 64), (32, 1, 3, 48), 'WIDE', True),           # Q = 1, one side row
    ((5, 9, 60, 50, 64), (64, 0, 3, 48), 'WIDE', True),           # Q = 2
    ((4, 5, 66, 40, 64), (64, 1, 3, 40), 'TALL', True),           # Q = 2 + side row
    ((5, 9, 34, 67, 64), (32, 1, 4, 64), 'WIDE', True),           # tp16 = 4
    ((9, 21, 36, 27, 64), (32, 3, 2, 24), 'WIDE', True),          # half class, 3 side rows
    ((6, 50, 34, 11, 64), (32, 1, 1, 8), 'WIDE', True),           # 8-word class
    ((6, 18, 34, 43, 64), (32, 1, 3, 40), 'TALL', True),          # two-wave 128 x 160
    ((6, 6, 51, 38, 768), (48, 2, 3, 40), 'R48', True),           # 2 side rows, 40 words
    ((5, 4, 57, 90, 64), (48, 8, 6, 96), 'R48', True),            # 8 side rows
    ((9, 5, 49, 9, 64), (48, 0, 1, 8), 'R48', True),              # no side rows
    ((3, 4, 71, 71, 64), (96, 0, 6, 96), '32X32', None),
    # more than 64 workgroup tiles
    ((72, 96, 34, 50, 64), (32, 1, 3, 48), 'TALL', False),        # Q = 1
    ((36, 64, 60, 50, 64), (64, 0, 3, 48), 'TALL', False),        # Q = 2, whole tiles
    ((40, 72, 66, 50, 64), (64, 1, 3, 48), 'TALL', False),        # Q = 2 + side row
    ((72, 96, 34, 67, 64), (32, 1, 4, 64), 'WIDE', False),        # 4 x 2 waves
    ((72, 96, 51, 50, 64), (48, 2, 3, 48), 'R48', False),         # 2 x 4 waves
    ((254, 270, 51, 38, 256), (48, 2, 3, 40), 'R48X3', False),    # with the overhanging tile
    ((256, 256, 50, 36, 256), (48, 1, 3, 40), 'R48', False),      # 192 x 320
)
# (R, T) at B = 64, D = 256 -> (mrows, rem) of the arg-max kernel's class
ARGMAX_CASES = (((34, 50), (32, 1)), ((38, 30), (32, 5)), ((51, 38), (48, 2)), ((50, 38), (48, 1)), ((49, 38), (48, 0)), ((58, 38), (64, 0)))


# (R, T, D) at Bi = 3, Bc = 2 -> (mrows, rem, trows), also in split precision?
PACK_CASES = (
    ((34, 50, 64), (32, 1, 48), True), ((51, 38, 768), (48, 2, 40), True), ((20, 11, 64), (32, 0, 8), False),
    ((42, 27, 128), (48, 0, 24), False), ((41, 50, 64), (32, 8, 48), False), ((66, 50, 64), (64, 1, 48), False),
    ((71, 71, 64), (96, 0, 96), False), ((34, 50, 66), (32, 1, 48), False), ((34, 50, 1088), (32, 1, 48), True),
    ((100, 20, 64), (128, 0, 32), False), ((34, 100, 64), (64, 0, 112), False),
)


LONG_CASES = ((5, 6, 98, 50, 64), (6, 5, 34, 100, 64), (3, 3, 512, 512, 32))


def score_body(g):
    """(body, small-grid variant) of a geometry: select_scores of csrc/align_fwd.hip."""
    words40 = g.trows == 40
    M, N = g.xm_rows, g.y_rows
    if g.mrows == 96:
        return '32X32', None
    if g.mrows == 48:
        small = (M // 192) * (N // (320 if words40 else 384)) <= 64
        if words40 and not small:
            n_n = N // 320
            r192, r288 = -(-(M // 192) * n_n // 256), -(-(-(-M // 288)) * n_n // 256)
            if 1.37 * r288 < 0.97 * r192:
                return 'R48X3', False
        return 'R48', small
    if words40:
        return 'TALL', (M // 256) * (N // 320) <= 64
    small = (M // 256) * (N // 384) <= 64
    return ('WIDE' if small or 6 % g.tp16 else 'TALL'), small


def score_cases(ops, synth, dev):
    """-> {name: scores} of SCORE_CASES, ragged, in both precisions."""
    out = {}
    for (Bi, Bc, R, Tn, D), cls, body, small in SCORE_CASES:
        im, s, il, sl = synth.alignment_batch(Bi, R, Tn, D, seed=8000 + 100 * R + Tn, ragged=True, Bc=Bc)
        il[0], sl[0] = R, Tn
        a, b = torch.from_numpy(im).to(dev), torch.from_numpy(s).to(dev)
        for prec in ('fp16', 'split'):
            g = ops.align_geometry(Bi, Bc, R, Tn, D, precision=prec)
            assert (g.mrows, g.rem, g.tp16, g.trows) == cls and score_body(g) == (body, small), ((Bi, Bc, R, Tn, D), prec, score_body(g))
            with torch.no_grad():
                out['scores-%dx%d-R%d-T%d-D%d-%s' % (Bi, Bc, R, Tn, D, prec)] = ops.alignment_scores(a, b, il, sl, precision=prec).cpu()
    return out


def argmax_cases(ops, synth, dev):
    """-> {name: tensor}: loss and gradients of the sum-of-violations step through the dense arg-max table."""
    from aladin_amd.loss import AlignmentContrastiveLoss
    out = {}
    crit = AlignmentContrastiveLoss(margin=0.2, measure='dot', max_violation=False, aggregation='MrSw')
    saved = ops.DENSE_BACKWARD, ops.DENSE_ROWS_GEMM, ops.DENSE_MIN_FRACTION, ops.DENSE_GEMM_FORCE, ops.DENSE_MIN_PAIRS
    try:
        # B = 64 is below the batch size from which the dense table pays: forced all the same
        ops.DENSE_BACKWARD, ops.DENSE_ROWS_GEMM, ops.DENSE_MIN_FRACTION, ops.DENSE_GEMM_FORCE, ops.DENSE_MIN_PAIRS = True, True, 0.0, True, 0
        for (R, Tn), cls in ARGMAX_CASES:
            g = ops.align_geometry(64, 64, R, Tn, 256, precision='split')
            assert (g.mrows, g.rem) == cls and 6 % g.tp16 == 0, ((R, Tn), g.mrows, g.rem, g.tp16)
            im, s, il, sl = synth.alignment_batch(64, R, Tn, 256, seed=8500 + R, ragged=True)
            a = torch.from_numpy(im).to(dev).requires_grad_(True)
            b = torch.from_numpy(s).to(dev).requires_grad_(True)
            loss = crit(a, b, il, sl)
            loss.backward()
            assert ops._LAST_BWD_FLAGS[0] & 2, 'the dense path was not taken'
            tag = 'argmax64-R%d-T%d' % (R, Tn)
            out[tag + '/loss'], out[tag + '/d_im'], out[tag + '/d_s'] = loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()
    finally:
        ops.DENSE_BACKWARD, ops.DENSE_ROWS_GEMM, ops.DENSE_MIN_FRACTION, ops.DENSE_GEMM_FORCE, ops.DENSE_MIN_PAIRS = saved
    return out


def gradient_cases(ops, synth, dev):
    """-> {name: tensor} of losses and input gradients."""
    from aladin_amd.loss import AlignmentContrastiveLoss
    out = {}
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    leaves = lambda im, s: (T(im).requires_grad_(True), T(s).requires_grad_(True))

    def keep(tag, loss, a, b):
        out[tag + '/loss'], out[tag + '/d_im'], out[tag + '/d_s'] = loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()

    # 1. the fused triplet step (hinge table in the forward, row step in the backward), ragged
    im, s, il, sl = synth.alignment_batch(256, 34, 50, 768, seed=99, ragged=True)
    for mode in ('exact', 'fp16', 'fp16-own'):
        ops.set_backward_precision(mode)
        a, b = leaves(im, s)
        loss, _ = ops.alignment_triplet_loss(a, b, il, sl, 0.2, True)
        loss.backward()
        keep('triplet256-' + mode, loss, a, b)
    ops.set_backward_precision('exact')

    # 2. / 3. sum of violations: dense table, then the GEMM / the gather row step
    im, s, il, sl = synth.alignment_batch(128, 34, 50, 768, seed=133, ragged=True)
    crit = AlignmentContrastiveLoss(margin=0.2, measure='dot', max_violation=False, aggregation='MrSw')
    saved = ops.DENSE_BACKWARD, ops.DENSE_ROWS_GEMM, ops.DENSE_MIN_FRACTION, ops.DENSE_GEMM_FORCE
    try:
        for gemm in (True, False):
            ops.DENSE_BACKWARD, ops.DENSE_ROWS_GEMM, ops.DENSE_MIN_FRACTION, ops.DENSE_GEMM_FORCE = True, gemm, 0.0, True
            a, b = leaves(im, s)
            loss = crit(a, b, il, sl)
            loss.backward()
            assert ops._LAST_BWD_FLAGS[0] & 2, 'the dense path was not taken'
            keep('sum128-' + ('gemm' if gemm else 'gather'), loss, a, b)
    finally:
        ops.DENSE_BACKWARD, ops.DENSE_ROWS_GEMM, ops.DENSE_MIN_FRACTION, ops.DENSE_GEMM_FORCE = saved

    # 4. a sparse gradient on the score matrix: list from dS, then the table from the list
    for R in (65, 71):
        im, s, il, sl = synth.alignment_batch(7, R, 20, 256, seed=700 + R, ragged=True)
        a, b = leaves(im, s)
        S = ops.alignment_scores(a, b, il, sl)
        w = np.zeros((7, 7), np.float32)
        w[np.arange(7), np.arange(7)] = -1.0
        w[np.arange(7), (np.arange(7) + 3) % 7] = 0.5
        w[2, 5] = 0.25
        loss = (S * T(w)).sum()
        loss.backward()
        keep('sparse7-R%d' % R, loss, a, b)

    # 5. long sets
    im, s, il, sl = synth.alignment_batch(4, 101, 50, 64, seed=401, ragged=True)
    w = T(np.random.RandomState(5).randn(4, 4).astype(np.float32))
    for mode in ('exact', 'fp16-own'):
        ops.set_backward_precision(mode)
        a, b = leaves(im, s)
        loss = (ops.alignment_scores(a, b, il, sl) * w).sum()
        loss.backward()
        keep('long4-' + mode, loss, a, b)
    ops.set_backward_precision('exact')

    # 6. the small-batch loss heads (statistics -> hinge table -> rows)
    im, s, il, sl = synth.structured_alignment_batch(32, 34, 50, 768, seed=321, noise=3.0, ragged=True)
    ge, gc = synth.global_embeddings(32, 768, seed=322, noise=1.0)
    a, b = leaves(im, s)
    e, c = T(ge).requires_grad_(True), T(gc).requires_grad_(True)
    total, _, _, _ = ops.small_batch_loss_heads(e, c, a, b, il, sl, 0.2, True, ('matching', 'alignment', 'distillation'),
                                                {'matching': 0.1, 'alignment': 1.0, 'distillation': 0.75})
    total.backward()
    keep('heads32', total, a, b)
    out['heads32/d_img'], out['heads32/d_cap'] = e.grad.cpu(), c.grad.cpu()
    return out


def long_cases(ops, synth, dev):
    """-> {name: tensor}: scores, losses and gradients of long-set problems (and of a tile-class shape sent to the long kernels)."""
    from aladin_amd.loss import AlignmentContrastiveLoss
    out = {}
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def scores(tag, shape, aggregations):
        Bi, Bc, R, Tn, D = shape
        im, s, il, sl = synth.alignment_batch(Bi, R, Tn, D, seed=9000 + R + Tn, ragged=True, Bc=Bc)
        il[0], sl[0] = R, Tn
        for agg in aggregations:
            for prec in ('fp16', 'split'):
                with torch.no_grad():
                    out['%s-%dx%d-R%d-T%d-D%d-%s-%s' % (tag, Bi, Bc, R, Tn, D, agg, prec)] = \
                        ops.alignment_scores(T(im), T(s), il, sl, agg, precision=prec).cpu()
        return im, s, il, sl

    for k, shape in enumerate(LONG_CASES):
        scores('long', shape, ('MrSw', 'MwSr') if k == 0 else ('MrSw',))
    old = ops.LONG_PATH_FORCE
    ops.LONG_PATH_FORCE = True
    try:
        im, s, il, sl = scores('forced-long', (8, 8, 34, 50, 64), ('MrSw',))
        a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
        loss = (ops.alignment_scores(a, b, il, sl) * T(np.random.RandomState(6).randn(8, 8).astype(np.float32))).sum()
        loss.backward()
        out['forced-long8/loss'], out['forced-long8/d_im'], out['forced-long8/d_s'] = loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()
    finally:
        ops.LONG_PATH_FORCE = old
    im, s, il, sl = synth.alignment_batch(5, 98, 50, 64, seed=9500, ragged=True)
    try:
        for mode in ('exact', 'fp16'):
            ops.set_backward_precision(mode)
            for max_violation in (True, False):
                crit = AlignmentContrastiveLoss(margin=0.2, measure='dot', max_violation=max_violation, aggregation='MrSw')
                a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
                loss = crit(a, b, il, sl)
                loss.backward()
                tag = 'long-hinge5-%s-%s' % ('max' if max_violation else 'sum', mode)
                out[tag + '/loss'], out[tag + '/d_im'], out[tag + '/d_s'] = loss.detach().cpu(), a.grad.cpu(), b.grad.cpu()
    finally:
        ops.set_backward_precision('exact')
    return out


def pack_cases(ops, synth, dev):
    """-> {name: bit patterns} of the packed operands of PACK_CASES, every way the library packs them."""
    from aladin_amd import _lib, eval_grid
    from aladin_amd.store import PackedSetStore
    out = {}
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def keep(tag, g, xm, xe, y, rnorm):
        out[tag + '/xm'], out[tag + '/y'] = xm[:g.xm_bytes // 2].view(torch.int16).cpu(), y[:g.y_bytes // 2].view(torch.int16).cpu()
        if g.xe_bytes:
            out[tag + '/xe'] = xe[:g.xe_bytes // 2].view(torch.int16).cpu()
        if rnorm is not None:
            out[tag + '/rnorm'] = rnorm[:g.rnorm_bytes // 4].view(torch.int32).cpu()

    for (R, Tn, D), cls, split in PACK_CASES:
        im, s, il, sl = synth.alignment_batch(3, R, Tn, D, seed=8800 + R + Tn + D, ragged=True, Bc=2)
        il, sl = [R - 5, 0, R + 3], [Tn - 4, 1]
        a, b = T(im), T(s)
        ilt, slt = ops.lengths_tensor(il, dev), ops.lengths_tensor(sl, dev)
        for prec in ('fp16', 'split') if split else ('fp16',):
            g = ops.align_geometry(3, 2, R, Tn, D, precision=prec, layout='auto')
            assert (g.mrows, g.rem, g.trows) == cls, ((R, Tn, D), g.mrows, g.rem, g.trows)
            tag = 'pack-R%d-T%d-D%d-%s' % (R, Tn, D, prec)
            pk = ops.pack_sets(a, b, ilt, slt, g)
            keep(tag + '/joint', g, pk.xm, pk.xe, pk.y, pk.rnorm)
            rn = torch.zeros(g.rnorm_bytes // 4, device=dev)
            xm, xe = ops.pack_images(a, ilt, g, rnorm=rn)
            keep(tag + '/single', g, xm, xe, ops.pack_captions(b, slt, g, rnorm=rn), rn)
            if g.layout == _lib.LAYOUT_LONG:
                continue
            si, sc = PackedSetStore(D, 0, dev, precision=prec), PackedSetStore(D, 2, dev, precision=prec)
            for k in (2, 0, 1):
                si.append(a[k:k + 1], il[k:k + 1])
            for k in (1, 0):
                sc.append(b[k:k + 1], sl[k:k + 1])
            out[tag + '/store/x'], out[tag + '/store/y'] = si.rows[:si.n_rows].view(torch.int16).cpu(), sc.rows[:sc.n_rows].view(torch.int16).cpu()
            xm, xe = eval_grid.StoreSide(si.view([1, 2, 0])).pack_max(g)
            keep(tag + '/store-ids', g, xm, xe, eval_grid.StoreSide(sc.view([1, 0])).pack_sum(g, 0, 2), None)
        # the triplet forward's prologue on the square problem of the same shape, where the fused call covers it
        im, s, il3, sl3 = synth.alignment_batch(3, R, Tn, D, seed=8900 + R + Tn + D, ragged=True)
        fused = ops._triplet_forward(T(im), T(s), ops.lengths_tensor(il3, dev), ops.lengths_tensor(sl3, dev), 0.2)
        if fused is not None:
            saved = fused[2]
            pk = ops.Packed.from_buf(saved.tensors()[4], saved.geom, saved.offs)
            keep('pack-R%d-T%d-D%d-fp16/prologue' % (R, Tn, D), saved.geom, pk.xm, pk.xe, pk.y, pk.rnorm)
    return out


def losses_cases(ops, synth, dev):
    """-> {name: tensor}: the loss heads on B x B score matrices, general path and B <= 64 path."""
    from aladin_amd import ops_losses
    out = {}
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for mv in (True, False):
        mode = 'max' if mv else 'sum'
        for B in (1, 63, 64, 65, 257):
            loss, dS, (pairs, count) = ops_losses._hinge_raw(T(synth.normal((B, B), 7000 + B)), 0.2, mv, True, want_pairs=True)
            tag = 'hinge-%s-B%d' % (mode, B)
            out[tag + '/loss'], out[tag + '/dS'], out[tag + '/pair_count'] = loss.cpu(), dS.cpu(), count.cpu()
            out[tag + '/pairs'] = pairs[:int(count)].sort().values.cpu()
        S = synth.normal((65, 65), 7100)
        S[3, 40] = np.nan
        out['hinge-%s-B65-nan/loss_bits' % mode] = ops_losses._hinge_raw(T(S), 0.2, mv, False)[0].view(torch.int32).cpu()
        for B, D in ((1, 8), (33, 30), (64, 768)):
            ge, gc = synth.global_embeddings(B, D, seed=7300 + B, noise=1.0)
            e, c = T(ge).requires_grad_(True), T(gc).requires_grad_(True)
            h, l, M = ops.small_batch_match_distill(e, c, T(synth.normal((B, B), 7400 + B)), 0.2, mv)
            (h + l).backward()
            tag = 'small-%s-B%d-D%d' % (mode, B, D)
            out[tag + '/hinge'], out[tag + '/listnet'], out[tag + '/M'] = h.detach().cpu(), l.detach().cpu(), M.detach().cpu()
            out[tag + '/d_img'], out[tag + '/d_cap'] = e.grad.cpu(), c.grad.cpu()
    for B in (1, 63, 257):
        m = T(synth.normal((B, B), 7200 + B)).requires_grad_(True)
        loss = ops.listnet_loss(T(synth.normal((B, B), 7250 + B)), m)
        loss.backward()
        out['listnet-B%d/loss' % B], out['listnet-B%d/dM' % B] = loss.detach().cpu(), m.grad.cpu()
    for B in (2, 257):
        m = T(synth.normal((B, B), 7500 + B)).requires_grad_(True)
        loss = ops.distillation_loss(T(synth.normal((B, B), 7550 + B)), m, 'contrastive', margin=0.2)
        loss.backward()
        out['tcon-B%d/loss' % B], out['tcon-B%d/d_student' % B] = loss.detach().cpu(), m.grad.cpu()
    im, s, il, sl = synth.structured_alignment_batch(65, 34, 50, 64, seed=7600, noise=3.0, ragged=True)
    ge, gc = synth.global_embeddings(65, 64, seed=7601, noise=1.0)
    a, b, e, c = (T(x).requires_grad_(True) for x in (im, s, ge, gc))
    total, terms, _, _ = ops.loss_heads(e, c, a, b, il, sl, 0.2, True, ('matching', 'alignment', 'distillation'),
                                        {'matching': 0.1, 'alignment': 1.0, 'distillation': 0.75})
    total.backward()
    out['heads65/total'], out['heads65/terms'] = total.detach().cpu(), terms.detach().cpu()
    out['heads65/d_im'], out['heads65/d_s'], out['heads65/d_img'], out['heads65/d_cap'] = a.grad.cpu(), b.grad.cpu(), e.grad.cpu(), c.grad.cpu()
    return out


def adversarial_retrieval(case, n_img, cpi, D, seed):
    """The 'bulk' and 'exact_ties' recipes of tests/test_gpu_parity.py::_adversarial_retrieval."""
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((n_img, D)).astype(np.float32)
    img /= np.linalg.norm(img, axis=1, keepdims=True)
    if case == 'bulk':                   # ground truths inside the bulk of the scores: captions unrelated to their images
        cap = rng.standard_normal((n_img * cpi, D)).astype(np.float32)
        cap /= np.linalg.norm(cap, axis=1, keepdims=True)
    elif case == 'exact_ties':           # bit-identical caption rows under different images, duplicated images too
        cap = np.repeat(img, cpi, axis=0) + 0.8 * rng.standard_normal((n_img * cpi, D)).astype(np.float32)
        cap /= np.linalg.norm(cap, axis=1, keepdims=True)
        k = n_img * cpi
        src = rng.integers(0, k, size=k // 3)
        dst = rng.permutation(k)[:src.size]
        cap[dst] = cap[src]
        isrc = rng.integers(0, n_img, size=n_img // 4)
        idst = rng.permutation(n_img)[:isrc.size]
        img[idst] = img[isrc]
    else:
        raise ValueError(case)
    return img, cap.astype(np.float32)


def retrieval_cases(ops, synth, dev):
    """-> {name: tensor}: every output of the evaluation similarity paths, for equality between two builds."""
    out = {}
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    names = ('rank_i2t', 'top1_i2t', 'rank_t2i', 'top1_t2i')
    # the stored matrix and its ranks: the three row splits of aladin_recall_ranks (below 256 images, from 256, from 2048)
    for n_img, cpi, D in ((7, 1, 33), (300, 5, 64), (2050, 1, 40)):
        img, cap = synth.retrieval_embeddings(n_img, D, seed=300 + n_img, sigma=2.0, caps_per_img=cpi)
        sim = ops.sim_matrix(T(img[::cpi]), T(cap))
        tag = 'stored-%dx%d-D%d' % (n_img, cpi, D)
        out[tag + '/sim'] = sim.cpu()
        for nm, t in zip(names, ops.recall_ranks(sim, caps_per_img=cpi)):
            out[tag + '/' + nm] = t.cpu()
        for dim in (0, 1):
            for k in (1, 50):
                out['%s/topk-dim%d-k%d' % (tag, dim, k)] = ops.topk_indices(sim, k, dim=dim).cpu()
    for n_img, cpi, D in ((1, 5, 8), (257, 8, 50), (700, 5, 768)):
        img_rep, cap = synth.retrieval_embeddings(n_img, D, seed=400 + n_img, sigma=2.0, caps_per_img=cpi)
        data = [('clean', img_rep[::cpi], cap)]
        data += [(case,) + adversarial_retrieval(case, n_img, cpi, D, seed=500 + n_img) for case in ('bulk', 'exact_ties')]
        for case, img, cap in data:
            for exact in (False, True):
                for nm, t in zip(names, ops.retrieval_ranks(T(img), T(cap), caps_per_img=cpi, exact=exact)):
                    out['fused-%dx%d-D%d-%s-%s/%s' % (n_img, cpi, D, case, 'exact' if exact else 'screened', nm)] = t.cpu()
    img, cap = T(synth.normal((70, 64), 601)), T(synth.normal((4000, 64), 602))
    for dim in (0, 1):
        for k in (1, 50, 256):
            idx, val = ops.search_topk(img, cap, k, dim=dim, return_scores=True)
            out['search-70x4000-D64-dim%d-k%d/idx' % (dim, k)], out['search-70x4000-D64-dim%d-k%d/val' % (dim, k)] = idx.cpu(), val.cpu()
    return out


def eval_cases(ops, synth, dev):
    """-> {name: scores} of the no-grad evaluation grids."""
    from aladin_amd import evaluation as E
    from aladin_amd.store import PackedSetStore
    try:
        from aladin_amd import eval_grid as knobs
    except ImportError:                                    # a checkout from before the grid had a module of its own
        knobs = ops
    out = {}
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def stores(images, captions, il, cl, prec, batch):
        si, sc = PackedSetStore(images.shape[2], 0, dev, precision=prec), PackedSetStore(images.shape[2], 2, dev, precision=prec)
        for k0 in range(0, images.shape[0], batch):
            k1 = min(images.shape[0], k0 + batch)
            si.append(T(images[k0:k1, :max(il[k0:k1])]), il[k0:k1])
            sc.append(T(captions[k0:k1, :max(cl[k0:k1])]), cl[k0:k1])
        return si.view(slice(0, None, 5)), sc

    def grids(tag, images, captions, il, cl, aggregations, batch):
        ims, caps, ils = T(images[0::5]), T(captions), il[0::5]
        for prec in ('fp16', 'split'):
            vi, sc = stores(images, captions, il, cl, prec, batch)
            knobs._PLAN_CACHE.clear()
            with torch.no_grad():
                for agg in aggregations:
                    out['%s-%s-%s' % (tag, agg, prec)] = ops.alignment_scores(ims, caps, ils, cl, agg, precision=prec).cpu()
                out['%s-stores-%s' % (tag, prec)] = E.compute_sim_matrix(vi, sc, mode='alignment').cpu()
    saved = knobs.BUCKET_MIN_PAIRS, knobs.BUCKET_MIN_SAMPLES, knobs.E_SCRATCH_LIMIT
    try:
        small = synth.eval_sets(90, 128, seed=77, img_len_range=(6, 70), cap_len_range=(5, 66), n_full=4)
        knobs.BUCKET_MIN_PAIRS, knobs.BUCKET_MIN_SAMPLES = 1, 8
        grids('eval90x450-bucketed', *small, ('MrSw', 'MwSr', 'symm'), 53)
        knobs.E_SCRATCH_LIMIT = 1 << 18
        grids('eval90x450-chunked', *small, ('MrSw', 'MwSr', 'symm'), 53)
    finally:
        knobs.BUCKET_MIN_PAIRS, knobs.BUCKET_MIN_SAMPLES, knobs.E_SCRATCH_LIMIT = saved
    grids('eval1000x5000', *synth.eval_sets(1000, 64, seed=9), ('MrSw',), 500)
    knobs._PLAN_CACHE.clear()
    return out


def main():
    if sys.argv[1] == 'cmp':
        a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
        ok = sorted(a) == sorted(b)
        if not ok:
            print('the two files hold different tensors:', sorted(set(a) ^ set(b)))
        for k in a:
            if k not in b:
                continue
            same = torch.equal(a[k], b[k])
            ok &= same
            comparable = a[k].shape == b[k].shape and a[k].numel() > 0          # not: an empty pair list, two lists of different length
            diff = float((a[k].double() - b[k].double()).abs().max()) if comparable else float('nan')
            print('%-34s %s  max |diff| %.3g' % (k, 'bit-identical' if same else 'DIFFERENT', diff))
        sys.exit(0 if ok else 1)
    from aladin_amd import ops, synth
    dev = torch.device('cuda:0')
    out = {}
    group = sys.argv[3] if len(sys.argv) > 3 else 'alignment'
    assert group in ('alignment', 'retrieval', 'eval', 'pack', 'losses', 'all'), group
    if group in ('alignment', 'all'):
        for tag, ragged, seed in (('full', False, 1234), ('ragged', True, 99)):
            im, s, il, sl = synth.alignment_batch(256, 34, 50, 768, seed=seed, ragged=ragged)
            with torch.no_grad():
                out[tag] = ops.alignment_scores(torch.from_numpy(im).to(dev), torch.from_numpy(s).to(dev), il, sl, precision='fp16').cpu()
        out.update(score_cases(ops, synth, dev))
        out.update(argmax_cases(ops, synth, dev))
        out.update(gradient_cases(ops, synth, dev))
        out.update(long_cases(ops, synth, dev))
    if group in ('retrieval', 'all'):
        out.update(retrieval_cases(ops, synth, dev))
    if group in ('eval', 'all'):
        out.update(eval_cases(ops, synth, dev))
    if group in ('pack', 'all'):
        out.update(pack_cases(ops, synth, dev))
    if group in ('losses', 'all'):
        out.update(losses_cases(ops, synth, dev))
    torch.save(out, sys.argv[2])
    print('saved', sys.argv[2], {k: float(v.double().sum()) for k, v in out.items()})


if __name__ == '__main__':
    main()
