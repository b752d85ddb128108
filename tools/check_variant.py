#!/usr/bin/env python3
"""Scores and gradients of seeded problems from the library ALADIN_LIB selects, saved for a bit-for-bit comparison between two
builds (an old library built from another checkout against the new one):

    ALADIN_LIB=/path/to/old/libaladin_hip.so python tools/check_variant.py save old.pt
    python tools/check_variant.py save new.pt
    python tools/check_variant.py cmp old.pt new.pt

Scores: the bench batch (B = 256, full lengths) and a ragged batch.  Gradients (exact backward precision unless the name says
otherwise), one case per stage of the alignment backward: the fused triplet step in the three precision modes; the
sum-of-violations step with the GEMM and with the gather row step; a sparse gradient on the score matrix (fp16 pair kernel at
R = 65, fp32 fallback at R = 71); a long problem; the small-batch loss heads.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


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
            print('%-26s %s  max |diff| %.3g' % (k, 'bit-identical' if same else 'DIFFERENT', float((a[k] - b[k]).abs().max())))
        sys.exit(0 if ok else 1)
    from aladin_amd import ops, synth
    dev = torch.device('cuda:0')
    out = {}
    for tag, ragged, seed in (('full', False, 1234), ('ragged', True, 99)):
        im, s, il, sl = synth.alignment_batch(256, 34, 50, 768, seed=seed, ragged=ragged)
        with torch.no_grad():
            out[tag] = ops.alignment_scores(torch.from_numpy(im).to(dev), torch.from_numpy(s).to(dev), il, sl, precision='fp16').cpu()
    out.update(gradient_cases(ops, synth, dev))
    torch.save(out, sys.argv[2])
    print('saved', sys.argv[2], {k: float(v.double().sum()) for k, v in out.items()})


if __name__ == '__main__':
    main()
