"""GPU tier: the triplet forward's prologue.  With side rows aladin_align_triplet_fwd packs [xe | y], then runs the side GEMM in a
launch whose trailing blocks pack the main image rows (align_side_pack_kernel), instead of packing everything first.  The packed
bytes and E must not depend on that: the fused call is compared, bit for bit, with the composable calls on the same inputs
(aladin_align_pack + aladin_align_scores, the composed hinge head, aladin_align_bwd) -- operand buffer, scores, loss, dS and,
after the backward, both gradients under the exact and the default row step.

The shapes are the smallest at which each piece can go wrong (one case each):
  b5        B = 5, R = 34, T = 50, D = 64: rem 1, xe and y rows padded well past the batch, fewer main rows than the pack blocks
            take in one sweep; ragged lengths with an image of length 1 (no region) and a caption of length 3 (no word)
  b5_views  the same through (S, B, D) -> (B, S, D) permuted views, as the model hands its sets over
  b70       B = 70, D = 256: two side row blocks, many pack batches, images that only pad the last tile
  b12_r51   B = 12, R = 51, T = 38, D = 768: the 48-row class, rem 2, 40-word captions
  b9_r41    B = 9, R = 41, T = 27, D = 128: rem 8, 24-word captions
  b8_r33    B = 8, R = 33: rem 0 -- the old order is still taken and still equal
  b264      B = 264, D = 64: more batches of main rows than the pack blocks have waves (the batch loop runs twice)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {
    'b5': (5, 34, 50, 64, False),
    'b5_views': (5, 34, 50, 64, True),
    'b70': (70, 34, 50, 256, False),
    'b12_r51': (12, 51, 38, 768, False),
    'b9_r41': (9, 41, 27, 128, False),
    'b8_r33': (8, 33, 50, 64, False),
    'b264': (264, 34, 50, 64, False),
}
EXPECT = {'b5': (32, 1), 'b5_views': (32, 1), 'b70': (32, 1), 'b12_r51': (48, 2), 'b9_r41': (32, 8), 'b8_r33': (32, 0), 'b264': (32, 1)}


def _inputs(name):
    from aladin_amd import synth
    B, R, Tn, D, views = CASES[name]
    im, s, il, sl = synth.structured_alignment_batch(B, R, Tn, D, seed=100 + B + R, noise=2.0, ragged=True)
    il, sl = list(il), list(sl)
    il[0], sl[0] = R, Tn
    if B == 5:
        il[1], sl[2] = 1, 3
    dev = torch.device('cuda:0')
    if views:
        a = torch.from_numpy(np.ascontiguousarray(im.transpose(1, 0, 2))).to(dev).permute(1, 0, 2)
        b = torch.from_numpy(np.ascontiguousarray(s.transpose(1, 0, 2))).to(dev).permute(1, 0, 2)
        assert not a.is_contiguous() and a.stride(2) == 1
    else:
        a, b = torch.from_numpy(im).to(dev), torch.from_numpy(s).to(dev)
    return a, b, il, sl


_RUNS = {}


def _run(name):
    """Both forwards of a case, once: (fused, composed) with everything their backwards need."""
    if name in _RUNS:
        return _RUNS[name]
    from aladin_amd import ops
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    a, b, il, sl = _inputs(name)
    ilt, slt = ops.lengths_tensor(il, a.device), ops.lengths_tensor(sl, a.device)
    fused = ops._triplet_forward(a, b, ilt, slt, 0.2)
    assert fused is not None, 'the fused call does not cover this case'
    loss, S, saved = fused
    geom = saved.geom
    assert (geom.mrows, geom.rem) == EXPECT[name]
    tensors = saved.tensors()
    ar, br = ops._rows_inner_contig(a), ops._rows_inner_contig(b)
    packed = ops.pack_sets(ar, br, ilt, slt, geom)
    S2 = ops.scores_from_packed(packed.xm, packed.xe, packed.y, geom)
    loss2, dS2, pairs = ops._hinge_raw(S2, 0.2, True, True, want_pairs=True)
    torch.cuda.synchronize()
    _RUNS[name] = dict(a=ar, b=br, ilt=ilt, slt=slt, geom=geom, saved=saved, tensors=tensors, loss=loss, S=S,
                       packed=packed, S2=S2, loss2=loss2, dS2=dS2, pairs=pairs)
    return _RUNS[name]


@pytest.mark.parametrize('name', list(CASES))
def test_forward_equals_the_composable_calls(name):
    from aladin_amd import ops
    r = _run(name)
    geom = r['geom']
    buf = r['tensors'][4]
    mine = ops.Packed.from_buf(buf, geom, r['saved'].offs)
    ref = r['packed']
    n_xm, n_xe, n_y = int(geom.xm_rows), int(geom.xe_rows), int(geom.y_rows)
    assert torch.equal(mine.xm, ref.xm), 'xm'
    if n_xe:
        assert torch.equal(mine.xe[:geom.xe_bytes // 2], ref.xe[:geom.xe_bytes // 2]), 'xe'
    assert torch.equal(mine.y, ref.y), 'y'
    # rnorm bit patterns, region by region (a zero row's entry is 0)
    rn, rn2 = mine.rnorm.view(torch.int32), ref.rnorm.view(torch.int32)
    assert torch.equal(rn[:n_xm], rn2[:n_xm]), 'rnorm of xm'
    assert torch.equal(rn[n_xm:n_xm + n_xe], rn2[n_xm:n_xm + n_xe]), 'rnorm of xe'
    assert torch.equal(rn[n_xm + n_xe:n_xm + n_xe + n_y], rn2[n_xm + n_xe:n_xm + n_xe + n_y]), 'rnorm of y'
    assert torch.equal(r['S'], r['S2']), 'S'
    assert torch.equal(r['loss'].reshape(()), r['loss2'].reshape(())), (float(r['loss']), float(r['loss2']))
    assert torch.equal(r['tensors'][2], r['dS2']), 'dS'
    assert bool(torch.isfinite(r['S']).all())


@pytest.mark.parametrize('mode', ['exact', 'fp16'])
@pytest.mark.parametrize('name', list(CASES))
def test_backward_equals_the_composable_calls(name, mode):
    from aladin_amd import ops
    r = _run(name)
    old = ops.set_backward_precision(mode)
    try:
        one = torch.ones((), device=r['a'].device)
        d_im, d_s = r['saved'].backward(r['tensors'], r['ilt'], r['slt'], one)
        d_im2, d_s2 = ops._align_backward(r['a'], r['b'], r['ilt'], r['slt'], r['dS2'], gscale=one, packed=r['packed'], pairs=r['pairs'])
        torch.cuda.synchronize()
    finally:
        ops.set_backward_precision(old)
    assert torch.equal(d_im, d_im2), 'd_im'
    assert torch.equal(d_s, d_s2), 'd_s'
    assert bool(torch.isfinite(d_im).all()) and bool(torch.isfinite(d_s).all())
    assert float(d_im.abs().max()) > 0 and float(d_s.abs().max()) > 0
