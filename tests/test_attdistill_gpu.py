"""GPU tier (-m gpu): the attention-distillation loss -- aladin_attdistill_fwd / _bwd (csrc/attdistill.hip) through
ops.attention_distillation_loss, loss.AttentionDistillationLoss and ALADModel with loss-type 'matching-attdistillation'.

References are float64, never the code under test: the restatement tests/helpers/attdistill_numpy.py, which the CPU tier pins to the
reference's recorded float64 run (tests/golden/attdistill.npz), evaluated on the kernels' split operands (the design's accepted
error and nothing else).  Gates: |loss - ref| <= GATE_LOSS_REL |ref| and max|grad - ref| <= GATE_GRAD_MAXNORM max|ref|, both
4 x the float32 floor the CPU tier measures over the same inputs (attdistill_numpy: 5.6e-7 and 2.4e-6).  Every value test prints its
figures before asserting.

Worst figures measured on the MI355X: DESIGN.md 4.3.1 (loss 3.3e-7 relative, gradients 1.9e-6 of their largest entry)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import attdistill_numpy as A             # noqa: E402

pytestmark = pytest.mark.gpu

UPSTREAM = 3.5
CONFIG = {'training': {'loss-type': 'matching-attdistillation', 'loss-weights': [1.0, 0.5], 'margin': 0.2, 'measure': 'dot',
                       'max-violation': True}}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(dev())               # a copy: the shared inputs are read-only


def bits(v):
    return v.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, float64 (loss, d_im, d_s) on the split operands) of a GPU case: computed once, shared, never written to"""
    x = A.make_inputs(**dict(A.GPU_CASES)[name])
    return x, A.attdistill(x['im'], x['s'], x['im_len'], x['s_len'], x['teacher'], rounded='split')


def run(x, teacher=None, upstream=UPSTREAM, lens_on_device=False):
    """-> (loss, d_im, d_s) of the module on the device, the loss multiplied by `upstream` before backward()"""
    from aladin_amd.loss import AttentionDistillationLoss
    im, s = T(x['im']).requires_grad_(True), T(x['s']).requires_grad_(True)
    il, sl = x['im_len'], x['s_len']
    if lens_on_device:
        il, sl = (torch.tensor(v, dtype=torch.int32, device=dev()) for v in (il, sl))
    loss = AttentionDistillationLoss()(im, s, il, sl, T(x['teacher']) if teacher is None else teacher)
    (loss * upstream).backward()
    return loss.detach(), im.grad, s.grad


def check(name, got, ref, upstream=UPSTREAM):
    loss, d_im, d_s = got
    want = (ref[0], ref[1] * upstream, ref[2] * upstream)
    el, ei, es = A.errors((float(loss), d_im.cpu().numpy(), d_s.cpu().numpy()), want)
    print('%-34s loss %.9g (ref %.9g) rel %.2e [gate %.1e]   d_im %.2e  d_s %.2e [gate %.1e]'
          % (name, float(loss), ref[0], el, A.GATE_LOSS_REL, ei, es, A.GATE_GRAD_MAXNORM))
    assert np.isfinite(float(loss)) and bool(torch.isfinite(d_im).all()) and bool(torch.isfinite(d_s).all())
    assert el <= A.GATE_LOSS_REL, (name, el)
    assert ei <= A.GATE_GRAD_MAXNORM and es <= A.GATE_GRAD_MAXNORM, (name, ei, es)


def test_the_class_is_importable():
    from aladin_amd.loss import AttentionDistillationLoss
    assert list(AttentionDistillationLoss().parameters()) == []


@pytest.mark.parametrize('name', [n for n, _ in A.GPU_CASES])
def test_loss_and_gradients_match_the_float64_restatement(name):
    """Every boundary of the kernels (attdistill_numpy.GPU_CASES): loss and both gradients under an upstream gradient of 3.5 inside
    the gates; slot 0 and every position past a length exactly 0; a second run bit-identical."""
    x, ref = case(name)
    got = run(x, lens_on_device=name.endswith('_over'))
    check(name, got, ref)
    n, m = A.counts(x['im_len'], x['s_len'], x['im'].shape[1] - 1, x['s'].shape[1] - 1)
    d_im, d_s = got[1].cpu().numpy(), got[2].cpu().numpy()
    assert d_im.shape == x['im'].shape and d_s.shape == x['s'].shape
    assert not d_im[:, 0].any() and not d_s[:, 0].any()
    assert all(not d_im[i, 1 + n[i]:].any() for i in range(len(n))) and all(not d_s[j, 1 + m[j]:].any() for j in range(len(m)))
    if 'empty' in name:
        assert (n == 0).sum() == 1 and not d_im[int(np.argmin(n))].any()
    again = run(x, lens_on_device=name.endswith('_over'))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again))


def test_teacher_is_read_in_place_through_its_strides():
    """A non-contiguous, misaligned view (batch, word and region offsets inside a larger tensor; unit innermost stride): the same
    bits as its contiguous copy, and no copy is made.  A view with a non-unit innermost stride is refused."""
    x, ref = case('b9x9_r33_t17_d64_ragged')
    t = x['teacher']
    big = torch.full((t.shape[0], t.shape[1] + 1, t.shape[2] + 2, t.shape[3] + 3), 7.0, device=dev())
    view = big[:, 1:, 2:, 3:]
    view.copy_(T(t))
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0
    got = run(x, teacher=view)
    check('strided teacher', got, ref)
    base = run(x)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, base))
    with pytest.raises(ValueError, match='unit innermost stride'):
        run(x, teacher=T(np.repeat(t, 2, axis=3))[:, :, :, ::2])
    with pytest.raises(ValueError, match='do not overlap'):                     # an expanded word axis: stride 0 < Rt
        run(x, teacher=T(t[:, :, :1]).expand(-1, -1, t.shape[2], -1))


def test_no_word_at_all_gives_zero_loss_and_zero_gradients():
    x = dict(A.make_inputs(Bi=3, Bc=2, R=6, T=5, D=8, seed=41))
    x['s_len'] = [1, 0]
    loss, d_im, d_s = run(x)
    assert float(loss) == 0.0 and not bool(d_im.any()) and not bool(d_s.any())


def test_only_the_wanted_gradient_is_computed_and_no_grad_runs():
    from aladin_amd import ops
    x, ref = case('b5x3_r15_t16_d20_ragged')
    both = run(x, upstream=1.0)
    im, s = T(x['im']).requires_grad_(True), T(x['s'])
    loss = ops.attention_distillation_loss(im, s, x['im_len'], x['s_len'], T(x['teacher']))
    loss.backward()
    assert s.grad is None and torch.equal(bits(im.grad), bits(both[1])) and torch.equal(bits(loss.detach()), bits(both[0]))
    with torch.no_grad():
        quiet = ops.attention_distillation_loss(T(x['im']), T(x['s']), x['im_len'], x['s_len'], T(x['teacher']))
    assert torch.equal(bits(quiet), bits(both[0]))


def test_limits_and_teacher_checks_raise_before_any_launch():
    from aladin_amd import ops
    z = lambda *shape: torch.zeros(*shape, device=dev())
    ok = (z(2, 5, 8), z(3, 4, 8), [5, 5], [4, 4, 4])
    with pytest.raises(ValueError, match='at most 96 scored positions'):
        ops.attention_distillation_loss(z(2, 98, 8), z(3, 4, 8), [5, 5], [4, 4, 4], z(2, 3, 3, 97))
    with pytest.raises(ValueError, match='at most 96 scored positions'):
        ops.attention_distillation_loss(z(2, 5, 8), z(3, 98, 8), [5, 5], [4, 4, 4], z(2, 3, 97, 4))
    for bad in (z(2, 3, 2, 4), z(2, 3, 3, 3), z(2, 2, 3, 4), z(3, 4), z(2, 3, 3, 4).double(), torch.zeros(2, 3, 3, 4)):
        with pytest.raises(ValueError, match='teacher'):
            ops.attention_distillation_loss(*ok, bad)
    with pytest.raises(ValueError, match='feature sizes differ'):
        ops.attention_distillation_loss(z(2, 5, 8), z(3, 4, 12), [5, 5], [4, 4, 4], z(2, 3, 3, 4))
    with pytest.raises(ValueError, match='one length per sample'):
        ops.attention_distillation_loss(z(2, 5, 8), z(3, 4, 8), [5], [4, 4, 4], z(2, 3, 3, 4))
    assert float(ops.attention_distillation_loss(*ok, z(2, 3, 3, 4))) == 0.0       # the smallest good call; a zero teacher: P = 0, loss 0


def test_model_end_to_end_with_the_term():
    """'matching-attdistillation': (loss, loss_dict) with both terms, the logger key with n = the batch size, the weighted total, and
    backward() reaching the stand-ins of all four encoder outputs; the term's value is the module's on the permuted views."""
    from aladin_amd.alad_model import ALADModel
    from aladin_amd.loss import AttentionDistillationLoss

    class Log:
        def __init__(self):
            self.seen = {}

        def update(self, k, v, n=0):
            self.seen[k] = (v, n)
    x, ref = case('b5x5_r50_t37_d768_teacher69x70')
    B, D = 5, 768
    emb = A.synth.global_embeddings(B, D, seed=9, noise=3.0)                       # noisy enough for the matching hinge to be active
    img_emb, cap_emb = T(emb[0]).requires_grad_(True), T(emb[1]).requires_grad_(True)
    img_set = T(x['im']).permute(1, 0, 2).contiguous().requires_grad_(True)        # (R, B, D), as the encoder hands them over
    cap_seq = T(x['s']).permute(1, 0, 2).contiguous().requires_grad_(True)
    m = ALADModel(CONFIG)
    m.logger = Log()
    teacher = T(x['teacher'])
    total, d = m.forward_loss_total(img_emb, cap_emb, img_set, cap_seq, x['im_len'], x['s_len'], None, teacher_attentions=teacher)
    assert list(d) == ['matching', 'attdistillation']
    assert set(m.logger.seen) == {'matching_loss', 'attdistillation_loss'} and m.logger.seen['attdistillation_loss'][1] == B
    alone = AttentionDistillationLoss()(T(x['im']), T(x['s']), x['im_len'], x['s_len'], teacher)
    assert torch.equal(bits(d['attdistillation'].detach()), bits(alone))
    assert abs(m.logger.seen['attdistillation_loss'][0] - ref[0]) <= A.GATE_LOSS_REL * abs(ref[0])
    want = float(d['matching']) + 0.5 * float(d['attdistillation'])
    assert abs(float(total) - want) <= 1e-6 * abs(want)
    total.backward()
    for t in (img_emb, cap_emb, img_set, cap_seq):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool(t.grad.any())
    el, ei, es = A.errors((ref[0], img_set.grad.permute(1, 0, 2).cpu().numpy(), cap_seq.grad.permute(1, 0, 2).cpu().numpy()),
                          (ref[0], 0.5 * ref[1], 0.5 * ref[2]))
    print('model: d img_set %.2e  d cap_seq %.2e [gate %.1e]' % (ei, es, A.GATE_GRAD_MAXNORM))
    assert ei <= A.GATE_GRAD_MAXNORM and es <= A.GATE_GRAD_MAXNORM
    # without the tensor the term is skipped, as the reference (which never calls the criterion) leaves it out
    total2, d2 = m.forward_loss_total(img_emb, cap_emb, img_set, cap_seq, x['im_len'], x['s_len'], None)
    assert list(d2) == ['matching'] and torch.equal(bits(d2['matching'].detach()), bits(d['matching'].detach()))
