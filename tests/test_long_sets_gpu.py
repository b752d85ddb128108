"""GPU tier (-m gpu): alignment sets longer than the tile classes (more than 96 scored positions on either side, up to 512
positions per set) through the long-set kernels of csrc/align_long.hip, against the oracle, the reference's own fixture, the
tile-class kernels inside their limits, and the model's composed and graphed steps."""
import numpy as np
import pytest
import torch

from conftest import load_golden, golden_alignment_inputs
import alad_oracle as O
import faithful_torch as FT

pytestmark = pytest.mark.gpu

RTOL = 1e-3
FP16_BWD_GATE, FP16_BWD_GATE_TOY = 5e-4, 1e-3      # the row step's absolute term per mode, as in test_gpu_parity.py


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def assert_scores_close(S, ref, rtol=RTOL, atol_rel=3e-4):
    S = np.asarray(S, np.float64)
    ref = np.asarray(ref, np.float64)
    np.testing.assert_allclose(S, ref, rtol=rtol, atol=atol_rel * max(1e-6, float(np.abs(ref).max())))


def assert_grads_close(got, ref, mode, exact_atol=2e-5, rtol=1e-3):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    scale = max(1e-9, float(np.abs(ref).max()))
    gate = exact_atol if mode == 'exact' else (FP16_BWD_GATE if ref.shape[-1] >= 64 else FP16_BWD_GATE_TOY)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=gate * scale)


def assert_dropped_rows_zero(d_im, d_s, il, sl):
    """Region 0, token 0, the last two tokens and every padded position carry exactly no gradient."""
    d_im = d_im.detach().cpu().numpy()
    d_s = d_s.detach().cpu().numpy()
    for i, L in enumerate(il):
        assert not d_im[i, 0].any() and not d_im[i, L:].any()
    for j, L in enumerate(sl):
        assert not d_s[j, 0].any() and not d_s[j, max(L - 2, 1):].any()


@pytest.fixture(params=['exact', 'fp16'])
def bwd_mode(request):
    from aladin_amd import ops
    old = ops.set_backward_precision(request.param)
    yield request.param
    ops.set_backward_precision(old)


@pytest.fixture
def exact_backward():
    from aladin_amd import ops
    old = ops.set_backward_precision('exact')
    yield
    ops.set_backward_precision(old)


def ragged_batch(Bi, Bc, R, T_, D, seed):
    """Seeded sets whose lengths include a sample that fills each set and samples short enough for the zero fill."""
    from aladin_amd import synth
    im = synth.normal((Bi, R, D), seed)
    s = synth.normal((Bc, T_, D), seed + 4444)
    il = [int(v) for v in synth.integers((Bi,), min(10, R), R, seed + 17)]
    sl = [int(v) for v in synth.integers((Bc,), min(6, T_), T_, seed + 29)]
    il[seed % Bi] = R
    sl[(seed + 1) % Bc] = T_
    il[(seed + 2) % Bi] = max(2, R // 3)
    sl[(seed + 3) % Bc] = max(4, T_ // 3)
    return im, s, il, sl


SCORE_SHAPES = [(5, 6, 98, 50, 64), (6, 5, 34, 100, 64), (4, 4, 200, 180, 96), (3, 3, 512, 512, 32)]


@pytest.mark.parametrize('shape', SCORE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('precision', ['fp16', 'split'])
def test_long_scores_match_the_oracle(shape, precision):
    """No-grad scores of every pooling in both evaluation precisions (ops.alignment_scores, the loss module's 'MrAVGw', the
    evaluation grid) on the first shapes the tile classes reject and on long ones."""
    from aladin_amd import ops
    from aladin_amd import evaluation as E
    from aladin_amd.loss import AlignmentContrastiveLoss
    Bi, Bc, R, T_, D = shape
    im, s, il, sl = ragged_batch(Bi, Bc, R, T_, D, seed=R + T_)
    assert ops.is_long(R, T_)
    a, b = T(im), T(s)
    with torch.no_grad():
        for mode in ('MrSw', 'MrAVGw', 'MwSr', 'symm'):
            if mode == 'MrAVGw':
                S = AlignmentContrastiveLoss(margin=0.2, measure='dot', max_violation=True, aggregation=mode)(
                    a, b, il, sl, return_loss=False, return_similarity_mat=True)
            else:
                S = ops.alignment_scores(a, b, il, sl, mode, precision=precision)
            ref = O.alignment_scores(im, s, il, sl, mode, dtype=np.float64)
            S = S.cpu().numpy()
            if mode == 'MrAVGw':          # the module scores in the evaluation precision of the library (default 'split')
                np.testing.assert_allclose(S, ref, rtol=3e-6, atol=3e-6)
            elif precision == 'split':
                np.testing.assert_allclose(S, ref, rtol=3e-6, atol=3e-6)
            else:
                assert_scores_close(S, ref)
        Sg = E.compute_sim_matrix(a, b, il, sl, mode='alignment', precision=precision).cpu().numpy()
    ref = O.alignment_scores(im, s, il, sl, 'MrSw', dtype=np.float64)
    if precision == 'split':
        np.testing.assert_allclose(Sg, ref, rtol=3e-6, atol=3e-6)
    else:
        assert_scores_close(Sg, ref)


@pytest.mark.parametrize('shape', [(5, 98, 50, 64), (6, 34, 100, 64), (4, 200, 180, 96)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('max_violation', [True, False])
def test_long_loss_and_gradients_match_the_oracle(shape, max_violation, bwd_mode):
    """AlignmentContrastiveLoss('MrSw') on long sets: loss, S and the gradients of both sets against the oracle's hinge and
    backward, with only the loss back-propagated and with a gradient on S as well.  Dropped and padded positions get exactly 0."""
    from aladin_amd.loss import AlignmentContrastiveLoss
    B, R, T_, D = shape
    im, s, il, sl = ragged_batch(B, B, R, T_, D, seed=3 * R + T_)
    ref_S = O.alignment_scores(im, s, il, sl, 'MrSw', dtype=np.float64)
    ref_loss, ref_dS = O.hinge_loss(ref_S, 0.2, max_violation, return_grad=True)
    w = np.asarray(np.random.default_rng(R).standard_normal((B, B)), np.float32) * 0.1
    crit = AlignmentContrastiveLoss(margin=0.2, measure='dot', max_violation=max_violation, aggregation='MrSw')
    for with_S in (False, True):
        a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
        loss, S = crit(a, b, il, sl, return_similarity_mat=True)
        (loss + (S * T(w)).sum() if with_S else loss).backward()
        assert_scores_close(S.detach().cpu().numpy(), ref_S)
        np.testing.assert_allclose(float(loss), float(ref_loss), rtol=RTOL, atol=1e-4)
        dS = ref_dS + (w if with_S else 0.0)
        ref_dim, ref_ds = O.alignment_scores_backward(im, s, il, sl, dS)
        assert_grads_close(a.grad, ref_dim, bwd_mode)
        assert_grads_close(b.grad, ref_ds, bwd_mode)
        assert_dropped_rows_zero(a.grad, b.grad, il, sl)


@pytest.mark.parametrize('mode', ['MwSr', 'symm'])
def test_long_gradients_of_the_other_poolings(mode, bwd_mode):
    """ops.alignment_scores('MwSr' / 'symm') on long sets, a gradient on S, against the reference's dataflow under autograd."""
    from aladin_amd import ops
    B, R, T_, D = 4, 110, 105, 64
    im, s, il, sl = ragged_batch(B, B, R, T_, D, seed=7)
    w = np.asarray(np.random.default_rng(5).standard_normal((B, B)), np.float32)
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    S = ops.alignment_scores(a, b, il, sl, mode)
    (S * T(w)).sum().backward()
    ra = torch.from_numpy(im).double().requires_grad_(True)
    rb = torch.from_numpy(s).double().requires_grad_(True)
    Sr = FT.alignment_scores_faithful(ra, rb, il, sl, mode)
    (Sr * torch.from_numpy(w).double()).sum().backward()
    assert_scores_close(S.detach().cpu().numpy(), Sr.detach().numpy())
    assert_grads_close(a.grad, ra.grad.numpy(), bwd_mode)
    assert_grads_close(b.grad, rb.grad.numpy(), bwd_mode)
    assert_dropped_rows_zero(a.grad, b.grad, il, sl)


@pytest.mark.parametrize('mode', ['MrSw', 'MwSr'])
def test_padding_across_the_old_limit_changes_nothing(mode, exact_backward):
    """The same batch at R = 60, T = 40 (tile-class kernels) and zero-padded to R = T = 130 (long-set kernels), every length
    shorter than its set so that the zero fill takes part at both shapes: scores, loss and the gradients of the real positions
    agree to 1e-5; the added positions get exactly 0."""
    from aladin_amd import ops, synth
    from aladin_amd.loss import AlignmentContrastiveLoss
    B, R, T_, D = 8, 60, 40, 64
    im = synth.normal((B, R, D), 61)
    s = synth.normal((B, T_, D), 62)
    il = [int(v) for v in synth.integers((B,), 10, R - 1, 63)]
    sl = [int(v) for v in synth.integers((B,), 6, T_ - 1, 64)]
    assert max(il) < R and max(sl) < T_
    imp = np.zeros((B, 130, D), np.float32)
    sp = np.zeros((B, 130, D), np.float32)
    imp[:, :R] = im
    sp[:, :T_] = s
    assert not ops.is_long(R, T_) and ops.is_long(130, 130)
    out = []
    for x, y in ((im, s), (imp, sp)):
        a, b = T(x).requires_grad_(True), T(y).requires_grad_(True)
        if mode == 'MrSw':
            loss, S = AlignmentContrastiveLoss(margin=0.2, measure='dot', max_violation=True, aggregation='MrSw')(
                a, b, il, sl, return_similarity_mat=True)
        else:
            S = ops.alignment_scores(a, b, il, sl, 'MwSr')
            loss = ops.hinge_loss(S, 0.2, True)
        loss.backward()
        out.append((float(loss), S.detach().cpu().numpy(), a.grad.cpu().numpy(), b.grad.cpu().numpy()))
    (l0, S0, gi0, gs0), (l1, S1, gi1, gs1) = out
    np.testing.assert_allclose(S1, S0, rtol=1e-5, atol=1e-5 * np.abs(S0).max())
    np.testing.assert_allclose(l1, l0, rtol=1e-5)
    np.testing.assert_allclose(gi1[:, :R], gi0, rtol=1e-5, atol=1e-5 * np.abs(gi0).max())
    np.testing.assert_allclose(gs1[:, :T_], gs0, rtol=1e-5, atol=1e-5 * np.abs(gs0).max())
    assert not gi1[:, R:].any() and not gs1[:, T_:].any()


@pytest.mark.parametrize('shape', [(6, 6, 97, 99, 64), (128, 128, 34, 50, 768)], ids=['96x96', 'headline'])
def test_long_kernel_agrees_with_the_tile_kernels(shape):
    """ops.LONG_PATH_FORCE: the long-set kernels on shapes the tile classes cover (R' = T' = 96 and the headline shape) against
    the tile kernels: <= 2e-6 max|S| with fp16 operands, <= 1e-6 max|S| with split operands."""
    from aladin_amd import _lib, ops
    Bi, Bc, R, T_, D = shape
    im, s, il, sl = ragged_batch(Bi, Bc, R, T_, D, seed=11)
    a, b = T(im), T(s)
    for precision, bound in (('fp16', 2e-6), ('split', 1e-6)):
        with torch.no_grad():
            ref = ops.alignment_scores(a, b, il, sl, 'MrSw', precision=precision).cpu().numpy()
            old = ops.LONG_PATH_FORCE
            ops.LONG_PATH_FORCE = True
            try:
                assert ops.align_geometry(Bi, Bc, R, T_, D, 0, 2, precision, layout='auto').layout == _lib.LAYOUT_LONG
                got = ops.alignment_scores(a, b, il, sl, 'MrSw', precision=precision).cpu().numpy()
            finally:
                ops.LONG_PATH_FORCE = old
        assert np.abs(got - ref).max() <= bound * np.abs(ref).max(), (precision, np.abs(got - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize('loss_type', ['alignment', 'alignment-distillation'])
def test_model_on_long_sets_eager_and_graphed(loss_type):
    """ALADModel at bs 32 with R = 101, T = 110 (the composed path; the small-batch heads stop at the tile classes): loss and
    loss_dict against the oracle, and graphed=True equal to eager bit for bit -- loss, terms, logger entries, the gradients that
    reach the four encoder outputs."""
    from aladin_amd import synth
    from aladin_amd.alad_model import ALADModel
    from aladin_amd.evaluation import LogCollector
    weights = [1] if loss_type == 'alignment' else [1, 1]
    config = {'training': {'loss-type': loss_type, 'loss-weights': weights, 'margin': 0.2, 'measure': 'dot',
                           'max-violation': True, 'alignment-mode': 'MrSw', 'distillation-mode': 'listnet'}}
    B, R, Tn, D = 32, 101, 110, 64
    models = [ALADModel(config, graphed=False), ALADModel(config, graphed=True)]
    for m in models:
        m.logger = LogCollector()
    for seed, epoch in ((1, 5), (2, 0)):
        im, s, il, sl = synth.structured_alignment_batch(B, R, Tn, D, seed=seed, noise=3.0, ragged=True)
        ge, gc = synth.global_embeddings(B, D, seed=seed + 50, noise=1.0)
        ref = O.forward_loss(ge, gc, im.transpose(1, 0, 2), s.transpose(1, 0, 2), il, sl, loss_type)
        ref_total, ref_terms = O.total_loss(ref, dict(zip(['alignment', 'distillation'], weights)), epoch, 2)
        outs = []
        for m in models:
            t = [T(ge).requires_grad_(True), T(gc).requires_grad_(True), T(im.transpose(1, 0, 2).copy()).requires_grad_(True),
                 T(s.transpose(1, 0, 2).copy()).requires_grad_(True)]
            m.forward_emb = lambda a, b, _t=t: (_t[0], _t[1], _t[2], _t[3], il, sl, 0)
            loss, d = m(None, None, epoch=epoch, distill_epoch=2)
            loss.backward()
            outs.append((loss.detach().clone(), {k: v.detach().clone() for k, v in d.items()}, [None if x.grad is None else x.grad.clone() for x in t],
                         {k: (mm.val, mm.count) for k, mm in m.logger.meters.items()}, str(m.logger)))
        (l0, d0, g0, log0, s0), (l1, d1, g1, log1, s1) = outs
        np.testing.assert_allclose(float(l0), float(ref_total), rtol=RTOL, atol=1e-4)
        assert list(d0) == list(ref_terms)
        for k in ref_terms:
            np.testing.assert_allclose(float(d0[k]), float(ref_terms[k]), rtol=RTOL, atol=1e-4)
        assert torch.equal(l0, l1) and list(d0) == list(d1) and log0 == log1 and s0 == s1
        assert all(torch.equal(d0[k], d1[k]) for k in d0)
        for a, b in zip(g0, g1):
            if a is None or b is None:
                assert (a is None or float(a.abs().max()) == 0.0) and (b is None or float(b.abs().max()) == 0.0)
            else:
                assert torch.equal(a, b)
        assert g0[2] is not None and float(g0[2].abs().max()) > 0 and float(g0[3].abs().max()) > 0


def test_long_golden_from_the_reference(bwd_mode):
    """tests/golden/align_long_b4.npz (make_golden_long.py: the reference itself, B = 4, R = 130, T = 120, D = 64, ragged):
    'MrSw' scores, the max_violation loss and both gradients."""
    from aladin_amd.loss import AlignmentContrastiveLoss
    g = load_golden('align_long_b4')
    im, s, il, sl = golden_alignment_inputs(g)
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    loss, S = AlignmentContrastiveLoss(margin=float(g['margin']), measure='dot', max_violation=True, aggregation='MrSw')(
        a, b, il, sl, return_similarity_mat=True)
    loss.backward()
    assert_scores_close(S.detach().cpu().numpy(), g['S_MrSw'])
    np.testing.assert_allclose(float(loss), float(g['loss_mv']), rtol=RTOL, atol=1e-4)
    assert_grads_close(a.grad, g['dim_mv'], bwd_mode)
    assert_grads_close(b.grad, g['ds_mv'], bwd_mode)
    assert_dropped_rows_zero(a.grad, b.grad, il, sl)


@pytest.mark.parametrize('R,T_', [(513, 50), (50, 513)])
def test_past_512_positions_is_refused_at_forward_time(R, T_):
    """R = 513 or T = 513 with requires_grad: ValueError from the forward, before any launch."""
    from aladin_amd import ops
    from aladin_amd.loss import AlignmentContrastiveLoss
    B, D = 2, 16
    a = torch.zeros((B, R, D), device=dev(), requires_grad=True)
    b = torch.zeros((B, T_, D), device=dev(), requires_grad=True)
    with pytest.raises(ValueError, match='512 positions'):
        ops.alignment_scores(a, b, [R] * B, [T_] * B)
    with pytest.raises(ValueError, match='512 positions'):
        AlignmentContrastiveLoss(margin=0.2, measure='dot', max_violation=True, aggregation='MrSw')(a, b, [R] * B, [T_] * B)
