"""GPU tier (-m gpu): the cross-entropy (InfoNCE) criterion -- aladin_xent_fwd_bwd (csrc/xent.hip) through
ops.cross_entropy_scores, ops.match_cross_entropy, loss.CrossEntropyCriterion, loss.AlignmentCrossEntropyLoss and ALADModel with
loss-type 'matching-crossentropy'.

References are float64, never the code under test: the reference's recorded float64 run (tests/golden/xent.npz,
make_golden_xent.py) and the float64 restatement tests/helpers/xent_numpy.py that the CPU tier pins to it.  Tolerances: loss and
d temperature rtol 1e-5 / atol 1e-6 (ListNet's); gradients |got - ref| <= 1e-4 |ref| + a max|ref| with a = 4 x the family's recorded
float32 floor (xent_numpy.XENT_A; the rule of assert_cancelling_grad_close).  Every value test prints its figures before asserting."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_alignment_inputs, load_golden
import alad_oracle as O

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import xent_numpy as X                   # noqa: E402

pytestmark = pytest.mark.gpu

CONFIG = {'training': {'loss-type': X.MODEL_LOSS_TYPE, 'loss-weights': X.MODEL_WEIGHTS, 'margin': 0.2, 'measure': 'dot', 'max-violation': True}}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(dev())               # a copy: the shared inputs are read-only


def bits(v):
    return v.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def fixture():
    """(golden, [(case index, family, B, D, t, img, cap)]): inputs rebuilt from the recorded seeds, checksums checked."""
    from aladin_amd import synth
    g = load_golden('xent')
    cases = []
    for ci, ((fam, B, D, s1, s2), t) in enumerate(zip(g['cases'], g['temperatures'])):
        fam = X.FIXTURE_FAMILIES[int(fam)]
        img, cap = X.case_inputs(fam, int(B), int(D), int(s1), int(s2))
        for a, key in ((img, 'img'), (cap, 'cap')):
            want = float(g['c%d_%s_checksum' % (ci, key)])
            assert abs(synth.checksum(a) - want) <= 1e-6 * max(1.0, abs(want))
        cases.append((ci, fam, int(B), int(D), float(t), img, cap))
    assert len(cases) == len(X.SHAPES) * len(X.TEMPERATURES) * len(X.FIXTURE_FAMILIES)
    return g, cases


@functools.lru_cache(maxsize=None)
def matrix_case(B, family):
    """(S, t, float64 (loss, dS, dt)) of a helper input: computed once, shared, never written to"""
    S, t = X.matrix_inputs(B, family)
    ref = X.xent_f64(S, t)
    S.setflags(write=False)
    ref[1].setflags(write=False)
    return S, t, ref


def run_scores(S, t, g=None, leaf=None):
    """ops.cross_entropy_scores forward + backward -> (loss, dS, dt); S: a tensor (a view of `leaf` when given), t: float -> a parameter"""
    from aladin_amd import ops
    s = S.detach().requires_grad_(True) if leaf is None else S
    tt = torch.full((1,), t, dtype=torch.float32, device=dev(), requires_grad=True)
    loss = ops.cross_entropy_scores(s, tt)
    (loss if g is None else loss * g).backward()
    return loss.detach(), (s if leaf is None else leaf).grad, tt.grad


def run_criterion(img, cap, t):
    from aladin_amd.loss import CrossEntropyCriterion
    crit = CrossEntropyCriterion().to(dev())
    with torch.no_grad():
        crit.temperature.fill_(t)
    a, b = T(img).requires_grad_(True), T(cap).requires_grad_(True)
    loss = crit(a, b)
    loss.backward()
    return loss.detach(), a.grad, b.grad, crit.temperature.grad


def test_criterion_matches_every_fixture_case(fixture):
    """Fails without the feature: aladin_amd.loss has no CrossEntropyCriterion."""
    g, cases = fixture
    for ci, fam, B, D, t, img, cap in cases:
        loss, d_im, d_s, d_t = run_criterion(img, cap, t)
        assert tuple(d_t.shape) == (1,) and loss.dim() == 0
        want_loss, want_dt = float(g['c%d_loss' % ci]), float(g['c%d_dt' % ci])
        r64 = X.criterion_f64(img, cap, t)
        cols = X.grad_columns(B, D)
        print('xent case %2d %-11s (%2d, %3d) t %.4f: loss %.8g ref %.8g |diff| %.2e;  dt %.8g ref %.8g |diff| %.2e;  d im %.3g  d s %.3g of '
              'the largest entry (gate %.3g)' % (ci, fam, B, D, t, loss.item(), want_loss, abs(loss.item() - want_loss), d_t.item(), want_dt,
                                                 abs(d_t.item() - want_dt), X.floor_ratio(d_im.cpu().numpy(), r64[1]),
                                                 X.floor_ratio(d_s.cpu().numpy(), r64[2]), X.XENT_A[fam]))
        np.testing.assert_allclose(loss.item(), want_loss, **X.LOSS_TOL)
        np.testing.assert_allclose(d_t.item(), want_dt, **X.LOSS_TOL)
        for got, key, whole in ((d_im, 'dimg', r64[1]), (d_s, 'dcap', r64[2])):
            got = got.cpu().numpy()
            X.assert_grad_close(got[:, cols], g['c%d_%s' % (ci, key)], fam, (ci, key))
            X.assert_grad_close(got, whole, fam, (ci, key, 'restatement'))           # where the fixture keeps every 4th column only
        if B == 1:
            assert loss.item() == 0.0 and d_t.item() == 0.0 and not d_im.any() and not d_s.any()


@pytest.mark.parametrize('family', X.FAMILIES)
@pytest.mark.parametrize('B', X.SIZES)
def test_matrix_op_matches_float64(B, family):
    S, t, (ref_loss, ref_dS, ref_dt) = matrix_case(B, family)
    loss, dS, d_t = run_scores(T(S), t)
    dS = dS.cpu().numpy()
    print('xent matrix %-6s B %4d: loss %.8g ref %.8g |diff| %.2e;  dt %.8g ref %.8g |diff| %.2e;  dS %.3g of the largest entry %.3g (gate %.3g)'
          % (family, B, loss.item(), ref_loss, abs(loss.item() - ref_loss), d_t.item(), ref_dt, abs(d_t.item() - ref_dt),
             X.floor_ratio(dS, ref_dS) if B > 1 else 0.0, np.abs(ref_dS).max(), X.XENT_A[family]))
    if B == 1:
        assert loss.item() == 0.0 and d_t.item() == 0.0 and not dS.any()             # exactly
        return
    np.testing.assert_allclose(loss.item(), ref_loss, **X.LOSS_TOL)
    np.testing.assert_allclose(d_t.item(), ref_dt, **X.LOSS_TOL)
    X.assert_grad_close(dS, ref_dS, family, (B, family))
    if family == 'sharp':
        # the cancellation trap: both softmaxes near one-hot, and the gradient is still there, diagonal included
        assert dS.any() and (np.diag(dS) < 0).all()
        assert np.abs(dS.sum()) <= 1e-4 * np.abs(dS).sum()                           # sum_ij dL_ij = 0: the diagonal balances its lines


@pytest.mark.parametrize('B', [16, 17, 48, 49, 113])
def test_matrix_op_matches_float64_at_the_line_walk_edges(B):
    """The edges of the walk xent_stats_kernel shares (line_walk.hpp) that X.SIZES misses: 16 / 17, the last block of 16 wave-rows full
    and one over; 48 / 49, the last size at which a strip's waves run the tail loop only and the first at which wave 0 has four rows
    in flight; 113, both loops in waves 1 to 15.  The same gates, on the family with the cancellation trap."""
    test_matrix_op_matches_float64(B, 'sharp')


def test_upstream_gradient_loss_only_and_constant_temperature():
    from aladin_amd import ops
    B = 257
    S, t, (ref_loss, ref_dS, ref_dt) = matrix_case(B, 'mild')
    t = 0.75                                                                          # another temperature than the family's
    ref_loss, ref_dS, ref_dt = X.xent_f64(S, t)
    base = run_scores(T(S), t)
    scaled = run_scores(T(S), t, g=2.5)
    assert torch.equal(bits(scaled[0]), bits(base[0]))
    np.testing.assert_allclose(scaled[1].cpu().numpy(), 2.5 * base[1].cpu().numpy(), rtol=2e-7, atol=0)
    np.testing.assert_allclose(scaled[2].item(), 2.5 * base[2].item(), rtol=2e-7)
    X.assert_grad_close(scaled[1].cpu().numpy(), 2.5 * ref_dS, 'mild', 'upstream 2.5')
    np.testing.assert_allclose(scaled[2].item(), 2.5 * ref_dt, **X.LOSS_TOL)
    # a Python float is a constant: the same loss, the same dS, nothing for the temperature
    s = T(S).requires_grad_(True)
    loss = ops.cross_entropy_scores(s, t)
    loss.backward()
    assert torch.equal(bits(loss.detach()), bits(base[0])) and torch.equal(bits(s.grad), bits(base[1]))
    # only the temperature wants a gradient
    tt = torch.full((1,), t, device=dev(), requires_grad=True)
    ops.cross_entropy_scores(T(S), tt).backward()
    assert torch.equal(bits(tt.grad), bits(base[2]))
    # loss-only: no B x B buffer is allocated
    big = T(matrix_case(1500, 'mild')[0])
    torch.cuda.synchronize()
    for want_grad in (False, True):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        x = big.detach().requires_grad_(want_grad)
        out = ops.cross_entropy_scores(x, 0.0)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - before
        assert (grew >= 4 * 1500 * 1500) == want_grad, (want_grad, grew)
        assert out.requires_grad == want_grad
    with torch.no_grad():
        quiet = ops.cross_entropy_scores(T(S).requires_grad_(True), tt)
    assert not quiet.requires_grad and torch.equal(bits(quiet), bits(base[0]))


def test_views_give_the_contiguous_result_and_the_gradient_lands_in_the_base():
    B = 65
    S, t, _ = matrix_case(B, 'sharp')
    want = run_scores(T(S), t)
    # (a) a row-strided view, ld = B + 5: used in place
    base = torch.zeros((B, B + 5), device=dev())
    base[:, 2:2 + B] = T(S)
    base.requires_grad_(True)
    view = base[:, 2:2 + B]
    assert view.stride() == (B + 5, 1) and not view.is_contiguous()
    got = run_scores(view, t, leaf=base)
    mask = torch.zeros_like(base, dtype=torch.bool)
    mask[:, 2:2 + B] = True
    # (b) every second column of a wider matrix, (c) the transpose of a column-major buffer: copied
    wide = torch.zeros((B, 2 * B), device=dev())
    wide[:, ::2] = T(S)
    wide.requires_grad_(True)
    got_b = run_scores(wide[:, ::2], t, leaf=wide)
    mask_b = torch.zeros_like(wide, dtype=torch.bool)
    mask_b[:, ::2] = True
    colmajor = T(S).t().contiguous().requires_grad_(True)
    assert colmajor.t().stride() == (1, B)
    got_c = run_scores(colmajor.t(), t, leaf=colmajor)
    for (loss, grad, d_t), m, back in ((got, mask, lambda x: x[:, 2:2 + B]), (got_b, mask_b, lambda x: x[:, ::2]), (got_c, None, lambda x: x.t())):
        assert torch.equal(bits(loss), bits(want[0])) and torch.equal(bits(d_t), bits(want[2]))
        assert torch.equal(bits(back(grad)), bits(want[1]))
        if m is not None:
            assert not grad[~m].any()                                               # zero elsewhere in the base tensor


@pytest.mark.parametrize('B', [5, 257])
def test_a_nan_score_gives_a_nan_loss(B):
    from aladin_amd import ops
    S, t, _ = matrix_case(B, 'mild')
    for i, j in ((1, 3), (2, 2), (B - 1, 0)):
        bad = S.copy()
        bad[i, j] = np.nan
        x = T(bad).requires_grad_(True)
        loss = ops.cross_entropy_scores(x, torch.zeros(1, device=dev(), requires_grad=True))
        loss.backward()
        assert torch.isnan(loss).item(), (B, i, j)
        rows, cols = [r for r in range(B) if r != i], [c for c in range(B) if c != j]
        assert torch.isfinite(x.grad[rows][:, cols]).all()                           # unspecified on the NaN's row and column only
    ok = ops.cross_entropy_scores(T(S), 0.0)
    assert torch.isfinite(ok).item()


def test_two_runs_give_the_same_bits_and_a_graph_replay_gives_the_eager_bits():
    from aladin_amd import ops
    B = 257
    first, second = matrix_case(B, 'scaled')[0], matrix_case(B, 'mild')[0]
    r1, r2 = run_scores(T(first), 0.3), run_scores(T(first), 0.3)
    for u, v in zip(r1, r2):
        assert torch.equal(bits(u), bits(v))
    x = T(first).requires_grad_(True)
    tt = torch.full((1,), 0.3, device=dev(), requires_grad=True)
    out = {}

    def run():
        loss = ops.cross_entropy_scores(x, tt)
        out['loss'] = loss.detach()
        out['dS'], out['dt'] = torch.autograd.grad(loss, (x, tt))
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run()                                                                         # warm-up outside the capture
    cur.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    seen = []
    for S, t in ((second, 0.3), (second, 2.0), (first, -1.0)):                        # fresh contents, and the temperature alone changed
        with torch.no_grad():
            x.copy_(T(S))
            tt.fill_(t)
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        eager = run_scores(T(S), t)
        for k, v in (('loss', eager[0]), ('dS', eager[1]), ('dt', eager[2])):
            assert torch.equal(bits(replayed[k]), bits(v)), (k, t)
        np.testing.assert_allclose(replayed['loss'].item(), X.xent_f64(S, t)[0], **X.LOSS_TOL)
        seen.append(replayed['loss'].item())
    assert seen[0] != seen[1]                                                          # the temperature is read on the device


def test_match_node_returns_differentiable_scores():
    """ops.match_cross_entropy(return_scores=True): a gradient arriving on M adds to the loss's."""
    from aladin_amd import ops
    img, cap = X.case_inputs('independent', 33, 64, *X.SEED_INDEPENDENT)
    t = 1.5
    a, b = T(img).requires_grad_(True), T(cap).requires_grad_(True)
    tt = torch.full((1,), t, device=dev(), requires_grad=True)
    loss, M = ops.match_cross_entropy(a, b, tt, return_scores=True)
    W = T(np.linspace(-1, 1, 33 * 33).reshape(33, 33))
    (2.0 * loss + (M * W).sum()).backward()
    r = X.criterion_f64(img, cap, t, g=2.0)
    np.testing.assert_allclose(M.detach().cpu().numpy(), r[4], rtol=1e-5, atol=1e-6)
    W64, i64, c64 = W.cpu().numpy().astype(np.float64), img.astype(np.float64), cap.astype(np.float64)
    X.assert_grad_close(a.grad.cpu().numpy(), r[1] + W64 @ c64, 'independent', 'd im')
    X.assert_grad_close(b.grad.cpu().numpy(), r[2] + W64.T @ i64, 'independent', 'd s')
    np.testing.assert_allclose(tt.grad.item(), r[3], **X.LOSS_TOL)
    # the scores alone
    a2, b2 = T(img).requires_grad_(True), T(cap).requires_grad_(True)
    _, M2 = ops.match_cross_entropy(a2, b2, t, return_scores=True)
    (M2 * W).sum().backward()
    np.testing.assert_allclose(a2.grad.cpu().numpy(), W64 @ c64, rtol=1e-4, atol=1e-5)


# The backward's row step, as tests/test_gpu_parity.py runs every comparison of alignment gradient VALUES: under both modes, with
# that file's per-mode absolute term (a fraction of the largest reference entry) on top of rtol 1e-3.
EXACT_BWD_GATE, FP16_BWD_GATE = 3e-5, 5e-4          # assert_grads_close(exact_atol=3e-5) of the 'MrAVGw' test; FP16_BWD_GATE for D >= 64


@pytest.fixture(params=['exact', 'fp16'])
def bwd_mode(request):
    from aladin_amd import ops
    old = ops.set_backward_precision(request.param)
    yield request.param
    ops.set_backward_precision(old)


def test_alignment_head_cross_entropy(bwd_mode):
    """AlignmentCrossEntropyLoss('MrAVGw') on the align_b5_d64 golden's sets.  Loss: the float64 restatement on the ORACLE's score
    matrix (rtol 1e-3 / atol 1e-3, the alignment losses' tolerance: the scores come from fp16 operands).  Set gradients: the oracle's
    alignment_scores_backward fed with the restatement's dS -- taken at the HIP scores, so that the comparison is about the backward
    (the self-consistent form of test_alignment_other_modes_loss_and_gradients)."""
    from aladin_amd.loss import AlignmentCrossEntropyLoss
    g = load_golden('align_b5_d64')
    im, s, il, sl = golden_alignment_inputs(g)
    t = 1.5
    crit = AlignmentCrossEntropyLoss('MrAVGw').to(dev())
    with torch.no_grad():
        crit.temperature.fill_(t)
    a, b = T(im).requires_grad_(True), T(s).requires_grad_(True)
    loss, S = crit(a, b, il, sl, return_similarity_mat=True)
    loss.backward()
    S_oracle = O.alignment_scores(im, s, il, sl, 'MrAVGw', dtype=np.float64)
    ref_loss = X.xent_f64(S_oracle, t)[0]
    S_hip = S.detach().cpu().numpy()
    hip_loss, dS, hip_dt = X.xent_f64(S_hip, t)
    print('alignment cross-entropy (%s): loss %.7g, restatement on the oracle\'s scores %.7g, on the HIP scores %.7g;  dt %.7g, on the HIP '
          'scores %.7g' % (bwd_mode, loss.item(), ref_loss, hip_loss, crit.temperature.grad.item(), hip_dt))
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(S_hip, S_oracle, rtol=1e-3, atol=3e-4)
    np.testing.assert_allclose(loss.item(), hip_loss, **X.LOSS_TOL)                   # the criterion itself, on the very matrix it was given
    np.testing.assert_allclose(crit.temperature.grad.item(), hip_dt, **X.LOSS_TOL)
    dS_sum = dS / (np.asarray(sl, np.float64) - 3.0)[None, :]                         # 'MrAVGw' = 'MrSw' / (caption length - 3)
    d_im, d_s = O.alignment_scores_backward(im, s, il, sl, dS_sum)
    gate = EXACT_BWD_GATE if bwd_mode == 'exact' else FP16_BWD_GATE
    for got, ref, what in ((a.grad, d_im, 'd im_set'), (b.grad, d_s, 'd s_seq')):
        got = got.cpu().numpy()
        scale = float(np.abs(ref).max())
        print('   %s (%s): max |err| / max |ref| %.3g (gate %.3g)' % (what, bwd_mode, np.abs(got - ref).max() / scale, gate))
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=gate * scale)


class _Log:
    """the part of the reference's LogCollector that forward_loss uses"""

    def __init__(self):
        self.seen = []

    def update(self, k, v, n=0):
        self.seen.append((k, v, n))


def model_step(config, img, cap, t, **kw):
    from aladin_amd.alad_model import ALADModel
    B, D = img.shape
    m = ALADModel(config, **kw)
    assert m.crossentropy_criterion.temperature.is_cuda                                # placed where the 'auto' weights are
    with torch.no_grad():
        m.crossentropy_criterion.temperature.fill_(t)
    m.logger = _Log()
    a, b = T(img).requires_grad_(True), T(cap).requires_grad_(True)
    sets = (a, b, torch.zeros((1, B, D), device=dev()), torch.zeros((1, B, D), device=dev()), [1] * B, [1] * B, 0)
    m.forward_emb = lambda x, y: sets
    total, d = m(None, None, epoch=0, distill_epoch=2)
    total.sum().backward()
    torch.cuda.synchronize()
    return m, total, d, a.grad, b.grad


@pytest.mark.parametrize('weights', ['fixed', 'auto'])
def test_model_with_the_crossentropy_term_matches_the_fixture_totals(fixture, weights):
    """Fails without the feature: the token was ignored, 'crossentropy' missing from the loss dict."""
    g, cases = fixture
    config = {'training': dict(CONFIG['training'], **({'loss-weights': 'auto'} if weights == 'auto' else {}))}
    pre = 'auto_' if weights == 'auto' else ''
    for ci, fam, B, D, t, img, cap in cases:
        if B > X.MODEL_MAX_B:
            continue
        results = []
        for graphed in (False, True):
            m, total, d, d_img, d_cap = model_step(config, img, cap, t, graphed=graphed)
            assert m._graph_step is None and not m._fused_heads_ok(T(img))             # graphed=True: the composed path, nothing captured
            assert list(d) == ['matching', 'crossentropy']
            vals = g['c%d_%svals' % (ci, pre)]
            np.testing.assert_allclose([float(v.detach()) for v in d.values()], vals, **X.LOSS_TOL)
            np.testing.assert_allclose(float(total.detach()), float(g['c%d_%stotal' % (ci, pre)]), **X.LOSS_TOL)
            logged = [(k, v, n) for k, v, n in m.logger.seen if k != 'Eit']
            assert [k for k, _, _ in logged] == ['matching_loss', 'crossentropy_loss'] and [n for _, _, n in logged] == [B, B]
            np.testing.assert_allclose([v for _, v, _ in logged], vals, **X.LOSS_TOL)
            t_grad = m.crossentropy_criterion.temperature.grad
            assert t_grad is not None and tuple(t_grad.shape) == (1,)
            np.testing.assert_allclose(t_grad.item(), float(g['c%d_%sdt_total' % (ci, pre)]), rtol=1e-5, atol=1e-6 * (0.5 * np.exp(2.3) if pre else 1))
            X.assert_grad_close(d_img.cpu().numpy(), g['c%d_%sdimg_total' % (ci, pre)], fam, (ci, 'd img'))
            X.assert_grad_close(d_cap.cpu().numpy(), g['c%d_%sdcap_total' % (ci, pre)], fam, (ci, 'd cap'))
            results.append((total.detach(), d_img, d_cap, t_grad))
        for u, v in zip(*results):                                                      # the same numbers either way
            assert torch.equal(bits(u), bits(v))


def test_sharded_step_still_refuses_the_token(fixture):
    from aladin_amd.alad_model import ALADModel
    g, cases = fixture
    img, cap = T(cases[12][5]), T(cases[12][6])
    m = ALADModel(CONFIG, shard_group=None)
    with pytest.raises(NotImplementedError, match='sharded'):
        m.forward_loss_total(img, cap, img[None], cap[None], [1] * len(img), [1] * len(img), 0)


def test_out_of_range_and_bad_input_are_refused_without_a_launch():
    import ctypes as C
    from aladin_amd import _lib, ops
    lib = _lib.load()
    out = torch.full((64,), 7.0, device=dev())
    p = lambda x: C.c_void_p(x.data_ptr())                                              # noqa: E731
    B = _lib.XENT_MAX_B + 1
    rc = lib.aladin_xent_fwd_bwd(p(out), B, B, p(out), p(out), p(out), p(out), p(out), None)
    assert rc == 2 and str(_lib.XENT_MAX_B) in lib.aladin_last_error().decode()        # ALADIN_ERR_UNSUPPORTED
    assert lib.aladin_xent_fwd_bwd(p(out), 3, 4, p(out), p(out), p(out), p(out), p(out), None) == 1
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 64                                                   # nothing ran
    with pytest.raises(ValueError, match='square'):
        ops.cross_entropy_scores(torch.zeros((4, 5), device=dev()), 0.0)
    with pytest.raises(ValueError, match='one element'):
        ops.cross_entropy_scores(torch.zeros((4, 4), device=dev()), torch.zeros(2, device=dev()))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cross_entropy_scores(torch.zeros((4, 4), device=dev()), torch.zeros(1))
