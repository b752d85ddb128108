"""GPU tier (-m gpu): the 'entropy' loss term -- aladin_nn_entropy_fwd / _bwd (csrc/entropy.hip) through ops.nn_entropy_loss,
ops.pairwise_nns_inner, alad_model.pairwise_NNs_inner and ALADModel with loss-type 'matching-entropy'.

Against the reference's recorded values (tests/golden/entropy.npz, its float64 run; make_golden_entropy.py): neighbours exactly,
on inputs whose best and second-best products differ by >= 1e-4 in every row (asserted again here, in float64; fp32 summation noise
of unit-norm rows is ~1e-7), loss within rtol 1e-5 / atol 1e-6, gradients within rtol 1e-4 / atol 1e-6 -- the figures of the
project's exact-fp32 heads (test_gpu_parity.test_matching_head).  Where the fixture keeps every 4th gradient column only, the whole
gradient is also held to the float64 restatement (tests/helpers/entropy_numpy.py, pinned to the fixture by the CPU tier)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import entropy_numpy as E                # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)
CONFIG = {'training': {'loss-type': 'matching-entropy', 'loss-weights': [1.0, 0.1], 'margin': 0.2, 'measure': 'dot', 'max-violation': True}}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())


def bits(v):
    return v.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def fixture():
    """(golden, [(case index, family, B, D, img, cap)]): inputs rebuilt from the recorded seeds, checksums and the gap condition checked."""
    from aladin_amd import synth
    g = load_golden('entropy')
    cases = []
    for ci, (fam, B, D, s1, s2) in enumerate(g['cases']):
        img, cap = E.case_inputs(chr(fam), int(B), int(D), int(s1), int(s2))
        for a, key in ((img, 'img'), (cap, 'cap')):
            want = float(g['c%d_%s_checksum' % (ci, key)])
            assert abs(synth.checksum(a) - want) <= 1e-6 * max(1.0, abs(want))
        assert E.gaps(np.concatenate([img, cap], 0)).min() >= E.MIN_GAP                   # every row of every case
        cases.append((ci, chr(fam), int(B), int(D), img, cap))
    assert len(cases) == 2 * len(E.SHAPES) + 1
    return g, cases


def run_op(img, cap, g=None):
    """ops.nn_entropy_loss forward + backward -> (loss, nn, d_img, d_cap) tensors"""
    from aladin_amd import ops
    a, b = img.detach().requires_grad_(True), cap.detach().requires_grad_(True)
    loss, nn = ops.nn_entropy_loss(a, b, return_neighbours=True)
    (loss if g is None else loss * g).backward()
    return loss.detach(), nn, a.grad, b.grad


def test_every_fixture_case_matches_the_reference(fixture):
    from aladin_amd import ops
    from aladin_amd.alad_model import pairwise_NNs_inner
    g, cases = fixture
    for ci, fam, B, D, img, cap in cases:
        loss, nn, d_img, d_cap = run_op(T(img), T(cap))
        assert nn.dtype == torch.int64 and np.array_equal(nn.cpu().numpy(), g['c%d_I' % ci]), (ci, fam, B, D)
        want = float(g['c%d_vals' % ci][1])
        print('entropy case %2d %s (%3d, %3d): loss %.7f  reference %.7f  |diff| %.2e' % (ci, fam, B, D, loss.item(), want, abs(loss.item() - want)))
        np.testing.assert_allclose(loss.item(), want, **LOSS_TOL)
        cols = E.grad_columns(B, D)
        _, _, _, r_img, r_cap = E.entropy_loss(img, cap)
        for got, key, rest in ((d_img, 'dimg_entropy', r_img), (d_cap, 'dcap_entropy', r_cap)):
            got = got.cpu().numpy()
            ref = g['c%d_%s' % (ci, key)]
            print('   %s: max |err| %.2e  max |ref| %.2e' % (key, np.abs(got[:, cols] - ref).max(), np.abs(ref).max()))
            np.testing.assert_allclose(got[:, cols], ref, **GRAD_TOL)
            np.testing.assert_allclose(got, rest, **GRAD_TOL)
        # the reference's helper on the concatenated matrix: one source, odd splits of the tiles
        x = torch.cat([T(img), T(cap)], 0)
        for fn in (ops.pairwise_nns_inner, pairwise_NNs_inner):
            I = fn(x)
            assert I.dtype == torch.int64 and np.array_equal(I.cpu().numpy(), g['c%d_I' % ci]), (ci, fn)
    # an upstream gradient other than 1 scales the input gradients
    ci, fam, B, D, img, cap = cases[4]
    _, _, s_img, s_cap = run_op(T(img), T(cap), g=-2.5)
    _, _, _, r_img, r_cap = E.entropy_loss(img, cap, g=-2.5)
    np.testing.assert_allclose(s_img.cpu().numpy(), r_img, **GRAD_TOL)
    np.testing.assert_allclose(s_cap.cpu().numpy(), r_cap, **GRAD_TOL)


def test_two_runs_give_the_same_bits(fixture):
    from aladin_amd.ops_losses import _nn_entropy_raw
    g, cases = fixture
    for ci, fam, B, D, img, cap in cases:
        if (B, D) not in ((33, 70), (96, 768), (130, 100)):
            continue
        a, b = T(img), T(cap)
        first, second = run_op(a, b), run_op(a, b)
        assert torch.equal(first[1], second[1])
        for u, v in zip(first[::2] + first[3:], second[::2] + second[3:]):
            assert torch.equal(bits(u), bits(v))
        r1, r2 = _nn_entropy_raw(a, b, True), _nn_entropy_raw(a, b, True)
        assert torch.equal(bits(r1[0]), bits(r2[0])) and torch.equal(r1[1], r2[1]) and torch.equal(bits(r1[2]), bits(r2[2]))
        assert torch.equal(bits(r1[0]), bits(first[0])) and torch.equal(r1[1].long(), first[1])
        _, nn, dist, _, _ = E.entropy_loss(img, cap)
        np.testing.assert_allclose(r1[2].cpu().numpy(), dist, rtol=1e-5, atol=0)


def test_ties_go_to_the_lowest_index():
    """One vector at three positions spanning two column tiles (and both sources): every other row whose neighbour is that vector
    reports the lowest of the three, and the copies report each other -- the lowest other copy."""
    from aladin_amd import ops, synth
    B, D = 100, 48
    img, cap = synth.global_embeddings(B, D, 72, 1.0)
    dup = (5, 70, B + 30)                                              # column tiles 0 and 1 of img, tile 0 of cap
    x = np.concatenate([img, cap], 0)
    v = x[dup[0]].copy()
    x[:, :] = 0.5 * x + 0.5 * v                                        # pull every row towards v: it is the neighbour of many
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = x.astype(np.float32)
    for p in dup:
        x[p] = x[dup[0]]
    want = E.neighbours(x)                                             # numpy's argmax: the first maximum
    others = [i for i in range(2 * B) if i not in dup]
    to_dup = [i for i in others if want[i] in dup]
    assert len(to_dup) >= 20 and all(want[i] == dup[0] for i in to_dup)
    assert [want[p] for p in dup] == [dup[1], dup[0], dup[0]]
    gap = E.gaps(np.delete(x, dup[1:], axis=0))                        # without the copies every row's decision is clear of fp32 noise
    assert gap.min() >= E.MIN_GAP, gap.min()
    a, b = T(x[:B]), T(x[B:])
    _, nn = ops.nn_entropy_loss(a, b, return_neighbours=True)
    assert np.array_equal(nn.cpu().numpy(), want)
    assert np.array_equal(ops.pairwise_nns_inner(torch.cat([a, b], 0)).cpu().numpy(), want)


def test_self_neighbour_case(fixture):
    g, cases = fixture
    ci, fam, B, D, img, cap = cases[0]
    assert fam == 'c'
    loss, nn, d_img, d_cap = run_op(T(img), T(cap))
    assert nn.tolist() == [0, 1] == g['c0_I'].tolist()
    assert np.isfinite(loss.item())
    np.testing.assert_allclose(loss.item(), float(g['c0_vals'][1]), **LOSS_TOL)
    assert d_img.tolist() == [[0.0, 0.0]] and d_cap.tolist() == [[0.0, 0.0]]             # exactly, as autograd's
    _, _, s_img, s_cap = run_op(T(img), T(cap), g=3.0)
    assert not s_img.any() and not s_cap.any()


def test_strided_inputs_give_the_result_of_their_contiguous_copies(fixture):
    g, cases = fixture
    ci, fam, B, D, img, cap = next(c for c in cases if c[1] == 'b' and c[2:4] == (33, 70))
    base = run_op(T(img), T(cap))
    wide_i, wide_c = torch.zeros((B, 2 * D + 3), device=dev()), torch.zeros((2 * B, D), device=dev())
    wide_i[:, 3:3 + D] = T(img)
    wide_c[::2] = T(cap)
    rows_i, rows_c = wide_i[:, 3:3 + D], wide_c[::2]                   # row-strided views, unit column stride
    assert not rows_i.is_contiguous() and not rows_c.is_contiguous() and rows_i.stride(1) == 1
    cols_i = torch.zeros((B, 2 * D), device=dev())
    cols_i[:, ::2] = T(img)
    cols_i = cols_i[:, ::2]                                            # a column slice: stride 2 along D
    assert cols_i.stride(1) == 2
    for a, b in ((rows_i, rows_c), (cols_i, T(cap)), (cols_i, rows_c)):
        got = run_op(a, b)
        assert torch.equal(got[1], base[1])
        for u, v in zip(got[::2] + got[3:], base[::2] + base[3:]):
            assert torch.equal(bits(u), bits(v))


def test_forward_and_backward_replay_in_a_graph(fixture):
    from aladin_amd import ops
    g, cases = fixture
    by_key = {(c[1], c[2], c[3]): c for c in cases}
    first, second = by_key[('a', 32, 64)], by_key[('b', 32, 64)]
    a, b = T(first[4]).requires_grad_(True), T(first[5]).requires_grad_(True)
    out = {}

    def run():
        loss, nn = ops.nn_entropy_loss(a, b, return_neighbours=True)
        out['loss'], out['nn'] = loss.detach(), nn
        out['d_img'], out['d_cap'] = torch.autograd.grad(loss, (a, b))
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        run()                                                             # warm-up outside the capture (one-time kernel attributes)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for case in (second, first):                                          # fresh contents twice
        with torch.no_grad():
            a.copy_(T(case[4]))
            b.copy_(T(case[5]))
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.clone() for k, v in out.items()}
        eager = run_op(a, b)
        assert torch.equal(replayed['nn'], eager[1]) and np.array_equal(eager[1].cpu().numpy(), g['c%d_I' % case[0]])
        for k, v in (('loss', eager[0]), ('d_img', eager[2]), ('d_cap', eager[3])):
            assert torch.equal(bits(replayed[k]), bits(v)), k
        np.testing.assert_allclose(replayed['loss'].item(), float(g['c%d_vals' % case[0]][1]), **LOSS_TOL)


class _Log:
    """the part of the reference's LogCollector that forward_loss uses"""

    def __init__(self):
        self.seen = []

    def update(self, k, v, n=0):
        self.seen.append((k, v, n))


def model_step(config, img, cap, **kw):
    from aladin_amd.alad_model import ALADModel
    B, D = img.shape
    m = ALADModel(config, **kw)
    m.logger = _Log()
    a, b = T(img).requires_grad_(True), T(cap).requires_grad_(True)
    sets = (a, b, torch.zeros((1, B, D), device=dev()), torch.zeros((1, B, D), device=dev()), [1] * B, [1] * B, 0)
    m.forward_emb = lambda x, y: sets
    total, d = m(None, None, epoch=0, distill_epoch=2)
    total.sum().backward()
    torch.cuda.synchronize()
    return m, total, d, a.grad, b.grad


@pytest.mark.parametrize('weights', ['fixed', 'auto'])
def test_model_with_the_entropy_term_matches_the_reference(fixture, weights):
    """Fails without the feature: forward_loss raised NotImplementedError for 'entropy'."""
    g, cases = fixture
    config = {'training': dict(CONFIG['training'], **({'loss-weights': 'auto'} if weights == 'auto' else {}))}
    pre = 'auto_' if weights == 'auto' else ''
    for ci, fam, B, D, img, cap in cases:
        if B > E.MODEL_MAX_B:
            continue
        results = []
        for graphed in (False, True):
            m, total, d, d_img, d_cap = model_step(config, img, cap, graphed=graphed)
            assert m._graph_step is None and not m._fused_heads_ok(T(img))            # graphed=True: the eager fallback, nothing captured
            assert list(d) == [str(k) for k in g['c%d_keys' % ci]] == ['matching', 'entropy']
            vals = g['c%d_%svals' % (ci, pre)]
            np.testing.assert_allclose([float(v.detach()) for v in d.values()], vals, **LOSS_TOL)
            np.testing.assert_allclose(float(total.detach()), float(g['c%d_%stotal' % (ci, pre)]), **LOSS_TOL)
            assert ['Eit'] + [k for k, _, _ in m.logger.seen if k != 'Eit'] == [str(k) for k in g['c%d_logged' % ci]]
            logged = [(v, n) for k, v, n in m.logger.seen if k != 'Eit']
            np.testing.assert_allclose([v for v, _ in logged], vals, **LOSS_TOL)
            assert [n for _, n in logged] == g['c%d_logged_n' % ci].tolist() == [B, B]
            np.testing.assert_allclose(d_img.cpu().numpy(), g['c%d_%sdimg_total' % (ci, pre)], **GRAD_TOL)
            np.testing.assert_allclose(d_cap.cpu().numpy(), g['c%d_%sdcap_total' % (ci, pre)], **GRAD_TOL)
            results.append((total.detach(), d_img, d_cap))
        for u, v in zip(*results):                                                      # the same numbers either way
            assert torch.equal(bits(u), bits(v))


def test_sharded_step_still_refuses_the_term(fixture):
    from aladin_amd.alad_model import ALADModel
    g, cases = fixture
    img, cap = T(cases[3][4]), T(cases[3][5])
    m = ALADModel(CONFIG, shard_group=None)
    with pytest.raises(NotImplementedError, match='sharded'):
        m.forward_loss_total(img, cap, img[None], cap[None], [1] * len(img), [1] * len(img), 0)


def test_out_of_range_is_refused_without_a_launch():
    from aladin_amd import _lib, ops
    lib = _lib.load()
    B = _lib.NN_ENTROPY_MAX_N // 2 + 1
    x = torch.zeros((B, 1), device=dev())
    out = torch.full((4,), 7.0, device=dev())
    p = lambda t: C.c_void_p(t.data_ptr())                                              # noqa: E731
    rc = lib.aladin_nn_entropy_fwd(p(x), 1, p(x), 1, B, 1, p(out), p(out), p(out), p(out), None)
    assert rc == 2 and str(_lib.NN_ENTROPY_MAX_N) in lib.aladin_last_error().decode()          # ALADIN_ERR_UNSUPPORTED
    rc = lib.aladin_nn_entropy_bwd(p(x), 1, p(x), 1, B, 1, p(out), p(out), p(out), p(x), p(x), None)
    assert rc == 2
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 4 and not x.any()                                    # nothing ran
    with pytest.raises(ValueError, match=str(_lib.NN_ENTROPY_MAX_N)):
        ops.nn_entropy_loss(x, x)
    with pytest.raises(ValueError, match=str(_lib.NN_ENTROPY_MAX_N)):
        ops.pairwise_nns_inner(torch.zeros((_lib.NN_ENTROPY_MAX_N + 1, 1), device=dev()))
    one = ops.pairwise_nns_inner(torch.ones((1, 3), device=dev()))                      # N = 1: the row is its own neighbour
    assert one.tolist() == [0]
