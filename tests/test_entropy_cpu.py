"""CPU tier of the 'entropy' loss term (aladin_nn_entropy_fwd / _bwd, ops.nn_entropy_loss, ops.pairwise_nns_inner,
alad_model.pairwise_NNs_inner, the 'entropy' branch of ALADModel.forward_loss): the numpy restatement
(tests/helpers/entropy_numpy.py) pinned to the reference's recorded values of tests/golden/entropy.npz, the fixture's input
condition, the binding's new symbols, the drop-in signatures, and the checks that must hold before a device is touched."""
import ctypes as C
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import entropy_numpy as E                # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 2          # ALADIN_ERR_* of include/aladin_hip.h
MAX_N = 32768                            # ALADIN_NN_ENTROPY_MAX_N
# Gradients are recorded rounded to float32: 2^-24 relative; the restatement and the reference's float64 run differ by a few
# float64 roundings of the operands (<= 1, unit-norm rows), far below the absolute term.
GRAD_RTOL, GRAD_ATOL = 2.0 ** -23, 1e-12


def fixture_cases(g):
    """-> [(case index, family, B, D, seed, seed2, img, cap)] of tests/golden/entropy.npz, inputs rebuilt and checksummed."""
    from aladin_amd import synth
    out = []
    for ci, (fam, B, D, s1, s2) in enumerate(g['cases']):
        img, cap = E.case_inputs(chr(fam), int(B), int(D), int(s1), int(s2))
        for a, key in ((img, 'img'), (cap, 'cap')):
            want = float(g['c%d_%s_checksum' % (ci, key)])
            assert abs(synth.checksum(a) - want) <= 1e-6 * max(1.0, abs(want))
        out.append((ci, chr(fam), int(B), int(D), int(s1), int(s2), img, cap))
    return out


def test_fixture_covers_the_families_and_shapes_and_meets_the_gap_condition():
    g = load_golden('entropy')
    cases = fixture_cases(g)
    assert len(cases) == int(g['n_cases']) == 2 * len(E.SHAPES) + 1
    assert sorted((f, B, D) for _, f, B, D, *_ in cases if f != 'c') == sorted((f, B, D) for B, D in E.SHAPES for f in 'ab')
    assert [(f, B, D) for _, f, B, D, *_ in cases if f == 'c'] == [('c', 1, 2)]
    for ci, fam, B, D, s1, s2, img, cap in cases:
        gap = E.gaps(np.concatenate([img, cap], 0))
        assert gap.min() >= E.MIN_GAP == float(g['min_gap']), (ci, fam, B, D, gap.min())          # every row, no exception
        assert abs(gap.min() - float(g['c%d_gap' % ci])) < 1e-12
        if fam == 'b':
            assert s1 != s2
            if B >= 32:                  # neighbours in all four quadrants, several rows sharing one
                I = g['c%d_I' % ci]
                assert len({(int(i >= B), int(j >= B)) for i, j in enumerate(I)}) == 4 and 2 * B - len(set(I.tolist())) >= 3


def test_restatement_gives_the_reference_values():
    """Indices exactly; loss and gradients at float64 accuracy (gradients: at the float32 the fixture stores them in)."""
    g = load_golden('entropy')
    worst_loss = worst_grad = 0.0
    for ci, fam, B, D, s1, s2, img, cap in fixture_cases(g):
        loss, nn, dist, d_img, d_cap = E.entropy_loss(img, cap)
        assert np.array_equal(nn, g['c%d_I' % ci]) and g['c%d_I' % ci].dtype == np.int64
        assert [str(k) for k in g['c%d_keys' % ci]] == ['matching', 'entropy']
        want = float(g['c%d_vals' % ci][1])
        assert abs(loss - want) <= 1e-12 * max(1.0, abs(want)), (ci, loss, want)
        worst_loss = max(worst_loss, abs(loss - want))
        assert abs(float(g['c%d_vals_f32run' % ci][1]) - want) <= 1e-5 * abs(want) + 1e-6          # the reference's own float32 run
        cols = E.grad_columns(B, D)
        for got, key in ((d_img, 'dimg_entropy'), (d_cap, 'dcap_entropy')):
            ref = g['c%d_%s' % (ci, key)].astype(np.float64)
            assert ref.shape == got[:, cols].shape
            err = np.abs(got[:, cols] - ref)
            assert (err <= GRAD_RTOL * np.abs(ref) + GRAD_ATOL).all(), (ci, key, err.max())
            worst_grad = max(worst_grad, float((err / (np.abs(ref) + 1e-30)).max()) if ref.any() else 0.0)
        # the weighted total of the reference's forward: 1.0 * matching + 0.1 * entropy; 'auto': 0.5 * sum(L e^2.3 - 2.3)
        vals, w = g['c%d_vals' % ci], g['weights']
        assert abs(float(g['c%d_total' % ci]) - float((vals * w).sum())) <= 1e-12 * max(1.0, abs(float(g['c%d_total' % ci])))
        auto = 0.5 * float((g['c%d_auto_vals' % ci] * np.exp(2.3) - 2.3).sum())
        assert abs(float(g['c%d_auto_total' % ci]) - auto) <= 1e-5 * max(1.0, abs(auto))          # the reference's -2.3 is a float32
        assert [str(k) for k in g['c%d_logged' % ci]] == ['Eit', 'matching_loss', 'entropy-uniform-loss']
        assert g['c%d_logged_n' % ci].tolist() == [B, B]
    print('restatement vs recorded reference: worst |loss diff| %.3g, worst relative gradient diff %.3g' % (worst_loss, worst_grad))


def test_self_neighbour_case_is_finite_with_zero_gradient():
    g = load_golden('entropy')
    ci, fam, B, D, _, _, img, cap = fixture_cases(g)[0]
    assert fam == 'c' and img.tolist() == [[2.0, 0.0]] and cap.tolist() == [[-2.0, 0.0]]
    loss, nn, dist, d_img, d_cap = E.entropy_loss(img, cap)
    assert nn.tolist() == [0, 1] == g['c0_I'].tolist()
    assert np.allclose(dist, 1e-6 * np.sqrt(2), rtol=1e-12) and np.isfinite(loss)
    assert abs(loss + np.log(2 * 1e-6 * np.sqrt(2))) < 1e-12
    assert not d_img.any() and not d_cap.any() and not g['c0_dimg_entropy'].any() and not g['c0_dcap_entropy'].any()


def test_restatement_tie_rule_and_many_to_one():
    x = np.zeros((6, 4))
    x[:, 0] = [1, 1, 1, 0, 0, 0]
    x[3:, 1] = 1
    assert E.neighbours(x).tolist() == [1, 0, 0, 4, 3, 3]                # equal products: the lowest other index
    img, cap = np.array([[.5, 0, 0], [.4, .1, 0], [.3, 0, .1]]), np.array([[1.0, 0, 0], [.9, 0, 0], [.8, 0, 0]])
    loss, nn, dist, d_img, d_cap = E.entropy_loss(img, cap)
    assert nn.tolist() == [3, 3, 3, 4, 3, 3]                              # several rows share row 3
    num = np.zeros((3, 3))                                                  # central differences with the neighbours held fixed
    for r in range(3):
        for c in range(3):
            for sgn in (1, -1):
                p = cap.copy()
                p[r, c] += sgn * 1e-6
                xx = np.concatenate([img, p], 0)
                u = xx - xx[nn] + E.EPS
                num[r, c] += sgn * -np.mean(np.log(6 * np.sqrt((u * u).sum(1)))) / 2e-6
    assert np.abs(num - d_cap).max() < 1e-6


def test_new_symbols_are_bound_and_exported():
    from aladin_amd import _lib
    names = ['aladin_nn_entropy_workspace_bytes', 'aladin_nn_entropy_fwd', 'aladin_nn_entropy_bwd']
    assert [n for n in _lib.SIGNATURES if 'nn_entropy' in n] == names
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    assert _lib.ABI_VERSION == lib.aladin_version() == 13                 # added entry points do not move the version
    assert _lib.NN_ENTROPY_MAX_N == MAX_N
    hdr = open(os.path.join(ROOT, 'include', 'aladin_hip.h')).read()
    assert '#define ALADIN_NN_ENTROPY_MAX_N %d' % MAX_N in hdr


def test_entry_points_check_arguments_and_the_limit_before_touching_a_device():
    from aladin_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)

    def fwd(**kw):
        a = dict(img=p, ld_img=4, cap=p, ld_cap=4, B=2, D=4, loss=p, nn=p, dist=p, ws=p)
        a.update(kw)
        return lib.aladin_nn_entropy_fwd(a['img'], a['ld_img'], a['cap'], a['ld_cap'], a['B'], a['D'], a['loss'], a['nn'], a['dist'], a['ws'], None)

    def bwd(**kw):
        a = dict(img=p, ld_img=4, cap=p, ld_cap=4, B=2, D=4, nn=p, dist=p, g=p, d_img=p, d_cap=p)
        a.update(kw)
        return lib.aladin_nn_entropy_bwd(a['img'], a['ld_img'], a['cap'], a['ld_cap'], a['B'], a['D'], a['nn'], a['dist'], a['g'], a['d_img'],
                                         a['d_cap'], None)
    for kw in ({'img': null}, {'B': 0}, {'D': 0}, {'ld_img': 3}, {'ld_cap': 3}, {'nn': null}, {'dist': null}, {'ws': null}):
        assert fwd(**kw) == ERR_ARG, kw
        assert b'nn_entropy_fwd' in lib.aladin_last_error()
    for kw in ({'img': null}, {'B': 0}, {'D': 0}, {'ld_img': 3}, {'nn': null}, {'dist': null}, {'g': null}, {'d_img': null}, {'d_cap': null}):
        assert bwd(**kw) == ERR_ARG, kw
        assert b'nn_entropy_bwd' in lib.aladin_last_error()
    # the limit, named: N = 2 B with two sources, N = B with cap NULL
    for call, kw in ((fwd, {'B': MAX_N // 2 + 1}), (bwd, {'B': MAX_N // 2 + 1}), (fwd, {'B': MAX_N + 1, 'cap': null}), (bwd, {'B': MAX_N + 1, 'cap': null})):
        assert call(ld_img=4, **kw) == ERR_UNSUPPORTED, kw
        msg = lib.aladin_last_error().decode()
        assert 'nn_entropy' in msg and str(MAX_N) in msg and str(kw['B'] * (1 if 'cap' in kw else 2)) in msg, msg
    ws = lib.aladin_nn_entropy_workspace_bytes
    assert ws(0) == ws(-1) == ws(MAX_N + 1) == 0
    assert ws(2) >= 2 * 2 * 8 + 2 * 4 and ws(130) >= 130 * 4 * 8 + 130 * 4 and ws(MAX_N) >= MAX_N * 512 * 8 + MAX_N * 4
    assert all(ws(n) <= ws(n + 1) for n in (1, 2, 63, 64, 127, 128, 129, 1000))


def test_ops_refuse_bad_input_before_the_device():
    from aladin_amd import ops
    from aladin_amd.alad_model import pairwise_NNs_inner
    x = torch.zeros((4, 8))
    for call in (lambda: ops.nn_entropy_loss(x, x), lambda: ops.pairwise_nns_inner(x), lambda: pairwise_NNs_inner(x)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    with pytest.raises(TypeError):
        ops.pairwise_nns_inner(x.numpy())


def test_drop_in_signatures_match_the_reference():
    """The rule of test_boundary_cpu.test_drop_in_signatures_match_the_reference for the two callables of this term."""
    from aladin_amd import alad_model as M
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'signatures_entropy.json')))
    homes = {'pairwise_NNs_inner': M.pairwise_NNs_inner, 'ALADModel.forward_loss': M.ALADModel.forward_loss}
    assert set(ref) == set(homes)
    for key, want in ref.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(homes[key]).parameters.values()]
        assert got[:len(want)] == want, (key, got, want)
        for extra in got[len(want):]:
            assert extra[2] is not None or extra[1] in ('VAR_POSITIONAL', 'VAR_KEYWORD'), (key, 'extra parameter without a default', extra)
    assert ref['pairwise_NNs_inner'] == [['x', 'POSITIONAL_OR_KEYWORD', None]]
    assert ref['ALADModel.forward_loss'] == json.load(open(os.path.join(ROOT, 'tests', 'golden', 'signatures.json')))['ALADModel.forward_loss']


def test_model_accepts_the_loss_type_and_the_sharded_step_still_refuses_it():
    """Construction and the routing decisions that need no device: the fused heads and the graphed step do not cover the term, and the
    sharded step refuses the configuration before it touches a process group or a tensor."""
    from aladin_amd.alad_model import ALADModel
    cfg = {'training': {'loss-type': 'matching-entropy', 'loss-weights': [1.0, 0.1], 'margin': 0.2, 'measure': 'dot', 'max-violation': True}}
    m = ALADModel(cfg, graphed=True)
    assert m.losses_types == ['matching', 'entropy'] and m.losses_weights == {'matching': 1.0, 'entropy': 0.1}
    x = torch.zeros((4, 8), requires_grad=True)
    assert not m._fused_heads_ok(x)
    assert not m._graph_heads_now(x, x, x[None], x[None], True)
    sharded = ALADModel(cfg, shard_group=None)
    with pytest.raises(NotImplementedError, match='sharded'):
        sharded.forward_loss_total(x, x, x[None], x[None], [1] * 4, [1] * 4, 0)
