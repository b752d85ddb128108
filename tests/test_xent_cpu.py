"""CPU tier of the cross-entropy (InfoNCE) criterion (aladin_xent_fwd_bwd, ops.cross_entropy_scores, ops.match_cross_entropy,
loss.CrossEntropyCriterion, loss.AlignmentCrossEntropyLoss, the 'crossentropy' token of ALADModel): the float64 restatement
(tests/helpers/xent_numpy.py) pinned to the reference's recorded float64 run of tests/golden/xent.npz, the fixture's coverage and
input condition, the float32 floor behind the GPU tier's gradient gate, the binding's new symbols, the drop-in signatures, and the
checks that must hold before a device is touched."""
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
import xent_numpy as X                   # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 2          # ALADIN_ERR_* of include/aladin_hip.h
MAX_B = 32768                            # ALADIN_XENT_MAX_B


def fixture_cases(g):
    """-> [(case index, family, B, D, t, img, cap)] of tests/golden/xent.npz, inputs rebuilt from the seeds and checksummed."""
    from aladin_amd import synth
    out = []
    for ci, ((fam, B, D, s1, s2), t) in enumerate(zip(g['cases'], g['temperatures'])):
        fam = X.FIXTURE_FAMILIES[int(fam)]
        img, cap = X.case_inputs(fam, int(B), int(D), int(s1), int(s2))
        for a, key in ((img, 'img'), (cap, 'cap')):
            want = float(g['c%d_%s_checksum' % (ci, key)])
            assert abs(synth.checksum(a) - want) <= 1e-6 * max(1.0, abs(want))
        out.append((ci, fam, int(B), int(D), float(t), img, cap))
    return out


def test_fixture_covers_the_shapes_temperatures_and_families_and_meets_the_mass_condition():
    g = load_golden('xent')
    cases = fixture_cases(g)
    assert len(cases) == int(g['n_cases']) == len(X.SHAPES) * len(X.TEMPERATURES) * len(X.FIXTURE_FAMILIES)
    assert [(f, B, D, t) for _, f, B, D, t, _, _ in cases] == [c[:4] for c in X.fixture_cases()]
    assert X.SHAPES == [(1, 8), (2, 8), (5, 30), (33, 64), (65, 768)]
    assert X.TEMPERATURES == (0.0, 1.5, float(np.float32(np.log(100.0))))
    assert float(g['min_top_mass']) == X.MIN_TOP_MASS and float(g['matched_noise']) == X.MATCHED_NOISE
    for ci, fam, B, D, t, img, cap in cases:
        mass = X.offdiag_mass(img.astype(np.float64) @ cap.astype(np.float64).T, t)
        assert abs(mass.max() - float(g['c%d_top_mass' % ci])) <= 1e-12
        assert B == 1 or mass.max() >= X.MIN_TOP_MASS, (ci, fam, B, D, t, mass.max())
        assert g['c%d_dimg' % ci].dtype == np.float32 and g['c%d_dimg' % ci].shape == img[:, X.grad_columns(B, D)].shape
        assert ('c%d_total' % ci in g) == (B <= X.MODEL_MAX_B) == ('c%d_auto_total' % ci in g)
    # the sharp case: every diagonal dominates; in float32 a diagonal gradient formed as softmax - 1 (rounded at 6e-8 absolute) would
    # be off by a part in a thousand on most lines and lost on the sharpest
    ci, fam, B, D, t, img, cap = cases[-2]
    assert (fam, B, D, t) == ('matched', 65, 768, X.LN100)
    mass = X.offdiag_mass(img.astype(np.float64) @ cap.astype(np.float64).T, t)
    assert mass.max() < 0.05 and np.median(mass) < 6e-5 and mass.min() < 2.0 ** -25


def test_restatement_gives_the_reference_values():
    """loss and dt to 1e-12 relative, gradients to 1e-12 of their largest entry (the fixture stores them as float32: 2^-24 relative
    on top)."""
    g = load_golden('xent')
    worst = dict(loss=0.0, dt=0.0, grad=0.0)
    for ci, fam, B, D, t, img, cap in fixture_cases(g):
        loss, d_im, d_s, dt, _ = X.criterion_f64(img, cap, t)
        for got, key in ((loss, 'loss'), (dt, 'dt')):
            want = float(g['c%d_%s' % (ci, key)])
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (ci, key, got, want)
            worst[key] = max(worst[key], abs(got - want) / max(1.0, abs(want)))
        f32run = g['c%d_f32run' % ci]                                      # the reference's own float32 run, for orientation
        np.testing.assert_allclose(f32run, [float(g['c%d_loss' % ci]), float(g['c%d_dt' % ci])], rtol=1e-4, atol=1e-6)
        cols = X.grad_columns(B, D)
        for got, key in ((d_im, 'dimg'), (d_s, 'dcap')):
            ref = g['c%d_%s' % (ci, key)].astype(np.float64)
            top = max(np.abs(got).max(), 1e-300)
            err = np.abs(got[:, cols] - ref)
            assert (err <= 2.0 ** -23 * np.abs(ref) + 1e-12 * top).all(), (ci, key, err.max(), top)
            worst['grad'] = max(worst['grad'], float(((err - 2.0 ** -23 * np.abs(ref)).clip(0) / top).max()))
        if B == 1:
            assert loss == 0.0 and dt == 0.0 and not d_im.any() and not d_s.any()
            assert float(g['c%d_loss' % ci]) == 0.0 and float(g['c%d_dt' % ci]) == 0.0 and not g['c%d_dimg' % ci].any()
    print('restatement vs recorded reference: worst relative diff %r' % (worst,))


def test_model_totals_of_the_fixture_follow_the_weighting_rule():
    g = load_golden('xent')
    assert str(g['model_loss_type']) == X.MODEL_LOSS_TYPE == 'matching-crossentropy' and g['model_weights'].tolist() == X.MODEL_WEIGHTS == [1.0, 0.5]
    n = 0
    for ci, fam, B, D, t, img, cap in fixture_cases(g):
        if B > X.MODEL_MAX_B:
            continue
        n += 1
        vals = g['c%d_vals' % ci]
        assert abs(vals[1] - float(g['c%d_loss' % ci])) <= 1e-15 and np.array_equal(vals, g['c%d_auto_vals' % ci])
        assert abs(float(g['c%d_total' % ci]) - float((vals * g['model_weights']).sum())) <= 1e-12 * max(1.0, abs(float(g['c%d_total' % ci])))
        auto = 0.5 * float((vals * np.exp(2.3) - 2.3).sum())
        assert abs(float(g['c%d_auto_total' % ci]) - auto) <= 1e-12 * max(1.0, abs(auto))
        # d total / d temperature = the term's weight times the criterion's dt
        assert abs(float(g['c%d_dt_total' % ci]) - 0.5 * float(g['c%d_dt' % ci])) <= 1e-12 * max(1.0, abs(float(g['c%d_dt' % ci])))
        assert abs(float(g['c%d_auto_dt_total' % ci]) - 0.5 * np.exp(2.3) * float(g['c%d_dt' % ci])) <= 1e-11 * max(1.0, abs(float(g['c%d_dt' % ci])))
    assert n == 24


def test_float32_floor_is_within_its_recorded_value():
    """The distance of the plain float32 restatement from float64, per family: the live measurement stays under the constant the
    GPU tier's gradient gate is derived from (XENT_A = 4 x)."""
    worst = {fam: 0.0 for fam in X.XENT_FLOOR}
    for fam in X.FAMILIES:
        for B in X.SIZES:
            S, t = X.matrix_inputs(B, fam)
            l64, d64, t64 = X.xent_f64(S, t)
            l32, d32, t32 = X.xent_f32(S, t)
            r = X.floor_ratio(d32, d64)
            print('floor %-7s B %4d: dS %.3g of max|dS| %.3g;  |loss diff| %.2e of %.6g;  |dt diff| %.2e of %.6g' % (
                fam, B, r, np.abs(d64).max(), abs(l32 - l64), l64, abs(t32 - t64), t64))
            np.testing.assert_allclose(l32, l64, **X.LOSS_TOL)
            np.testing.assert_allclose(t32, t64, **X.LOSS_TOL)
            worst[fam] = max(worst[fam], r)
    for fam, B, D, t, s1, s2 in X.fixture_cases():
        img, cap = X.case_inputs(fam, B, D, s1, s2)
        r64, r32 = X.criterion_f64(img, cap, t), X.criterion_f32(img, cap, t)
        r = max(X.floor_ratio(r32[1], r64[1]), X.floor_ratio(r32[2], r64[2]))
        print('floor %-11s (%2d, %3d) t %.4f: d im / d s %.3g' % (fam, B, D, t, r))
        np.testing.assert_allclose(r32[0], r64[0], **X.LOSS_TOL)
        np.testing.assert_allclose(r32[3], r64[3], **X.LOSS_TOL)
        worst[fam] = max(worst[fam], r)
    print('worst floors %r, recorded %r' % (worst, X.XENT_FLOOR))
    for fam, v in worst.items():
        assert 0.5 * X.XENT_FLOOR[fam] < v <= X.XENT_FLOOR[fam], (fam, v, X.XENT_FLOOR[fam])      # recorded close above the measurement
    assert X.XENT_A == {fam: 4 * v for fam, v in X.XENT_FLOOR.items()}


def test_restatement_properties():
    """B = 1 is exactly zero; the gradient is that of the loss (central differences); NaN in, NaN out; the sharp family's
    diagonal balances its rows (no cancellation in either restatement)."""
    for fn in (X.xent_f64, X.xent_f32):
        loss, dS, dt = fn(np.array([[0.37]], np.float32), 1.5)
        assert loss == 0 and dt == 0 and not dS.any()
    S, t = X.matrix_inputs(5, 'mild')[0].astype(np.float64), 0.7
    loss, dS, dt = X.xent_f64(S, t, g=2.5)
    num = np.zeros_like(S)
    for i in range(5):
        for j in range(5):
            for sgn in (1, -1):
                P = S.copy()
                P[i, j] += sgn * 1e-6
                num[i, j] += sgn * 2.5 * X.xent_f64(P, t)[0] / 2e-6
    assert np.abs(num - dS).max() < 1e-8
    assert abs(2.5 * (X.xent_f64(S, t + 1e-6)[0] - X.xent_f64(S, t - 1e-6)[0]) / 2e-6 - dt) < 1e-8
    bad = S.copy()
    bad[1, 3] = np.nan
    assert np.isnan(X.xent_f64(bad, t)[0])
    S, t = X.matrix_inputs(65, 'sharp')
    for fn, tol in ((X.xent_f64, 1e-12), (X.xent_f32, 1e-5)):
        dS = np.asarray(fn(S, t)[1], np.float64)
        assert np.abs(dS).max() > 0 and np.abs(dS.sum()) <= tol * np.abs(dS).sum()          # sum_ij dL_ij = 0
        assert (np.diag(dS) < 0).all()


def test_new_symbols_are_declared_exported_and_bound():
    from aladin_amd import _lib
    names = ['aladin_xent_workspace_bytes', 'aladin_xent_fwd_bwd']
    assert [n for n in _lib.SIGNATURES if 'xent' in n] == names
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    assert _lib.ABI_VERSION == lib.aladin_version() == 13                 # added entry points do not move the version
    assert _lib.XENT_MAX_B == MAX_B
    hdr = open(os.path.join(ROOT, 'include', 'aladin_hip.h')).read()
    assert '#define ALADIN_XENT_MAX_B %d' % MAX_B in hdr and '#define ALADIN_ABI_VERSION 13' in hdr.replace('  ', ' ')
    assert 'ALADIN_API size_t aladin_xent_workspace_bytes(int B);' in hdr and 'ALADIN_API int aladin_xent_fwd_bwd(const float* S,' in hdr
    mk = open(os.path.join(ROOT, 'aladin_amd', 'csrc', 'Makefile')).read()
    assert ' xent.hip ' in next(line for line in mk.splitlines() if line.startswith('SRCS'))
    assert 'aladin_*' in open(os.path.join(ROOT, 'aladin_amd', 'csrc', 'exports.map')).read()


def _aligned_host_pointer(keep):
    buf = (C.c_char * 4096)()
    keep.append(buf)
    return C.c_void_p((C.addressof(buf) + 255) // 256 * 256)


def test_entry_point_checks_arguments_and_the_limit_before_touching_a_device():
    from aladin_amd import _lib
    lib = _lib.load()
    keep = []
    p, null = _aligned_host_pointer(keep), C.c_void_p(0)

    def call(**kw):
        a = dict(S=p, ld=4, B=4, t=p, loss=p, dS=p, dt=p, ws=p)
        a.update(kw)
        return lib.aladin_xent_fwd_bwd(a['S'], a['ld'], a['B'], a['t'], a['loss'], a['dS'], a['dt'], a['ws'], None)
    for kw in ({'S': null}, {'t': null}, {'loss': null}, {'ws': null}, {'B': 0}, {'B': -3}, {'ld': 3}, {'ws': C.c_void_p(p.value + 4)}):
        assert call(**kw) == ERR_ARG, kw
        assert b'xent_fwd_bwd' in lib.aladin_last_error()
    assert call(B=MAX_B + 1, ld=MAX_B + 1) == ERR_UNSUPPORTED
    msg = lib.aladin_last_error().decode()
    assert 'xent' in msg and str(MAX_B) in msg and str(MAX_B + 1) in msg, msg
    assert call(B=MAX_B + 1, ld=4) == ERR_ARG                               # the argument check comes first
    ws = lib.aladin_xent_workspace_bytes
    assert ws(0) == ws(-1) == ws(MAX_B + 1) == 0
    assert all(ws(b) >= 2 * b * 24 for b in (1, 2, 65, 1500, MAX_B))      # per line: a float4 of statistics and a float2 of shares
    assert all(ws(b) < ws(b + 1) for b in (1, 2, 63, 64, 65, 1000))


def test_ops_and_modules_refuse_cpu_tensors_and_non_square_input():
    from aladin_amd import ops
    from aladin_amd.loss import AlignmentCrossEntropyLoss, CrossEntropyCriterion
    x, sq = torch.zeros((4, 8)), torch.zeros((4, 4))
    sets, seq = torch.zeros((4, 5, 8)), torch.zeros((4, 7, 8))
    crit, acrit = CrossEntropyCriterion(), AlignmentCrossEntropyLoss()
    for call in (lambda: ops.cross_entropy_scores(sq, 0.0), lambda: ops.cross_entropy_scores(sq, torch.zeros(1)),
                 lambda: ops.match_cross_entropy(x, x, 0.0), lambda: ops.match_cross_entropy(x, x, torch.zeros(1), return_scores=True),
                 lambda: crit(x, x), lambda: acrit(sets, seq, [5] * 4, [7] * 4)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    for call in (lambda: ops.cross_entropy_scores(torch.zeros((4, 5)), 0.0), lambda: ops.cross_entropy_scores(torch.zeros(4), 0.0),
                 lambda: ops.cross_entropy_scores(torch.zeros((0, 0)), 0.0),
                 lambda: ops.match_cross_entropy(x, torch.zeros((5, 8)), 0.0), lambda: ops.match_cross_entropy(x, torch.zeros((4, 9)), 0.0),
                 lambda: crit(x, torch.zeros((3, 8))), lambda: acrit(sets, seq[:3], [5] * 4, [7] * 3)):
        with pytest.raises(ValueError, match='square'):
            call()
    with pytest.raises(TypeError):
        ops.cross_entropy_scores(sq.numpy(), 0.0)
    with pytest.raises(TypeError):
        ops.match_cross_entropy(x.numpy(), x, 0.0)
    with pytest.raises(ValueError, match='aggregation'):
        AlignmentCrossEntropyLoss(aggregation='nope')
    assert acrit.aggregation == 'MrAVGw' and 'not in the reference' in AlignmentCrossEntropyLoss.__doc__.lower()


def test_drop_in_signatures_and_state_dict_match_the_reference():
    """The rule of test_boundary_cpu.test_drop_in_signatures_match_the_reference for the criterion's two callables."""
    from aladin_amd import loss as L
    from aladin_amd.loss import AlignmentCrossEntropyLoss, CrossEntropyCriterion
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'signatures_xent.json')))
    homes = {'CrossEntropyCriterion.__init__': L.CrossEntropyCriterion.__init__, 'CrossEntropyCriterion.forward': L.CrossEntropyCriterion.forward}
    assert set(ref) == set(homes)
    for key, want in ref.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(homes[key]).parameters.values()]
        assert got == want, (key, got, want)
    assert ref['CrossEntropyCriterion.forward'] == [[n, 'POSITIONAL_OR_KEYWORD', None] for n in ('self', 'im', 's')]
    for crit in (CrossEntropyCriterion(), AlignmentCrossEntropyLoss()):
        sd = crit.state_dict()
        assert list(sd) == ['temperature'] and tuple(sd['temperature'].shape) == (1,) and sd['temperature'].tolist() == [0.0]
        assert crit.temperature.requires_grad and crit.temperature.dtype == torch.float32
        crit.load_state_dict({'temperature': torch.tensor([1.25])})          # a reference state dict loads unchanged
        assert crit.temperature.tolist() == [1.25]
    params = list(inspect.signature(AlignmentCrossEntropyLoss.forward).parameters)
    assert params == ['self', 'im_set', 's_seq', 'im_len', 's_len', 'return_similarity_mat']
    assert inspect.signature(AlignmentCrossEntropyLoss.__init__).parameters['aggregation'].default == 'MrAVGw'


class _Log:
    def __init__(self):
        self.seen = []

    def update(self, k, v, n=0):
        self.seen.append((k, v, n))


class _StubMatching(torch.nn.Module):
    """a matching criterion without `.sim`: forward_loss calls it directly instead of the small-batch HIP node"""

    def forward(self, im, s, return_similarity_mat=False):
        loss = (im * s).sum() * 0 + 3.0
        return (loss, im @ s.t()) if return_similarity_mat else loss


class _StubCrossEntropy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.temperature = torch.nn.Parameter(torch.zeros(1))
        self.calls = 0

    def forward(self, im, s):
        self.calls += 1
        return (7.0 * torch.exp(self.temperature)).sum()


def _stub_model(loss_type, weights, **kw):
    from aladin_amd.alad_model import ALADModel
    cfg = {'training': {'loss-type': loss_type, 'loss-weights': weights, 'margin': 0.2, 'measure': 'dot', 'max-violation': True}}
    m = ALADModel(cfg, **kw)
    return m, cfg


@pytest.mark.parametrize('weights', ['fixed', 'auto'])
def test_model_accepts_the_token_logs_it_and_keeps_the_dict_order(weights, monkeypatch):
    from aladin_amd import ops
    from aladin_amd.loss import CrossEntropyCriterion
    m, cfg = _stub_model('matching-crossentropy', [1.0, 0.5] if weights == 'fixed' else 'auto', graphed=True)
    assert m.losses_types == ['matching', 'crossentropy'] and m.auto_weight == (weights == 'auto')
    assert isinstance(m.crossentropy_criterion, CrossEntropyCriterion)
    assert [n for n, _ in m.named_parameters()] == ['crossentropy_criterion.temperature']          # learnable with the model
    if weights == 'auto':
        m.losses_weights = {k: v.detach().cpu() for k, v in m.losses_weights.items()}                # wherever 'auto' created them
    x = torch.ones((4, 8), requires_grad=True)
    assert not m._fused_heads_ok(x) and not m._graph_heads_now(x, x, x[None], x[None], True)
    m.matching_criterion, m.crossentropy_criterion = _StubMatching(), _StubCrossEntropy()
    entropy_calls = []
    monkeypatch.setattr(ops, 'nn_entropy_loss', lambda a, b: entropy_calls.append(1) or a.sum() * 0 + 11.0, raising=False)
    m.logger = _Log()
    total, d = m.forward_loss_total(x, x, x[None], x[None], [1] * 4, [1] * 4, 0)
    assert list(d) == ['matching', 'crossentropy'] and [float(v.detach()) for v in d.values()] == [3.0, 7.0]
    assert not entropy_calls and m.crossentropy_criterion.calls == 1          # 'crossentropy' is not 'entropy': list tests, not substring tests
    assert [(k, n) for k, _, n in m.logger.seen] == [('matching_loss', 4), ('crossentropy_loss', 4)]
    assert [v for _, v, _ in m.logger.seen] == [3.0, 7.0]
    want = 3.0 * 1.0 + 7.0 * 0.5 if weights == 'fixed' else 0.5 * ((3.0 + 7.0) * np.exp(2.3) - 2 * 2.3)
    np.testing.assert_allclose(float(total.detach()), want, rtol=1e-6)
    total.sum().backward()
    np.testing.assert_allclose(m.crossentropy_criterion.temperature.grad.item(), 7.0 * (0.5 if weights == 'fixed' else 0.5 * np.exp(2.3)), rtol=1e-6)


def test_model_term_order_and_the_shipped_configurations_are_untouched(monkeypatch):
    from aladin_amd import ops
    m, _ = _stub_model('matching-entropy-crossentropy-regularizehidden', [1.0, 0.1, 0.5, 0.2])
    m.matching_criterion, m.crossentropy_criterion = _StubMatching(), _StubCrossEntropy()
    monkeypatch.setattr(ops, 'nn_entropy_loss', lambda a, b: a.sum() * 0 + 11.0, raising=False)
    m.logger = _Log()
    x = torch.ones((4, 8), requires_grad=True)
    total, d = m.forward_loss_total(x, x, x[None], x[None], [1] * 4, [1] * 4, torch.tensor(2.0))
    assert list(d) == ['matching', 'entropy', 'crossentropy', 'regularizehidden']
    assert [k for k, _, _ in m.logger.seen] == ['matching_loss', 'entropy-uniform-loss', 'crossentropy_loss', 'regularize_hidden_loss']
    np.testing.assert_allclose(float(total.detach()), 3.0 + 1.1 + 3.5 + 0.4, rtol=1e-6)
    # without the token nothing of it exists: a shipped configuration's state dict and parameters are what they were
    plain, _ = _stub_model('matching-entropy', [1.0, 0.1])
    assert not hasattr(plain, 'crossentropy_criterion') and not list(plain.state_dict()) and not list(plain.parameters())


def test_sharded_step_still_refuses_the_token():
    m, _ = _stub_model('matching-crossentropy', [1.0, 0.5], shard_group=None)
    x = torch.zeros((4, 8), requires_grad=True)
    with pytest.raises(NotImplementedError, match='sharded'):
        m.forward_loss_total(x, x, x[None], x[None], [1] * 4, [1] * 4, 0)
