"""CPU tier of the autograd contract (tests/helpers/autograd_contract.py; the device half is tests/test_autograd_contract_gpu.py).

  * every float64 torch restatement of the registry against the closed-form values and gradients the project already has
    (oracle/alad_oracle.py, tests/helpers/*_numpy.py) at the base shapes, both sides float64: 1e-12 relative to the largest entry.
    Worst figure measured: 7.8e-16 (loss_heads at B = 65);
  * every input layout yields the strides it claims, back() restores the values, overlapping leaves sum;
  * every upstream composite hands a node the gradient stride it is named for (a dummy Function records it);
  * the registry's gpu_calls bind to the signatures of aladin_amd.ops, and the alignment entries run end to end over the CPU
    stand-ins of tests/helpers/cpu_standins.py;
  * over a library stand-in that records every call: the entry points each autograd node issues, in order, and what the
    saved-gradient loss nodes keep for their backward, and for how long."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import autograd_contract as AC           # noqa: E402
import cpu_standins                      # noqa: E402
from autograd_contract import A, E, H, O, S2, SM, X      # noqa: E402

PIN = 1e-12


def f64(x):
    return np.asarray(x, np.float64)


def closed_form(entry, data, W):
    """(outs, grads) of the base composite -- (M * W).sum() or L -- from the closed forms; None where the project has none for a part"""
    diff, aux, st = data
    v = {k: f64(x) for k, x in dict(diff, **aux).items() if x.dtype.kind == 'f'}
    name = entry.name
    if name.startswith('alignment_scores'):
        mode = name[len('alignment_scores['):].split(',')[0]
        S = O.alignment_scores(v['im'], v['s'], st['im_len'], st['s_len'], mode, dtype=np.float64)
        if mode != 'MrSw':
            return (S,), None
        d_im, d_s = O.alignment_scores_backward(v['im'], v['s'], st['im_len'], st['s_len'], W)
        return (S,), {'im': d_im, 's': d_s}
    if name.startswith('alignment_triplet_loss'):
        mv = 'mv=1' in name
        S = O.alignment_scores(v['im'], v['s'], st['im_len'], st['s_len'], 'MrSw', dtype=np.float64)
        loss, dS = O.hinge_loss(S, 0.2, mv, return_grad=True)
        d_im, d_s = O.alignment_scores_backward(v['im'], v['s'], st['im_len'], st['s_len'], f64(dS))
        return (loss, S), {'im': d_im, 's': d_s}
    if name == 'alignment_scan_scores':
        S, d_im, d_s, _ = S2.scan_eval(v['im'], v['s'], st['im_len'], st['s_len'], W)
        assert np.allclose(S, O.scan_sentences_scores(diff['im'], diff['s'], st['im_len'], st['s_len']), rtol=1e-4, atol=1e-5)
        return (S,), {'im': d_im, 's': d_s}
    if name.startswith('alignment_sum_scores'):
        S, d_im, d_s, _ = S2.sum_scores(v['im'], v['s'], st['im_len'], st['s_len'], W, st['mean'])
        return (S,), {'im': d_im, 's': d_s}
    if name == 'dot_scores':
        (C, d_im, d_s), _ = H.gemm_refs(v['im'], v['s'], W)
        return (C,), {'im': d_im, 's': d_s}
    if name == 'order_scores':
        sc, d_im, d_s = S2.order_eval(v['im'], v['s'], W)
        return (sc,), {'im': d_im, 's': d_s}
    if name == 'l2norm_rows':
        out, dx = H.l2norm_ref(v['x'], W)
        return (out,), {'x': dx}
    if name.startswith('hinge_loss'):
        loss, dS = O.hinge_loss(v['scores'], H.HINGE_MARGIN_Q, 'mv=1' in name, return_grad=True)
        return (loss,), {'scores': dS}
    if name == 'listnet_loss':
        loss, dM = O.listnet_loss(v['teacher'], v['student'], return_grad=True)
        return (loss,), {'student': dM}
    if name == 'distillation_loss[mse]':
        (loss, dM, dwb), _ = S2.mse_ref(v['teacher'], v['student'], diff['wb'])
        return (loss,), {'student': dM, 'wb': dwb}
    if name == 'distillation_loss[contrastive]':
        loss, dM, _ = S2.contrastive_eval(v['teacher'], v['student'], st['margin'])
        return (loss,), {'student': dM}
    if name == 'distillation_loss[ordinal]':
        loss, gr, gc, _, _, _ = S2.ordinal_parts(v['teacher'], v['student'], st['margin'], st['threshold'], st['stride'])
        return (loss,), {'student': gr + gc}
    if name == 'cross_entropy_scores':
        loss, dS, dt = X.xent_f64(v['scores'], float(diff['log_t'][0]))
        return (loss,), {'scores': dS, 'log_t': np.asarray([dt])}
    if name == 'match_cross_entropy':
        loss, d_im, d_s, dt, S = X.criterion_f64(v['im'], v['s'], float(diff['log_t'][0]))
        return (loss, S), {'im': d_im, 's': d_s, 'log_t': np.asarray([dt])}
    if name == 'semantic_hinge_loss':
        loss, dS, _ = SM.semantic_f64(v['scores'], aux['rel'], AC.SEM_MARGIN, AC.SEM_THRESHOLD, aux['draws'], False)
        return (loss,), {'scores': dS}
    if name == 'nn_entropy_loss':
        loss, _, _, d_img, d_cap = E.entropy_loss(v['img'], v['cap'])
        return (loss,), {'img': d_img, 'cap': d_cap}
    if name == 'attention_distillation_loss':
        loss, d_im, d_s = A.attdistill(diff['im'], diff['s'], st['im_len'], st['s_len'], aux['teacher'])
        return (loss,), {'im': d_im, 's': d_s}
    if name.startswith('match_hinge') or name == 'small_batch_match_distill':
        M = v['im'] @ v['s'].T
        loss, dM = O.hinge_loss(M, H.HINGE_MARGIN_Q, True, return_grad=True)
        outs = (loss, M) if name.startswith('match_hinge') else (loss, O.listnet_loss(v['teacher'], M), M)
        return outs, {'im': f64(dM) @ v['s'], 's': f64(dM).T @ v['im']}
    if name.startswith('loss_heads'):
        heads, w = st['heads'], st['weights']
        terms, g = np.zeros(3), {k: None for k in ('img', 'cap', 'im', 's')}
        S = M = None
        if 'alignment' in heads or 'distillation' in heads:
            S = O.alignment_scores(v['im'], v['s'], st['im_len'], st['s_len'], 'MrSw', dtype=np.float64)
        if 'matching' in heads or 'distillation' in heads:
            M = v['img'] @ v['cap'].T
        C = 0
        if 'matching' in heads:
            terms[0], dM = O.hinge_loss(M, st['margin'], True, return_grad=True)
            C = C + w['matching'] * f64(dM)
        if 'alignment' in heads:
            terms[1], dS = O.hinge_loss(S, st['margin'], True, return_grad=True)
            g['im'], g['s'] = O.alignment_scores_backward(v['im'], v['s'], st['im_len'], st['s_len'], w['alignment'] * f64(dS))
        if 'distillation' in heads:
            terms[2], dM = O.listnet_loss(S, M, return_grad=True)
            C = C + w['distillation'] * f64(dM)
        if M is not None:
            g['img'], g['cap'] = C @ v['cap'], C.T @ v['img']
        total = sum(w[k] * terms[i] for i, k in enumerate(('matching', 'alignment', 'distillation')) if k in heads)
        return (total, terms, S, M), g
    raise AssertionError('no closed form listed for %s' % name)


def rel_err(got, ref):
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top = np.abs(ref).max() if ref.size else 0.0
    return float(np.abs(got - ref).max() / top) if top > 0 else float(np.abs(got).max())


@pytest.mark.parametrize('name', AC.BASE)
def test_restatement_equals_the_closed_form(name):
    entry = AC.REGISTRY[name]
    data = entry.build(0)
    comp = AC.base_composite(entry)
    outs, grads, up, _ = AC.reference(entry, data, AC.composites(entry)[comp][0])
    W = next((f64(u) for i, u in sorted(up.items()) if entry.outputs[i] == 'M' and u is not None), None)
    want_outs, want_grads = closed_form(entry, data, W)
    worst = 0.0
    for i, (g, r) in enumerate(zip(outs, want_outs)):
        if r is not None:
            worst = max(worst, rel_err(g, r))
    for n, r in (want_grads or {}).items():
        if r is None:
            assert grads[n] is None or not grads[n].any(), n
        else:
            worst = max(worst, rel_err(grads[n], r))
    print('%s: worst relative distance from the closed form %.3g' % (name, worst))
    assert worst <= PIN, (name, worst)


def test_every_base_shape_has_two_variants_and_another_shape():
    for name in AC.BASE:
        e = AC.REGISTRY[name]
        d0, d1, d2 = (e.build(v)[0] for v in (0, 1, 2))
        for n in d0:
            if e.kinds.get(n) in ('set', 'mat'):
                assert d0[n].shape == d1[n].shape and not np.array_equal(d0[n], d1[n]), (name, n)
                assert d2[n].shape != d0[n].shape, (name, n)


# ------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------
CPU32 = AC.to_device('cpu', torch.float32)


def _sample(kind):
    rng = np.random.default_rng(3)
    shape = {'set': (5, 12, 64), 'mat': (5, 7), 'scalar': (1,), 'vec': (2,)}[kind]
    return rng.standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize('kind,layout', [(k, l) for k, d in AC.LAYOUTS.items() for l in d])
def test_layout_has_its_strides_and_back_restores(kind, layout):
    x = _sample(kind)
    lay = AC.LAYOUTS[kind][layout](x, lambda a: CPU32(a).requires_grad_(True))
    assert tuple(lay.view.stride()) == tuple(lay.stride), (lay.view.stride(), lay.stride)
    assert lay.view.numel() == lay.values.size and np.array_equal(lay.view.detach().numpy().reshape(lay.values.shape), lay.values)
    if layout not in AC.SUMMED:
        assert np.array_equal(lay.values, x)
    if (kind, layout) == ('set', 'misaligned'):
        assert lay.view.data_ptr() % 16 == 4                     # rows off the 16-byte boundary
    if (kind, layout) == ('set', 'offset'):
        assert lay.view.data_ptr() != lay.leaf.data_ptr()
    # a gradient of the view's shape lands in the leaf; back() returns it in the array's layout, the rest of the leaf exactly 0
    w = torch.from_numpy(np.random.default_rng(4).standard_normal(tuple(lay.view.shape)).astype(np.float32))
    (lay.view * w).sum().backward()
    assert lay.leaf.grad.shape == lay.leaf.shape
    got = lay.back(lay.leaf.grad.numpy().copy())
    want = AC.to_leaf(kind, layout, w.numpy().astype(np.float64).reshape(lay.values.shape))      # overlapping leaves sum
    assert got.shape == want.shape and np.allclose(got, want, rtol=1e-6, atol=1e-6), (kind, layout)
    if layout in ('expanded', 'row', 'col'):
        assert want.size < w.numel() and 0 in lay.view.stride()


# ------------------------------------------------------------------------------------------------
# upstream composites
# ------------------------------------------------------------------------------------------------
class Recorder(torch.autograd.Function):
    seen = []

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        return x.clone(), x.sum()

    @staticmethod
    def backward(ctx, g_M, g_L):
        Recorder.seen.append((None if g_M is None else (tuple(g_M.stride()), g_M.dtype, g_M.clone()), g_L))
        return g_M


@pytest.mark.parametrize('shape', [(5, 5), (5, 4)])
def test_matrix_composites_hand_over_the_stride_they_are_named_for(shape):
    rng = np.random.default_rng(9)
    for name, (f, stride) in AC.m_composites(0).items():
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).requires_grad_(True)
        del Recorder.seen[:]
        M, L = Recorder.apply(x)
        hook = []
        M.register_hook(lambda g: hook.append(tuple(g.stride())))
        f((M, L)).backward()
        (got, dtype, g), g_L = Recorder.seen[0]
        assert g_L is None and dtype == torch.float32
        assert got == stride(M) == hook[0], (name, got, stride(M), hook)
        if name == 'onehot':
            assert int((g != 0).sum()) == 1 and float(g[1, 2]) == 3.0
        if name == 'zerocols':
            assert not g[:, 0].any() and not g[:, 3:].any() and bool((g[:, 1:3] == 1).all())


def test_scalar_composites_and_the_sibling_graph():
    x = torch.ones(3, 3, requires_grad=True)
    for name, f in AC.l_composites(1).items():
        del Recorder.seen[:]
        out = Recorder.apply(x)
        f(out).backward()
        g_M, g_L = Recorder.seen[0]
        want = {'double3': 3.0}.get(name, AC.L_SCALES.get(name))
        assert g_M is None and g_L.dtype == torch.float32 and float(g_L) == want, (name, g_L)
    # neither output used: the node still runs, with None for both
    del Recorder.seen[:]
    y = torch.ones(2, requires_grad=True)
    out = Recorder.apply(x)
    AC.Drop.apply(y.sum(), *out).backward()
    assert Recorder.seen == [(None, None)]
    assert x.grad is None or not x.grad.any()
    assert torch.equal(y.grad, torch.ones(2))


def test_composites_cover_every_differentiable_output():
    for name, e in AC.REGISTRY.items():
        c = AC.composites(e)
        n_m, n_l = e.outputs.count('M'), e.outputs.count('L')
        assert len(c) == 8 * n_m + 5 * n_l + (1 if n_m + n_l > 1 else 0), (name, list(c))


# ------------------------------------------------------------------------------------------------
# the gpu_calls
# ------------------------------------------------------------------------------------------------
class Bound(Exception):
    pass


PUBLIC = ['alignment_scores', 'alignment_triplet_loss', 'alignment_scan_scores', 'alignment_sum_scores', 'dot_scores', 'order_scores',
          'l2norm_rows', 'hinge_loss', 'listnet_loss', 'distillation_loss', 'cross_entropy_scores', 'match_cross_entropy',
          'semantic_hinge_loss', 'nn_entropy_loss', 'attention_distillation_loss', 'match_hinge', 'small_batch_match_distill',
          'loss_heads']


@pytest.mark.parametrize('name', list(AC.REGISTRY))
def test_gpu_call_binds_to_the_signature_of_its_entry_point(name, monkeypatch):
    from aladin_amd import ops
    entry = AC.REGISTRY[name]
    for fn in PUBLIC:
        sig = inspect.signature(getattr(ops, fn))

        def stub(*a, _fn=fn, _sig=sig, **k):
            raise Bound(_fn, _sig.bind(*a, **k))
        monkeypatch.setattr(ops, fn, stub, raising=False)
    p = AC.Prepared(entry, entry.build(0), CPU32)
    with pytest.raises(Bound) as info:
        entry.gpu_call(p.t, p.st)
    fn, bound = info.value.args
    assert name.startswith(fn), (name, fn)
    assert all(isinstance(p.t[n], torch.Tensor) and any(v is p.t[n] for v in bound.arguments.values()) for n in p.names), name


@pytest.mark.parametrize('name', [n for n in AC.REGISTRY if n.startswith('alignment_scores[MrSw') and 'long' not in n])
def test_alignment_entries_run_over_the_cpu_standins(name, monkeypatch):
    """the differentiable path of ops.alignment_scores (geometry, packing layout, autograd nodes) with the kernels replaced by the
    stand-ins, which cover the 'MrSw' pooling of the tile classes: the registry's call, composites and layouts work end to end, within the fp16 bars of the float64 reference"""
    from aladin_amd import ops
    for attr, fn in (('pack_images', cpu_standins.pack_images), ('pack_captions', cpu_standins.pack_captions),
                     ('pack_sets', cpu_standins.pack_sets), ('scores_from_packed', cpu_standins.scores_from_packed),
                     ('_hinge_raw', cpu_standins.hinge_raw), ('_align_backward', cpu_standins.align_backward),
                     ('_check_sets', cpu_standins.check_sets)):
        monkeypatch.setattr(ops, attr, fn)
    entry = AC.REGISTRY[name]
    data = entry.build(0)
    for comp in ('dense', 'cols'):
        f = AC.composites(entry)[comp][0]
        for layouts in (None, {'im': 'permuted'}, {'s': 'expanded'}):
            run_data, values = entry.with_layout(data, *next(iter(layouts.items()))) if layouts else (data, data)
            p = AC.Prepared(entry, run_data, CPU32, layouts)
            outs = entry.gpu_call(p.t, p.st)
            f(outs).backward()
            ref = AC.reference(entry, run_data, f, layouts)
            entry.check_outs(AC.np_outs(outs), ref[0])
            entry.check_grads(p.grads(), ref[1], AC.context(entry, values, layouts, 'exact', ref, AC.np_outs(outs)))


# ------------------------------------------------------------------------------------------------
# what reaches _ld in the fused head nodes (the C ABI refuses a row stride below the row length)
# ------------------------------------------------------------------------------------------------
class _AnyCall:
    """stands for the loaded library: every entry point accepts its arguments and reports success"""

    def __getattr__(self, name):
        return lambda *a: 0


def test_fused_head_nodes_never_hand_over_a_row_stride_below_the_row_length(monkeypatch):
    """_SmallMatchDistill with an expanded embedding row, an expanded teacher row and the (0, 1)- / (0, 0)-strided upstream gradients
    of M.sum(0) / M.sum(): every leading dimension that reaches a kernel is at least the row length (aladin_heads_small_fwd / _bwd
    return ALADIN_ERR_ARG below it).  Fails with the raw `stride(1) == 1` decisions: they pass 0."""
    from aladin_amd import _lib, ops_heads
    seen = []
    real_ld = ops_heads._ld
    monkeypatch.setattr(ops_heads, '_ld', lambda t: seen.append((real_ld(t), t.shape[1])) or seen[-1][0])
    monkeypatch.setattr(ops_heads, '_stream', lambda: None)
    monkeypatch.setattr(_lib, 'load', lambda: _AnyCall())
    B, D = 5, 64
    rng = np.random.default_rng(1)
    new = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    row, trow = new(1, D).requires_grad_(True), new(B)
    for im, teacher, f in ((new(B, D).requires_grad_(True), new(B, B), lambda M: (M.sum(0) * new(B)).sum()),
                           (new(B, D).requires_grad_(True), new(B, B), lambda M: M.sum()),
                           (row.expand(B, D), new(B, B), lambda M: (M * new(B, B)).sum()),
                           (new(B, D).requires_grad_(True), trow.expand(B, B), lambda M: (M * new(B, B)).sum())):
        del seen[:]
        lh, ll, M = ops_heads._SmallMatchDistill.apply(im, new(B, D).requires_grad_(True), teacher, 0.2, True, True, 6.0, 1e-10)
        arrived = []
        M.register_hook(lambda g: arrived.append(tuple(g.stride())))
        f(M).backward()
        assert len(seen) >= 5 and all(ld >= cols for ld, cols in seen), (arrived, seen)
    assert arrived == [(B, 1)]
    assert row.grad.shape == (1, D)


@pytest.mark.parametrize('node', ['_SmallHeads', '_BigHeads', '_MatchHinge', '_MatchCrossEntropy'])
def test_the_other_fused_nodes_hand_over_rows_that_do_not_overlap(node, monkeypatch):
    """the four other nodes of ops_heads.py with an expanded embedding row on either side, forward and backward: no leading
    dimension below the row length reaches _ld and no zero stride reaches aladin_sgemm_strided (the raw `stride(1) == 1` decisions
    hand the expanded row over as it is)"""
    from aladin_amd import _lib, ops_heads, ops_losses
    lds, gemms = [], []
    real_ld = ops_heads._ld

    def sgemm(M, N, K, A_, a_rs, a_cs, B_, b_rs, b_cs, out):
        gemms.append((a_rs, a_cs, b_rs, b_cs))
        return out
    monkeypatch.setattr(ops_losses, '_sgemm', sgemm)           # the product pair of the four nodes lives there
    for mod in (ops_heads, ops_losses):
        monkeypatch.setattr(mod, '_ld', lambda t: lds.append((real_ld(t), t.shape[1])) or lds[-1][0])
        monkeypatch.setattr(mod, '_stream', lambda: None)
    monkeypatch.setattr(_lib, 'load', lambda: _AnyCall())
    B, D = 5, 64
    rng = np.random.default_rng(2)
    new = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    for side in (0, 1):
        row = new(1, D).requires_grad_(True)
        pair = [new(B, D).requires_grad_(True), new(B, D).requires_grad_(True)]
        pair[side] = row.expand(B, D)
        assert pair[side].stride() == (0, 1)
        del lds[:], gemms[:]
        if node == '_SmallHeads':
            out = ops_heads._SmallHeads.apply(pair[0], pair[1], None, None, None, None, 0.2, True, ops_heads.HEAD_MATCH_HINGE,
                                              (1.0, 0.0, 0.0), 6.0, 1e-10)[0]
        elif node == '_BigHeads':
            out = ops_heads._BigHeads.apply(pair[0], pair[1], None, None, None, None, 0.2, True, ops_heads.HEAD_MATCH_HINGE,
                                            (1.0, 0.0, 0.0), 6.0, 1e-10, None)[0]
        elif node == '_MatchHinge':
            loss, M = ops_heads._MatchHinge.apply(pair[0], pair[1], 0.2, True)
            out = loss + (M.sum(0) * new(B)).sum()
        else:
            loss, M = ops_heads._MatchCrossEntropy.apply(pair[0], pair[1], new(1).requires_grad_(True))
            out = loss + (M.sum(0) * new(B)).sum()
        out.backward()
        assert lds or gemms
        assert all(ld >= cols for ld, cols in lds), (node, side, lds)
        assert all(0 not in g for g in gemms), (node, side, gemms)
        assert row.grad is not None and row.grad.shape == (1, D)


# ------------------------------------------------------------------------------------------------
# which entry points a node calls, in which order; what the saved-gradient nodes keep, and for how long
# ------------------------------------------------------------------------------------------------
class _RecordingLib:
    """stands for the loaded library: the host-only functions (the geometry, every workspace size) go to the real one, every other
    entry point is recorded with its arguments and reports success"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name == 'aladin_align_geometry' or name.endswith('_workspace_bytes'):
            return getattr(self.real, name)
        return lambda *a: self.calls.append((name[len('aladin_'):], a)) or 0

    def names(self):
        return [n for n, _ in self.calls]

    def null_pointers(self):
        return sum(isinstance(v, ctypes.c_void_p) and not v.value for _, a in self.calls for v in a)


@pytest.fixture
def recording_lib(monkeypatch):
    from aladin_amd import _lib, ops, ops_heads, ops_losses
    lib = _RecordingLib(_lib.load())
    for mod in (ops, ops_heads, ops_losses):
        monkeypatch.setattr(mod, '_stream', lambda: None)
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    return lib


def _node_inputs(B, seed=5):
    rng = np.random.default_rng(seed)
    new = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    leaf = lambda *shape: new(*shape).requires_grad_(True)
    full = lambda n: torch.full((B,), n, dtype=torch.int32)
    return new, leaf, full(6), full(8)


def _sequence_cases():
    """name -> (B, run(new, leaf, il, sl) -> the scalar to back-propagate, the expected calls): the table of the parent commit"""
    from aladin_amd import ops, ops_heads as OH, ops_losses as OL
    gemm, W = 'sgemm_strided', (1.0, 1.0, 1.0)
    embs = lambda leaf, B: (leaf(B, 16), leaf(B, 16))
    sets = lambda leaf, B: (leaf(B, 6, 8), leaf(B, 8, 8))
    both = lambda out: out[0] + out[1].sum()
    cases = {
        '_Hinge': (5, lambda new, leaf, il, sl: OL._Hinge.apply(leaf(5, 5), 0.2, True), ['hinge_fused']),
        '_ListNet': (5, lambda new, leaf, il, sl: OL._ListNet.apply(new(5, 5), leaf(5, 5), 6.0, 1e-10), ['listnet_fwd_bwd']),
        '_SemanticHinge': (5, lambda new, leaf, il, sl: OL._SemanticHinge.apply(
            leaf(5, 5), new(5, 5), torch.zeros(10, dtype=torch.int32), 0.2, 0.4, 0, False), ['semantic_hinge_fwd_bwd']),
        '_CrossEntropy': (5, lambda new, leaf, il, sl: OL._CrossEntropy.apply(leaf(5, 5), leaf(1)), ['xent_fwd_bwd', 'grad_combine']),
        '_DotScores': (5, lambda new, leaf, il, sl: OL._DotScores.apply(*embs(leaf, 5)).sum(), [gemm] * 3),
        '_SmallMatchDistill': (5, lambda new, leaf, il, sl: (lambda o: o[0] + o[1] + o[2].sum())(
            OH._SmallMatchDistill.apply(*embs(leaf, 5), new(5, 5), 0.2, True, True, 6.0, 1e-10)), ['heads_small_fwd', 'heads_small_bwd']),
        '_AlignScores': (5, lambda new, leaf, il, sl: ops._AlignScores.apply(*sets(leaf, 5), il, sl, 0, 2).sum(),
                         ['align_pack', 'align_scores', 'align_bwd']),
        '_AttDistill': (5, lambda new, leaf, il, sl: OL._AttDistill.apply(*sets(leaf, 5), il, sl, new(5, 5, 7, 5)),
                        ['attdistill_fwd', 'attdistill_bwd']),
        '_SmallHeads[7]': (5, lambda new, leaf, il, sl: OH._SmallHeads.apply(*embs(leaf, 5), *sets(leaf, 5), il, sl, 0.2, True, 7, W, 6.0, 1e-10)[0],
                           ['align_pack', 'align_scores', 'heads_small_fwd_argmax', 'heads_small_bwd', 'align_triplet_bwd']),
        '_SmallHeads[7,sum]': (5, lambda new, leaf, il, sl: OH._SmallHeads.apply(*embs(leaf, 5), *sets(leaf, 5), il, sl, 0.2, False, 7, W, 6.0, 1e-10)[0],
                               ['align_pack', 'align_scores', 'heads_small_fwd', 'heads_small_bwd', 'align_bwd']),
        '_SmallHeads[1]': (5, lambda new, leaf, il, sl: OH._SmallHeads.apply(*embs(leaf, 5), None, None, None, None, 0.2, True, 1, W, 6.0, 1e-10)[0],
                           ['heads_small_fwd', 'heads_small_bwd']),
        '_BigHeads[7]': (65, lambda new, leaf, il, sl: OH._BigHeads.apply(*embs(leaf, 65), *sets(leaf, 65), il, sl, 0.2, True, 7, W, 6.0, 1e-10, None)[0],
                         ['align_triplet_fwd', gemm, 'hinge_fused', 'listnet_fwd_bwd', 'loss_total', 'grad_combine', gemm, gemm, 'align_triplet_bwd']),
        '_BigHeads[1]': (65, lambda new, leaf, il, sl: OH._BigHeads.apply(*embs(leaf, 65), None, None, None, None, 0.2, True, 1, W, 6.0, 1e-10, None)[0],
                         [gemm, 'hinge_fused', 'loss_total', 'grad_combine', gemm, gemm]),
    }
    for mode in ('mse', 'contrastive', 'ordinal'):
        cases['_DistillMode[%s]' % mode] = (5, lambda new, leaf, il, sl, mode=mode: OL._DistillMode.apply(
            new(5, 5), leaf(5, 5), leaf(2), mode, 0.2, 0.1, 3), ['distill_%s_fwd_bwd' % mode])
    for B in (5, 65):
        cases['_MatchHinge[%d]' % B] = (B, lambda new, leaf, il, sl, B=B: both(OH._MatchHinge.apply(*embs(leaf, B), 0.2, True)),
                                        [gemm, 'hinge_fused', 'grad_combine', gemm, gemm])
        cases['_MatchCrossEntropy[%d]' % B] = (B, lambda new, leaf, il, sl, B=B: both(OH._MatchCrossEntropy.apply(*embs(leaf, B), leaf(1))),
                                               [gemm, 'xent_fwd_bwd', 'grad_combine', gemm, gemm])
        cases['_AlignTriplet[%d]' % B] = (B, lambda new, leaf, il, sl, B=B: ops._AlignTriplet.apply(*sets(leaf, B), il, sl, 0.2, True, None)[0],
                                          ['align_triplet_fwd', 'align_triplet_bwd'])
    return cases


SEQUENCE_NODES = ['_Hinge', '_ListNet', '_DistillMode[mse]', '_DistillMode[contrastive]', '_DistillMode[ordinal]', '_SemanticHinge',
                  '_CrossEntropy', '_DotScores', '_SmallMatchDistill', '_MatchHinge[5]', '_MatchHinge[65]', '_MatchCrossEntropy[5]',
                  '_MatchCrossEntropy[65]', '_SmallHeads[7]', '_SmallHeads[7,sum]', '_SmallHeads[1]', '_BigHeads[7]', '_BigHeads[1]',
                  '_AlignTriplet[5]', '_AlignTriplet[65]', '_AlignScores', '_AttDistill']


@pytest.mark.parametrize('name', SEQUENCE_NODES)
def test_every_node_issues_the_entry_points_of_its_row_in_order(name, recording_lib):
    """forward, then backward() of the loss (plus M.sum() where M is differentiable), on CPU tensors over the recording library:
    embeddings (B, 16), sets (B, 6, 8) and (B, 8, 8) at full lengths, hardest-negative hinge, weights (1, 1, 1); B = 65 is the first
    batch past SMALL_BATCH_MAX.  (The sum of violations at B = 65 asks the density probe about stream capture: the GPU tests' path.)"""
    cases = _sequence_cases()
    assert sorted(cases) == sorted(SEQUENCE_NODES)
    B, run, want = cases[name]
    new, leaf, il, sl = _node_inputs(B)
    run(new, leaf, il, sl).backward()
    assert recording_lib.names() == want, (name, recording_lib.names())


def _saved_gradient_cases():
    """name -> (apply(inputs) -> loss, the differentiable inputs' positions among the node's arguments)"""
    from aladin_amd import ops_losses as OL
    draws = torch.zeros(6, dtype=torch.int32)
    cases = {'_Hinge': (OL._Hinge, lambda x: (x['scores'], 0.2, True), ['scores']),
             '_ListNet': (OL._ListNet, lambda x: (x['teacher'], x['student'], 6.0, 1e-10), ['student']),
             '_SemanticHinge': (OL._SemanticHinge, lambda x: (x['scores'], x['teacher'], draws, 0.2, 0.4, 0, False), ['scores'])}
    for mode in ('mse', 'contrastive', 'ordinal'):
        cases['_DistillMode[%s]' % mode] = (OL._DistillMode, lambda x, mode=mode: (x['teacher'], x['student'], x['wb'], mode, 0.2, 0.1, 1),
                                            ['student', 'wb'] if mode == 'mse' else ['student'])
    return cases


@pytest.mark.parametrize('name', ['_Hinge', '_ListNet', '_DistillMode[mse]', '_DistillMode[contrastive]', '_DistillMode[ordinal]',
                                  '_SemanticHinge'])
def test_saved_gradient_nodes_keep_their_matrices_until_the_graph_is_released(name, recording_lib):
    """the loss nodes whose forward leaves the gradient for an upstream 1: the matrices travel through save_for_backward, so two
    retained backwards accumulate exactly twice the single gradient, a further backward() succeeds and releases them, the one after
    that raises; an input that takes no gradient gets no buffer (one more null pointer reaches the kernel) and None from backward."""
    node, args, diff = _saved_gradient_cases()[name]
    B = 3
    rng = np.random.default_rng(11)
    new = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))

    def inputs(requires):
        x = {'scores': new(B, B), 'teacher': new(B, B), 'student': new(B, B), 'wb': new(2)}
        for n in requires:
            x[n].requires_grad_(True)
        return x

    x = inputs(diff)
    loss = node.apply(*args(x))
    nulls_all = recording_lib.null_pointers()
    saved = [t for t in loss.grad_fn.saved_tensors if t is not None]          # (the mse mode's dwb slot is empty in the other modes)
    assert [tuple(t.shape) for t in saved] == [tuple(x[n].shape) for n in diff] and all(t.dtype == torch.float32 for t in saved)
    assert not any(isinstance(v, torch.Tensor) for v in vars(loss.grad_fn).values()), 'a gradient kept as a plain attribute of ctx'
    for t in saved:                                  # the recording library wrote nothing: give the saved gradients values
        t.data.copy_(new(*t.shape))
    single = [t.clone() for t in saved]
    loss.backward(retain_graph=True)
    assert all(torch.equal(x[n].grad, g) for n, g in zip(diff, single))
    loss.backward(retain_graph=True)
    assert all(torch.equal(x[n].grad, 2 * g) for n, g in zip(diff, single))
    loss.backward()
    assert all(torch.equal(x[n].grad, 3 * g) for n, g in zip(diff, single))
    with pytest.raises(RuntimeError):
        loss.backward()
    # one input at a time without a gradient: no buffer for it, None from backward
    for off in diff:
        del recording_lib.calls[:]
        on = [n for n in diff if n != off]
        x = inputs(on)
        loss = node.apply(*args(x))
        assert recording_lib.null_pointers() == nulls_all + 1, (name, off)
        if not on:
            assert loss.grad_fn is None and not loss.requires_grad
            continue
        assert [t is None for t in loss.grad_fn.saved_tensors[:len(diff)]] == [n == off for n in diff]
        out = node.backward(loss.grad_fn, torch.ones(()))
        for i, v in enumerate(args(x)):
            assert (out[i] is not None) == (isinstance(v, torch.Tensor) and v.requires_grad), (name, off, i)
