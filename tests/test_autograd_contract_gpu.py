"""GPU tier (-m gpu) of the autograd contract: every differentiable entry point of tests/helpers/autograd_contract.py, one axis at a
time away from the base case (contiguous leaves, one call, (M * W).sum() or L):

  (a) the base case against the float64 reference at the gates the project already holds for the op (imported by the helper);
  (b) every way a caller consumes an output -- the gradient reaching the node dense, (0, 0)-, (0, 1)-, (1, 0)-, (1, B)-strided,
      one-hot, with zero columns, through a float64 cast; scalar scales 1, 1/4, -2, 0, a float64 3; unused outputs (None);
  (c) every memory layout of every tensor input, one input at a time: the bits of the contiguous run;
  (d) every subset of gradients asked for;  (e) backward twice, two forwards before the backwards, a forward of another shape in
  between;  (f) a side stream;  (g) an input edited in place between forward and backward;  (h) one dense-table backward.

The alignment entries run under both backward precisions, as the existing gradient tests do.  No tolerance is introduced here.
tests/test_autograd_contract_cpu.py pins the references, the layouts and the composites."""
import contextlib
import gc
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import autograd_contract as AC           # noqa: E402
from autograd_contract import O           # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def cases(names):
    """(entry name, backward precision): both precisions for the alignment entries, the default for the rest"""
    return [pytest.param(n, m, id='%s-%s' % (n, m) if m else n) for n in names for m in (('exact', 'fp16') if AC.REGISTRY[n].align else (None,))]


@contextlib.contextmanager
def precision(mode):
    from aladin_amd import ops
    old = ops.set_backward_precision(mode) if mode else None
    try:
        yield
    finally:
        if mode:
            ops.set_backward_precision(old)


class Failures:
    """collects what goes wrong in the sub-cases of one test, so that one run shows all of them; a fault of the device ends the
    session at once (nothing more is started on a card after one)"""

    def __init__(self):
        self.items = []

    @contextlib.contextmanager
    def case(self, *label):
        try:
            yield
        except (AssertionError, RuntimeError, ValueError, TypeError) as e:
            text = str(e)
            if isinstance(e, RuntimeError) and any(k in text for k in ('illegal memory access', 'HIP error', 'hipError', 'device-side')):
                pytest.exit('GPU fault in %r: %s' % (label, text), returncode=3)
            self.items.append('%s: %s: %s' % (' / '.join(map(str, label)), type(e).__name__, text.strip().splitlines()[0][:300] if text.strip() else ''))

    def done(self):
        assert not self.items, '%d sub-case(s) failed:\n  ' % len(self.items) + '\n  '.join(self.items)


class Run:
    pass


def forward(entry, data, layouts=None, requires=None):
    r = Run()
    r.p = AC.Prepared(entry, data, AC.to_device(dev(), torch.float32), layouts, requires)
    r.raw = entry.gpu_call(r.p.t, r.p.st)
    r.arrived = {}
    for i, k in enumerate(entry.outputs):
        if k == 'M' and r.raw[i] is not None and r.raw[i].requires_grad:
            r.raw[i].register_hook(lambda g, i=i: r.arrived.__setitem__(i, (tuple(g.stride()), g.detach().contiguous().clone())) if g is not None else None)
    return r


def finish(r):
    torch.cuda.synchronize()
    r.outs, r.grads = AC.np_outs(r.raw), r.p.grads()
    return r


def run(entry, data, f, layouts=None, requires=None):
    r = forward(entry, data, layouts, requires)
    loss = f(r.raw)
    if loss.requires_grad:
        loss.backward()
    return finish(r)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_grads(got, want, what):
    for n in want:
        assert same(got[n], want[n]), '%s: gradient of %s differs in %s entries' % (
            what, n, 'presence' if got[n] is None or want[n] is None else int((got[n] != want[n]).sum()))


def assert_same_outs(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), '%s: output %d differs' % (what, i)


def gated(entry, r, data, values, f, mode, layouts=None, requires=None, loss_only=False):
    """the run r against the float64 reference of the same call at the op's gates"""
    ref = AC.reference(entry, data, f, layouts, requires)
    entry.check_outs(r.outs, ref[0])
    ctx = AC.context(entry, values, layouts, mode or 'fp16', ref, r.outs, loss_only)
    ctx['arrived'] = {i: g.cpu().numpy().astype(np.float64) for i, (_, g) in getattr(r, 'arrived', {}).items()}
    entry.check_grads(r.grads, ref[1], ctx)
    return ref


def base_f(entry):
    return AC.composites(entry)[AC.base_composite(entry)][0]


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,mode', cases(list(AC.REGISTRY)))
def test_a_base_case_meets_the_gate_of_its_op(name, mode):
    entry = AC.REGISTRY[name]
    data = entry.build(0)
    with precision(mode):
        r = run(entry, data, base_f(entry))
    gated(entry, r, data, data, base_f(entry), mode, loss_only=True)


@pytest.mark.parametrize('name,mode', cases(list(AC.REGISTRY)))
def test_b_upstream_gradient_layouts(name, mode):
    entry = AC.REGISTRY[name]
    data = entry.build(0)
    fails = Failures()
    comps = AC.composites(entry)
    scaled = {}
    with precision(mode):
        for cname, (f, strides) in comps.items():
            with fails.case(cname):
                r = run(entry, data, f)
                for i, stride in strides.items():
                    got, G = r.arrived[i]
                    assert got == stride(r.raw[i]), ('the composite no longer hands over its stride', got, stride(r.raw[i]))
                f_ref = f
                if cname.endswith('double'):
                    # the gradient is made from the device's own float32 M: exactly 2 M (M itself is gated), and the reference
                    # back-propagates that very gradient
                    (i, _), = strides.items()
                    G = r.arrived[i][1]
                    assert torch.equal(G, 2 * r.raw[i].detach())
                    f_ref = lambda o, i=i, G=G: (o[i] * G.to(device=o[i].device, dtype=o[i].dtype)).sum()         # noqa: E731
                    entry.check_outs(r.outs, AC.reference(entry, data, f)[0])
                gated(entry, r, data, data, f_ref, mode, loss_only=not strides)
                if not strides:
                    scaled[cname] = r.grads
                for i in ([] if cname == 'all' else strides):     # the same values as a dense contiguous gradient: the same bits
                    G = r.arrived[i][1]
                    dense = run(entry, data, lambda o, i=i, G=G: (o[i] * G).sum())
                    assert dense.arrived[i][0] == (G.shape[1], 1) and torch.equal(dense.arrived[i][1], G)
                    assert_same_grads(dense.grads, r.grads, 'stride %s against its contiguous copy' % (r.arrived[i][0],))
        # powers of two commute with rounding: exactly 1/4 x and -2 x the bits of scale 1; scale 0: exact zeros, no NaN
        for tag in sorted({c[:-1] for c in scaled if c.endswith('L') and (c == 'L' or c.endswith('.L'))}):
            one = scaled.get(tag + 'L')
            for cname, c in (('quarter', 0.25), ('neg2', -2.0), ('zero', 0.0)):
                with fails.case(tag + cname, 'bits'):
                    got = scaled[tag + cname]
                    for n, g in one.items():
                        if g is None:
                            assert got[n] is None or not got[n].any(), n
                        elif c == 0.0:
                            assert got[n] is None or (not got[n].any() and not np.isnan(got[n]).any()), n
                        else:
                            assert np.array_equal(got[n], np.float32(c) * g), (n, int((got[n] != np.float32(c) * g).sum()))
        if sum(k in 'ML' for k in entry.outputs) > 1:
            with fails.case('neither output used'):
                r = forward(entry, data)
                sibling = torch.ones((), device=dev(), requires_grad=True)
                AC.Drop.apply(sibling * 2, *[o for o, k in zip(r.raw, entry.outputs) if k in 'ML']).backward()
                finish(r)
                assert float(sibling.grad) == 2.0 and not r.arrived
                assert all(g is None or not g.any() for g in r.grads.values())
    fails.done()


@pytest.mark.parametrize('name,mode', cases(list(AC.REGISTRY)))
def test_c_input_layouts(name, mode):
    entry = AC.REGISTRY[name]
    data = entry.build(0)
    f = base_f(entry)
    fails = Failures()
    diff, aux, _ = data
    with precision(mode):
        for n in list(diff) + list(aux):
            for layout in entry.layouts(n):
                if layout == 'contig':
                    continue
                with fails.case(n, layout):
                    run_data, values = entry.with_layout(data, n, layout)
                    r = run(entry, run_data, f, {n: layout})
                    contig = run(entry, values, f)
                    assert_same_outs(r.outs, contig.outs, 'layout')
                    assert_same_grads(r.grads, {k: v for k, v in contig.grads.items() if k != n or layout not in AC.EXPANDED}, 'layout')
                    if layout in AC.EXPANDED and n in diff:       # the leaf's gradient is a sum: within the gate of the reference's
                        gated(entry, r, run_data, values, f, mode, {n: layout}, loss_only=True)
    fails.done()


@pytest.mark.parametrize('name,mode', cases(list(AC.REGISTRY)))
def test_d_which_gradients_are_asked_for(name, mode):
    entry = AC.REGISTRY[name]
    data = entry.build(0)
    f = base_f(entry)
    fails = Failures()
    with precision(mode):
        full = run(entry, data, f)
        for n in data[0]:
            with fails.case('only', n):
                r = run(entry, data, f, requires=[n])
                assert_same_outs(r.outs, full.outs, 'only %s' % n)
                assert same(r.grads[n], full.grads[n]), 'gradient of %s alone differs from the all-inputs run' % n
                assert all(g is None for k, g in r.grads.items() if k != n)
        for what, ctx in (('no input requires grad', contextlib.nullcontext()), ('no_grad', torch.no_grad())):
            with fails.case(what):
                with ctx:
                    r = run(entry, data, f, requires=[] if what != 'no_grad' else None)
                assert all(o is None or not o.requires_grad for o in r.raw)
                assert all(g is None for g in r.grads.values())
                ref = AC.reference(entry, data, f, requires=[])
                entry.check_outs(r.outs, ref[0])                   # (alignment scores without autograd: the evaluation precision)
                if not entry.align:                                # the same kernels with or without a gradient buffer: the same bits
                    assert_same_outs(r.outs, full.outs, what)
    fails.done()


@pytest.mark.parametrize('name,mode', cases(list(AC.REGISTRY)))
def test_e_repeat_and_order(name, mode):
    entry = AC.REGISTRY[name]
    f = base_f(entry)
    d0, d1, d2 = entry.build(0), entry.build(1), entry.build(2)
    fails = Failures()
    with precision(mode):
        solo0, solo1 = run(entry, d0, f), run(entry, d1, f)
        with fails.case('backward twice'):
            r = forward(entry, d0)
            loss = f(r.raw)
            loss.backward(retain_graph=True)
            first = finish(r).grads
            assert_same_grads(first, solo0.grads, 'first pass')
            loss.backward(retain_graph=True)
            twice = finish(r).grads
            for n, g in first.items():
                assert (g is None and twice[n] is None) or np.array_equal(twice[n], np.float32(2) * g), 'accumulated gradient of %s is not 2 x' % n
            r.p.clear()
            loss.backward()
            assert_same_grads(finish(r).grads, first, 'second pass after clearing .grad')
        for order in ((0, 1), (1, 0)):
            with fails.case('two forwards, backwards in order', order):
                rs = [forward(entry, d0), forward(entry, d1)]
                losses = [f(r.raw) for r in rs]
                for k in order:
                    losses[k].backward()
                for r, solo in zip(rs, (solo0, solo1)):
                    finish(r)
                    assert_same_outs(r.outs, solo.outs, 'two forwards')
                    assert_same_grads(r.grads, solo.grads, 'two forwards')
        with fails.case('another shape between forward and backward'):
            r = forward(entry, d0)
            loss = f(r.raw)
            other = run(entry, d2, f)
            loss.backward()
            assert_same_grads(finish(r).grads, solo0.grads, 'interleaved')
            solo2 = run(entry, d2, f)
            assert_same_outs(other.outs, solo2.outs, 'the call in between')
            assert_same_grads(other.grads, solo2.grads, 'the call in between')
    fails.done()


@pytest.mark.parametrize('name,mode', cases(list(AC.REGISTRY)))
def test_f_side_stream(name, mode):
    entry = AC.REGISTRY[name]
    data = entry.build(0)
    f = base_f(entry)
    with precision(mode):
        want = run(entry, data, f)
        p = AC.Prepared(entry, data, AC.to_device(dev(), torch.float32))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            raw = entry.gpu_call(p.t, p.st)
            f(raw).backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    assert_same_outs(AC.np_outs(raw), want.outs, 'side stream')
    assert_same_grads(p.grads(), want.grads, 'side stream')


@pytest.mark.parametrize('name,mode', cases(list(AC.REGISTRY)))
def test_g_in_place_edit_between_forward_and_backward(name, mode):
    """autograd's version counter refuses the backward, or the node saved what it needs and the gradients are those of the unedited
    run; anything else is a silent wrong result"""
    entry = AC.REGISTRY[name]
    data = entry.build(0)
    f = base_f(entry)
    fails = Failures()
    with precision(mode):
        want = run(entry, data, f)
        for n in data[0]:
            with fails.case('edit', n):
                r = forward(entry, data)
                loss = f(r.raw)
                with torch.no_grad():
                    r.p.lay[n].leaf.mul_(1.5)
                try:
                    loss.backward()
                except RuntimeError as e:
                    assert 'modified by an inplace operation' in str(e), str(e)
                    continue
                assert_same_grads(finish(r).grads, want.grads, 'after an in-place edit of %s' % n)
    fails.done()


def test_h_dense_table_backward_of_a_generic_gradient(bwd_mode):
    """ops.alignment_scores('MrSw') at the shape of test_dense_backward_table_equals_the_per_pair_path (B = 128, R = 34, T = 50) with
    D = 64 and S.sum().backward(): a (0, 0)-strided all-ones gradient, every pair carrying one -- the dense table must be taken once
    the density probe has seen LAG steps, and the gradients are the oracle's for dS = 1."""
    from aladin_amd import _lib, ops, synth
    from test_long_sets_gpu import assert_grads_close, assert_scores_close
    B, R, Tn, D = 128, 34, 50, 64
    im, s, il, sl = synth.alignment_batch(B, R, Tn, D, seed=B + 5, ragged=True)
    assert B * B >= ops.DENSE_MIN_PAIRS
    to = AC.to_device(dev(), torch.float32)
    ops._generic_probes.clear()
    old = ops.DENSE_GEMM_FORCE
    ops.DENSE_GEMM_FORCE = True
    try:
        flags = []
        for _ in range(ops._DensityProbe.LAG + 1):
            a, b = to(im).requires_grad_(True), to(s).requires_grad_(True)
            S = ops.alignment_scores(a, b, il, sl, 'MrSw')
            arrived = []
            S.register_hook(lambda g: arrived.append(tuple(g.stride())))
            S.sum().backward()
            flags.append(ops._LAST_BWD_FLAGS[0])
        torch.cuda.synchronize()
    finally:
        ops.DENSE_GEMM_FORCE = old
        ops._generic_probes.clear()
    assert arrived == [(0, 0)]
    assert [bool(v & _lib.BWD_DENSE) for v in flags] == [False] * ops._DensityProbe.LAG + [True], flags
    assert_scores_close(S.detach().cpu().numpy(), O.alignment_scores(im, s, il, sl, 'MrSw', dtype=np.float64))
    d_im, d_s = O.alignment_scores_backward(im, s, il, sl, np.ones((B, B)))
    assert_grads_close(a.grad, d_im, bwd_mode)
    assert_grads_close(b.grad, d_s, bwd_mode)


def _square_float_tensors_held_by(node, B, skip):
    """the (B, B) float32 tensors reachable from an autograd node: its Python attributes (and what they hold) and, while the graph
    is alive, its saved tensors"""
    found, seen, todo = [], set(), [node]
    while todo:
        obj = todo.pop()
        if id(obj) in seen:
            continue
        seen.add(id(obj))
        if isinstance(obj, torch.Tensor):
            if tuple(obj.shape) == (B, B) and obj.dtype == torch.float32 and obj.data_ptr() not in skip:
                found.append(obj)
        elif not isinstance(obj, (type, type(gc))):
            todo.extend(gc.get_referents(obj))
    try:
        found += [t for t in node.saved_tensors if t is not None and tuple(t.shape) == (B, B) and t.data_ptr() not in skip]
    except RuntimeError:          # released: "Trying to backward through the graph a second time ..."
        pass
    return found


@pytest.mark.parametrize('B', [3, 65])
@pytest.mark.parametrize('loss_fn', ['hinge_loss', 'listnet_loss'])
def test_i_saved_gradient_nodes_accumulate_exactly_and_release_their_matrix(loss_fn, B):
    """the nodes whose forward leaves the gradient for an upstream 1, on the real kernels: two retained backwards give exactly twice
    the single gradient, and after a plain backward() no (B, B) float32 tensor is reachable from the node any more (the saved
    tensors are the only holders of the gradient matrix)"""
    from aladin_amd import ops
    rng = np.random.default_rng(B)
    to = AC.to_device(dev(), torch.float32)
    scores = to(rng.standard_normal((B, B)).astype(np.float32)).requires_grad_(True)
    teacher = to(rng.standard_normal((B, B)).astype(np.float32))
    loss = ops.hinge_loss(scores, 0.2, True) if loss_fn == 'hinge_loss' else ops.listnet_loss(teacher, scores)
    skip = {scores.data_ptr(), teacher.data_ptr()}
    assert len(_square_float_tensors_held_by(loss.grad_fn, B, skip)) == 1
    loss.backward(retain_graph=True)
    single = scores.grad.clone()
    assert bool(single.any())
    loss.backward(retain_graph=True)
    assert torch.equal(scores.grad, 2 * single)
    assert len(_square_float_tensors_held_by(loss.grad_fn, B, skip | {scores.grad.data_ptr(), single.data_ptr()})) == 1
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(scores.grad, 3 * single)
    assert _square_float_tensors_held_by(loss.grad_fn, B, skip | {scores.grad.data_ptr(), single.data_ptr()}) == []


from test_long_sets_gpu import bwd_mode          # noqa: E402,F401  (the fixture of the existing gradient tests)
