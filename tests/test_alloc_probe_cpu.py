"""CPU tier: the allocation probe (tests/helpers/alloc_probe.py) on small fake "ops" -- plain Python on CPU tensors that allocate
through torch.empty / torch.empty_like from a module named like a library module.  The correct op passes record / stale / clean;
every planted defect (an unwritten element, an accumulator that is not zeroed, a write one element past either end, a changed
allocation order, an unsupported keyword) is reported, and the report names the allocation."""
import os
import sys
import types

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import alloc_probe as P                  # noqa: E402

FAKE_OPS = '''
import torch

ORDER = [0]


def correct(x):
    ws = torch.empty(x.numel() * 4, dtype=torch.uint8, device=x.device)        # a workspace, sliced and viewed as the library does
    acc = ws[0:4 * x.numel()].view(torch.float32)
    acc.zero_()
    acc += x.reshape(-1)
    out = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32)
    out.copy_(acc.view_as(x) * 2)
    count = torch.empty(1, dtype=torch.int32)
    count[0] = int((x > 0).sum())
    scalar = torch.empty((), dtype=torch.float32)
    scalar.fill_(float(x.sum()))
    return out, count, scalar


def unwritten(x):
    out = torch.empty(x.shape, dtype=torch.float32)
    rows = x.shape[0] if float(x[0, 0]) > 0 else x.shape[0] - 1              # a "length": full on the donor, short on the probed problem
    out[:rows] = x[:rows] * 2
    out[rows:, :-1] = 0                                                        # past the length all but the last element is zeroed
    return (out,)


def accumulates(x):
    acc = torch.empty(x.shape[1], dtype=torch.float32)                         # (no zeroing)
    for row in x:
        acc += row
    return (acc,)


def past_the_end(x):
    out = torch.empty_like(x)
    out.copy_(x)
    out.as_strided((1,), (1,), out.storage_offset() + x.numel()).fill_(7.0)
    return (out,)


def before_the_start(x):
    out = torch.empty(x.numel(), dtype=torch.int16)
    out.zero_()
    out.as_strided((1,), (1,), out.storage_offset() - 1).fill_(7)
    return (out,)


def reorders(x):
    shapes = [(3,), (5,)] if ORDER[0] % 2 == 0 else [(5,), (3,)]
    ORDER[0] += 1
    outs = [torch.empty(s, dtype=torch.float32) for s in shapes]
    for o in outs:
        o.fill_(1.0)
    return tuple(outs)


def one_more(x):
    n = 1 + ORDER[0] % 2
    ORDER[0] += 1
    outs = [torch.empty(3, dtype=torch.float32) for _ in range(n)]
    for o in outs:
        o.fill_(1.0)
    return tuple(outs)


def out_keyword(x):
    y = torch.zeros(3)
    return (torch.empty(3, out=y),)


def channels_last(x):
    return (torch.empty_like(x.reshape(1, 1, *x.shape), memory_format=torch.channels_last),)


def pinned(x):
    return (torch.empty(3, pin_memory=True),)


def permuted_like(x):
    out = torch.empty_like(x.t(), dtype=torch.float32)                         # a dense permutation keeps its strides
    out.copy_(x.t())
    return (out,)
'''


def load_fake(name):
    """the fake ops as a module whose __name__ is `name` (never registered: only its frames' module name matters)"""
    mod = types.ModuleType(name)
    mod.__file__ = os.path.join('fake', name.replace('.', '/') + '.py')
    exec(compile(FAKE_OPS, mod.__file__, 'exec'), mod.__dict__)
    return mod


FAKE = load_fake('fakelib.ops')
IS_FAKE = lambda name: name.startswith('fakelib')         # noqa: E731 -- the injected module-name test
X = torch.arange(1.0, 13.0).reshape(3, 4)                 # the donor problem: every element non-zero
Y = -torch.arange(2.0, 14.0).reshape(3, 4) / 3.0          # the probed problem: other values, same shapes


def three(op):
    return P.run_three_passes(op, X, Y, is_library=IS_FAKE)


def test_a_correct_op_passes_all_three_modes():
    probes, stale, clean = three(FAKE.correct)
    assert [p.mode for p in probes] == ['record', 'stale', 'clean']
    for p in probes:
        assert p.intercepted == 4 and p.passed_through_device == 0
        assert [a.shape for a in p.allocations] == [(48,), (3, 4), (1,), ()]
        assert [a.dtype for a in p.allocations] == [torch.uint8, torch.float32, torch.int32, torch.float32]
    assert probes[1].seeded == 4 and probes[0].seeded == probes[2].seeded == 0
    P.assert_same_outputs(probes[1], stale, probes[2], clean)
    assert torch.equal(clean[0], Y * 2) and int(clean[1]) == 0 and float(clean[2]) == float(Y.sum())
    assert torch.empty is P._REAL_EMPTY and torch.empty_like is P._REAL_EMPTY_LIKE         # restored


def test_the_views_are_contiguous_aligned_and_seeded_from_the_donor():
    with P.AllocProbe('record', is_library=IS_FAKE) as rec:
        out, count, scalar = FAKE.correct(X)
        mine = torch.empty(5)                             # this module is not the library: falls through
    assert rec.foreign == 1 and rec.intercepted == 4 and mine.shape == (5,)
    assert out.is_contiguous() and out.data_ptr() % 16 == 0 and scalar.dim() == 0 and count.data_ptr() % 16 == 0
    with P.AllocProbe('stale', donor=rec, is_library=IS_FAKE) as st:
        assert FAKE.__dict__['torch'].empty is not P._REAL_EMPTY        # the patched function, as the fake module sees it
        FAKE.correct(Y)
    assert st.seeded == st.intercepted == 4
    with P.AllocProbe('stale', donor=rec, is_library=IS_FAKE) as st2:                      # what an allocation starts as
        got = eval('torch.empty(48, dtype=torch.uint8)', FAKE.__dict__)                    # (evaluated as code of the fake module)
        assert torch.equal(got, rec.allocations[0].data())
        for a in rec.allocations[1:]:
            eval('torch.empty(%r, dtype=%s)' % (a.shape, a.dtype), FAKE.__dict__)
    assert st2.seeded == 4
    with P.AllocProbe('clean', is_library=IS_FAKE):
        z = eval('torch.empty((2, 3), dtype=torch.float64)', FAKE.__dict__)
        assert z.dtype == torch.float64 and z.shape == (2, 3) and not bool(z.any())
        e = eval('torch.empty((0, 3))', FAKE.__dict__)
        assert e.shape == (0, 3)


def test_the_default_module_test_is_the_library_package():
    assert P.library_module('aladin_amd') and P.library_module('aladin_amd.ops_losses')
    assert not P.library_module('aladin_amd_extra') and not P.library_module('tests.aladin_amd') and not P.library_module('torch')
    named = load_fake('aladin_amd._probe_selftest')
    probes, stale, clean = P.run_three_passes(named.correct, X, Y)
    assert all(p.intercepted == 4 for p in probes)
    with P.AllocProbe('record') as p:                     # the same code under another name is nobody's business
        FAKE.correct(X)
    assert p.intercepted == 0 and p.foreign == 4


def test_an_unwritten_element_is_reported_with_its_allocation():
    probes, stale, clean = three(FAKE.unwritten)
    assert float(stale[0][-1, -1]) == float(X[-1, -1]) * 2 and float(clean[0][-1, -1]) == 0.0        # the donor's value shows
    assert torch.equal(stale[0].reshape(-1)[:-1], clean[0].reshape(-1)[:-1])
    with pytest.raises(P.ProbeError, match=r'output 0 depends on what its memory held.*allocation #0 at fake/fakelib/ops\.py:\d+, '
                                           r'shape \(3, 4\), dtype torch\.float32'):
        P.assert_same_outputs(probes[1], stale, probes[2], clean)


def test_an_accumulator_that_is_not_zeroed_is_reported():
    probes, stale, clean = three(FAKE.accumulates)
    assert torch.equal(clean[0], Y.sum(0)) and not torch.equal(stale[0], clean[0])
    with pytest.raises(P.ProbeError, match=r'allocation #0 at fake/fakelib/ops\.py:\d+, shape \(4,\)'):
        P.assert_same_outputs(probes[1], stale, probes[2], clean, names=['acc'])


@pytest.mark.parametrize('mode', ['record', 'clean'])
def test_a_write_past_the_end_hits_the_back_guard(mode):
    with pytest.raises(P.ProbeError, match=r'back guard band overwritten \(4 bytes changed, reaching 4 byte\(s\) past its end\) of '
                                           r'allocation #0 at fake/fakelib/ops\.py:\d+, shape \(3, 4\), dtype torch\.float32'):
        with P.AllocProbe(mode, is_library=IS_FAKE):
            FAKE.past_the_end(X)
    assert torch.empty is P._REAL_EMPTY


def test_a_write_before_the_start_hits_the_front_guard():
    with pytest.raises(P.ProbeError, match=r'front guard band overwritten \(2 bytes changed, reaching 2 byte\(s\) before its start\) '
                                           r'of allocation #0 at fake/fakelib/ops\.py:\d+, shape \(12,\), dtype torch\.int16'):
        with P.AllocProbe('record', is_library=IS_FAKE):
            FAKE.before_the_start(X)


def test_a_changed_allocation_sequence_raises():
    FAKE.ORDER[0] = 0
    with pytest.raises(P.ProbeError, match=r'allocation sequence changed: allocation #0 at .* shape \(5,\).*donor pass made '
                                           r'allocation #0 at .* shape \(3,\)'):
        three(FAKE.reorders)
    FAKE.ORDER[0] = 0                                     # one allocation in the donor pass, two in the stale one
    with pytest.raises(P.ProbeError, match='no counterpart in the donor pass'):
        three(FAKE.one_more)
    FAKE.ORDER[0] = 1                                     # two in the donor pass, one in the stale one
    with pytest.raises(P.ProbeError, match='donor pass made 2 allocations, this pass 1'):
        three(FAKE.one_more)
    assert torch.empty is P._REAL_EMPTY


@pytest.mark.parametrize('op, what', [('out_keyword', 'unsupported keyword.*out'), ('channels_last', 'unsupported memory_format'),
                                      ('pinned', 'pin_memory')])
def test_an_unsupported_keyword_raises(op, what):
    with pytest.raises(P.ProbeError, match=what + r'.*fake/fakelib/ops\.py:\d+'):
        with P.AllocProbe('clean', is_library=IS_FAKE):
            getattr(FAKE, op)(X)
    assert torch.empty is P._REAL_EMPTY


def test_empty_like_of_a_dense_permutation_keeps_its_strides():
    probes, stale, clean = three(FAKE.permuted_like)
    assert stale[0].shape == (4, 3) and stale[0].stride() == (1, 4) and torch.equal(clean[0], Y.t())
    P.assert_same_outputs(probes[1], stale, probes[2], clean)


def test_misuse_of_the_modes_raises():
    with pytest.raises(ValueError):
        P.AllocProbe('dirty')
    with pytest.raises(ValueError):
        P.AllocProbe('stale')
    rec = P.AllocProbe('record', is_library=IS_FAKE)
    with pytest.raises(ValueError):
        P.AllocProbe('stale', donor=rec)                  # not finished
    with rec:
        with pytest.raises(RuntimeError, match='do not nest'):
            P.AllocProbe('clean').__enter__()
    with pytest.raises(P.ProbeError, match='0 allocations intercepted'):
        with P.AllocProbe('stale', donor=rec, is_library=IS_FAKE):
            pass                                          # nothing intercepted: a stale pass that probes nothing is no pass

