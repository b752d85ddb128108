"""CPU tier: the host side of ROUGE-L relevance (aladin_rouge_l, ops.rouge_l_relevance, aladin_amd.rouge, DCG.from_captions) --
argument and limit checks that must hold before a device is touched, the tokenizer, the drop-in signatures -- and the two
restatements (tests/helpers/rouge_numpy.py) pinned bit for bit to the reference's recorded float32 matrix, which is what the GPU
tier compares the kernel with."""
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
import rouge_numpy as R                  # noqa: E402

ERR_ARG, ERR_UNSUPPORTED = 1, 2          # ALADIN_ERR_* of include/aladin_hip.h
AWKWARD = ['a  b', ' a b', 'a b ', '', ' ', 'A b\tC d', 'The DOG', 'a\nb c', '  ']


def lib():
    from aladin_amd import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rouge(p, **kw):
    """aladin_rouge_l on HOST buffers: every call below must be refused before a launch."""
    a = dict(q_tok=p, q_off=p, q_rows=p, n_q=2, q_max_len=20, g_tok=p, g_off=p, n_g=10, g_max_len=20, grp_off=p, n_img=2, out=p, ld_out=2,
             flags=0)
    a.update(kw)
    return lib().aladin_rouge_l(a['q_tok'], a['q_off'], a['q_rows'], a['n_q'], a['q_max_len'], a['g_tok'], a['g_off'], a['n_g'],
                                a['g_max_len'], a['grp_off'], a['n_img'], a['out'], a['ld_out'], a['flags'], None)


def test_entry_point_checks_arguments_before_touching_a_device():
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    for kw in ({'q_tok': null}, {'q_off': null}, {'g_tok': null}, {'g_off': null}, {'grp_off': null}, {'out': null}, {'n_q': 0}, {'n_q': -3},
               {'n_g': 0}, {'n_img': 0}, {'ld_out': 1}, {'flags': 2}, {'flags': -1}, {'flags': 3},
               {'q_tok': null, 'q_max_len': 300}):                           # a bad argument is reported before a bad limit
        assert _rouge(p, **kw) == ERR_ARG, kw
        assert b'rouge_l' in lib().aladin_last_error()
    for kw in ({'q_max_len': 0}, {'q_max_len': 257}, {'g_max_len': 0}, {'g_max_len': 257}, {'q_max_len': -1, 'q_rows': null}):
        assert _rouge(p, **kw) == ERR_UNSUPPORTED, kw
        msg = lib().aladin_last_error().decode()
        assert 'rouge_l' in msg and '256' in msg, msg
    assert lib().aladin_version() == 13                  # 13: the alignment geometry's layout field (this entry point: unchanged since it was added)


def test_tokenize_is_the_reference_split():
    from aladin_amd import rouge
    tok, off, vocab = rouge.tokenize(AWKWARD)
    assert tok.dtype == np.int32 and off.dtype == np.int64 and off[0] == 0 and len(off) == len(AWKWARD) + 1
    back = {i: t for t, i in vocab.items()}
    assert len(back) == len(vocab) and sorted(back) == list(range(len(vocab)))
    for c, (b, e) in zip(AWKWARD, zip(off[:-1], off[1:])):
        assert [back[i] for i in tok[b:e]] == c.lower().split(" ") == R.tokens(c), c
    assert [int(e - b) for b, e in zip(off[:-1], off[1:])] == [3, 3, 3, 1, 2, 3, 2, 2, 3]
    assert vocab[''] == vocab.get('') and 'b\tc' in vocab and 'a\nb' in vocab and 'the' in vocab and 'The' not in vocab
    tok2, off2, v2 = rouge.tokenize(['cat the'], vocab)
    assert v2 is vocab and tok2[1] == vocab['the'] and tok2[0] == len(back)
    with pytest.raises(TypeError):
        rouge.tokenize([['a', 'b']])


def test_restatements_give_the_reference_matrix_bit_for_bit():
    g = load_golden('rouge_small')
    caps = [str(c) for c in g['captions']]
    rel = g['relevance']
    n_img = rel.shape[1]
    assert rel.dtype == np.float32 and rel.shape == (120, 24) and len(caps) == 120 and int(g['caps_per_img']) == 5
    loner, twin_a, twin_b, cased, doubled, empty = (int(v) for v in g['specials'])
    lens = {len(R.tokens(c)) for c in caps}
    assert {1, 2, 3, 5, 8, 12, 13, 20, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 256} <= lens
    assert caps[empty] == '' and '  ' in caps[doubled] and '' in R.tokens(caps[doubled]) and caps[cased] != caps[cased].lower()
    assert caps[twin_a] == caps[twin_b] and twin_a // 5 != twin_b // 5
    assert (rel[np.arange(120), np.arange(120) // 5] == 1.0).all()
    assert (np.delete(rel[loner], loner // 5) == 0.0).all() and 0 < (rel == 0).mean() < 0.5
    assert rel[twin_a, twin_b // 5] == 1.0 and rel[twin_b, twin_a // 5] == 1.0
    assert 1.2 * 1.2 == 1.2 ** 2 == R.BETA2
    fast = R.caption_relevance(caps, 5, R.lcs_bits)
    assert np.array_equal(bits(fast), bits(rel)), int((bits(fast) != bits(rel)).sum())
    slow = R.caption_relevance(caps, 5, R.lcs_dp)
    assert np.array_equal(bits(slow), bits(rel)), int((bits(slow) != bits(rel)).sum())
    assert n_img == 24 and R.score(R.tokens('a  b'), [R.tokens('a b')]) == 0.8299319727891156


def test_drop_in_signatures_match_the_reference():
    """Same names, order, kinds and defaults as the reference's; trailing parameters only with a default."""
    from aladin_amd import rouge
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'signatures_rouge.json')))
    homes = {'Rouge.score': rouge.Rouge.score, 'my_lcs': rouge.my_lcs}
    assert set(ref) == set(homes)
    for key, want in ref.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(homes[key]).parameters.values()]
        assert got[:len(want)] == want, (key, got, want)
        for extra in got[len(want):]:
            assert extra[2] is not None or extra[1] in ('VAR_POSITIONAL', 'VAR_KEYWORD'), (key, 'extra parameter without a default', extra)
    assert rouge.Rouge().beta == 1.2
    assert [p for p in inspect.signature(rouge.relevance_matrix).parameters] == ['captions', 'caps_per_img', 'queries']
    assert [p for p in inspect.signature(rouge.write_relevance_file).parameters] == ['config', 'split', 'captions', 'method', 'chunk']


def test_python_layer_raises_value_error_before_the_device(tmp_path):
    from aladin_amd import dcg, ops, rouge
    caps = ['a b c'] * 10
    for call in (lambda: rouge.relevance_matrix([]), lambda: rouge.relevance_matrix(caps[:7]), lambda: rouge.relevance_matrix(caps, 3),
                 lambda: rouge.relevance_matrix(caps, 0), lambda: dcg.DCG.from_captions([]), lambda: dcg.DCG.from_captions(caps[:9]),
                 lambda: dcg.DCG.from_captions(caps, caps_per_img=2),
                 lambda: rouge.write_relevance_file({'dataset': {'data': str(tmp_path), 'name': 'toy'}}, 'test', caps, method='spice'),
                 lambda: rouge.write_relevance_file({'dataset': {'data': str(tmp_path), 'name': 'toy'}}, 'test', caps[:3]),
                 lambda: rouge.write_relevance_file({'dataset': {'data': str(tmp_path), 'name': 'toy'}}, 'test', caps, chunk=0)):
        with pytest.raises(ValueError):
            call()
    assert not os.path.exists(tmp_path / 'toy')
    tok = torch.zeros(12, dtype=torch.int32)
    off = torch.tensor([0, 4, 8, 12])
    grp = torch.tensor([0, 3])
    good = dict(q_tok=tok, q_off=off, g_tok=tok, g_off=off, grp_off=grp)
    bad = [dict(q_tok=tok.long()), dict(q_tok=tok.reshape(3, 4)), dict(q_off=off.int()), dict(q_off=off[:1]), dict(g_tok=tok.float()),
           dict(g_off=off.tolist()), dict(grp_off=grp.int()), dict(grp_off=grp[:1]), dict(q_rows=torch.zeros(3, dtype=torch.int32))]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.rouge_l_relevance(**a)
    out = torch.zeros((3, 1))
    for kw in (dict(q_max_len=0), dict(q_max_len=257), dict(g_max_len=0), dict(g_max_len=300), dict(out=torch.zeros((3, 2))),
               dict(out=torch.zeros((2, 1))), dict(out=out.double()), dict(q_rows=torch.zeros(3, dtype=torch.int64)),
               dict(q_rows=torch.zeros(2, dtype=torch.int32))):
        a = dict(q_tok=tok, q_off=off, q_max_len=4, g_tok=tok, g_off=off, g_max_len=4, grp_off=grp, out=out)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.rouge_l_launch(**a)


def test_cpu_tensors_are_refused_never_computed(monkeypatch):
    from aladin_amd import ops, rouge
    tok = torch.zeros(12, dtype=torch.int32)
    off = torch.tensor([0, 4, 8, 12])
    grp = torch.tensor([0, 3])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.rouge_l_relevance(tok, off, tok, off, grp)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.rouge_l_launch(tok, off, 4, tok, off, 4, grp, torch.zeros((3, 1)))
    if not torch.cuda.is_available():
        for call in (lambda: rouge.relevance_matrix(['a b'] * 5), lambda: rouge.Rouge().score(['a b'], ['a b']),
                     lambda: rouge.my_lcs(['a', 'b'], ['a'])):
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                call()
    with pytest.raises(AssertionError):
        rouge.Rouge().score(['a', 'b'], ['a'])
    with pytest.raises(AssertionError):
        rouge.Rouge().score(['a'], [])
