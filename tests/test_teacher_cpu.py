"""CPU tier of the cross-encoder teacher (teacher.get_teacher_scores, backbone.BertImgModel.forward(attention_window=),
ops.attention_window_mean / aladin_attn_window_mean): the float64 restatement (tests/helpers/teacher_numpy.py) pinned to the reference's
recorded float64 run of tests/golden/teacher.npz, the plain path against that run inside 4 x the float32 floor of the same inputs,
the grid shapes, the refusals that must come before a device is touched, the untouched default outputs, the binding and the
drop-in signatures."""
import functools
import inspect
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import teacher_numpy as TN               # noqa: E402

CASE_NAMES = [c[0] for c in TN.GOLDEN_CASES]


@functools.lru_cache(maxsize=None)
def golden():
    from aladin_amd import synth
    g, sig = TN.load_golden()
    assert int(g['n_cases']) == len(TN.GOLDEN_CASES) and int(g['text_len']) == TN.TEXT_LEN
    assert str(g['route']) in ('reference_function', 'recorded_outputs')
    out = {}
    for ci, (name, n, num_labels, subdivs, seed) in enumerate(TN.GOLDEN_CASES):
        pre = 'c%d_' % ci
        args = json.loads(str(g[pre + 'args']))
        assert str(g[pre + 'name']) == name
        assert args == dict(n=n, num_labels=num_labels, subdivs=subdivs, seed=seed, cfg=TN.golden_cfg(num_labels),
                            param_seed=TN.PARAM_SEED, param_scale=TN.PARAM_SCALE)
        ids, mask, _, feats, _ = TN.golden_inputs(n, seed)
        for key, val in (('ids', ids), ('mask', mask), ('feats', feats)):
            want = float(g[pre + key + '_checksum'])
            assert abs(synth.checksum(val) - want) <= 1e-9 * max(1.0, abs(want)), (name, key)
        out[name] = (n, num_labels, subdivs, seed, [str(x) for x in g[pre + 'param_names']], g[pre + 'scores'], g[pre + 'attentions'])
    return out, sig


def args_for(num_labels, device='cpu'):
    return types.SimpleNamespace(device=torch.device(device), num_labels=num_labels)


@functools.lru_cache(maxsize=None)
def teacher_floor(name):
    """(scores floor, attentions floor) of a golden case: the float32 all-layers path (output_attentions=True, every layer keeping
    its probabilities) against the reference's float64 run"""
    n, num_labels, _, seed, _, scores, att = golden()[0][name]
    side = int(round(n ** 0.5))
    m, _ = TN.build_model(num_labels, torch.float32, output_attentions=True)
    s32, a32 = TN.all_layers_teacher(m, TN.torch_batch(n, seed, torch.float32), num_labels, (side, side))
    return float(np.abs(s32 - scores).max()), float(np.abs(a32 - att).max())


@pytest.mark.parametrize('name', CASE_NAMES)
def test_restatement_equals_the_reference_run(name):
    """float64 model (the golden's weights; its parameter names are the reference's), the last layer's query / key outputs and the
    logits taken with hooks, then the numpy window formula and bookkeeping: the reference's scores and attentions to round-off"""
    n, num_labels, _, seed, names, scores, att = golden()[0][name]
    m, own_names = TN.build_model(num_labels, torch.float64)
    assert own_names == names
    keep = {}
    last = m.bert.encoder.layer[-1].attention.self
    hooks = [last.query.register_forward_hook(lambda mod, i, o: keep.__setitem__('q', o.detach().numpy())),
             last.key.register_forward_hook(lambda mod, i, o: keep.__setitem__('k', o.detach().numpy()))]
    batch = TN.torch_batch(n, seed, torch.float64)
    with torch.no_grad():
        logits = m(input_ids=batch[0], attention_mask=batch[1], token_type_ids=batch[2], img_feats=batch[3])[0].numpy()
    for h in hooks:
        h.remove()
    L = batch[1].shape[1]
    win = TN.window_mean(keep['q'], keep['k'], batch[1].numpy(), TN.GOLDEN_CFG['num_attention_heads'], (1, TN.TEXT_LEN - 1),
                         (TN.TEXT_LEN, L - TN.TEXT_LEN))
    side = int(round(n ** 0.5))
    s, a = TN.teacher_bookkeeping(logits, win, num_labels, (side, side))
    es, ea = float(np.abs(s - scores).max()), float(np.abs(a - att).max())
    print('%-20s restatement: scores %.2e attentions %.2e [tol %.0e]' % (name, es, ea, TN.RESTATEMENT_TOL))
    assert s.shape == scores.shape and a.shape == att.shape
    assert es <= TN.RESTATEMENT_TOL and ea <= TN.RESTATEMENT_TOL


@pytest.mark.parametrize('name', CASE_NAMES)
def test_get_teacher_scores_plain_path_matches_the_reference_run(name):
    from aladin_amd import teacher
    n, num_labels, subdivs, seed, _, scores, att = golden()[0][name]
    fs, fa = teacher_floor(name)
    m, _ = TN.build_model(num_labels, torch.float32)
    s, a = teacher.get_teacher_scores(args_for(num_labels), m, TN.torch_batch(n, seed, torch.float32), subdivs)
    es, ea = float(np.abs(s.double().numpy() - scores).max()), float(np.abs(a.double().numpy() - att).max())
    print('%-20s plain path: scores %.2e [floor %.2e gate %.2e]  attentions %.2e [floor %.2e gate %.2e]'
          % (name, es, fs, TN.GATE_FACTOR * fs, ea, fa, TN.GATE_FACTOR * fa))
    assert tuple(s.shape) == scores.shape and tuple(a.shape) == att.shape and s.dtype == a.dtype == torch.float32
    assert a.stride(3) == 1 and a.stride(2) >= a.shape[3]                 # what AttentionDistillationLoss reads in place
    assert es <= TN.GATE_FACTOR * fs and ea <= TN.GATE_FACTOR * fa
    # the reference's positional call and forcing the plain path are the same computation
    s2, a2 = teacher.get_teacher_scores(args_for(num_labels), m, TN.torch_batch(n, seed, torch.float32), subdivs, fused=False)
    assert torch.equal(s, s2) and torch.equal(a, a2)


def test_rectangular_grid_and_the_square_assertion():
    from aladin_amd import teacher
    n, num_labels, _, seed, _, scores, att = golden()[0]['grid3x3_labels2']
    fs, fa = teacher_floor('grid3x3_labels2')
    m, _ = TN.build_model(num_labels, torch.float32)
    six = tuple(t[:6] for t in TN.torch_batch(n, seed, torch.float32))
    s, a = teacher.get_teacher_scores(args_for(num_labels), m, six, 4, shape=(2, 3))
    assert tuple(s.shape) == (2, 3) and tuple(a.shape) == (2, 3, TN.TEXT_LEN - 1, TN.N_REGIONS)
    assert np.abs(s.double().numpy() - scores.reshape(-1)[:6].reshape(2, 3)).max() <= TN.GATE_FACTOR * fs
    assert np.abs(a.double().numpy() - att.reshape(9, TN.TEXT_LEN - 1, -1)[:6].reshape(a.shape)).max() <= TN.GATE_FACTOR * fa
    with pytest.raises(AssertionError):
        teacher.get_teacher_scores(args_for(num_labels), m, six)                      # 6 is no square: the reference's assertion
    with pytest.raises(ValueError):
        teacher.get_teacher_scores(args_for(num_labels), m, six, shape=(2, 2))
    with pytest.raises(ValueError):
        teacher.get_teacher_scores(args_for(num_labels), m, six, 0, shape=(2, 3))


def test_text_len_moves_the_window():
    from aladin_amd import teacher
    n, num_labels, _, seed, _, _, _ = golden()[0]['grid2x2_subdivs2']
    m, _ = TN.build_model(num_labels, torch.float32)
    batch = TN.torch_batch(n, seed, torch.float32)
    _, a = teacher.get_teacher_scores(args_for(num_labels), m, batch, text_len=60)
    L = batch[1].shape[1]
    assert tuple(a.shape) == (2, 2, 59, L - 60)
    _, a70 = teacher.get_teacher_scores(args_for(num_labels), m, batch)
    assert torch.equal(a[:, :, :, 10:], a70[:, :, :59])                      # the same probabilities, another cut
    with pytest.raises(ValueError):
        teacher.get_teacher_scores(args_for(num_labels), m, batch, text_len=L)


def test_fused_true_raises_without_a_gpu_tensor():
    from aladin_amd import ops, teacher
    n, num_labels, _, seed, _, _, _ = golden()[0]['grid2x2_subdivs2']
    m, _ = TN.build_model(num_labels, torch.float32)
    with pytest.raises(RuntimeError, match='fused attention window cannot run'):
        teacher.get_teacher_scores(args_for(num_labels), m, TN.torch_batch(n, seed, torch.float32), fused=True)
    q = torch.zeros(2, 5, 8)
    with pytest.raises(ValueError):
        ops.attention_window_mean(q, q, torch.ones(2, 5), 2, (0, 5), (0, 5))


def test_python_refusals_name_the_limit():
    from aladin_amd import ops
    q = torch.zeros(2, 5, 8)
    assert 'GPU' in ops.attention_window_unsupported(q, q, torch.ones(2, 5), 2)
    assert ops.attention_window_unsupported(q, q, torch.ones(2, 5, 5), 2) is not None
    for rows, cols in (((0, 6), (0, 5)), ((0, 5), (3, 3)), ((-1, 2), (0, 5)), ((0, 0), (0, 5))):
        with pytest.raises(ValueError):
            ops._window_args(5, rows, cols)
    assert ops._window_args(5, (1, 4), (2, 3)) == (1, 4, 2, 3)


def test_plain_window_of_the_model_is_the_all_layers_slice():
    """attention_window on the CPU: the last layer's probabilities cut with torch ops -- bit-equal to slicing what output_attentions
    returns for that layer, while the layers below stay on SDPA"""
    n, num_labels, _, seed, _, _, _ = golden()[0]['grid2x2_subdivs2']
    m, _ = TN.build_model(num_labels, torch.float32)
    ma, _ = TN.build_model(num_labels, torch.float32, output_attentions=True)
    b = TN.torch_batch(n, seed, torch.float32)
    with torch.no_grad():
        o = m.bert(b[0], token_type_ids=b[2], attention_mask=b[1], img_feats=b[3], attention_window=(1, 69, 70, 12))
        oa = ma.bert(b[0], token_type_ids=b[2], attention_mask=b[1], img_feats=b[3])
        o3 = m.bert(b[0], token_type_ids=b[2], attention_mask=b[1][:, None, :].expand(-1, 82, -1), img_feats=b[3],
                    attention_window=(1, 69, 70, 12))
    assert len(o) == 3 and tuple(o[-1].shape) == (n, 69, 12)
    np.testing.assert_allclose(o[-1].numpy(), oa[2][-1].mean(dim=1)[:, 1:70, 70:].numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose(o3[-1].numpy(), o[-1].numpy(), rtol=0, atol=2e-7)      # a 3-D mask takes the plain path too
    with pytest.raises(ValueError):
        m.bert(b[0], token_type_ids=b[2], attention_mask=b[1], img_feats=b[3], attention_window=(1, 69, 70, 13))


@pytest.mark.parametrize('flags', [dict(), dict(output_attentions=True, output_hidden_states=True)])
def test_default_outputs_are_untouched(flags):
    from aladin_amd import backbone
    torch.manual_seed(3)
    cfg = backbone.BertConfig(**dict(TN.GOLDEN_CFG, **flags))
    m = backbone.BertImgModel(cfg).eval()
    b = TN.torch_batch(4, 1813, torch.float32)
    with torch.no_grad():
        o0 = m(b[0], token_type_ids=b[2], attention_mask=b[1], img_feats=b[3])
        o1 = m(b[0], token_type_ids=b[2], attention_mask=b[1], img_feats=b[3], attention_window=None)
        ow = m(b[0], token_type_ids=b[2], attention_mask=b[1], img_feats=b[3], attention_window=(1, 69, 70, 12))
    assert len(o0) == len(o1) == (4 if flags else 2) and len(ow) == len(o0) + 1

    def flat(o):
        return [t for x in o for t in (x if isinstance(x, tuple) else (x,))]
    assert all(torch.equal(x, y) for x, y in zip(flat(o0), flat(o1)))
    params = list(inspect.signature(backbone.BertImgModel.forward).parameters)
    assert params[:8] == ['self', 'input_ids', 'token_type_ids', 'attention_mask', 'position_ids', 'head_mask', 'img_feats',
                          'encoder_history_states']


def test_symbol_version_and_limit_constants():
    from aladin_amd import _lib
    assert 'aladin_attn_window_mean' in _lib.SYMBOLS and _lib.ABI_VERSION == 13
    hdr = open(os.path.join(ROOT, 'include', 'aladin_hip.h')).read()
    assert re.search(r'#define\s+ALADIN_ABI_VERSION\s+13\b', hdr)
    for name, val in (('ALADIN_ATTN_WINDOW_MAX_L', _lib.ATTN_WINDOW_MAX_L), ('ALADIN_ATTN_WINDOW_MAX_DH', _lib.ATTN_WINDOW_MAX_DH),
                      ('ALADIN_ATTN_WINDOW_MAX_HEADS', _lib.ATTN_WINDOW_MAX_HEADS)):
        mt = re.search(r'#define\s+%s\s+(\d+)' % name, hdr)
        assert mt and int(mt.group(1)) == val, name
    assert (_lib.ATTN_WINDOW_MAX_L, _lib.ATTN_WINDOW_MAX_DH, _lib.ATTN_WINDOW_MAX_HEADS) == (256, 128, 32)
    assert re.search(r'ALADIN_API int aladin_attn_window_mean\(', hdr)
    lib = _lib.load()
    assert lib.aladin_version() == 13 and hasattr(lib, 'aladin_attn_window_mean')
    assert len(_lib.SIGNATURES['aladin_attn_window_mean'][1]) == 22


def test_signatures_are_the_references():
    from aladin_amd import backbone, teacher
    _, sig = golden()

    def record(fn):
        return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                for p in inspect.signature(fn).parameters.values()]
    own = record(teacher.get_teacher_scores)
    ref = sig['get_teacher_scores']
    assert own[:len(ref)] == ref
    assert [p[:2] for p in own[len(ref):]] == [['shape', 'KEYWORD_ONLY'], ['text_len', 'KEYWORD_ONLY'], ['fused', 'KEYWORD_ONLY']]
    own = record(backbone.ImageBertForSequenceClassification.forward)
    ref = sig['ImageBertForSequenceClassification.forward']
    assert own[:len(ref)] == ref and all(p[2] == 'None' for p in own[len(ref):])
