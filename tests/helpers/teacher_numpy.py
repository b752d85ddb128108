"""numpy restatement of the cross-encoder teacher's attention window and bookkeeping (reference alad/train.py:340-384 over
oscar/modeling/modeling_bert.py:47-53), the inputs of its tests, and their gates.

    window_mean(q, k, mask, heads, rows, cols, dtype)   the formula of include/aladin_hip.h (aladin_attn_window_mean) in float64, or in
                                                        float32 to measure what that format alone costs (the fp32 floor)
    teacher_bookkeeping(logits, window, num_labels, shape)   softmax column 1 / logits, the two views
    fp32_floor(...)                                     max |float32 evaluation - float64 evaluation| on the SAME float32 inputs

Gates (the project's convention): a result may be GATE_FACTOR x the fp32 floor of its own inputs away from the float64 value.
Measured floors of the window formula (max over the kernel cases of tests/test_teacher_gpu.py, numpy float32 against float64):
FLOOR_WINDOW_MEASURED below; of get_teacher_scores on the golden cases (the float32 `output_attentions=True` path of the backbone,
every layer keeping its probabilities, against the reference's float64 run): FLOOR_TEACHER_SCORES_MEASURED /
FLOOR_TEACHER_ATT_MEASURED.  The tests measure the floor of each case again and gate on THAT figure; the constants are the record
(DESIGN.md 4.3.2).
"""
import json
import os

import numpy as np

from aladin_amd import synth

GATE_FACTOR = 4.0
FLOOR_WINDOW_MEASURED = 1.0e-6            # logits of +-60 (scaled q, k); the other kernel cases 7.8e-9 .. 7.0e-8
FLOOR_TEACHER_SCORES_MEASURED = 1.3e-7    # worst golden case (grid3x3_labels1: raw logits); the two-label cases 3.8e-8 .. 5.4e-8
FLOOR_TEACHER_ATT_MEASURED = 2.6e-8       # worst golden case; the others 6.6e-9 .. 1.8e-8
ZERO_MASK_ABS = 2e-3                      # an all-zero mask: -10000 + s rounds s to ulp(1e4) = 2^-10; against the float32 plain path
RESTATEMENT_TOL = 1e-12                   # float64 against float64

TEXT_LEN = 70                             # the reference's slice: rows [1, 70), columns [70, L)
GOLDEN_CFG = dict(vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=160,
                  hidden_act='gelu', hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, max_position_embeddings=70,
                  type_vocab_size=2, initializer_range=0.02, layer_norm_eps=1e-12, img_feature_dim=22,
                  img_feature_type='faster_r-cnn', use_img_layernorm=1, img_layer_norm_eps=1e-12, num_labels=2, loss_type='sfmx')
N_REGIONS = 12
PARAM_SEED, PARAM_SCALE = 1801, 0.08

# name, sequences (a square grid), num_labels, subdivs, input seed
GOLDEN_CASES = [
    ('grid3x3_labels2', 9, 2, 40, 1811),
    ('grid3x3_labels1', 9, 1, 40, 1812),
    ('grid2x2_subdivs2', 4, 2, 2, 1813),        # len % subdivs == 0: no empty chunk
    ('grid2x2_subdivs40', 4, 2, 40, 1814),      # one chunk larger than the batch
]


def golden_cfg(num_labels):
    cfg = dict(GOLDEN_CFG)
    cfg['num_labels'] = num_labels
    return cfg


def golden_inputs(n, seed, n_tok=TEXT_LEN, n_reg=N_REGIONS, vocab=120, feat=22):
    """(input_ids, attention_mask (n, n_tok + n_reg), token_type_ids, img_feats, labels): ragged captions padded with id 0 and ragged
    region counts, one full caption and one full region set."""
    ids = synth.integers((n, n_tok), 1, vocab - 1, seed).astype(np.int64)
    cap_len = synth.integers((n,), 6, n_tok, seed + 1)
    reg_len = synth.integers((n,), 3, n_reg, seed + 2)
    cap_len[0], reg_len[1] = n_tok, n_reg
    tmask = (np.arange(n_tok)[None, :] < cap_len[:, None]).astype(np.int64)
    rmask = (np.arange(n_reg)[None, :] < reg_len[:, None]).astype(np.int64)
    ids = ids * tmask
    types = np.zeros((n, n_tok), np.int64)
    feats = (synth.normal((n, n_reg, feat), seed + 3) * rmask[:, :, None]).astype(np.float32)
    labels = (np.arange(n) % 2).astype(np.int64)
    return ids, np.concatenate([tmask, rmask], 1), types, feats, labels


def load_golden():
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
    with open(os.path.join(here, 'signatures_teacher.json')) as f:
        sig = json.load(f)
    return np.load(os.path.join(here, 'teacher.npz')), sig


def window_mean(q, k, mask, heads, rows, cols, dtype=np.float64):
    """q, k (N, L, heads * dh), mask (N, L) of 0 / 1 -> (N, W, Rw): every operation carried out in `dtype`."""
    q, k = np.asarray(q, dtype), np.asarray(k, dtype)
    N, L, HD = q.shape
    dh = HD // heads
    qh = q.reshape(N, L, heads, dh).transpose(0, 2, 1, 3)
    kh = k.reshape(N, L, heads, dh).transpose(0, 2, 3, 1)
    add = ((dtype(1.0) - np.asarray(mask, dtype)) * dtype(-10000.0))[:, None, None, :]
    s = np.matmul(qh, kh) / dtype(np.sqrt(dtype(dh))) + add
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True, dtype=dtype)
    assert p.dtype == dtype
    return p.mean(axis=1, dtype=dtype)[:, rows[0]:rows[0] + rows[1], cols[0]:cols[0] + cols[1]]


def fp32_floor(q, k, mask, heads, rows, cols):
    """-> (floor, float64 reference): what evaluating the formula in float32 costs on these float32 inputs"""
    ref = window_mean(q, k, mask, heads, rows, cols, np.float64)
    return float(np.abs(window_mean(q, k, mask, heads, rows, cols, np.float32).astype(np.float64) - ref).max()), ref


def window_plain_torch(q, k, mask, heads, rows, cols):
    """the same formula in torch ops on the tensors' device and dtype (matmul, add the mask, softmax, mean over heads, slice): what a
    model without the kernel computes for one layer"""
    import torch
    N, L, HD = q.shape
    dh = HD // heads
    qh = q.view(N, L, heads, dh).permute(0, 2, 1, 3)
    kh = k.view(N, L, heads, dh).permute(0, 2, 1, 3)
    add = ((1.0 - mask.to(q.dtype)) * -10000.0)[:, None, None, :]
    probs = torch.softmax(torch.matmul(qh, kh.transpose(-1, -2)) / (dh ** 0.5) + add, dim=-1)
    return probs.mean(dim=1)[:, rows[0]:rows[0] + rows[1], cols[0]:cols[0] + cols[1]]


def teacher_bookkeeping(logits, window, num_labels, shape):
    """the reference's five lines after the model call: softmax column 1 (two labels) or the logits, and the views"""
    logits = np.asarray(logits, np.float64)
    if num_labels == 2:
        e = np.exp(logits - logits.max(axis=1, keepdims=True))
        result = (e / e.sum(axis=1, keepdims=True))[:, 1]
    else:
        result = logits
    Bi, Bc = shape
    window = np.asarray(window, np.float64)
    return result.reshape(Bi, Bc), window.reshape(Bi, Bc, window.shape[1], window.shape[2])


def build_model(num_labels, dtype, device='cpu', output_attentions=False):
    """-> (this package's ImageBertForSequenceClassification on the golden's tiny config with the golden's weights, eval mode;
    its parameter names)"""
    import torch
    from aladin_amd import backbone
    m = backbone.ImageBertForSequenceClassification(backbone.BertConfig(output_attentions=output_attentions, **golden_cfg(num_labels))).eval()
    named = [(k, tuple(p.shape)) for k, p in m.named_parameters()]
    vals = synth.module_parameters(named, PARAM_SEED, scale=PARAM_SCALE)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.from_numpy(vals[k]))
    return m.to(dtype).to(device), [k for k, _ in named]


def torch_batch(n, seed, dtype, device='cpu'):
    """golden_inputs as the 5-tuple get_teacher_scores takes"""
    import torch
    ids, mask, types, feats, labels = golden_inputs(n, seed)
    return (torch.from_numpy(ids).to(device), torch.from_numpy(mask).to(device), torch.from_numpy(types).to(device),
            torch.from_numpy(feats).to(dtype).to(device), torch.from_numpy(labels).to(device))


def all_layers_teacher(model_with_attentions, batch, num_labels, shape, text_len=TEXT_LEN):
    """The reference's dataflow on this package's model without the window (output_attentions=True: every layer
    keeps its probabilities) with the reference's bookkeeping: what measures the float32 floor of the teacher, and the third row of
    tools/bench_teacher.py."""
    import torch
    with torch.no_grad():
        o = model_with_attentions(input_ids=batch[0], attention_mask=batch[1], token_type_ids=batch[2], img_feats=batch[3])
        win = o[1][-1].mean(dim=1)[:, 1:text_len, text_len:]                       # in the model's dtype, like the reference
        result = torch.softmax(o[0], dim=1)[:, 1] if num_labels == 2 else o[0]
    Bi, Bc = shape
    return (result.double().cpu().numpy().reshape(Bi, Bc),
            win.double().cpu().numpy().reshape(Bi, Bc, win.shape[1], win.shape[2]))


# ------------------------------------------------------------------------------------------------ kernel cases
def ragged_mask(N, L, seed, full_first=True):
    keep = synth.integers((N,), max(1, L // 3), L, seed)
    if full_first:
        keep[0] = L
    return (np.arange(L)[None, :] < keep[:, None]).astype(np.int64)


def qk(N, L, heads, dh, seed, scale=1.0):
    """float32 q, k ~ N(0, scale^2) (N, L, heads * dh)"""
    return ((synth.normal((N, L, heads * dh), seed) * scale).astype(np.float32),
            (synth.normal((N, L, heads * dh), seed + 1) * scale).astype(np.float32))


# name, (N, H, dh, L, (row0, W), (col0, Rw))
def _c(N, H, dh, L, r, c):
    return ('n%d_h%d_dh%d_l%d_r%d-%d_c%d-%d' % (N, H, dh, L, r[0], r[1], c[0], c[1]), (N, H, dh, L, (r[0], r[1] - r[0]), (c[0], c[1] - c[0])))


KERNEL_CASES = [_c(3, 2, 4, 5, (1, 4), (2, 5))] + \
    [_c(2, 3, 8, L, (1, min(L, 20)), (L // 2, L)) for L in (16, 17, 31, 33, 144, 256)] + \
    [_c(2, 2, 8, 40, (1, 17), (7, 27)), _c(2, 2, 8, 40, (3, 5), (0, 40)), _c(2, 2, 8, 256, (0, 256), (250, 256))] + \
    [_c(2, 2, dh, 37, (1, 20), (20, 37)) for dh in (4, 16, 64, 128)] + \
    [_c(2, H, 8, 37, (1, 20), (20, 37)) for H in (1, 12, 32)] + \
    [_c(1, 2, 128, 256, (100, 140), (0, 256)), _c(4, 12, 64, 140, (1, 70), (70, 140))]
