"""The cross-encoder teacher of the distillation losses: `get_teacher_scores`, reference alad/train.py:340-384.

For a grid of Bi x Bc (image, caption) sequences the VinVL cross-encoder (`backbone.ImageBertForSequenceClassification`) gives
  * scores (Bi, Bc): the matching confidence of every pair -- the teacher of DistillationLoss;
  * attentions (Bi, Bc, text_len - 1, L - text_len): the last layer's attention, mean over heads, of every word (rows
    [1, text_len)) over the image regions (columns [text_len, L)) -- the teacher of AttentionDistillationLoss, in the layout
    `ALADModel.forward(teacher_attentions=)` / csrc/attdistill.hip read in place.

The reference asks every layer for its (N, heads, L, L) probabilities (`output_attentions=True`) to slice one corner of the last
layer's, which is why it cuts the batch into `subdivs` chunks.  Here the model runs through `attention_window=`
(backbone.BertImgModel.forward): all layers stay on SDPA and csrc/attn_window.hip writes the window of each chunk straight into
its slice of the preallocated result.  `subdivs` keeps its meaning (the activations of the BERT pass still scale with it).
"""
import math

import torch
from torch.nn import functional as F


def get_teacher_scores(args, model, batch, subdivs=40, *, shape=None, text_len=70, fused=None):
    """args: `.device` and `.num_labels` are read.  model: an ImageBertForSequenceClassification (called with the reference's
    keywords plus `attention_window`).  batch: (input_ids, attention_mask, token_type_ids, img_feats[, labels]) of Bi * Bc
    sequences in image-major order.  shape: None = a square grid, as the reference asserts; (Bi, Bc) otherwise.
    fused: None automatic, False the plain path (torch ops on the last layer), True raises where the kernel cannot run.
    -> (scores (Bi, Bc), attentions (Bi, Bc, text_len - 1, L - text_len)), both allocated once."""
    device = args.device
    batch = [x.to(device) for x in batch]
    n = len(batch[0])
    if shape is None:
        side = int(math.sqrt(n))
        assert side ** 2 == n
        Bi = Bc = side
    else:
        Bi, Bc = int(shape[0]), int(shape[1])
        if Bi < 1 or Bc < 1 or Bi * Bc != n:
            raise ValueError('aladin_amd.teacher: shape %s does not hold the %d sequences of the batch' % ((Bi, Bc), n))
    subdivs = int(subdivs)
    if subdivs < 1:
        raise ValueError('aladin_amd.teacher: subdivs must be at least 1')
    L = batch[0].shape[1] + batch[3].shape[1]
    W, Rw = text_len - 1, L - text_len
    if W < 1 or Rw < 1:
        raise ValueError('aladin_amd.teacher: text_len %d leaves no word rows or no region columns in sequences of %d positions'
                         % (text_len, L))
    dtype = next(model.parameters()).dtype
    scores = torch.empty((n,) if args.num_labels == 2 else (n, args.num_labels), dtype=dtype, device=batch[3].device)
    attentions = torch.empty((n, W, Rw), dtype=dtype, device=batch[3].device)
    with torch.no_grad():
        for b in range(0, n, subdivs):                                # whole chunks and the rest; never an empty one
            e = min(b + subdivs, n)
            out = model(input_ids=batch[0][b:e], attention_mask=batch[1][b:e], token_type_ids=batch[2][b:e], img_feats=batch[3][b:e],
                        labels=batch[4][b:e] if len(batch) > 4 else None, attention_window=(1, W, text_len, Rw),
                        attention_window_fused=fused, attention_window_out=attentions[b:e])      # the window lands in its slice
            logits = out[0]
            scores[b:e] = F.softmax(logits, dim=1)[:, 1] if args.num_labels == 2 else logits     # two labels: P(label 1 = the pair matches)
        return scores.view(Bi, Bc), attentions.view(Bi, Bc, W, Rw)
