"""Drop-in loss modules with the reference's names, constructor arguments and forward signatures
(reference alad/loss.py), computed by the HIP kernels behind include/aladin_hip.h.

    AlignmentContrastiveLoss  <- alad/loss.py:70-159
    ContrastiveLoss           <- alad/loss.py:162-186
    DistillationLoss          <- alad/loss.py:359-447
    Contrastive               <- alad/loss.py:29-67 (shared hinge)
    CrossEntropyCriterion     <- alad/loss.py:190-201
    SemanticContrastiveLoss   <- alad/loss.py:203-270
    AttentionDistillationLoss <- alad/loss.py:273-334
    AlignmentCrossEntropyLoss    (not in the reference: the same criterion on the alignment head's scores)
    AlignmentSemanticContrastiveLoss (not in the reference: SemanticContrastiveLoss's criterion on the alignment head's scores)

None of them holds parameters or buffers, except DistillationLoss(mode='mse') whose learnable pair
`wb` the reference has too (:366) and the cross-entropy criteria's `temperature` (:193) -- state dicts
saved by the reference load unchanged (checkpoint row).  Every aggregation /
distillation mode / measure of the reference is computed by HIP kernels; nothing falls back to eager
PyTorch.
"""
import torch
from torch import nn

from . import ops


def l2norm(X):
    """X / sqrt(sum_dim1 X^2), no eps -- reference alad/utils.py:134-139 (zero rows give NaN), HIP kernel."""
    return ops.l2norm_rows(X)


def dot_sim(im, s):
    """reference alad/loss.py:8-11."""
    return ops.dot_scores(im, s)


def cosine_sim(im, s):
    """reference alad/loss.py:13-18."""
    return ops.dot_scores(l2norm(im), l2norm(s))


def order_sim(im, s):
    """reference alad/loss.py:20-26."""
    return ops.order_scores(im, s)


class Contrastive(nn.Module):
    """reference alad/loss.py:29-67."""

    def __init__(self, margin=0, measure=False, max_violation=False):
        super().__init__()
        self.margin = margin
        if measure == 'order':
            self.sim = order_sim
        elif measure == 'cosine':
            self.sim = cosine_sim
        elif measure == 'dot':
            self.sim = dot_sim
        self.max_violation = max_violation

    def compute_contrastive_loss(self, scores):
        return ops.hinge_loss(scores, self.margin, self.max_violation)


ALIGNMENT_AGGREGATIONS = ('MrSw', 'MrAVGw', 'MwSr', 'symm', 'sum', 'mean', 'scan-sentences')


def _check_aggregation(aggregation):
    if aggregation not in ALIGNMENT_AGGREGATIONS:
        # the reference leaves aggr_similarity unbound and dies with a NameError (:151-159)
        raise ValueError("aladin_amd: unknown alignment aggregation %r (supported: 'MrSw', 'MrAVGw', 'MwSr', "
                         "'symm', 'sum', 'mean', 'scan-sentences')" % (aggregation,))


def alignment_similarity(aggregation, im_set, s_seq, im_len, s_len):
    """The differentiable (Bi, Bc) score matrix of an alignment aggregation, reference alad/loss.py:120-149."""
    if aggregation == 'scan-sentences':
        aggr_similarity = ops.alignment_scan_scores(im_set, s_seq, im_len, s_len)
    elif aggregation in ('sum', 'mean'):
        aggr_similarity = ops.alignment_sum_scores(im_set, s_seq, im_len, s_len, mean=(aggregation == 'mean'))
    elif aggregation in ('MwSr', 'symm'):
        aggr_similarity = ops.alignment_scores(im_set, s_seq, im_len, s_len, aggregation)
    else:
        aggr_similarity = ops.alignment_scores(im_set, s_seq, im_len, s_len)
    if aggregation == 'MrAVGw':
        lens = ops.lengths_tensor(s_len, aggr_similarity.device).to(torch.float32) - 3.0
        aggr_similarity = aggr_similarity / lens.unsqueeze(0)
    return aggr_similarity


class AlignmentContrastiveLoss(Contrastive):
    """reference alad/loss.py:70-159.  aggregation: 'MrSw' (all shipped configs), 'MrAVGw' (= MrSw
    divided by the caption length, :126-129), 'MwSr' / 'symm' (the MrSw kernels with the sets'
    roles swapped, :130-135), 'sum' / 'mean' (:120-123: the double sum of cosines factorises into
    one dot product of the summed unit vectors), 'scan-sentences' (:136-149, fp32 throughout)."""

    def __init__(self, margin=0, measure=False, max_violation=False, aggregation='sum-max-sentences'):
        super().__init__(margin, measure, max_violation)
        self.aggregation = aggregation

    def forward(self, im_set, s_seq, im_len, s_len, return_loss=True, return_similarity_mat=False):
        _check_aggregation(self.aggregation)
        if return_loss and self.aggregation == 'MrSw':
            # fused scores + hinge node; both outputs are differentiable, as the reference's (ops.alignment_triplet_loss)
            loss, aggr_similarity = ops.alignment_triplet_loss(im_set, s_seq, im_len, s_len, self.margin,
                                                               self.max_violation)
            return (loss, aggr_similarity) if return_similarity_mat else loss
        aggr_similarity = alignment_similarity(self.aggregation, im_set, s_seq, im_len, s_len)
        if return_loss:
            loss = self.compute_contrastive_loss(aggr_similarity)
        if return_loss and return_similarity_mat:
            return loss, aggr_similarity
        elif return_loss:
            return loss
        elif return_similarity_mat:
            return aggr_similarity


class ContrastiveLoss(Contrastive):
    """reference alad/loss.py:162-186."""

    def forward(self, im, s, return_similarity_mat=False):
        if self.sim is dot_sim and getattr(im, 'is_cuda', False) and im.dim() == 2 and tuple(im.shape) == tuple(s.shape):
            # measure 'dot' (every shipped config): scores + hinge behind ONE autograd node (ops.match_hinge)
            loss, scores = ops.match_hinge(im, s, self.margin, self.max_violation)
            return (loss, scores) if return_similarity_mat else loss
        scores = self.sim(im, s)
        loss = self.compute_contrastive_loss(scores)
        if return_similarity_mat:
            return loss, scores
        return loss


class DistillationLoss(nn.Module):
    """reference alad/loss.py:359-447: modes 'mse', 'ordinal', 'contrastive', 'listnet' (the one every
    shipped config uses)."""

    def __init__(self, mode='mse', margin=0.2, threshold=0.1, stride=3):
        super().__init__()
        if mode not in ('mse', 'ordinal', 'contrastive', 'listnet'):
            # the reference would leave `loss` unbound and fail at :447
            raise ValueError('aladin_amd: unknown distillation mode %r' % (mode,))
        self.mode = mode
        self.margin = margin
        self.threshold = threshold
        self.stride = stride
        if mode == 'mse':
            self.wb = nn.Parameter(torch.FloatTensor([0.5, 0.5]), requires_grad=True)     # :366

    def forward(self, teacher_scores, student_scores):
        if self.mode == 'listnet':
            return ops.listnet_loss(teacher_scores, student_scores, temperature=6.0, eps=1e-10)
        return ops.distillation_loss(teacher_scores, student_scores, self.mode, self.margin, self.threshold,
                                     self.stride, wb=self.wb if self.mode == 'mse' else None)


class CrossEntropyCriterion(nn.Module):
    """reference alad/loss.py:190-201: the symmetric cross-entropy (InfoNCE) of im @ s.T * exp(temperature), `temperature` a
    learnable (1,) parameter starting at 0 -- a reference state dict (['temperature']) loads unchanged."""

    def __init__(self):
        super().__init__()
        self.temperature = nn.Parameter(torch.zeros(1), requires_grad=True)       # :193

    def forward(self, im, s):
        return ops.match_cross_entropy(im, s, self.temperature)


class SemanticContrastiveLoss(nn.Module):
    """reference alad/loss.py:203-270: the hinge anchored, per row and per column, at ONE positive drawn among the pairs whose
    relevance exceeds `threshold` (ops.semantic_hinge_loss).  relevances: (B, B) float32 on the GPU, images x captions --
    rouge.relevance_matrix(captions, caps_per_img=1).t() is the natural source.  Where it differs from the reference
    (INTEGRATION.md section 2): the draws come from the DEVICE generator (or the caller's `draws`, int32 (2B,)), not from the
    host stream; a line without a candidate falls back to its diagonal cell instead of raising; column_positives='aligned' and
    mask_positives=True are options the reference does not have."""

    def __init__(self, margin=0, threshold=0.4, measure=False, max_violation=False, *, column_positives='reference',
                 mask_positives=False):
        super().__init__()
        if measure == 'order':
            self.sim = order_sim
        elif measure == 'cosine':
            self.sim = cosine_sim
        elif measure == 'dot':
            self.sim = dot_sim
        if column_positives not in ops.SEMANTIC_COLUMN_ORDERS:
            raise ValueError("aladin_amd: column_positives is 'reference' or 'aligned', got %r" % (column_positives,))
        self.margin = margin
        self.max_violation = max_violation
        self.threshold = threshold
        self.column_positives = column_positives
        self.mask_positives = mask_positives

    def compute_semantic_contrastive_loss(self, scores, relevances, *, draws=None):
        return ops.semantic_hinge_loss(scores, relevances, self.margin, self.threshold, self.max_violation, draws=draws,
                                       column_positives=self.column_positives, mask_positives=self.mask_positives)

    def forward(self, im, s, relevances, return_similarity_mat=False, *, draws=None):
        scores = self.sim(im, s)
        loss = self.compute_semantic_contrastive_loss(scores, relevances, draws=draws)
        if return_similarity_mat:
            return loss, scores
        return loss


class AttentionDistillationLoss(nn.Module):
    """reference alad/loss.py:273-334: the KL divergence between a cross-encoder teacher's word-by-region attentions
    (teacher_attentions, (Bi, Bc, Wt, Rt) -- the reference's 69 x 70, sliced in place) and the softmax over regions of the scaled
    dot products of the fine-grained head's sets, 'batchmean' over every pair's words.  One fused kernel pass per direction: the
    (Bi, Bc, R - 1, T - 1) tensor of the reference is never formed.  Masked regions drop out of the loss, where the reference
    evaluates 0 * -inf (NaN on a batch with a short image); the gradients are the reference's whenever the teacher puts no mass on
    masked regions."""

    def __init__(self):
        super().__init__()

    def forward(self, im_set, s_seq, im_len, s_len, teacher_attentions):
        return ops.attention_distillation_loss(im_set, s_seq, im_len, s_len, teacher_attentions)


class AlignmentCrossEntropyLoss(nn.Module):
    """NOT in the reference: CrossEntropyCriterion's loss on the alignment head's score matrix (FILIP-style training of the
    fine-grained head) -- the (B, B) matrix AlignmentContrastiveLoss(aggregation=...) scores, times exp(temperature), through the
    symmetric cross-entropy.  It has its own learnable `temperature` (1,), initial value 0.  The default 'MrAVGw' keeps the
    scores in [-1, 1] whatever the caption length.  The score functions are AlignmentContrastiveLoss's; their backward here is the
    dense-dS one (every pair carries a gradient), several times the cost of the hardest-negative triplet step."""

    def __init__(self, aggregation='MrAVGw'):
        super().__init__()
        _check_aggregation(aggregation)
        self.aggregation = aggregation
        self.temperature = nn.Parameter(torch.zeros(1), requires_grad=True)

    def forward(self, im_set, s_seq, im_len, s_len, return_similarity_mat=False):
        _check_aggregation(self.aggregation)
        if im_set.shape[0] != s_seq.shape[0]:
            raise ValueError('aladin_amd: the cross-entropy criterion needs a square score matrix: one caption per image set, '
                             'got %d image sets and %d captions' % (im_set.shape[0], s_seq.shape[0]))
        aggr_similarity = alignment_similarity(self.aggregation, im_set, s_seq, im_len, s_len)
        loss = ops.cross_entropy_scores(aggr_similarity, self.temperature)
        return (loss, aggr_similarity) if return_similarity_mat else loss


class AlignmentSemanticContrastiveLoss(nn.Module):
    """NOT in the reference: SemanticContrastiveLoss's criterion on the alignment head's score matrix -- the (B, B) matrix
    AlignmentContrastiveLoss(aggregation=...) scores, through ops.semantic_hinge_loss.  The score functions are
    AlignmentContrastiveLoss's; their backward here is the dense-dS one, as under AlignmentCrossEntropyLoss (in max_violation mode
    dS has at most 4 B non-zeros, but they are not the triplet step's diagonal pairs)."""

    def __init__(self, margin=0, threshold=0.4, max_violation=False, aggregation='MrSw', *, column_positives='reference',
                 mask_positives=False):
        super().__init__()
        _check_aggregation(aggregation)
        if column_positives not in ops.SEMANTIC_COLUMN_ORDERS:
            raise ValueError("aladin_amd: column_positives is 'reference' or 'aligned', got %r" % (column_positives,))
        self.margin = margin
        self.threshold = threshold
        self.max_violation = max_violation
        self.aggregation = aggregation
        self.column_positives = column_positives
        self.mask_positives = mask_positives

    def forward(self, im_set, s_seq, im_len, s_len, relevances, return_similarity_mat=False, *, draws=None):
        _check_aggregation(self.aggregation)
        if im_set.shape[0] != s_seq.shape[0]:
            raise ValueError('aladin_amd: the semantic contrastive loss needs a square score matrix: one caption per image set, '
                             'got %d image sets and %d captions' % (im_set.shape[0], s_seq.shape[0]))
        aggr_similarity = alignment_similarity(self.aggregation, im_set, s_seq, im_len, s_len)
        loss = ops.semantic_hinge_loss(aggr_similarity, relevances, self.margin, self.threshold, self.max_violation, draws=draws,
                                       column_positives=self.column_positives, mask_positives=self.mask_positives)
        return (loss, aggr_similarity) if return_similarity_mat else loss
