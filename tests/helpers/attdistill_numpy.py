"""The attention-distillation loss (aladin_attdistill_fwd / _bwd, ops.attention_distillation_loss) restated in numpy: the formulas
of include/aladin_hip.h, reference alad/loss.py:273-334, in float64 (the reference of every test), in float32 (the FLOOR: what the
same formulas cost in the kernels' own arithmetic) and with ROUNDED OPERANDS (what the kernels' design accepts: the logits run on
unit rows in split fp16 precision, [hi | lo], times fp32 norms; everything else, the backward's second products on the raw fp32 rows
included, is exact).
Seeded input makers over aladin_amd.synth, and the deliberate slips the CPU tier must see move the result.

    Rq = R - 1, Tq = T - 1,  n_i = clamp(im_len[i] - 1, 0, Rq),  m_j = clamp(s_len[j] - 1, 0, Tq)
    L[i,j,w,r] = <s[j, w + 1], im[i, r + 1]> / sqrt(D),   logp = L - logsumexp_{r < n_i} L
    P = A / max(sum_{r' < Rq} |A|, 1e-12)                                   (A = teacher[:, :, :Tq, :Rq])
    loss = (1 / N) sum_{i, j, w < m_j, r < n_i} [xlogy(P, P) - P logp],     N = Bi * sum_j m_j
    g = (softmax_r L * sigma - P) / N,  sigma = sum_{r < n_i} P
    d im[i, r + 1] = sum_{j, w} g s[j, w + 1] / sqrt(D),   d s[j, w + 1] = sum_{i, r} g im[i, r + 1] / sqrt(D)
"""
import numpy as np

from aladin_amd import synth

SLIPS = ('mean_all', 'tail2', 'teacher_valid', 'inv_d', 'im_len')

# ---- the gates of the GPU tier (tests/test_attdistill_gpu.py), derived in the CPU tier (tests/test_attdistill_cpu.py) ----
# The float32 floor: |float32 restatement - float64 restatement| over gpu_cases(), both on the split operands, the worst case
# rounded up.  Loss: relative to |loss|.  Gradients: max-normalised, max|diff| / max|reference gradient|.
# test_float32_floor_and_the_operand_condition re-measures them and fails if a constant is below the measurement or more than
# 3x above it.
FLOOR_LOSS_REL = 1.4e-7             # measured 1.30e-7 (b3x3_r17_t16_d64_zero_row)
FLOOR_GRAD_MAXNORM = 6e-7           # measured 5.78e-7 (d s_seq of b3x3_r17_t17_d64_logits50)
GATE_FACTOR = 4.0                   # the house's rule (the secondary-heads tests): 4 x the float32 floor of the quantity
GATE_LOSS_REL = GATE_FACTOR * FLOOR_LOSS_REL
GATE_GRAD_MAXNORM = GATE_FACTOR * FLOOR_GRAD_MAXNORM
# the design condition: rounded operands against exact ones stay inside the project's fp16 tolerances ('split' does, 'fp16' does not)
FP16_LOSS_REL = 1e-3


def fp16_grad_tol(D):
    return 5e-4 if D >= 64 else 1e-3


def counts(im_len, s_len, Rq, Tq, slip=None):
    n = np.clip(np.asarray(im_len, np.int64) - (0 if slip == 'im_len' else 1), 0, Rq)
    m = np.clip(np.asarray(s_len, np.int64) - (3 if slip == 'tail2' else 1), 0, Tq)
    return n, m


SPLIT_SCALE = 16384.0               # ALADIN_SPLIT_SCALE of csrc/pack_rows.hpp


def round_operands(x, how):
    """(B, N, D) float32 -> (hi, lo, norm) in float64, the rows as the kernels' logits see them: the norm in float32
    (1 / max(|x|, 1e-12) and its reciprocal, as pack_rows.hpp forms them) and the unit row x * inv
      'split'  times 2^14 as hi + lo, both fp16 (write_split) -- what the kernels use;
      'fp16'   rounded to fp16 once (lo = 0, no scale) -- the cheaper format the design condition rules out."""
    assert how in ('split', 'fp16')
    x = np.asarray(x, np.float32)
    ss = np.sum(x * x, axis=-1, keepdims=True, dtype=np.float32)
    inv = (np.float32(1.0) / np.maximum(np.sqrt(ss), np.float32(1e-12))).astype(np.float32)
    norm = (np.float32(1.0) / inv).astype(np.float32).astype(np.float64)
    if how == 'fp16':
        hi = (x * inv).astype(np.float32).astype(np.float16)
        return hi.astype(np.float64), np.zeros(x.shape), norm
    v = (x * inv * np.float32(SPLIT_SCALE)).astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) / SPLIT_SCALE, lo.astype(np.float64) / SPLIT_SCALE, norm


def attdistill(im, s, im_len, s_len, teacher, dtype=np.float64, rounded=None, slip=None):
    """-> (loss, d_im (Bi, R, D), d_s (Bc, T, D)) in `dtype`.  rounded ('split' / 'fp16'): the logits from round_operands() -- the
    chain hi.hi + lo.hi + hi.lo (lo.lo is dropped, as in the kernels) times both norms; the second products of the gradient keep
    the raw rows.  slip: one of SLIPS, a deliberately wrong reading of the formulas."""
    assert slip is None or slip in SLIPS
    dt = np.dtype(dtype)
    Bi, R, D = im.shape
    Bc, T, _ = s.shape
    Rq, Tq = R - 1, T - 1
    X, Y = np.asarray(im, dt)[:, 1:, :], np.asarray(s, dt)[:, 1:, :]
    n, m = counts(im_len, s_len, Rq, Tq, slip)
    rmask = (np.arange(Rq)[None, :] < n[:, None])[:, None, None, :]              # (Bi, 1, 1, Rq)
    wmask = (np.arange(Tq)[None, :] < m[:, None])[None, :, :, None]              # (1, Bc, Tq, 1)
    scale = dt.type(1.0 / D if slip == 'inv_d' else 1.0 / np.sqrt(float(D)))
    # (Bi, Bc, Tq, Rq): the reference's expand + matmul (alad/loss.py:293-296)
    dots = lambda y, x: np.matmul(y[None, :, :, :], np.swapaxes(x, 1, 2)[:, None, :, :])
    if rounded:
        xh, xl, xn = (a[:, 1:, :].astype(dt) for a in round_operands(im, rounded))
        yh, yl, yn = (a[:, 1:, :].astype(dt) for a in round_operands(s, rounded))
        L = (dots(yh, xh) + dots(yh, xl) + dots(yl, xh)) * (np.swapaxes(xn, 1, 2)[:, None, :, :] * scale) * yn[None, :, :, :]
    else:
        L = dots(Y, X) * scale
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        Lm = np.where(rmask, L, -np.inf)
        mx = Lm.max(axis=-1, keepdims=True)
        mx = np.where(np.isfinite(mx), mx, 0).astype(dt)
        e = np.where(rmask, np.exp(Lm - mx), 0).astype(dt)
        se = e.sum(axis=-1, keepdims=True)
        lse = mx + np.log(se)
        A = np.asarray(teacher, dt)[:, :, :Tq, :Rq]
        l1 = np.abs(np.where(rmask, A, 0) if slip == 'teacher_valid' else A).sum(axis=-1, keepdims=True)
        P = A / np.maximum(l1, dt.type(1e-12))
        valid = rmask & wmask
        pos = valid & (P > 0)
        terms = np.where(pos, P * (np.log(np.where(pos, P, 1)) - (L - lse)), 0).astype(dt)
        N = Bi * Bc * Tq if slip == 'mean_all' else Bi * int(m.sum())
        d_im, d_s = np.zeros((Bi, R, D), dt), np.zeros((Bc, T, D), dt)
        if N == 0:
            return dt.type(0), d_im, d_s
        loss = terms.sum(dtype=dt) / dt.type(N)
        sigma = np.where(rmask, P, 0).sum(axis=-1, keepdims=True)
        g = (np.where(valid, (e / np.where(se > 0, se, 1)) * sigma - P, 0) / dt.type(N)).astype(dt)
    # d im[i] = sum_j G[i, j]^T (Rq x Tq) @ Y[j];  d s[j] = sum_i G[i, j] (Tq x Rq) @ X[i]
    d_im[:, 1:, :] = np.matmul(np.swapaxes(g, 2, 3), Y[None, :, :, :]).sum(axis=1, dtype=dt) * scale
    d_s[:, 1:, :] = np.matmul(g, X[:, None, :, :]).sum(axis=0, dtype=dt) * scale
    return loss, d_im, d_s


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def lengths(kind, B, S, seed):
    """lengths of B sets padded to S positions: 'full'; 'ragged' (one sample with ONE scored position, one full); 'over' (ragged, one
    length above the set size); 'empty' (ragged, one sample without a scored position)."""
    if kind == 'full':
        return [S] * B
    lens = [int(v) for v in synth.integers((B,), 2, S, seed)]
    lens[seed % B] = S
    if B > 1:
        lens[(seed + 1) % B] = 2 if kind != 'empty' else 1
    if kind == 'over':
        lens[seed % B] = S + 3
    if kind == 'empty' and B == 1:
        lens[0] = 1
    return lens


def make_inputs(Bi, Bc, R, T, D, seed, im_kind='ragged', s_kind='ragged', teacher_kind='dense', Wt=None, Rt=None, logit_peak=None,
                im_len=None, s_len=None):
    """-> dict(im, s, im_len, s_len, teacher): float32 sets ~N(0, 1), a non-negative teacher (Bi, Bc, Wt, Rt) with peaked rows.
    teacher_kind: 'dense' (mass everywhere, masked regions included), 'masked' (zero on the regions past an image's length: what an
    attention-masked teacher produces), 'zero_row' (dense, one pair's first word row all zero).  logit_peak: the sets are
    rescaled so that the largest |logit| is that value.  im_len / s_len: explicit lengths instead of the kinds'."""
    Wt, Rt = Wt or T - 1, Rt or R - 1
    im, s, _, _ = synth.alignment_batch(Bi, R, T, D, seed, False, Bc)
    im_len = list(im_len) if im_len is not None else lengths(im_kind, Bi, R, seed + 3)
    s_len = list(s_len) if s_len is not None else lengths(s_kind, Bc, T, seed + 5)
    if logit_peak is not None:
        L = np.einsum('jwd,ird->ijwr', s[:, 1:].astype(np.float64), im[:, 1:].astype(np.float64)) / np.sqrt(D)
        f = np.float32(np.sqrt(logit_peak / np.abs(L).max()))
        im, s = im * f, s * f
    teacher = (synth.uniform((Bi, Bc, Wt, Rt), seed + 7) ** 4).astype(np.float32)
    if teacher_kind == 'masked':
        n, _ = counts(im_len, s_len, R - 1, T - 1)
        teacher = np.where(np.arange(Rt)[None, None, None, :] < n[:, None, None, None], teacher, 0).astype(np.float32)
    elif teacher_kind == 'zero_row':
        teacher[Bi // 2, Bc // 2, 0, :] = 0
    else:
        assert teacher_kind == 'dense'
    return dict(im=im.astype(np.float32), s=s.astype(np.float32), im_len=im_len, s_len=s_len, teacher=teacher)


# The GPU tier's value cases: (name, make_inputs arguments).  The smallest shapes that cross each boundary of the kernels: the
# chunk of waves per workgroup (3 x 5, 5 x 3, 9 x 9), the 16-row tiles on both sides (Rq in 1, 15, 16, 17, 33, 96; Tq in 1, 16, 17, 96),
# D in 8, 20 (padded to a multiple of 4), 64 and one case at 768, the reference's 69 x 70 teacher read through its strides.
GPU_CASES = [
    ('b3x5_r16_t17_d8_full', dict(Bi=3, Bc=5, R=17, T=18, D=8, seed=11, im_kind='full', s_kind='full')),
    ('b5x3_r15_t16_d20_ragged', dict(Bi=5, Bc=3, R=16, T=17, D=20, seed=12)),
    ('b9x9_r33_t17_d64_ragged', dict(Bi=9, Bc=9, R=34, T=18, D=64, seed=13)),
    ('b2x3_r1_t1_d8', dict(Bi=2, Bc=3, R=2, T=2, D=8, seed=14, im_kind='full', s_kind='full')),
    ('b3x2_r17_t96_d20_over', dict(Bi=3, Bc=2, R=18, T=97, D=20, seed=15, im_kind='over', s_kind='over')),
    ('b2x2_r96_t16_d64_ragged', dict(Bi=2, Bc=2, R=97, T=17, D=64, seed=16)),
    ('b5x5_r50_t37_d768_teacher69x70', dict(Bi=5, Bc=5, R=51, T=38, D=768, seed=17, Wt=69, Rt=70)),
    ('b4x5_r33_t17_d64_empty_image', dict(Bi=4, Bc=5, R=34, T=18, D=64, seed=18, im_kind='empty')),
    ('b3x3_r17_t16_d64_zero_row', dict(Bi=3, Bc=3, R=18, T=17, D=64, seed=19, teacher_kind='zero_row')),
    ('b3x4_r33_t17_d64_masked_teacher', dict(Bi=3, Bc=4, R=34, T=18, D=64, seed=20, teacher_kind='masked')),
    ('b3x3_r17_t17_d64_logits50', dict(Bi=3, Bc=3, R=18, T=18, D=64, seed=21, logit_peak=50.0)),
]


# The fixture tests/golden/attdistill.npz (make_golden_attdistill.py): (name, how the expected loss was obtained, arguments).
#   'whole'      the reference's loss and gradients on the batch as it is (full-length images: the reference is finite)
#   'per_image'  ragged images under a teacher without mass on masked regions: the reference's gradients on the batch (finite), its
#                loss per image on the set truncated to the image's valid length, averaged over the images (an identity of the formulas)
FIXTURE_CASES = [
    ('full_images_ragged_captions', 'whole', dict(Bi=3, Bc=4, R=7, T=9, D=8, seed=31, im_kind='full')),
    ('ragged_images_masked_teacher', 'per_image', dict(Bi=3, Bc=3, R=8, T=7, D=12, seed=32, teacher_kind='masked')),
    ('zero_teacher_row', 'whole', dict(Bi=3, Bc=3, R=6, T=6, D=8, seed=33, im_kind='full', teacher_kind='zero_row')),
    ('lengths_above_the_set_size', 'whole', dict(Bi=3, Bc=3, R=6, T=7, D=8, seed=34, im_len=[6, 8, 6], s_len=[7, 3, 10], Wt=9, Rt=8)),
]


def gpu_cases():
    return [(name, make_inputs(**kw)) for name, kw in GPU_CASES]


def errors(got, ref):
    """-> (relative loss error, max-normalised d_im error, max-normalised d_s error) of (loss, d_im, d_s) triples"""
    out = [abs(float(got[0]) - float(ref[0])) / max(abs(float(ref[0])), 1e-300)]
    for a, b in zip(got[1:], ref[1:]):
        b = np.asarray(b, np.float64)
        out.append(float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300)))
    return tuple(out)
