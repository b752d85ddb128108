"""Tensor-level entry points over the C ABI (include/aladin_hip.h): device memory, streams and
autograd plumbing only -- all arithmetic of the hot path happens in the HIP kernels.

Every function requires float32 tensors on an AMD GPU ("cuda" device of PyTorch-ROCm) and raises
otherwise; there is no CPU or eager-PyTorch fallback.
"""
import ctypes as C
from typing import NamedTuple

import torch

from . import _lib

from ._ops_common import (_RAW_STREAM, _stream, _ptr, _require_gpu, _rows_inner_contig, _LEN_CACHE, lengths_tensor, _ld, _workspace,
                          _set_view, _grad_view, _pad_features, _check_set_shapes, _check_sets, _sets_for_node, _upstream)
from .ops_losses import _DotScores, _hinge_raw        # (the other names of ops_losses / ops_heads / ops_retrieval: __getattr__ below)


def _pair_kernel_covers(geom):
    """Shapes the fp16 pair kernel of the backward covers (csrc/align_bwd.hip: bwd_pair_argmax16_kernel): a 64-row block per
    pair = the image's 32 / 48 main rows + a window on its side rows, or its 64 main rows; at most 64 padded words.
    The Python mirror of pair16_covers() in csrc/align_bwd.hip."""
    return geom.layout != _lib.LAYOUT_LONG and (geom.mrows in (32, 48) or (geom.mrows == 64 and geom.rem == 0)) and geom.tp16 <= 4


# ------------------------------------------------------------------------------------------------
# alignment scores
# ------------------------------------------------------------------------------------------------
_GEOM_CACHE = {}

# Operand precision of score matrices computed WITHOUT autograd (evaluation, validation, the reference's
# alignment_sim_fn closures -- train.py:495-498, test.py:260-263):
#   'split'  hi/lo fp16 split, three MFMA products per term: scores at the rounding level of the reference's
#            own fp32 bmm, so Recall@K ranks are the reference's (default);
#   'fp16'   the training operands (one fp16 rounding, ~1e-4 on a score): 3x faster, near-ties may swap.
# Differentiable scores always use fp16 operands (north_star's 1e-3 tolerance; the backward re-decides its
# arg-maxima in exact fp32 anyway).
_EVAL_PRECISION = ['split']


def set_eval_precision(precision):
    """'split' (rank-exact, default) or 'fp16' for no-grad alignment scores; returns the previous setting."""
    if precision not in ('split', 'fp16'):
        raise ValueError("aladin_amd: eval precision must be 'split' or 'fp16'")
    old = _EVAL_PRECISION[0]
    _EVAL_PRECISION[0] = precision
    return old


# Where the backward's row kernel takes its unit vectors from (tools/experiments/bwd_precision_probe.py on every reference fixture,
# profiles/r05_bwd_precision_probe.txt; the gate is 5e-4 of the largest gradient entry = half of north_star's 1e-3):
#   'fp16'      ALADIN_BWD_PARTNERS_FP16 (default since round 5, VERDICT r4 item 2 iii): the PARTNER rows -- the unit vectors a
#               gradient row is a weighted sum of -- from the forward's packed fp16 operands: worst 4.3e-4 over the fixtures (one
#               fp16 rounding: <= 2^-11 relative per component), row kernel 43.5 -> 34.0 us at B = 256, 302 -> 217 MB;
#   'fp16-own'  + ALADIN_BWD_OWN_ROW_FP16 (item 2 i): the output row's own unit vector and inverse norm from the packed operands too
#               -- the raw fp32 sets are not read by the row kernel at all: 30.4 us.  Same error wherever D >= 128; on the D = 64
#               structured fixture (cosines near 1: the projection term is as large as the gradient) 5.8e-4 -- past the gate, so an opt-in;
#   'exact'     the raw fp32 sets, normalised again in fp32: 3e-7 of the reference's autograd.
# The fp16 modes apply wherever the forward's packed operands (with their inverse norms) reach the backward.
_BWD_PARTNERS = ['fp16']
_BWD_OWN_ROW_FP16 = [False]


def set_backward_precision(mode):
    """'fp16' (default), 'fp16-own' or 'exact' unit vectors in the alignment backward's row step; returns the previous setting."""
    if mode not in ('exact', 'fp16', 'fp16-own'):
        raise ValueError("aladin_amd: backward precision must be 'exact', 'fp16' or 'fp16-own'")
    old = 'exact' if _BWD_PARTNERS[0] == 'exact' else ('fp16-own' if _BWD_OWN_ROW_FP16[0] else 'fp16')
    _BWD_PARTNERS[0] = 'exact' if mode == 'exact' else 'fp16'
    _BWD_OWN_ROW_FP16[0] = mode == 'fp16-own'
    return old


def _bwd_precision_bits(have_rnorm):
    """The set_backward_precision() mode as ALADIN_BWD_* flag bits, for a backward that holds the forward's fp16 packed operands;
    have_rnorm: their inverse norms are there too (without them only the exact row step can run)."""
    if _BWD_PARTNERS[0] != 'fp16' or not have_rnorm:
        return 0
    return _lib.BWD_PARTNERS_FP16 | (_lib.BWD_OWN_ROW_FP16 if _BWD_OWN_ROW_FP16[0] else 0)


class Packed(NamedTuple):
    """The fp16 MFMA operands of one problem as tensors, with its layout: what pack_sets / _align_forward return and the score
    and backward functions take as `packed` (they also accept a plain tuple (geom, xm, xe, y[, rnorm]) and make this of it); an
    operand that is not there is None."""
    geom: object
    xm: object
    xe: object
    y: object
    rnorm: object = None        # inverse norms of the [xm | xe | y] rows: None without norms or with split operands

    @classmethod
    def from_buf(cls, buf, geom, offs):
        """Tensor views of the one-allocation operand buffer of _triplet_forward (offs: byte offsets of xe, y, rnorm)."""
        return cls(geom, buf[:geom.xm_bytes].view(torch.float16),
                   buf[offs[0]:offs[0] + max(int(geom.xe_bytes), 16)].view(torch.float16),
                   buf[offs[1]:offs[1] + geom.y_bytes].view(torch.float16),
                   buf[offs[2]:offs[2] + geom.rnorm_bytes].view(torch.float32))

    def operands(self):
        return self.xm, self.xe, self.y, self.rnorm

    def struct(self):
        """struct aladin_packed of the operands that are there."""
        return _lib.Packed(*(t.data_ptr() if t is not None else None for t in self.operands()))

    def at_hand(self):
        """Do the forward's operands reach the backward (or does it recompute them in fp32)?"""
        return self.xm is not None

    def fp16_rows(self):
        """Can the backward's row step take its unit vectors from these operands?  Only with their inverse norms."""
        return self.xm is not None and self.y is not None and self.rnorm is not None and not self.geom.split


def _bwd_flags(packed):
    """flags word of the backward entry points for this problem: ALADIN_BWD_PARTNERS_FP16 when the setting asks for it and the
    forward's packed operands WITH their inverse norms are at hand."""
    return _bwd_precision_bits(packed is not None and Packed(*packed).fp16_rows())


def _precision_code(precision):
    if precision in (None, 'fp16', _lib.PRECISION_FP16):
        return _lib.PRECISION_FP16
    if precision in ('split', _lib.PRECISION_SPLIT):
        return _lib.PRECISION_SPLIT
    raise ValueError("aladin_amd: precision must be 'fp16' or 'split', got %r" % (precision,))


# Long sets: past the tile classes (more than _lib.TILE_MAX_SCORED scored positions on either side) the packed layout, the score
# kernel and the backward are those of csrc/align_long.hip, up to LONG_POSITIONS positions per set: a geometry whose layout is
# _lib.LAYOUT_LONG, which the same entry points take.  Shapes inside the classes never get one, except under LONG_PATH_FORCE
# (tests / tools: the long kernels against the tile kernels on the same shape).
LONG_POSITIONS = 512
LONG_PATH_FORCE = False
_LAYOUT_CODES = {'tiles': _lib.LAYOUT_TILES, 'auto': _lib.LAYOUT_AUTO, 'long': _lib.LAYOUT_LONG}


def _check_positions(R, T):
    """The long-set geometry's limit, as the ValueError of the Python layer."""
    if R > LONG_POSITIONS or T > LONG_POSITIONS:
        raise ValueError('aladin_amd: alignment scores support at most %d positions per set (got %d on the max side, %d on the '
                         'sum side)' % (LONG_POSITIONS, R, T))


def align_geometry(Bi, Bc, R, T, D, x_tail=0, y_tail=2, precision=None, layout='tiles'):
    """Packed layout (the cached struct aladin_align_geom) for a (max-side set Bi x R) x (sum-side set Bc x T) problem; the
    tails are the trailing positions each set drops (images 0, captions 2 -- reference alad/loss.py:87-90).
    layout: 'tiles' (the tile classes: at most 96 scored positions), 'long' (the long-set layout) or 'auto' (the tile classes,
    past them the long-set layout -- what the scoring path packs for)."""
    prec = _precision_code(precision)
    auto = layout == 'auto'
    if auto and LONG_PATH_FORCE:
        layout = 'long'
    key = (Bi, Bc, R, T, D, x_tail, y_tail, prec, layout)
    g = _GEOM_CACHE.get(key)
    if g is None:
        if auto:
            _check_positions(R, T)
        g = _lib.AlignGeom()
        _lib.check(_lib.load().aladin_align_geometry(Bi, Bc, R, T, D, x_tail, y_tail, prec, _LAYOUT_CODES[layout], C.byref(g)),
                   'align_geometry')
        if len(_GEOM_CACHE) < 1024:
            _GEOM_CACHE[key] = g
    return g


def is_long(R, T, x_tail=0, y_tail=2):
    """Does a (max side R positions) x (sum side T positions) problem take the long-set kernels?  What layout='auto' answers
    (tests/test_long_sets_cpu.py), for the callers that route without a geometry in hand."""
    return LONG_PATH_FORCE or R - 1 - x_tail > _lib.TILE_MAX_SCORED or T - 1 - y_tail > _lib.TILE_MAX_SCORED


def pack_images(im, im_len_t, geom, rnorm=None, out=None):
    """(xm, xe): L2-normalised, sliced, length-masked fp16 MFMA operands of the image sets.  rnorm (optional float32 tensor of
    geom.rnorm_bytes / 4 elements): receives the image rows' inverse norms in its [xm | xe] part.  out = (xm, xe): write into
    the caller's buffers (the sharded step packs straight into its all-gather segment)."""
    lib = _lib.load()
    im = _rows_inner_contig(im)
    if out is not None:
        xm, xe = out
    else:
        xm = torch.empty(geom.xm_bytes // 2, dtype=torch.float16, device=im.device)
        xe = torch.empty(max(geom.xe_bytes // 2, 8), dtype=torch.float16, device=im.device)
    v, pk = _set_view(im, im_len_t), Packed(geom, xm, xe, None, rnorm).struct()
    _lib.check(lib.aladin_align_pack(C.byref(v), None, C.byref(geom), C.byref(pk), _stream()), 'align_pack(images)')
    return xm, xe


def pack_captions(s, s_len_t, geom, rnorm=None):
    lib = _lib.load()
    s = _rows_inner_contig(s)
    y = torch.empty(geom.y_bytes // 2, dtype=torch.float16, device=s.device)
    v, pk = _set_view(s, s_len_t), Packed(geom, None, None, y, rnorm).struct()
    _lib.check(lib.aladin_align_pack(None, C.byref(v), C.byref(geom), C.byref(pk), _stream()), 'align_pack(captions)')
    return y


def scores_from_packed(xm, xe, y, geom, out=None, e_scratch=None, reuse_side=False):
    lib = _lib.load()
    S = out if out is not None else torch.empty((geom.Bi, geom.Bc), dtype=torch.float32, device=xm.device)
    pk = Packed(geom, xm, xe, y).struct()
    e = e_scratch if e_scratch is not None else _workspace(geom.e_bytes, xm.device)
    _lib.check(lib.aladin_align_scores(C.byref(pk), C.byref(geom), _ptr(e), _ptr(S), S.stride(0), 1 if reuse_side else 0, _stream()),
               'align_scores')
    return S


def _check_backward_supported(im, s, x_tail, y_tail):
    """The limits of aladin_align_bwd (align_bwd.hip), checked when the FORWARD of a differentiable score
    matrix is requested, so that an unsupported shape fails here and not inside loss.backward()."""
    Bi, R, D = im.shape
    Bc, T, _ = s.shape
    if D % 4 != 0 or D > 1024:
        raise ValueError('aladin_amd: differentiable alignment scores need D <= 1024 (got D=%d; the public entry points pad a '
                         'feature size that is not a multiple of 4); score under torch.no_grad()' % D)
    _check_positions(R, T)


def pack_sets(im, s, im_len_t, s_len_t, geom, norms=True):
    """Both sets in one launch -> Packed(geom, xm, xe, y, rnorm), the `packed` the score and backward functions take
    (rnorm None when norms=False or the operands are split)."""
    im, s = _rows_inner_contig(im), _rows_inner_contig(s)
    dev = im.device
    xm = torch.empty(geom.xm_bytes // 2, dtype=torch.float16, device=dev)
    xe = torch.empty(max(geom.xe_bytes // 2, 8), dtype=torch.float16, device=dev)
    y = torch.empty(geom.y_bytes // 2, dtype=torch.float16, device=dev)
    rnorm = torch.empty(geom.rnorm_bytes // 4, dtype=torch.float32, device=dev) if norms and not geom.split else None
    packed = Packed(geom, xm, xe, y, rnorm)
    vi, vs, pk = _set_view(im, im_len_t), _set_view(s, s_len_t), packed.struct()
    _lib.check(_lib.load().aladin_align_pack(C.byref(vi), C.byref(vs), C.byref(geom), C.byref(pk), _stream()), 'align_pack')
    return packed


def _align_forward(im, s, im_len_t, s_len_t, x_tail=0, y_tail=2, precision=None, norms=True):
    """-> (S, packed) where packed = Packed(geom, xm, xe, y, rnorm) is kept for the backward pass.
    `im` is the max-side set, `s` the sum-side set (images / captions for 'MrSw')."""
    Bi, R, D = im.shape
    Bc, T, D2 = s.shape
    if D != D2:
        raise ValueError('aladin_amd: feature sizes differ (%d vs %d)' % (D, D2))
    geom = align_geometry(Bi, Bc, R, T, D, x_tail, y_tail, precision, layout='auto')
    packed = Packed(*pack_sets(im, s, im_len_t, s_len_t, geom, norms=norms))
    return scores_from_packed(packed.xm, packed.xe, packed.y, geom), packed


def _grad_like(x):
    """Gradient buffer in x's own layout when x is a dense permutation with a unit inner stride (the model's
    (S,B,D)->(B,S,D) views): autograd then hands it to the leaf without a re-layout copy.  Contiguous otherwise."""
    if x.stride(-1) == 1 and torch.ops.aten.is_non_overlapping_and_dense(x) and all(st % 4 == 0 for st in x.stride()[:-1]):
        return torch.empty_like(x, dtype=torch.float32)
    return torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)


DENSE_MIN_FRACTION = 0.4     # of the pairs carrying a gradient: below, the list path (cost ~ 3.2 ms x fraction at B = 256) beats the dense one (~1.4 ms)
DENSE_MIN_PAIRS = 1 << 14    # below: the per-pair kernel is launch-bound and already faster (B = 64: 0.20 vs 0.26 ms)
DENSE_ROWS_GEMM = True       # False: ALADIN_BWD_DENSE_GATHER -- the dense table with the per-row gather (bit-identical to the list path)
DENSE_BACKWARD = True        # False: always one workgroup per gradient-carrying pair (the A/B switch of tests/ and tools/experiments/bench_dense_ds.py)


class _DensityProbe:
    """How dense is dloss/dS of the sum-of-violations hinge?  Early in training nearly every pair violates the margin, late
    few do -- and only the device knows (the hinge kernel's pair count).  Reading it at once would stall the host, so each
    step's count leaves by ONE asynchronous copy and the choice between the dense and the list backward at step n follows
    the count of step n - LAG (the density drifts slowly).  The lag is FIXED, not "whatever has arrived": the two paths sum
    in different orders, and which one runs must not depend on timing (bitwise reproducible runs); waiting for a copy
    issued LAG steps ago costs nothing unless the host is more than LAG steps ahead of the device.
    Before step LAG: `unknown` (dense for the fused sum-of-violations node, the list path for a generic gradient)."""
    LAG = 2

    def __init__(self, unknown=True):
        self._hist = []                                     # [buffer, event, total] of the last LAG + 1 recorded steps, oldest first
        self.fraction = None
        self.unknown = unknown

    def step(self, count, total):
        """Record this step's count; -> dense? for this step."""
        if torch.cuda.is_current_stream_capturing():        # no host copies inside a graph: keep the last answer
            return self.dense()
        if len(self._hist) >= self.LAG:
            buf, ev, tot = self._hist[-self.LAG]
            ev.synchronize()
            self.fraction = int(buf[0]) / tot
        if len(self._hist) > self.LAG:
            slot = self._hist.pop(0)
        else:
            slot = [torch.empty(1, dtype=count.dtype).pin_memory(), torch.cuda.Event(), 1.0]
        if slot[0].dtype != count.dtype:
            slot[0] = torch.empty(1, dtype=count.dtype).pin_memory()
        slot[0].copy_(count.reshape(1), non_blocking=True)
        slot[1].record()
        slot[2] = float(total)
        self._hist.append(slot)
        return self.dense()

    def dense(self):
        return self.unknown if self.fraction is None else self.fraction >= DENSE_MIN_FRACTION

    def newest(self):
        """The fraction of the most recent recorded step (waits for it; for tests / tools)."""
        if not self._hist:
            return None
        buf, ev, tot = self._hist[-1]
        ev.synchronize()
        return int(buf[0]) / tot


_density_probe = _DensityProbe()
# a gradient arriving on a score matrix from OUTSIDE the fused nodes (ops.alignment_scores + any loss: the 'MwSr' / 'symm'
# poolings, a caller's own criterion): its non-zeros are counted (one small launch) and, as above, steer the backward of
# the same shape LAG steps later; until then the list path (the usual dS is the hardest-negative hinge's: <= 3B entries)
_generic_probes = {}
_LAST_BWD_FLAGS = [0]
DENSE_GEMM_FORCE = False     # tests / tools: the GEMM row step whatever the captions' fill


def _caption_fill(s_len, T, y_tail=2):
    """Mean share of a caption's 16-word tiles that holds real words (None: lengths only on the device).  The gather row
    step costs ~ real words, the GEMM one the padded tiles: measured crossover (B = 256, tools/experiments/dense_backward_probe.py fill)
    at a fill of 0.42 for R' = 33 and 0.50 for R' = 50 -- COCO captions (~12 of 35 tokens) are on the gather side."""
    if isinstance(s_len, torch.Tensor):
        return None
    Tq = T - 1 - y_tail
    if Tq < 1 or len(s_len) == 0:
        return None
    tile = (Tq + 15) // 16 * 16
    return sum(min(max(int(v) - 1 - y_tail, 0), Tq) for v in s_len) / float(len(s_len) * tile)


def _gemm_rows_pay(fill, Rq):
    if DENSE_GEMM_FORCE or fill is None:
        return True
    return fill >= min(0.7, max(0.35, 0.42 + 0.08 * (Rq - 33) / 17.0))


def _align_backward(im, s, im_len_t, s_len_t, dS, gscale=None, packed=None, pairs=None, x_tails=(0, 2), dense=False, fill=None):
    """aladin_align_bwd (a long-set problem: the pair-list path for any dS, a dense one included).
    packed: Packed / (geom, xm, xe, y[, rnorm]) of the forward (None: the exact fp32 recompute); with its operands at hand the row
    step's unit vectors are as set_backward_precision() says.
    dense: the caller knows that (almost) every pair carries a gradient (sum-of-violations hinge, a gradient on S):
    ALADIN_BWD_DENSE -- the arg-max table of all pairs from the split-precision tile kernel instead of one workgroup per pair."""
    lib = _lib.load()
    im = _rows_inner_contig(im)
    s = _rows_inner_contig(s)
    dS = dS.contiguous()
    ld_dS = dS.shape[1]            # (not stride(0): a contiguous (1, n) view may report any leading stride)
    Bi, R, D = im.shape
    Bc, T, _ = s.shape
    packed = Packed(*packed) if packed is not None else None
    have = packed is not None and packed.at_hand()
    geom = packed.geom if packed is not None else align_geometry(Bi, Bc, R, T, D, *x_tails, layout='auto')
    long = geom.layout == _lib.LAYOUT_LONG
    if packed is None and not long and x_tails != (0, 2):
        raise NotImplementedError('aladin_amd: the stand-alone backward entry point is the image/caption form')
    dense_flag = _lib.BWD_DENSE if (dense and not long and DENSE_BACKWARD and have and Bi * Bc >= DENSE_MIN_PAIRS) else 0
    if dense_flag and not (DENSE_ROWS_GEMM and _gemm_rows_pay(fill, R - 1 - geom.x_tail)):
        dense_flag |= _lib.BWD_DENSE_GATHER
    _LAST_BWD_FLAGS[0] = dense_flag                      # which path the last backward took (tests)
    d_im, d_s = _grad_like(im), _grad_like(s)
    pk = C.byref(packed.struct()) if have else None
    flags = (_bwd_flags(packed) if have else 0) | dense_flag
    vi, vs, gi, gs = _set_view(im, im_len_t), _set_view(s, s_len_t), _grad_view(d_im), _grad_view(d_s)
    ws = _workspace(lib.aladin_align_bwd_workspace_bytes(C.byref(geom), dense_flag), im.device)
    _lib.check(lib.aladin_align_bwd(C.byref(vi), C.byref(vs), C.byref(geom), pk, _ptr(dS), ld_dS, _ptr(gscale),
                                    _ptr(pairs[0] if pairs else None), _ptr(pairs[1] if pairs else None),
                                    C.byref(gi), C.byref(gs), _ptr(ws), flags, _stream()), 'align_bwd')
    return d_im, d_s


_TRIPLET_WS = {}


def _triplet_fused_ok(geom):
    """Shapes aladin_align_triplet_fwd covers (= the fp16 pair kernel's: every training config)."""
    return _pair_kernel_covers(geom) and geom.Bi == geom.Bc and not geom.split and geom.D % 4 == 0 and geom.D <= 1024


def _triplet_forward(im, s, im_len_t, s_len_t, margin, loss_out=None):
    """aladin_align_triplet_fwd: pack + side GEMM + scores + hinge statistics + [pair arg-max | hinge element-wise] in ONE C call.
    -> (loss, S, AlignSaved): the operands xm | xe | y | rnorm are ONE allocation, the node's workspace (side scratch, statistics,
    arg-max table, dS^T) another -- both untouched until the backward.  None when the shape is not covered (the caller composes
    the generic calls)."""
    Bi, R, D = im.shape
    Bc, T, _ = s.shape
    geom = align_geometry(Bi, Bc, R, T, D, layout='auto')
    if not _triplet_fused_ok(geom):
        return None
    lib = _lib.load()
    im, s = _rows_inner_contig(im), _rows_inner_contig(s)
    dev = im.device
    key = (Bi, R, T, D)
    lay = _TRIPLET_WS.get(key)
    if lay is None:
        up = lambda v: (int(v) + 255) // 256 * 256
        o_xe = up(geom.xm_bytes)
        o_y = o_xe + up(max(geom.xe_bytes, 16))
        o_rn = o_y + up(geom.y_bytes)
        lay = ((o_xe, o_y, o_rn), o_rn + up(geom.rnorm_bytes), int(lib.aladin_align_triplet_workspace_bytes(C.byref(geom))))
        if len(_TRIPLET_WS) < 256:
            _TRIPLET_WS[key] = lay
    offs, n_buf, n_ws = lay
    buf = torch.empty(n_buf, dtype=torch.uint8, device=dev)
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    S = torch.empty((Bi, Bc), dtype=torch.float32, device=dev)
    dS = torch.empty((Bi, Bc), dtype=torch.float32, device=dev)
    loss = loss_out if loss_out is not None else torch.empty((), dtype=torch.float32, device=dev)
    vi, vs, pk = _set_view(im, im_len_t), _set_view(s, s_len_t), _packed_from_buf(buf, offs)
    _lib.check(lib.aladin_align_triplet_fwd(C.byref(vi), C.byref(vs), C.byref(geom), float(margin), C.byref(pk), _ptr(S), S.stride(0),
                                            _ptr(loss), _ptr(dS), _ptr(ws), _stream()), 'align_triplet_fwd')
    return loss, S, AlignSaved(geom, im, s, dS, ws, (buf,), offs=offs, table=True)


def _packed_from_buf(buf, offs):
    """struct aladin_packed of the one-allocation operand buffer, without a tensor view (the fused step is host-bound)."""
    base = buf.data_ptr()
    return _lib.Packed(base, base + offs[0], base + offs[1], base + offs[2])


def _triplet_backward(im, s, im_len_t, s_len_t, geom, pk, dS, ws, gscale, base_workspace=False):
    """aladin_align_triplet_bwd: the row kernel on the table _triplet_forward (or, base_workspace=True, the small-batch heads)
    left in `ws`.  pk: struct aladin_packed of the forward's operands (with rnorm for the fp16 row step)."""
    lib = _lib.load()
    d_im, d_s = _grad_like(im), _grad_like(s)
    flags = _bwd_precision_bits(bool(pk.rnorm))
    if base_workspace:
        flags |= _lib.TRIPLET_BWD_BASE_WORKSPACE
    vi, vs, gi, gs = _set_view(im, im_len_t), _set_view(s, s_len_t), _grad_view(d_im), _grad_view(d_s)
    _lib.check(lib.aladin_align_triplet_bwd(C.byref(vi), C.byref(vs), C.byref(geom), C.byref(pk), _ptr(dS), _ptr(gscale), C.byref(gi),
                                            C.byref(gs), _ptr(ws), flags, _stream()), 'align_triplet_bwd')
    return d_im, d_s


class AlignSaved:
    """What the forward of an alignment head leaves for its backward.  Producers: _triplet_forward (the fused call),
    _align_head_forward (the composed calls), _SmallHeads (the small-batch heads' launch); one consumer: backward().
    The tensors go through the node's save_for_backward (tensors(), handed out once); the rest stays here, on the node's ctx:
      offs            byte offsets of xe, y, rnorm in the ONE operand buffer of the fused call; None: xm, xe, y, rnorm are four tensors
      table, base_ws  the arg-max table of dS's pairs is already in the saved workspace [which is laid out as aladin_align_bwd's]
      pairs, dense, fill   without a table, for _align_backward: the hinge's pair list, the density probe's answer, the captions' fill
      live            a dS was produced: there is something to back-propagate"""
    __slots__ = ('geom', 'offs', 'table', 'base_ws', 'pairs', 'dense', 'fill', 'live', '_tensors')

    def __init__(self, geom, im, s, dS, ws, operands, offs=None, table=False, base_ws=False, pairs=None, dense=False, fill=None):
        self.geom, self.offs, self.table, self.base_ws = geom, offs, table, base_ws
        self.pairs, self.dense, self.fill, self.live = pairs, dense, fill, dS is not None
        self._tensors = [im, s, dS, ws, *operands]

    def tensors(self):
        """[im, s (in the row layout the kernels were given), dS, workspace, operands...] for save_for_backward."""
        out, self._tensors = self._tensors, None
        return out

    def backward(self, saved, im_len_t, s_len_t, gscale, g_scores=None):
        """-> (d_im, d_s).  saved: tensors() as the node's ctx.saved_tensors returns them; gscale: the upstream gradient of the
        loss as a device scalar (None: none arrived); g_scores: a gradient on the returned score matrix."""
        im, s, dS, ws, *operands = saved
        if self.table and g_scores is None:
            # the training path: the table is already there (forward), only the row kernel is left; dloss/dS never leaves the
            # device and the upstream scalar goes to the kernels as a pointer
            pk = _packed_from_buf(operands[0], self.offs) if self.offs is not None else Packed(self.geom, *operands).struct()
            return _triplet_backward(im, s, im_len_t, s_len_t, self.geom, pk, dS, ws, gscale, base_workspace=self.base_ws)
        packed = Packed.from_buf(operands[0], self.geom, self.offs) if self.offs is not None else Packed(self.geom, *operands)
        if g_scores is None:
            return _align_backward(im, s, im_len_t, s_len_t, dS, gscale=gscale, packed=packed, pairs=self.pairs, dense=self.dense,
                                   fill=self.fill)
        # the returned score matrix was used too (the reference's S carries grad, alad/loss.py:151-159):
        # total dS = g_loss * dloss/dS + g_scores, generally dense
        total = g_scores.to(torch.float32)
        if gscale is not None:
            total = total + dS * gscale
        return _align_backward(im, s, im_len_t, s_len_t, total.contiguous(), packed=packed, dense=True, fill=self.fill)


def _align_head_forward(im, s, im_len_t, s_len_t, margin, max_violation, need, fill=None, hinge=True, loss_out=None):
    """Alignment scores [+ their hinge] -> (loss or None, S, AlignSaved).  need: the sets take a gradient.  With the
    hardest-negative hinge on the fp16 pair kernel's shapes -- every training config -- ONE call into the library
    (_triplet_forward); otherwise pack + scores, the hinge, and for the sum of violations the density probe."""
    if need and hinge:
        _check_backward_supported(im, s, 0, 2)
    fused = _triplet_forward(im, s, im_len_t, s_len_t, margin, loss_out) if (hinge and need and max_violation) else None
    if fused is not None:
        return fused
    S, packed = _align_forward(im, s, im_len_t, s_len_t, norms=need)
    loss = dS = pairs = None
    dense = False
    if hinge:
        loss, dS, pairs = _hinge_raw(S, margin, max_violation, need, want_pairs=True, loss_out=loss_out)
        # sum of violations: dloss/dS is dense while most pairs violate the margin (the previous steps' pair counts say)
        if need and not max_violation:
            dense = _density_probe.step(pairs[1], S.shape[0] * S.shape[1])
    return loss, S, AlignSaved(packed.geom, im, s, dS, None, packed.operands(), pairs=pairs, dense=dense, fill=fill)


class _AlignScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im, s, im_len_t, s_len_t, x_tail, y_tail):
        need = any(ctx.needs_input_grad[:2])
        if need:
            _check_backward_supported(im, s, x_tail, y_tail)
        S, packed = _align_forward(im, s, im_len_t, s_len_t, x_tail, y_tail, norms=need)
        if need:
            ctx.save_for_backward(im, s, im_len_t, s_len_t, *packed.operands())
            ctx.geom = packed.geom
        return S

    @staticmethod
    def backward(ctx, dS):
        im, s, im_len_t, s_len_t, *operands = ctx.saved_tensors
        dense = False
        if DENSE_BACKWARD and dS.numel() >= DENSE_MIN_PAIRS and not torch.cuda.is_current_stream_capturing():
            probe = _generic_probes.setdefault((tuple(dS.shape), ctx.geom.x_tail, ctx.geom.y_tail), _DensityProbe(unknown=False))
            dense = probe.step(torch.count_nonzero(dS), dS.numel())
        d_im, d_s = _align_backward(im, s, im_len_t, s_len_t, dS, packed=Packed(ctx.geom, *operands), dense=dense)
        return d_im, d_s, None, None, None, None


class _AlignTriplet(torch.autograd.Function):
    """scores + hinge in one autograd node (reference alad/loss.py:79-159 with return_loss=True):
    dloss/dS never leaves the device-side workspace and the upstream scalar gradient is handed to
    the backward kernels as a device pointer (no element-wise scaling launch).  With the hardest-negative hinge on the
    fp16 pair kernel's shapes -- every training config -- each direction is ONE call into the library
    (aladin_align_triplet_fwd / _bwd; rounds 1-4: six ctypes calls and nine allocations per step)."""

    @staticmethod
    def forward(ctx, im, s, im_len_t, s_len_t, margin, max_violation, fill):
        need = any(ctx.needs_input_grad[:2])
        loss, S, saved = _align_head_forward(im, s, im_len_t, s_len_t, margin, max_violation, need, fill)
        if need:
            ctx.align = saved
            ctx.save_for_backward(im_len_t, s_len_t, *saved.tensors())
        ctx.set_materialize_grads(False)
        return loss, S

    @staticmethod
    def backward(ctx, g_loss, g_scores):
        if g_loss is None and g_scores is None:
            return None, None, None, None, None, None, None
        im_len_t, s_len_t, *saved = ctx.saved_tensors
        g = _upstream(g_loss) if g_loss is not None else None
        d_im, d_s = ctx.align.backward(saved, im_len_t, s_len_t, g, g_scores)
        return d_im, d_s, None, None, None, None, None


def alignment_triplet_loss(im_set, s_seq, im_len, s_len, margin, max_violation):
    """(loss, S) of AlignmentContrastiveLoss(aggregation='MrSw') in one fused autograd node.  Both outputs
    are differentiable (as in the reference, alad/loss.py:151-159); when only the loss is back-propagated --
    every shipped config: S is fed, detached, to the distillation loss, alad/loss.py:370 -- the backward
    stays on the sparse dloss/dS path."""
    im_len_t, s_len_t = _check_sets(im_set, s_seq, im_len, s_len)
    if im_set.shape[0] != s_seq.shape[0]:
        raise ValueError('aladin_amd: the contrastive loss needs a square score matrix, got (%d, %d) '
                         '(the reference fails in diag/expand_as, alad/loss.py:43-45)' % (im_set.shape[0], s_seq.shape[0]))
    im_set, s_seq = _sets_for_node(im_set, s_seq)
    fill = None if max_violation else _caption_fill(s_len, s_seq.shape[1])
    return _AlignTriplet.apply(im_set, s_seq, im_len_t, s_len_t, margin, max_violation, fill)


def alignment_scores(im_set, s_seq, im_len, s_len, aggregation='MrSw', precision=None):
    """S (Bi, Bc); replaces reference alad/loss.py:80-135.  Differentiable when autograd is on and an
    input requires grad (fp16 operands); otherwise the evaluation grid of eval_grid.score_grid in the evaluation
    precision (`precision` overrides set_eval_precision()).
      'MrSw'  sum over words of the max over regions                       (:124-125)
      'MwSr'  sum over regions of the max over words: the same kernels with the two sets swapped --
              captions on the max side (tail 2), images on the sum side (tail 0) -- transposed (:134-135)
      'symm'  MrSw + MwSr                                                  (:130-133)"""
    if aggregation not in ('MrSw', 'MwSr', 'symm'):
        raise NotImplementedError('aladin_amd: aggregation %r' % (aggregation,))
    if not (torch.is_grad_enabled() and (im_set.requires_grad or s_seq.requires_grad)):
        _check_set_shapes(im_set, s_seq, im_len, s_len)
        prec = precision if precision is not None else _EVAL_PRECISION[0]
        from .eval_grid import TensorSide, _host_lengths, score_grid        # (eval_grid imports this module)
        with torch.no_grad():
            im, s, S = TensorSide(im_set, _host_lengths(im_len), 0), TensorSide(s_seq, _host_lengths(s_len), 2), None
            if aggregation in ('MrSw', 'symm'):
                S = score_grid(im, s, prec)
            if aggregation in ('MwSr', 'symm'):
                St = score_grid(s, im, prec).t()
                S = St if S is None else S + St
        return S
    if precision not in (None, 'fp16'):
        raise ValueError('aladin_amd: differentiable alignment scores use fp16 operands (split precision is forward-only)')
    im_len_t, s_len_t = _check_sets(im_set, s_seq, im_len, s_len)
    im_set, s_seq = _pad_features(im_set, s_seq)
    if aggregation == 'MrSw':
        return _AlignScores.apply(im_set, s_seq, im_len_t, s_len_t, 0, 2)
    if aggregation == 'MwSr':
        return _AlignScores.apply(s_seq, im_set, s_len_t, im_len_t, 2, 0).t()
    if aggregation == 'symm':
        return _AlignScores.apply(im_set, s_seq, im_len_t, s_len_t, 0, 2) + \
            _AlignScores.apply(s_seq, im_set, s_len_t, im_len_t, 2, 0).t()


class _ScanScores(torch.autograd.Function):
    """aggregation='scan-sentences' (reference alad/loss.py:136-149)."""

    @staticmethod
    def forward(ctx, im, s, im_len_t, s_len_t):
        lib = _lib.load()
        im = _rows_inner_contig(im)
        s = _rows_inner_contig(s)
        Bi, R, D = im.shape
        Bc, T, _ = s.shape
        S = torch.empty((Bi, Bc), dtype=torch.float32, device=im.device)
        ws = _workspace(lib.aladin_scan_workspace_bytes(Bi, Bc, R, T, D, 0), im.device)
        _lib.check(lib.aladin_scan_fwd(_ptr(im), im.stride(0), im.stride(1), _ptr(im_len_t), _ptr(s), s.stride(0), s.stride(1),
                                       _ptr(s_len_t), Bi, Bc, R, T, D, _ptr(S), S.stride(0), _ptr(ws), _stream()), 'scan_fwd')
        ctx.save_for_backward(im, s, im_len_t, s_len_t)
        return S

    @staticmethod
    def backward(ctx, dS):
        lib = _lib.load()
        im, s, im_len_t, s_len_t = ctx.saved_tensors
        Bi, R, D = im.shape
        Bc, T, _ = s.shape
        dS = dS.contiguous()
        d_im = torch.empty((Bi, R, D), dtype=torch.float32, device=im.device)
        d_s = torch.empty((Bc, T, D), dtype=torch.float32, device=im.device)
        ws = _workspace(lib.aladin_scan_workspace_bytes(Bi, Bc, R, T, D, 1), im.device)
        _lib.check(lib.aladin_scan_bwd(_ptr(im), im.stride(0), im.stride(1), _ptr(im_len_t), _ptr(s), s.stride(0), s.stride(1),
                                       _ptr(s_len_t), Bi, Bc, R, T, D, _ptr(dS), dS.shape[1], _ptr(None), _ptr(d_im), _ptr(d_s),
                                       _ptr(ws), _stream()), 'scan_bwd')
        return d_im, d_s, None, None


def alignment_scan_scores(im_set, s_seq, im_len, s_len):
    """(Bi, Bc) 'scan-sentences' scores, differentiable; replaces reference alad/loss.py:136-149 (+ :80-116)."""
    im_len_t, s_len_t = _check_sets(im_set, s_seq, im_len, s_len)
    if s_seq.shape[1] < 4:
        raise ValueError('aladin_amd: captions need at least 4 positions (token 0 and the last two are dropped)')
    return _ScanScores.apply(im_set, s_seq, im_len_t, s_len_t)


class _NormSum(torch.autograd.Function):
    """(B,N,D) set -> (B,D) sum of its L2-normalised rows 1 .. len-1-tail."""

    @staticmethod
    def forward(ctx, x, len_t, tail):
        x = _rows_inner_contig(x)
        B, N, D = x.shape
        out = torch.empty((B, D), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().aladin_normsum_fwd(_ptr(x), x.stride(0), x.stride(1), _ptr(len_t), B, N, D, tail, _ptr(out),
                                                  _stream()), 'normsum_fwd')
        ctx.save_for_backward(x, len_t)
        ctx.tail = tail
        return out

    @staticmethod
    def backward(ctx, g):
        x, len_t = ctx.saved_tensors
        B, N, D = x.shape
        g = g.contiguous()
        d_x = torch.empty((B, N, D), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().aladin_normsum_bwd(_ptr(x), x.stride(0), x.stride(1), _ptr(len_t), B, N, D, ctx.tail,
                                                  _ptr(g), _ptr(d_x), _stream()), 'normsum_bwd')
        return d_x, None, None


def alignment_sum_scores(im_set, s_seq, im_len, s_len, mean=False):
    """'sum' / 'mean' pooling (reference alad/loss.py:120-123): the double sum of masked cosines equals
    the dot product of the summed unit vectors, so no region x word tensor is formed."""
    im_len_t, s_len_t = _check_sets(im_set, s_seq, im_len, s_len)
    S = _DotScores.apply(_NormSum.apply(im_set, im_len_t, 0), _NormSum.apply(s_seq, s_len_t, 2))
    if mean:
        S = S / float((im_set.shape[1] - 1) * (s_seq.shape[1] - 3))
    return S


# ------------------------------------------------------------------------------------------------
# head-mean attention window (the cross-encoder teacher's read of its last layer)
# ------------------------------------------------------------------------------------------------
def _window_args(L, rows, cols):
    (row0, W), (col0, Rw) = (int(rows[0]), int(rows[1])), (int(cols[0]), int(cols[1]))
    if row0 < 0 or W < 1 or row0 + W > L or col0 < 0 or Rw < 1 or col0 + Rw > L:
        raise ValueError('aladin_amd: the attention window rows [%d, %d) x columns [%d, %d) must be non-empty and lie inside the '
                         '%d positions of a sequence' % (row0, row0 + W, col0, col0 + Rw, L))
    return row0, W, col0, Rw


def attention_window_unsupported(q, k, mask, heads):
    """None if aladin_attn_window_mean covers these tensors, else the reason as text (the limits of include/aladin_hip.h:
    float32 GPU tensors (N, L, heads * dh) with a unit innermost stride, L <= 256, dh a multiple of 4 up to 128, heads <= 32,
    a 2-D mask).  backbone.CaptionBertSelfAttention chooses between the kernel and its plain path with it."""
    if not (isinstance(q, torch.Tensor) and isinstance(k, torch.Tensor) and isinstance(mask, torch.Tensor)):
        return 'tensors expected'
    if not (q.is_cuda and k.is_cuda and mask.is_cuda):
        return 'the kernel runs on the GPU, got tensors on %s / %s / %s' % (q.device, k.device, mask.device)
    if q.dtype != torch.float32 or k.dtype != torch.float32:
        return 'float32 q and k expected, got %s / %s' % (q.dtype, k.dtype)
    if mask.dim() != 2:
        return 'a 2-D (N, L) mask expected, got %d-D' % mask.dim()
    if q.dim() != 3 or q.shape != k.shape:
        return 'q and k of one shape (N, L, heads * dh) expected, got %s / %s' % (tuple(q.shape), tuple(k.shape))
    N, L, HD = q.shape
    if N < 1 or L < 1 or heads < 1 or HD % heads:
        return 'non-empty (N, L, heads * dh) tensors expected, got %s for %d heads' % (tuple(q.shape), heads)
    dh = HD // heads
    if L > _lib.ATTN_WINDOW_MAX_L or heads > _lib.ATTN_WINDOW_MAX_HEADS or dh > _lib.ATTN_WINDOW_MAX_DH or dh % 4:
        return ('L <= %d, heads <= %d and a head size that is a multiple of 4 up to %d expected, got L=%d heads=%d dh=%d'
                % (_lib.ATTN_WINDOW_MAX_L, _lib.ATTN_WINDOW_MAX_HEADS, _lib.ATTN_WINDOW_MAX_DH, L, heads, dh))
    return None


def attention_window_mean(q, k, mask, heads, rows, cols, out=None):
    """out[n, i - row0, j - col0] = mean over heads of softmax_j(<q_i, k_j> / sqrt(dh) + (1 - mask_j) * -10000)[i, j] for
    rows = (row0, W), cols = (col0, Rw): the slice the cross-encoder teacher takes of `attention[-1].mean(dim=1)`, reference
    alad/train.py:373-376 over oscar/modeling/modeling_bert.py:47-53, from the layer's query(x) / key(x) outputs
    (N, L, heads * dh) -- one launch, no (N, heads, L, L) tensor.  q and k are read in place through their strides (unit innermost
    stride required, nothing is copied or transposed); mask: (N, L) of 0 / 1, int64 or float.  out: None or a float32
    (N, W, Rw) tensor or view with a unit innermost stride (a slice of a larger preallocated tensor); it is returned.
    No autograd: the teacher is a target."""
    why = attention_window_unsupported(q, k, mask, heads)
    if why is not None:
        raise ValueError('aladin_amd: attention_window_mean: ' + why)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad):
        raise RuntimeError('aladin_amd: attention_window_mean has no backward (the teacher is built under torch.no_grad()); '
                           'detach q and k or disable grad')
    _require_gpu(q, k)
    N, L, HD = q.shape
    row0, W, col0, Rw = _window_args(L, rows, cols)
    if mask.shape[0] != N or mask.shape[1] != L or mask.device != q.device or k.device != q.device:
        raise ValueError('aladin_amd: attention_window_mean: a mask of shape (%d, %d) on %s expected, got %s on %s'
                         % (N, L, q.device, tuple(mask.shape), mask.device))
    for name, t in (('q', q), ('k', k)):
        if t.stride(2) != 1 or t.stride(1) < HD or t.stride(0) < 0 or t.data_ptr() % 4:
            raise ValueError('aladin_amd: attention_window_mean: %s is read in place and needs a unit innermost stride and rows that '
                             'do not overlap (strides %s for shape %s)' % (name, tuple(t.stride()), tuple(t.shape)))
    if mask.dtype not in (torch.int64, torch.float32):
        mask = mask.to(torch.float32)
    if mask.stride(1) != 1 and L > 1:
        mask = mask.contiguous()
    if out is None:
        out = torch.empty((N, W, Rw), dtype=torch.float32, device=q.device)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != q.device or tuple(out.shape) != (N, W, Rw):
            raise ValueError('aladin_amd: attention_window_mean: out must be a float32 (%d, %d, %d) tensor on %s' % (N, W, Rw, q.device))
        if (Rw > 1 and out.stride(2) != 1) or (W > 1 and out.stride(1) < Rw) or (N > 1 and out.stride(0) < W * out.stride(1)):
            raise ValueError('aladin_amd: attention_window_mean: out needs a unit innermost stride and rows that do not overlap '
                             '(strides %s)' % (tuple(out.stride()),))
    o_sr = out.stride(1) if W > 1 else max(out.stride(1), Rw)
    o_sn = out.stride(0) if N > 1 else max(out.stride(0), W * o_sr)
    _lib.check(_lib.load().aladin_attn_window_mean(
        _ptr(q), q.stride(0), q.stride(1), _ptr(k), k.stride(0), k.stride(1), _ptr(mask), 2, int(mask.dtype == torch.int64),
        mask.stride(0), N, L, heads, HD // heads, row0, W, col0, Rw, _ptr(out), o_sn, o_sr, _stream()), 'attn_window_mean')
    return out


# ------------------------------------------------------------------------------------------------
# One namespace for callers (`from aladin_amd import ops; ops.hinge_loss(...)`): the losses, the loss heads and the retrieval
# functions live in ops_losses / ops_heads / ops_retrieval (round 5 split of a 1400-line module) and are looked up lazily, so that
# ops_heads may import THIS module (it builds on the alignment nodes) without a cycle.
# ------------------------------------------------------------------------------------------------
_SUBMODULES = ('ops_losses', 'ops_heads', 'ops_retrieval')


def __getattr__(name):
    import importlib
    if name.startswith('__'):
        raise AttributeError(name)
    for m in _SUBMODULES:
        mod = importlib.import_module('.' + m, __package__)
        if name in mod.__dict__:
            return mod.__dict__[name]
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
