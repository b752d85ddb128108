"""The no-grad alignment grid behind ops.alignment_scores, compute_sim_matrix(mode='alignment'), i2t and t2i: one planner, one
plan cache and one driver, score_grid(max side, sum side, precision), for (N, L, D) tensors and PackedSetStore / StoreView
operands alike -- so both give the same bits.  What the differentiable path does not do:
  * operands in the evaluation precision (split fp16 by default: rank-exact Recall);
  * both sets are trimmed to the positions that can matter (positions() below).  encode_data pads every set to 71 positions
    (alad/evaluation.py:98-99); positions past a set's length are masked to 0 by alad/loss.py:103-116 whatever they hold.  On
    the SUM side a masked position adds exactly 0; on the MAX side it still takes part in the max as a zero, so ONE is kept;
  * large ragged grids are scored in length classes.  The packed geometry pads the max side to its region classes (32 rows,
    32 + up to 8 side rows, 48, 48 + up to 8 side rows, 64, 96: align_fwd.hip geometry) and the sum side to 8, 16, 24, 32, 40,
    48, 64 or 96 words: one launch over the whole grid pays for the LONGEST image and caption at every pair.  Real sets are
    ragged (COCO: 10-50 boxes, captions of ~12 tokens), so each side's samples are grouped by the tile class their own length
    needs, every (image class x caption class) block gets its own geometry, and the blocks are laid back in the callers'
    order.  A score depends on its own image and caption rows only (masked positions are zero rows whatever the class): the
    scores are the single launch's up to the summation order of another kernel variant (~1e-7 in split precision);
  * the sum side is chunked so the score kernel's side-row scratch stays under E_SCRATCH_LIMIT (16 GB at 5000 x 25000
    otherwise); a score does not depend on the chunking.
"""
import ctypes as C

import torch

from . import _lib, ops

X_CLASS_BOUNDS = (32, 40, 48, 56, 64, 96)  # scored max-side positions (incl. the one masked position kept for the zero fill)
Y_CLASS_BOUNDS = (8, 16, 24, 32, 40, 48, 64, 96)   # scored sum-side positions (8 / 24 / 40: two captions share one / three / five 16-word tiles)
BUCKET_MIN_PAIRS = 1 << 18                 # below this a grid is one launch
BUCKET_MIN_SAMPLES = 64                    # smaller classes join the next longer one
BUCKET_MIN_GAIN = 0.10                     # padded work saved before bucketing is worth its extra launches
E_SCRATCH_LIMIT = 2 << 30                  # bytes of side-GEMM scratch per score launch before the sum side is chunked


def positions(c, cap, keep_masked):
    """Positions of the packed operand a sample needs.  c: its scored count len - 1 - tail (before clamping); cap: those of a
    sample that fills the padded set, total - 1 - tail.  The count is clamped to [1, cap]; on the max side (keep_masked) one
    masked position is added unless the sample fills the set (alad/loss.py:116,124: the zero fill takes part in the max).
    Monotone in c, so a block needs the positions of its longest sample."""
    cap = max(cap, 1)
    n = min(max(c, 1), cap)
    return n + 1 if keep_masked and n < cap else n


def bucket_plan(x_need, y_need):
    """-> (x_groups, y_groups) lists of index lists (callers' order inside a group), or None when one launch is the better
    choice.  x_need / y_need: positions per sample (positions())."""
    def groups(need, bounds):
        cls = [[] for _ in bounds]
        for k, n in enumerate(need):
            for c, b in enumerate(bounds):
                if n <= b or c == len(bounds) - 1:
                    cls[c].append(k)
                    break
        for c in range(len(cls) - 1):                               # small classes join the next longer one
            if 0 < len(cls[c]) < BUCKET_MIN_SAMPLES:
                cls[c + 1] = sorted(cls[c] + cls[c + 1])
                cls[c] = []
        last = [c for c in range(len(cls)) if cls[c]]
        if len(last) > 1 and len(cls[last[-1]]) < BUCKET_MIN_SAMPLES:   # a small LAST class takes its neighbour in
            cls[last[-1]] = sorted(cls[last[-2]] + cls[last[-1]])
            cls[last[-2]] = []
        return [(g, bounds[c]) for c, g in enumerate(cls) if g]
    if len(x_need) * len(y_need) < BUCKET_MIN_PAIRS:
        return None
    gx, gy = groups(x_need, X_CLASS_BOUNDS), groups(y_need, Y_CLASS_BOUNDS)
    if len(gx) == 1 and len(gy) == 1:
        return None

    def padded(n, bounds):
        return next((b for b in bounds if n <= b), bounds[-1])
    one = len(x_need) * len(y_need) * padded(max(x_need), X_CLASS_BOUNDS) * padded(max(y_need), Y_CLASS_BOUNDS)
    work = sum(len(a) * len(b) * padded(max(x_need[k] for k in a), X_CLASS_BOUNDS) * padded(max(y_need[k] for k in b), Y_CLASS_BOUNDS)
               for a, _ in gx for b, _ in gy)
    if work > (1.0 - BUCKET_MIN_GAIN) * one:
        return None
    return [a for a, _ in gx], [b for b, _ in gy]


def _index_tensor(ids, device, dtype=torch.int64):
    """Index list -> device tensor WITHOUT making the host wait for the device (torch.tensor(..., device=...) is a blocking
    copy: it drains the stream, and a grid scored in blocks would serialise host and GPU work block by block)."""
    return torch.tensor(ids, dtype=dtype).to(device, non_blocking=True)


class GridPlan:
    """The length classes of one evaluation grid, with everything the blocks need already on the device: per-class index
    tensors and the permutation that lays the class-ordered blocks back in the callers' order.  Built once per
    (lengths, device) and cached: validation scores the same sets twice per epoch (i2t, t2i) and every epoch again."""

    def __init__(self, gx, gy, device):
        self.gx, self.gy = gx, gy
        self.ix = [_index_tensor(g, device) for g in gx]
        self.iy = [_index_tensor(g, device) for g in gy]
        Bx, By = sum(len(g) for g in gx), sum(len(g) for g in gy)
        inv_x = torch.empty(Bx, dtype=torch.int64)
        inv_x[torch.tensor([k for g in gx for k in g], dtype=torch.int64)] = torch.arange(Bx, dtype=torch.int64)
        inv_y = torch.empty(By, dtype=torch.int64)
        inv_y[torch.tensor([k for g in gy for k in g], dtype=torch.int64)] = torch.arange(By, dtype=torch.int64)
        self.inv_x, self.inv_y = inv_x.to(device, non_blocking=True), inv_y.to(device, non_blocking=True)

    def assemble(self, blocks):
        """Blocks scored in class order -> the (Bx, By) matrix in the callers' order."""
        rows = [torch.cat([blocks[(a, b)] for b in range(len(self.gy))], dim=1) for a in range(len(self.gx))]
        return torch.cat(rows, dim=0).index_select(0, self.inv_x).index_select(1, self.inv_y)


_PLAN_CACHE = {}


def grid_plan(key, x_need_fn, y_need_fn, device):
    """Cached GridPlan (or None: one launch) for `key`; the *_need_fn callables are only evaluated on a miss."""
    key = key + (str(device),)
    if key in _PLAN_CACHE:
        return _PLAN_CACHE[key]
    plan = bucket_plan(x_need_fn(), y_need_fn())
    entry = GridPlan(plan[0], plan[1], device) if plan is not None else None
    if len(_PLAN_CACHE) >= 8:
        _PLAN_CACHE.clear()
    _PLAN_CACHE[key] = entry
    return entry


def _host_lengths(lens):
    return [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]


class _Side:
    """One set of a grid.  tail: the trailing positions the alignment head drops; total: the positions of the padded set (a
    class's sub(index list, device index tensor, keep_masked) keeps it: a sample fills THAT set or it does not); counts() /
    max_count: the scored counts len - 1 - tail; key(): what a cached plan depends on (nothing that keeps a store alive)."""
    long_sets = False                       # may the side's geometry be the long-set one (layout='auto')?
    pack_pair = None                        # optional: (y_side, R, T, precision) -> scores with ONE pack launch for both sets

    def top(self, keep_masked):
        """Positions the whole side needs: those of its longest sample."""
        return positions(self.max_count, self.total - 1 - self.tail, keep_masked)

    def need(self, keep_masked):
        return [positions(c, self.total - 1 - self.tail, keep_masked) for c in self.counts()]


class TensorSide(_Side):
    """(N, L, D) float32 sets on the device with their lengths as host ints (_host_lengths)."""
    long_sets = True

    def __init__(self, sets, lens, tail, total=None):
        self.sets, self.lens, self.tail, self.D, self.device = sets, lens, tail, sets.shape[2], sets.device
        self.total, self.max_count, self._lens_t = (sets.shape[1] if total is None else total), max(self.lens) - 1 - tail, None

    def __len__(self):
        return len(self.lens)

    def counts(self):
        return [v - 1 - self.tail for v in self.lens]

    def lens_t(self):
        if self._lens_t is None:
            self._lens_t = ops.lengths_tensor(self.lens, self.device)
        return self._lens_t

    def key(self):
        return ('dense', tuple(self.lens), self.tail, self.total)

    def sub(self, ids, ids_t, keep_masked):
        lens = [self.lens[k] for k in ids]
        n_pos = positions(max(lens) - 1 - self.tail, self.total - 1 - self.tail, keep_masked)      # the class is cut at what it needs
        return TensorSide(self.sets[:, :n_pos + 1 + self.tail].index_select(0, ids_t), lens, self.tail, self.total)

    def pack_pair(self, y, R, T, precision):
        return ops._align_forward(self.sets[:, :R], y.sets[:, :T], self.lens_t(), y.lens_t(), self.tail, y.tail, precision, norms=False)[0]

    def pack_max(self, geom):
        return ops.pack_images(self.sets[:, :geom.R], self.lens_t(), geom)

    def pack_sum(self, geom, j0, j1):
        return ops.pack_captions(self.sets[j0:j1, :geom.T], self.lens_t()[j0:j1].contiguous(), geom)


class StoreSide(_Side):
    """A PackedSetStore or StoreView: operands are row copies of its rows; total is the store's padded_len."""

    def __init__(self, src, ids=None, ids_t=None):
        self.store = getattr(src, 'store', src)
        if ids is None and src is not self.store:
            ids, ids_t = src.ids, src.ids_t
        self.ids, self.ids_t, self._base = ids, ids_t, ids_t        # None: the whole store
        st = self.store
        self.tail, self.total, self.D, self.device, self.precision = st.tail, st.padded_len, st.D, st.device, st.precision
        self.max_count = st.max_count(ids)

    def __len__(self):
        return len(self.store) if self.ids is None else len(self.ids)

    def counts(self):
        return self.store._counts if self.ids is None else [self.store._counts[k] for k in self.ids]

    def key(self):
        st = self.store                             # identity and fill state: an append invalidates the plan
        return ('store', id(st), st.n_rows, len(st), tuple(self.ids if self.ids is not None else range(len(st))))

    def _all_ids(self):
        if self._base is None:
            self._base = torch.arange(len(self), dtype=torch.int32, device=self.device)
        return self._base

    def sub(self, ids, ids_t, keep_masked):
        return StoreSide(self.store, ids if self.ids is None else [self.ids[k] for k in ids], self._all_ids().index_select(0, ids_t))

    def pack_max(self, geom):
        offs, cnt = self.store._tables()
        xm = torch.empty(geom.xm_bytes // 2, dtype=torch.float16, device=self.device)
        xe = torch.empty(max(geom.xe_bytes // 2, 8), dtype=torch.float16, device=self.device)
        _lib.check(_lib.load().aladin_align_pack_store_x(ops._ptr(self.store.rows), ops._ptr(offs), ops._ptr(cnt), ops._ptr(self.ids_t),
                                                         C.byref(geom), ops._ptr(xm), ops._ptr(xe), ops._stream()), 'align_pack_store_x')
        return xm, xe

    def pack_sum(self, geom, j0, j1):
        offs, cnt = self.store._tables()
        ids_t = self.ids_t if (j0, j1) == (0, len(self)) else self._all_ids()[j0:j1].contiguous()
        y = torch.empty(geom.y_bytes // 2, dtype=torch.float16, device=self.device)
        _lib.check(_lib.load().aladin_align_pack_store_y(ops._ptr(self.store.rows), ops._ptr(offs), ops._ptr(cnt), ops._ptr(ids_t),
                                                         C.byref(geom), ops._ptr(y), ops._stream()), 'align_pack_store_y')
        return y


def score_grid(x, y, precision):
    """(len(x), len(y)) float32 scores of the max side x against the sum side y: class blocks, or one launch for a grid below
    BUCKET_MIN_PAIRS, one the planner leaves alone, or one of the long-set kernels (no classes past 96, never chunked)."""
    plan = None
    if len(x) * len(y) >= BUCKET_MIN_PAIRS and \
            not (x.long_sets and ops.is_long(x.top(True) + 1 + x.tail, y.top(False) + 1 + y.tail, x.tail, y.tail)):
        plan = grid_plan(x.key() + y.key(), lambda: x.need(True), lambda: y.need(False), x.device)
    if plan is None:
        return score_block(x, y, precision)
    ys = [y.sub(g, ig, False) for g, ig in zip(plan.gy, plan.iy)]
    blocks = {}
    for a, (g, ig) in enumerate(zip(plan.gx, plan.ix)):
        xa = x.sub(g, ig, True)
        for b, yb in enumerate(ys):
            blocks[(a, b)] = score_block(xa, yb, precision)
    return plan.assemble(blocks)


def score_block(x, y, precision):
    """One geometry for the whole block: the max side packed once, then one score launch, or one per sum-side chunk when the
    side-row scratch (Bx x 16*tp16*By floats when R' = 33) would pass E_SCRATCH_LIMIT."""
    Bx, By = len(x), len(y)
    R, T = min(x.total, x.top(True) + 1 + x.tail), min(y.total, y.top(False) + 1 + y.tail)
    geom = ops.align_geometry(Bx, By, R, T, x.D, x.tail, y.tail, precision, 'auto' if x.long_sets else 'tiles')
    step = By if geom.e_bytes <= E_SCRATCH_LIMIT else max(geom.cap_unit, int(By * E_SCRATCH_LIMIT // geom.e_bytes) // geom.cap_unit * geom.cap_unit)
    if step >= By and x.pack_pair is not None:
        return x.pack_pair(y, R, T, precision)
    xm, xe = x.pack_max(geom)
    S = torch.empty((Bx, By), dtype=torch.float32, device=x.device)
    for j0 in range(0, By, step):
        j1 = min(By, j0 + step)
        g = ops.align_geometry(Bx, j1 - j0, R, T, x.D, x.tail, y.tail, precision,        # same max-side layout
                               'long' if geom.layout == _lib.LAYOUT_LONG else 'tiles')
        ops.scores_from_packed(xm, xe, y.pack_sum(g, j0, j1), g, out=S[:, j0:j1])
    return S
