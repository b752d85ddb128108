"""aladin_amd/eval_grid.py without a GPU: the planner, the class loop and the chunk loop run as they are, on CPU tensors, with the
four HIP entry points they call (ops.pack_images / pack_captions / pack_sets / scores_from_packed) replaced by the torch
restatements of tests/helpers/cpu_standins.py.  fp16 operands throughout: the stand-ins refuse split ones."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import alad_oracle as O
import cpu_standins
from aladin_amd import eval_grid, ops, synth

PACKERS = ('pack_images', 'pack_captions', 'pack_sets', 'scores_from_packed')


@pytest.fixture(scope='module')
def sets():
    """40 images x 200 captions, D = 32, ragged over the whole length range, four images filling the padded set."""
    images, captions, il, cl = synth.eval_sets(40, 32, seed=77, img_len_range=(6, 70), cap_len_range=(5, 66), n_full=4)
    ims, ils = np.ascontiguousarray(images[0::5]), il[0::5]
    ref = {agg: O.alignment_scores(ims, captions, ils, cl, aggregation=agg, dtype=np.float64) for agg in ('MrSw', 'MwSr')}
    return torch.from_numpy(ims), torch.from_numpy(captions), ils, cl, ref


@pytest.fixture
def grid(monkeypatch):
    """The stand-ins in place, every grid bucketed (as small as it is), an empty plan cache and call counter."""
    for name in PACKERS:
        monkeypatch.setattr(ops, name, getattr(cpu_standins, name))
    monkeypatch.setattr(eval_grid, 'BUCKET_MIN_PAIRS', 1)
    monkeypatch.setattr(eval_grid, 'BUCKET_MIN_SAMPLES', 4)
    monkeypatch.setattr(eval_grid, 'BUCKET_MIN_GAIN', 0.0)
    monkeypatch.setattr(eval_grid, '_PLAN_CACHE', {})
    cpu_standins.CALLS.clear()
    return monkeypatch


def assert_close(S, ref, rtol, atol_rel):
    """|S - ref| <= rtol |ref| + atol_rel max |ref| (tests/test_gpu_parity.py: assert_scores_close)."""
    S, ref = np.asarray(S, np.float64), np.asarray(ref, np.float64)
    err, mag = np.abs(S - ref), np.abs(ref).max()
    print('max |err| %.3g at a largest score of %.3g' % (err.max(), mag))
    np.testing.assert_allclose(S, ref, rtol=rtol, atol=atol_rel * mag)


def calls():
    return {k: cpu_standins.CALLS.get(k, 0) for k in PACKERS}


def test_bucketed_grid_is_one_pack_and_one_score_call_per_block(sets, grid):
    ims, caps, il, cl, ref = sets
    x, y = eval_grid.TensorSide(ims, il, 0), eval_grid.TensorSide(caps, cl, 2)
    plan = eval_grid.bucket_plan(x.need(True), y.need(False))
    assert (len(plan[0]), len(plan[1])) == (4, 7)
    S_b = eval_grid.score_grid(x, y, 'fp16')
    assert calls() == {'pack_images': 28, 'pack_captions': 28, 'pack_sets': 28, 'scores_from_packed': 28}     # (the stand-in pack_sets counts its two halves too)
    grid.setattr(eval_grid, 'bucket_plan', lambda *a: None)
    grid.setattr(eval_grid, '_PLAN_CACHE', {})
    cpu_standins.CALLS.clear()
    S_1 = eval_grid.score_grid(x, y, 'fp16')
    assert calls() == {'pack_images': 1, 'pack_captions': 1, 'pack_sets': 1, 'scores_from_packed': 1}
    assert_close(S_b, S_1, rtol=1e-6, atol_rel=1e-6)              # same operands: summation order only
    assert_close(S_b, ref['MrSw'], rtol=1e-3, atol_rel=3e-4)


def test_chunked_block_packs_the_max_side_once(sets, grid):
    ims, caps, il, cl, _ = sets
    il = [min(v, 40) for v in il]                                  # 40 scored positions + the masked one: 32 main rows + 8 side rows
    grid.setattr(eval_grid, 'bucket_plan', lambda *a: None)
    x, y = eval_grid.TensorSide(ims, il, 0), eval_grid.TensorSide(caps, cl, 2)
    S_1 = eval_grid.score_grid(x, y, 'fp16')
    assert calls()['pack_sets'] == 1 and calls()['scores_from_packed'] == 1
    geom = ops.align_geometry(40, 200, 41, max(cl), 32, 0, 2, 'fp16')
    assert geom.rem == 8 and geom.e_bytes > 1 << 22
    step = max(geom.cap_unit, int(200 * (1 << 22) // geom.e_bytes) // geom.cap_unit * geom.cap_unit)
    n_chunks = -(-200 // step)
    assert n_chunks > 1
    grid.setattr(eval_grid, 'E_SCRATCH_LIMIT', 1 << 22)
    cpu_standins.CALLS.clear()
    S_c = eval_grid.score_grid(x, y, 'fp16')
    assert calls() == {'pack_images': 1, 'pack_captions': n_chunks, 'pack_sets': 0, 'scores_from_packed': n_chunks}
    assert_close(S_c, S_1, rtol=1e-6, atol_rel=1e-6)              # (bit equality is the GPU tier's: CPU matmul blocking may differ)


def test_swapped_orientation_is_bucketed_too(sets, grid):
    """'MwSr': the captions on the max side (tail 2), the images on the sum side (tail 0), transposed."""
    ims, caps, il, cl, ref = sets
    x, y = eval_grid.TensorSide(caps, cl, 2), eval_grid.TensorSide(ims, il, 0)
    plan = eval_grid.bucket_plan(x.need(True), y.need(False))
    assert plan is not None and len(plan[0]) > 1 and len(plan[1]) > 1
    S = eval_grid.score_grid(x, y, 'fp16')
    n_blocks = len(plan[0]) * len(plan[1])
    assert calls()['pack_sets'] == n_blocks and calls()['scores_from_packed'] == n_blocks
    assert_close(S.t(), ref['MwSr'], rtol=1e-3, atol_rel=3e-4)


@pytest.mark.parametrize('tail', [0, 2])
def test_masked_position_rule(tail):
    total = 71
    cap = total - 1 - tail
    pos = lambda length, keep: eval_grid.positions(length - 1 - tail, cap, keep)
    assert pos(total, True) == cap and pos(total, False) == cap            # a sample that fills the set: no masked position
    assert pos(total + 5, True) == cap                                      # (a length past the set is clamped to it)
    assert pos(total - 1, True) == cap and pos(total - 1, False) == cap - 1  # one short of it: its masked position is the set's last
    assert pos(20, True) == 20 - tail and pos(20, False) == 19 - tail       # in between: the scored positions + one on the max side
    for length in (0, 1, 1 + tail):                                         # nothing scored: clamped to one position
        assert pos(length, False) == 1 and pos(length, True) == 2
    assert eval_grid.positions(0, 1, True) == 1 and eval_grid.positions(5, 0, True) == 1     # a one-position set has no room for more
