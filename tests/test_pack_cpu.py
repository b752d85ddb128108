"""CPU tier: the bounds tests/test_pack_gpu.py holds the packed operands to are satisfiable.  A float32 emulation of the row encoder
(sum of squares in float32, 1 / max(sqrt, 1e-12), one rounding to fp16 -- or the hi + lo split of x^ * 2^14) stays inside them
against the float64 unit vector of tests/helpers/pack_numpy.py, in every summation order tried, for every feature width the GPU
cases use and for input families that reach the fp16 subnormals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import pack_numpy as PN

WIDTHS = (64, 66, 768, 1024, 1088)
f32 = np.float32


def _families(D, rng):
    yield 'normal', rng.standard_normal(D)
    x = rng.standard_normal(D) * 1e-7                  # unit vector: one component near 1, the rest in the fp16 subnormal range
    x[rng.integers(D)] = 1.0
    yield 'subnormal', x
    yield 'large', rng.standard_normal(D) * 3e4
    yield 'heavy', rng.standard_normal(D) ** 5


def _sumsq_orders(x):
    """float32 sums of squares: forward chain, reversed chain, numpy's pairwise sum, and 64 lane chains over float4 then a tree."""
    sq = x * x
    acc = f32(0)
    for v in sq:
        acc = f32(acc + v)
    yield acc
    acc = f32(0)
    for v in sq[::-1]:
        acc = f32(acc + v)
    yield acc
    yield sq.sum(dtype=f32)
    pad = np.zeros(-len(x) % 256, f32)
    lanes = np.concatenate([sq, pad]).reshape(-1, 64, 4)       # [k][lane][4]
    part = np.zeros(64, f32)
    for k in range(lanes.shape[0]):
        for c in range(4):
            part = (part + lanes[k, :, c]).astype(f32)
    while part.size > 1:
        part = (part[:part.size // 2] + part[part.size // 2:]).astype(f32)
    yield part[0]


def _cases():
    for D in WIDTHS:
        rng = np.random.default_rng(1000 + D)
        for name, x in _families(D, rng):
            yield D, name, x.astype(f32)


@pytest.mark.parametrize('D,name,x', [pytest.param(D, n, x, id='D%d-%s' % (D, n)) for D, n, x in _cases()])
def test_float32_encoder_stays_inside_the_bounds(D, name, x):
    u = x.astype(np.float64)
    norm = np.sqrt((u * u).sum())
    u = u / norm
    worst16 = worst_split = worst_inv = 0.0
    for ss in _sumsq_orders(x):
        inv = f32(1) / np.maximum(np.sqrt(ss, dtype=f32), f32(1e-12))
        assert inv.dtype == f32
        worst_inv = max(worst_inv, abs(float(inv) * norm - 1.0) / PN.rnorm_rel_bound(D))
        h = (x * inv).astype(f32).astype(np.float16)
        worst16 = max(worst16, float((np.abs(h.astype(np.float64) - u) / PN.fp16_bound(u, D)).max()))
        v = ((x * inv).astype(f32) * f32(PN.SPLIT_SCALE)).astype(f32)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(f32)).astype(f32).astype(np.float16)
        got = (hi.astype(np.float64) + lo.astype(np.float64)) / PN.SPLIT_SCALE
        worst_split = max(worst_split, float((np.abs(got - u) / PN.split_bound(u, D)).max()))
    print('D=%d %s: fp16 %.4f, split %.4f, rnorm %.4f of the bound' % (D, name, worst16, worst_split, worst_inv))
    assert worst16 <= 1.0 and worst_split <= 1.0 and worst_inv <= 1.0, (worst16, worst_split, worst_inv)


def test_row_maps_cover_every_row_once():
    """pack_numpy's maps on a hand-made geometry: every row of xm, xe and y is named exactly once, copies only past R'."""
    class G:
        Bi, Bc, Rq, Tq, mrows, rem, trows = 3, 2, 33, 47, 32, 1, 48
        xm_rows, xe_rows, y_rows = 8 * 32, 64, 8 * 48
    rows = PN.max_side_rows(G)
    assert sorted(r[1] for r in rows if r[0] == 'xm') == list(range(G.xm_rows))
    assert sorted(r[1] for r in rows if r[0] == 'xe') == list(range(G.xe_rows))
    assert not any(r[4] for r in rows) and {r[3] for r in rows if r[0] == 'xe'} == {32}
    G.Rq, G.rem, G.xe_rows = 19, 0, 0
    rows = PN.max_side_rows(G)
    assert sum(r[4] for r in rows) == 8 * 13 and all(r[3] == 0 for r in rows if r[4])
    assert sorted(r[0] for r in PN.sum_side_rows(G)) == list(range(G.y_rows))
    assert [PN.scored_len(n, 2, 47) for n in (0, 1, 3, 4, 50, 60)] == [0, 0, 0, 1, 47, 47]
