"""GPU tier: the packed operand format (csrc/pack_rows.hpp) at the smallest shapes at which each of its branches can go wrong,
against the float64 restatement of tests/helpers/pack_numpy.py, and the ways of producing it against each other, bit for bit:
both sets in one launch, images alone + captions alone, and an evaluation store filled by aladin_store_append and packed through
aladin_align_pack_store_x / _y (tile classes only; with and without a shuffled ids).

Every case has Bi = 3 images and Bc = 2 captions with lengths 0, 1 (nothing scored either way), the maximum, more than the
maximum (clamped) and one partly masked set -- on the image side in the cases at even positions, on the caption side in the others.
The bounds (pack_numpy.fp16_bound / split_bound / rnorm_rel_bound) are the ones tests/test_pack_cpu.py shows to be satisfiable."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import pack_numpy as PN

pytestmark = pytest.mark.gpu

BI, BC = 3, 2
TILES, LONG = 0, 2
# name: (R, T, D), (mrows, rem, trows, tp16, img_unit, layout)
CASES = {
    'a': ((34, 50, 64), (32, 1, 48, 3, 8, TILES)),         # 32 main rows + 1 side row, 48-word captions, image unit 8
    'b': ((51, 38, 768), (48, 2, 40, 3, 4, TILES)),        # 48 + 2, the 40-word half class
    'c': ((20, 11, 64), (32, 0, 8, 1, 8, TILES)),          # 32 rows with 13 tile-filling copies, the 8-word class
    'd': ((42, 27, 128), (48, 0, 24, 2, 4, TILES)),        # 48 rows with copies, no side rows, the 24-word class
    'e': ((41, 50, 64), (32, 8, 48, 3, 8, TILES)),         # 8 side rows
    'f': ((66, 50, 64), (64, 1, 48, 3, 4, TILES)),         # 64 + 1
    'g': ((71, 71, 64), (96, 0, 96, 6, 4, TILES)),         # the 96-row class, tp16 5 -> 6
    'h': ((34, 50, 66), (32, 1, 48, 3, 8, TILES)),         # D % 4 != 0: scalar path, padded columns
    'i': ((34, 50, 1088), (32, 1, 48, 3, 8, TILES)),       # D > 1024: the streamed float4 path
    'j': ((100, 20, 64), (128, 0, 32, 2, 1, LONG)),        # long layout, max side
    'k': ((34, 100, 64), (64, 0, 112, 7, 1, LONG)),        # long layout, sum side
}
RUNS = [(n, 'fp16', False) for n in CASES] + [(n, 'split', False) for n in 'abi'] + [(n, 'fp16', True) for n in 'ab']
IDS = ['%s-%s%s' % (n, p, '-views' if v else '') for n, p, v in RUNS]


def _inputs(name):
    (R, T, D), _ = CASES[name]
    rng = np.random.default_rng(4200 + ord(name))
    im = rng.standard_normal((BI, R, D)).astype(np.float32)
    s = (rng.standard_normal((BC, T, D)) * 3.0).astype(np.float32)
    if sorted(CASES).index(name) % 2 == 0:
        il, sl = [R - 5, 0, R + 3], [T, 1]
    else:
        il, sl = [R, 1, R + 3], [0, T - 4]
    return im, s, il, sl


def _dev(x, views):
    dev = torch.device('cuda:0')
    if not views:
        return torch.from_numpy(x).to(dev)
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(dev).permute(1, 0, 2)       # (S, B, D) -> (B, S, D)
    assert not t.is_contiguous() and t.stride(2) == 1
    return t


def _bits(t, rows, width):
    return t[:rows * width].cpu().numpy().reshape(rows, width).view(np.uint16)


_CACHE = {}


def _run(name, prec, views):
    """One case, packed every way once: the geometry, the inputs, and {way: (xm, xe, y, rnorm or None)} as bit arrays."""
    key = (name, prec, views)
    if key in _CACHE:
        return _CACHE[key]
    from aladin_amd import eval_grid, ops
    from aladin_amd.store import PackedSetStore
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    (R, T, D), expect = CASES[name]
    g = ops.align_geometry(BI, BC, R, T, D, precision=prec, layout='auto')
    assert (g.mrows, g.rem, g.trows, g.tp16, g.img_unit, g.layout) == expect, (g.mrows, g.rem, g.trows, g.tp16, g.img_unit, g.layout)
    assert g.Dp == (3 if prec == 'split' else 1) * ((D + 63) // 64) * 64
    im, s, il, sl = _inputs(name)
    a, b = _dev(im, views), _dev(s, views)
    ilt, slt = ops.lengths_tensor(il, a.device), ops.lengths_tensor(sl, a.device)
    n_m, n_e, n_y = int(g.xm_rows), int(g.xe_rows), int(g.y_rows)

    def bits(xm, xe, y, rn):
        return (_bits(xm, n_m, g.Dp), _bits(xe, n_e, g.Dp), _bits(y, n_y, g.Dp),
                None if rn is None else rn.cpu().numpy().view(np.uint32)[:n_m + n_e + n_y])

    ways = {}
    pk = ops.pack_sets(a, b, ilt, slt, g)
    ways['joint'] = bits(pk.xm, pk.xe, pk.y, pk.rnorm)
    rn = None if prec == 'split' else torch.full((g.rnorm_bytes // 4,), float('nan'), device=a.device)
    xm, xe = ops.pack_images(a, ilt, g, rnorm=rn)
    y = ops.pack_captions(b, slt, g, rnorm=rn)
    ways['single'] = bits(xm, xe, y, rn)
    if g.layout == TILES:
        for tag, order_i, order_c in (('store', [0, 1, 2], [0, 1]), ('store-ids', [2, 0, 1], [1, 0])):
            si, sc = PackedSetStore(D, 0, a.device, precision=prec), PackedSetStore(D, 2, a.device, precision=prec)
            for k in order_i:
                si.append(a[k:k + 1], il[k:k + 1])
            for k in order_c:
                sc.append(b[k:k + 1], sl[k:k + 1])
            vi = si if tag == 'store' else si.view([order_i.index(k) for k in range(BI)])
            vc = sc if tag == 'store' else sc.view([order_c.index(k) for k in range(BC)])
            xm, xe = eval_grid.StoreSide(vi).pack_max(g)
            y = eval_grid.StoreSide(vc).pack_sum(g, 0, BC)
            ways[tag] = bits(xm, xe, y, None)
    torch.cuda.synchronize()
    _CACHE[key] = dict(g=g, im=im, s=s, il=il, sl=sl, ways=ways, expect=PN.expected(g, im, s, il, sl))
    return _CACHE[key]


def _f64(bits):
    return bits.view(np.float16).astype(np.float64)


@pytest.mark.parametrize('name,prec,views', RUNS, ids=IDS)
def test_structure_and_values(name, prec, views):
    r = _run(name, prec, views)
    g, D = r['g'], r['g'].D
    Dp0 = g.Dp // 3 if prec == 'split' else g.Dp
    xm, xe, y, rn = r['ways']['joint']
    offs = {'xm': 0, 'xe': int(g.xm_rows), 'y': int(g.xm_rows + g.xe_rows)}
    kinds_seen = set()
    for op, got in (('xm', xm), ('xe', xe), ('y', y)):
        unit, kind, inv = r['expect'][op]
        kinds_seen |= set(kind.tolist())
        # exact structure
        assert not got[kind == PN.ZERO].any(), '%s: a masked or padding-sample row is not all-zero bits' % op
        for seg in range(g.Dp // Dp0):
            assert not got[:, seg * Dp0 + D:(seg + 1) * Dp0].any(), '%s: padding columns of segment %d' % (op, seg)
        for row in np.nonzero(kind == PN.COPY)[0]:
            first = row - row % g.mrows
            assert kind[first] == PN.SCORED and np.array_equal(got[row], got[first]), '%s: tile-filling row %d' % (op, row)
        segs = [got[:, k * Dp0:k * Dp0 + D] for k in range(g.Dp // Dp0)]
        if prec == 'split':
            hi, hi2, lo = (segs[0], segs[2], segs[1]) if op != 'y' else (segs[0], segs[1], segs[2])      # [hi | lo | hi] / [hi | hi | lo]
            assert np.array_equal(hi, hi2), '%s: the two hi segments differ' % op
            val, bound = (_f64(hi) + _f64(lo)) / PN.SPLIT_SCALE, PN.split_bound(unit, D)
        else:
            val, bound = _f64(segs[0]), PN.fp16_bound(unit, D)
        # values: every element of every row (zero rows against 0)
        assert val.shape == unit.shape == (got.shape[0], D)
        ratio = np.abs(val - unit) / bound
        print('%s %s: worst |value - unit| = %.4f of the bound' % (IDS[RUNS.index((name, prec, views))], op, ratio.max() if ratio.size else 0.0))
        assert np.isfinite(val).all() and (ratio <= 1.0).all(), (op, float(ratio.max()))
        if rn is not None:
            slot = rn[offs[op]:offs[op] + got.shape[0]]
            assert not slot[kind == PN.ZERO].any(), '%s: rnorm of a zero row' % op
            live = kind != PN.ZERO
            rel = np.abs(slot.view(np.float32)[live].astype(np.float64) / inv[live] - 1.0)
            assert (rel <= PN.rnorm_rel_bound(D)).all(), (op, float(rel.max()))
    assert PN.ZERO in kinds_seen and PN.SCORED in kinds_seen
    if g.Rq < g.mrows:
        assert PN.COPY in kinds_seen


@pytest.mark.parametrize('name,prec,views', RUNS, ids=IDS)
def test_ways_of_packing_agree_bit_for_bit(name, prec, views):
    r = _run(name, prec, views)
    ref = r['ways']['joint']
    assert set(r['ways']) == ({'joint', 'single', 'store', 'store-ids'} if r['g'].layout == TILES else {'joint', 'single'})
    for way, got in r['ways'].items():
        for op, x, z in zip(('xm', 'xe', 'y'), ref, got):
            assert np.array_equal(x, z), '%s of %s differs from the joint launch' % (op, way)
        if got[3] is not None:
            assert np.array_equal(ref[3], got[3]), 'rnorm of %s differs from the joint launch' % way
    assert (ref[3] is None) == (prec == 'split')


def test_views_pack_the_bits_of_their_contiguous_copies():
    for name in 'ab':
        for x, z in zip(_run(name, 'fp16', False)['ways']['joint'], _run(name, 'fp16', True)['ways']['joint']):
            assert np.array_equal(x, z)


def test_pack_sets_on_a_non_unit_inner_stride():
    """(B, T, D) views of contiguous (B, D, T) tensors: pack_sets packs what it packs from their contiguous copies."""
    from aladin_amd import ops
    B, R, T, D = 2, 34, 50, 64
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(77)
    a = torch.from_numpy(rng.standard_normal((B, D, R)).astype(np.float32)).to(dev).transpose(1, 2)
    b = torch.from_numpy(rng.standard_normal((B, D, T)).astype(np.float32)).to(dev).transpose(1, 2)
    assert a.shape == (B, R, D) and a.stride(2) != 1 and b.stride(2) != 1
    g = ops.align_geometry(B, B, R, T, D)
    ilt, slt = ops.lengths_tensor([R, R - 9], dev), ops.lengths_tensor([T - 11, T], dev)
    got = ops.pack_sets(a, b, ilt, slt, g)
    ref = ops.pack_sets(a.contiguous(), b.contiguous(), ilt, slt, g)
    for name in ('xm', 'xe', 'y'):
        n = getattr(g, name + '_bytes') // 2
        assert torch.equal(getattr(got, name)[:n].view(torch.int16), getattr(ref, name)[:n].view(torch.int16)), name
    assert torch.equal(got.rnorm.view(torch.int32), ref.rnorm.view(torch.int32))
    assert bool((ref.xm.view(torch.int16) != 0).any())
