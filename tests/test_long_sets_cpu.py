"""CPU tier: the host side of the long-set path (csrc/align_long.hip) -- its geometry query, its workspace query, the routing
between it and the tile classes, and the shape check of the differentiable forward.  No kernel is launched."""
import os
import re

import pytest
import torch

from conftest import ROOT


@pytest.mark.parametrize('shape', [(5, 6, 98, 50, 64), (6, 5, 34, 100, 64), (4, 4, 200, 180, 96), (3, 3, 512, 512, 32),
                                   (4, 4, 130, 120, 64), (32, 32, 101, 110, 768)])
@pytest.mark.parametrize('precision', ['fp16', 'split'])
def test_long_geometry_rows_bytes_and_table(shape, precision):
    """aladin_align_long_geometry: mrows = round_up(R', 32) rows per max-side sample, trows = round_up(T', 16) per sum-side
    sample, whole sum-side samples per 512-column score workgroup, no side rows; the backward workspace holds the pair list and
    a 16-bit arg-max table of round_up(T', 16) entries per pair."""
    from aladin_amd import ops, _lib
    Bi, Bc, R, T, D = shape
    g = ops.long_geometry(Bi, Bc, R, T, D, precision=precision)
    assert isinstance(g, ops.LongGeom)
    Rq, Tq = R - 1, T - 3
    up = lambda v, m: (v + m - 1) // m * m
    assert (g.Rq, g.Tq, g.x_tail, g.y_tail) == (Rq, Tq, 0, 2)
    assert g.mrows == up(Rq, 32) and g.rem == 0 and g.trows == up(Tq, 16) and g.tp16 == g.trows // 16
    assert g.cap_unit == 512 // g.trows >= 1 and g.Bc_pad == up(Bc, g.cap_unit) and g.Bi_pad == Bi
    assert g.Dp == up(D, 64) * (3 if precision == 'split' else 1) and g.split == (precision == 'split')
    assert g.xm_rows == Bi * g.mrows and g.xe_rows == 0 and g.y_rows == g.Bc_pad * g.trows
    assert g.xm_bytes == g.xm_rows * g.Dp * 2 and g.xe_bytes == 0 and g.y_bytes == g.y_rows * g.Dp * 2
    assert g.e_bytes == 0 and g.rnorm_bytes == (g.xm_rows + g.y_rows) * 4
    ws = _lib.load().aladin_align_long_bwd_workspace_bytes(g)
    assert ws == 256 + up(Bi * Bc * 4, 256) + up(Bi * Bc * up(Tq, 16) * 2, 256)
    # the role swap ('MwSr'): captions on the max side (tail 2), images on the sum side (tail 0)
    gs = ops.long_geometry(Bc, Bi, T, R, D, 2, 0, precision)
    assert (gs.Rq, gs.Tq) == (Tq, Rq) and gs.mrows == up(Tq, 32) and gs.trows == up(Rq, 16)


def test_long_geometry_limits_and_the_tile_classes_keep_theirs():
    """The long layout takes up to 512 positions per set; aladin_align_geometry still rejects R' > 96 (and T' > 96); the long
    entry points refuse a tile-class geometry."""
    from aladin_amd import ops, _lib
    for R, T in ((512, 512), (512, 5), (2, 512)):
        ops.long_geometry(2, 2, R, T, 8)
    for R, T in ((513, 50), (50, 513)):
        with pytest.raises(RuntimeError, match='512 positions'):
            ops.long_geometry(1, 1, R, T, 8)
    for R, T in ((98, 50), (34, 100), (200, 50)):
        with pytest.raises(RuntimeError):
            ops.align_geometry(1, 1, R, T, 8)
    ops.align_geometry(1, 1, 97, 99, 8)                          # R' = T' = 96: still a tile class
    assert _lib.load().aladin_align_long_bwd_workspace_bytes(ops.align_geometry(4, 4, 34, 50, 64)) == 0


def test_routing_between_the_tile_classes_and_the_long_kernels():
    """Shapes inside the tile classes keep their geometry; only shapes past them (either side, either role) take the long
    layout; LONG_PATH_FORCE (tests) sends every shape there."""
    from aladin_amd import ops
    assert not ops.is_long(97, 99) and not ops.is_long(34, 50) and not ops.is_long(99, 97, 2, 0)
    assert ops.is_long(98, 50) and ops.is_long(34, 100) and ops.is_long(100, 34, 2, 0) and ops.is_long(50, 98, 2, 0)
    g = ops._scoring_geometry(8, 8, 34, 50, 64, 0, 2)
    assert not isinstance(g, ops.LongGeom) and g.mrows == ops.align_geometry(8, 8, 34, 50, 64).mrows
    assert isinstance(ops._scoring_geometry(8, 8, 98, 50, 64, 0, 2), ops.LongGeom)
    with pytest.raises(ValueError, match='512 positions'):
        ops._scoring_geometry(8, 8, 513, 50, 64, 0, 2)
    old = ops.LONG_PATH_FORCE
    ops.LONG_PATH_FORCE = True
    try:
        assert isinstance(ops._scoring_geometry(8, 8, 34, 50, 64, 0, 2), ops.LongGeom)
    finally:
        ops.LONG_PATH_FORCE = old


def test_backward_shape_check_moves_to_512_positions():
    """_check_backward_supported: sets up to 512 positions pass, 513 on either side raises ValueError; D > 1024 keeps its error."""
    from aladin_amd import ops
    for R, T in ((98, 50), (34, 100), (512, 512)):
        ops._check_backward_supported(torch.empty(2, R, 64), torch.empty(2, T, 64), 0, 2)
    for R, T in ((513, 50), (50, 513)):
        with pytest.raises(ValueError, match='512 positions'):
            ops._check_backward_supported(torch.empty(2, R, 64), torch.empty(2, T, 64), 0, 2)
    with pytest.raises(ValueError, match='D <= 1024'):
        ops._check_backward_supported(torch.empty(2, 200, 1028), torch.empty(2, 50, 1028), 0, 2)


def test_long_entry_points_are_declared_bound_and_exported():
    """The four long-set entry points: in include/aladin_hip.h, in the ctypes table, exported by the library, ABI 12."""
    from aladin_amd import _lib
    names = ['aladin_align_long_geometry', 'aladin_align_long_scores', 'aladin_align_long_bwd_workspace_bytes', 'aladin_align_long_bwd']
    hdr = open(os.path.join(ROOT, 'include', 'aladin_hip.h')).read()
    for n in names:
        assert re.search(r'ALADIN_API\s+[\w\s\*]+\b%s\s*\(' % n, hdr), n
        assert n in _lib.SYMBOLS
        assert getattr(_lib.load(), n) is not None
    assert _lib.ABI_VERSION == 12 and '#define ALADIN_ABI_VERSION 12' in hdr and _lib.load().aladin_version() == 12
