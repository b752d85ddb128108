"""CPU tier: the host side of the long-set path (csrc/align_long.hip) -- its geometry (layout ALADIN_LAYOUT_LONG), its workspace
query, the routing between it and the tile classes, and the shape check of the differentiable forward.  No kernel is launched."""
import os
import subprocess
import re

import pytest
import torch

from conftest import ROOT


@pytest.mark.parametrize('shape', [(5, 6, 98, 50, 64), (6, 5, 34, 100, 64), (4, 4, 200, 180, 96), (3, 3, 512, 512, 32),
                                   (4, 4, 130, 120, 64), (32, 32, 101, 110, 768)])
@pytest.mark.parametrize('precision', ['fp16', 'split'])
def test_long_geometry_rows_bytes_and_table(shape, precision):
    """aladin_align_geometry, ALADIN_LAYOUT_LONG: mrows = round_up(R', 32) rows per max-side sample, trows = round_up(T', 16) per sum-side
    sample, whole sum-side samples per 512-column score workgroup, no side rows; the backward workspace holds the pair list and
    a 16-bit arg-max table of round_up(T', 16) entries per pair."""
    from aladin_amd import ops, _lib
    Bi, Bc, R, T, D = shape
    g = ops.align_geometry(Bi, Bc, R, T, D, precision=precision, layout='long')
    assert g.layout == _lib.LAYOUT_LONG
    Rq, Tq = R - 1, T - 3
    up = lambda v, m: (v + m - 1) // m * m
    assert (g.Rq, g.Tq, g.x_tail, g.y_tail) == (Rq, Tq, 0, 2)
    assert g.mrows == up(Rq, 32) and g.rem == 0 and g.trows == up(Tq, 16) and g.tp16 == g.trows // 16
    assert g.cap_unit == 512 // g.trows >= 1 and g.Bc_pad == up(Bc, g.cap_unit) and g.Bi_pad == Bi
    assert g.Dp == up(D, 64) * (3 if precision == 'split' else 1) and g.split == (precision == 'split')
    assert g.xm_rows == Bi * g.mrows and g.xe_rows == 0 and g.y_rows == g.Bc_pad * g.trows
    assert g.xm_bytes == g.xm_rows * g.Dp * 2 and g.xe_bytes == 0 and g.y_bytes == g.y_rows * g.Dp * 2
    assert g.e_bytes == 0 and g.rnorm_bytes == (g.xm_rows + g.y_rows) * 4
    ws = _lib.load().aladin_align_bwd_workspace_bytes(g, 0)
    assert ws == 256 + up(Bi * Bc * 4, 256) + up(Bi * Bc * up(Tq, 16) * 2, 256)
    # the dense bits mean nothing to a long geometry: the list path, the same workspace
    for flags in (_lib.BWD_DENSE, _lib.BWD_DENSE | _lib.BWD_DENSE_GATHER):
        assert _lib.load().aladin_align_bwd_workspace_bytes(g, flags) == ws
    # the role swap ('MwSr'): captions on the max side (tail 2), images on the sum side (tail 0)
    gs = ops.align_geometry(Bc, Bi, T, R, D, 2, 0, precision, layout='long')
    assert gs.layout == _lib.LAYOUT_LONG and (gs.Rq, gs.Tq) == (Tq, Rq) and gs.mrows == up(Tq, 32) and gs.trows == up(Rq, 16)


def test_long_geometry_limits_and_the_tile_classes_keep_theirs():
    """The long layout takes up to 512 positions per set; the tile layouts still reject R' > 96 (and T' > 96); a tile-class
    geometry relabelled as long is refused (recomputation), and the tile-only triplet workspace is 0 for a long geometry."""
    from aladin_amd import ops, _lib
    for R, T in ((512, 512), (512, 5), (2, 512)):
        assert ops.align_geometry(2, 2, R, T, 8, layout='long').layout == _lib.LAYOUT_LONG
    for R, T in ((513, 50), (50, 513)):
        with pytest.raises(RuntimeError, match='512 positions'):
            ops.align_geometry(1, 1, R, T, 8, layout='long')
    for R, T in ((98, 50), (34, 100), (200, 50)):
        with pytest.raises(RuntimeError):
            ops.align_geometry(1, 1, R, T, 8)
    ops.align_geometry(1, 1, 97, 99, 8)                          # R' = T' = 96: still a tile class
    tiles = ops.align_geometry(4, 4, 34, 50, 64)
    assert tiles.layout == _lib.LAYOUT_TILES and _lib.load().aladin_align_bwd_workspace_bytes(tiles, 0) > 0
    relabelled = _lib.AlignGeom.from_buffer_copy(tiles)                                # (a copy: the geometry cache hands out the struct itself)
    relabelled.layout = _lib.LAYOUT_LONG
    assert tiles.layout == _lib.LAYOUT_TILES and _lib.load().aladin_align_bwd_workspace_bytes(relabelled, 0) == 0
    long = ops.align_geometry(4, 4, 34, 50, 64, layout='long')
    assert _lib.load().aladin_align_bwd_workspace_bytes(long, 0) > 0 and _lib.load().aladin_align_triplet_workspace_bytes(long) == 0
    assert _lib.load().aladin_align_triplet_workspace_bytes(tiles) > 0


def test_routing_between_the_tile_classes_and_the_long_kernels():
    """Shapes inside the tile classes keep their geometry; only shapes past them (either side, either role) take the long
    layout; ops.is_long, the predicate of the callers without a geometry in hand, says what layout='auto' answers;
    LONG_PATH_FORCE (tests) sends every shape there."""
    from aladin_amd import ops, _lib
    auto = lambda R, T, xt=0, yt=2: ops.align_geometry(8, 8, R, T, 64, xt, yt, layout='auto').layout
    assert not ops.is_long(97, 99) and not ops.is_long(34, 50) and not ops.is_long(99, 97, 2, 0)
    assert ops.is_long(98, 50) and ops.is_long(34, 100) and ops.is_long(100, 34, 2, 0) and ops.is_long(50, 98, 2, 0)
    for args in ((34, 50), (97, 99), (99, 97, 2, 0)):
        assert auto(*args) == _lib.LAYOUT_TILES and not ops.is_long(*args)
    for args in ((98, 50), (34, 100), (100, 34, 2, 0)):
        assert auto(*args) == _lib.LAYOUT_LONG and ops.is_long(*args)
    assert _lib.TILE_MAX_SCORED == 96 and \
        '#define ALADIN_TILE_MAX_SCORED 96' in open(os.path.join(ROOT, 'include', 'aladin_hip.h')).read()
    g = ops.align_geometry(8, 8, 34, 50, 64, 0, 2, layout='auto')
    assert g.layout == _lib.LAYOUT_TILES and g.mrows == ops.align_geometry(8, 8, 34, 50, 64).mrows
    with pytest.raises(ValueError, match='512 positions'):
        ops.align_geometry(8, 8, 513, 50, 64, 0, 2, layout='auto')
    old = ops.LONG_PATH_FORCE
    ops.LONG_PATH_FORCE = True
    try:
        assert auto(34, 50) == _lib.LAYOUT_LONG and ops.is_long(34, 50)
        assert ops.align_geometry(8, 8, 34, 50, 64).layout == _lib.LAYOUT_TILES           # 'tiles' stays tiles
    finally:
        ops.LONG_PATH_FORCE = old
    assert auto(34, 50) == _lib.LAYOUT_TILES and not ops.is_long(34, 50)


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


def test_long_sets_have_no_entry_points_of_their_own():
    """One entry point per operation: the aladin_align_long_* family is in neither include/aladin_hip.h, the ctypes table nor the
    library's exports; ABI 13; the layout field fills the hole in front of the struct's 64-bit fields (its size stays 144)."""
    import ctypes
    from aladin_amd import _lib
    names = ['aladin_align_long_geometry', 'aladin_align_long_scores', 'aladin_align_long_bwd_workspace_bytes', 'aladin_align_long_bwd']
    hdr = open(os.path.join(ROOT, 'include', 'aladin_hip.h')).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert 'aladin_align_geometry' in exported and 'aladin_align_bwd' in exported
    for n in names:
        assert n not in hdr and n not in _lib.SYMBOLS and n not in exported, n
    assert 'aladin_align_long' not in hdr and 'align_long_' not in exported
    assert _lib.ABI_VERSION == 13 and '#define ALADIN_ABI_VERSION 13' in hdr and _lib.load().aladin_version() == 13
    assert ctypes.sizeof(_lib.AlignGeom) == 144 and _lib.AlignGeom.layout.offset == 76 and _lib.AlignGeom.xm_rows.offset == 80
