"""GPU tier (-m gpu): the argument checks of the alignment backward's entry points (csrc/align_bwd.hip, csrc/align_long.hip) and
the refusals of a long-set geometry by the tile-class entry points,
called through the C ABI with real device tensors of the smallest legal problem.  Every call here is refused before it reads
or writes device memory; the operands are valid all the same (zeroed workspaces: an all-zero arg-max table points at region 0,
an all-zero dS lists no pair), so a lost check would run its kernels inside the buffers."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 1, 2          # ALADIN_ERR_* of include/aladin_hip.h


def test_backward_entry_points_refuse_bad_arguments():
    from aladin_amd import _lib, ops
    from aladin_amd._ops_common import _stream
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    dev = torch.device('cuda:0')
    lib = _lib.load()
    B, D = 2, 8

    def problem(R, T, geom):
        im = torch.randn((B, R, D), device=dev)
        s = torch.randn((B, T, D), device=dev)
        il = torch.full((B,), R, dtype=torch.int32, device=dev)
        sl = torch.full((B,), T, dtype=torch.int32, device=dev)
        d_im, d_s = torch.zeros_like(im), torch.zeros_like(s)
        keep = (im, s, il, sl, d_im, d_s)
        return keep, (C.byref(ops._set_view(im, il)), C.byref(ops._set_view(s, sl)), C.byref(geom)), \
            (C.byref(ops._grad_view(d_im)), C.byref(ops._grad_view(d_s)))

    def zeros(nbytes):
        return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)

    dS = torch.zeros((B, B), device=dev)
    pairs = torch.zeros(B * B, dtype=torch.int32, device=dev)
    cases = []

    # the tile classes: Bi = Bc = 2, R = 4, T = 6, D = 8
    geom = ops.align_geometry(B, B, 4, 6, D)
    split = ops.align_geometry(B, B, 4, 6, D, precision='split')
    keep_t, (vi, vs, g), (gi, gs) = problem(4, 6, geom)
    ws = zeros(lib.aladin_align_bwd_workspace_bytes(C.byref(geom), 0))
    tws = zeros(lib.aladin_align_triplet_workspace_bytes(C.byref(geom)))

    def align_bwd(flags, geometry=g, pairs_ptr=None):
        return lib.aladin_align_bwd(vi, vs, geometry, None, dS.data_ptr(), B, None, pairs_ptr, None, gi, gs, ws.data_ptr(), flags,
                                    _stream())
    cases += [('align_bwd, flag bit 64', lambda: align_bwd(64), ERR_ARG, b'align_bwd'),
              ('align_bwd, pairs without pair_count', lambda: align_bwd(0, pairs_ptr=pairs.data_ptr()), ERR_ARG, b'align_bwd'),
              ('align_bwd, OWN_ROW_FP16 alone', lambda: align_bwd(_lib.BWD_OWN_ROW_FP16), ERR_ARG, b'align_bwd'),
              ('align_bwd, split-precision geometry', lambda: align_bwd(0, geometry=C.byref(split)), ERR_UNSUPPORTED, b'align_bwd'),
              ('align_triplet_bwd, ALADIN_BWD_DENSE',
               lambda: lib.aladin_align_triplet_bwd(vi, vs, g, None, dS.data_ptr(), None, gi, gs, tws.data_ptr(), _lib.BWD_DENSE, _stream()),
               ERR_ARG, b'align_triplet_bwd')]

    # long sets: R = 100 -- the same entry point on a geometry whose layout is ALADIN_LAYOUT_LONG
    lgeom = ops.align_geometry(B, B, 100, 6, D, layout='long')
    assert lgeom.layout == _lib.LAYOUT_LONG
    keep_l, (lvi, lvs, lg), (lgi, lgs) = problem(100, 6, lgeom)
    lws = zeros(lib.aladin_align_bwd_workspace_bytes(C.byref(lgeom), 0))

    def long_bwd(flags):
        return lib.aladin_align_bwd(lvi, lvs, lg, None, dS.data_ptr(), B, None, None, None, lgi, lgs, lws.data_ptr(), flags, _stream())
    cases += [('align_bwd on a long geometry, flag bit 64', lambda: long_bwd(64), ERR_ARG, b'align_bwd'),
              ('align_bwd on a long geometry, OWN_ROW_FP16 alone', lambda: long_bwd(_lib.BWD_OWN_ROW_FP16), ERR_ARG, b'align_bwd')]

    # the tile-class entry points refuse a long geometry (every other argument valid, buffers of the long geometry's sizes)
    lxm, ly, lrn = zeros(lgeom.xm_bytes), zeros(lgeom.y_bytes), zeros(lgeom.rnorm_bytes)
    lpk = _lib.Packed(lxm.data_ptr(), None, ly.data_ptr(), lrn.data_ptr())
    S, loss, dS2 = torch.zeros((B, B), device=dev), torch.zeros((), device=dev), torch.zeros((B, B), device=dev)
    assert lib.aladin_align_triplet_workspace_bytes(C.byref(lgeom)) == 0
    ltws = zeros(0)
    rows, offs = zeros(1024), torch.zeros(B, dtype=torch.int64, device=dev)
    cnts = torch.zeros(B, dtype=torch.int32, device=dev)
    cases += [('align_triplet_fwd on a long geometry',
               lambda: lib.aladin_align_triplet_fwd(lvi, lvs, lg, 0.2, C.byref(lpk), S.data_ptr(), B, loss.data_ptr(), dS2.data_ptr(),
                                                    ltws.data_ptr(), _stream()), ERR_UNSUPPORTED, b'align_triplet_fwd'),
              ('align_pack_store_x on a long geometry',
               lambda: lib.aladin_align_pack_store_x(rows.data_ptr(), offs.data_ptr(), cnts.data_ptr(), None, lg, lxm.data_ptr(), None,
                                                     _stream()), ERR_ARG, b'align_pack_store_x')]

    for what, call, code, entry in cases:
        rc = call()
        msg = lib.aladin_last_error() or b''
        assert rc == code, '%s: status %d, expected %d (%s)' % (what, rc, code, msg.decode())
        assert msg.startswith(entry + b':'), '%s: the message does not name the entry point: %r' % (what, msg)
    torch.cuda.synchronize()
    # and the same buffers are accepted without the bad argument
    assert align_bwd(0) == 0, lib.aladin_last_error()
    assert long_bwd(0) == 0, lib.aladin_last_error()
    torch.cuda.synchronize()
    assert not keep_t[4].any() and not keep_t[5].any() and not keep_l[4].any() and not keep_l[5].any()      # dS = 0: zero gradients
    assert not lxm.any() and not S.any() and not dS2.any() and not loss.any()          # the refused calls wrote nothing


def test_dense_flag_means_nothing_to_a_long_geometry():
    """aladin_align_bwd on a long geometry with ALADIN_BWD_DENSE: accepted, the list path as with flags 0 -- the same gradients
    bit for bit (B = 4, R = 100, T = 6, D = 16, a dense random dS)."""
    from aladin_amd import _lib, ops
    from aladin_amd._ops_common import _stream
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    dev = torch.device('cuda:0')
    lib = _lib.load()
    B, R, T, D = 4, 100, 6, 16
    gen = torch.Generator(device='cpu').manual_seed(11)
    im = torch.randn((B, R, D), generator=gen).to(dev)
    s = torch.randn((B, T, D), generator=gen).to(dev)
    dS = torch.randn((B, B), generator=gen).to(dev)
    il = torch.tensor([R, R - 7, 3, R], dtype=torch.int32, device=dev)
    sl = torch.tensor([T, T - 1, T, 4], dtype=torch.int32, device=dev)
    geom = ops.align_geometry(B, B, R, T, D, layout='long')
    assert geom.layout == _lib.LAYOUT_LONG
    vi, vs = ops._set_view(im, il), ops._set_view(s, sl)
    grads = []
    for flags in (0, _lib.BWD_DENSE):
        ws = torch.zeros(int(lib.aladin_align_bwd_workspace_bytes(C.byref(geom), flags)), dtype=torch.uint8, device=dev)
        d_im, d_s = torch.full_like(im, float('nan')), torch.full_like(s, float('nan'))
        gi, gs = ops._grad_view(d_im), ops._grad_view(d_s)
        rc = lib.aladin_align_bwd(C.byref(vi), C.byref(vs), C.byref(geom), None, dS.data_ptr(), B, None, None, None, C.byref(gi),
                                  C.byref(gs), ws.data_ptr(), flags, _stream())
        assert rc == 0, lib.aladin_last_error()
        torch.cuda.synchronize()
        grads.append((d_im, d_s))
    assert torch.isfinite(grads[0][0]).all() and torch.isfinite(grads[0][1]).all() and grads[0][0].abs().max() > 0
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
