"""CPU tier: ops._bwd_flags -- which row step of the alignment backward a `packed` argument allows, under every
ops.set_backward_precision mode.  No library call and no GPU: a hand-filled geometry and CPU stand-ins for the operands."""
import pytest
import torch


@pytest.mark.parametrize('mode', ['exact', 'fp16', 'fp16-own'])
def test_bwd_flags_truth_table(mode):
    from aladin_amd import _lib, ops
    P, O = _lib.BWD_PARTNERS_FP16, _lib.BWD_OWN_ROW_FP16
    g0, g1 = _lib.AlignGeom(), _lib.AlignGeom()
    g0.split, g1.split = 0, 1
    xm, xe, y, rnorm = (torch.empty(8) for _ in range(4))
    fp16 = {'exact': 0, 'fp16': P, 'fp16-own': P | O}[mode]           # the fp16 row step: only with xm, y, rnorm and unsplit operands
    table = [
        (None, 0),
        ((g0, xm, xe, y), 0),                           # an old caller's four-tuple: no inverse norms
        ((g0, xm, xe, y, None), 0),
        ((g0, xm, xe, y, rnorm), fp16),
        ((g0, None, xe, y, rnorm), 0),
        ((g1, xm, xe, y, rnorm), 0),
    ]
    old = ops.set_backward_precision(mode)
    try:
        for packed, want in table:
            assert ops._bwd_flags(packed) == want, (mode, packed is None or len(packed), want)
    finally:
        ops.set_backward_precision(old)
