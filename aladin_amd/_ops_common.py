"""Helpers shared by the ops modules: device checks, raw pointers, the current stream, length tensors, workspaces, the set
structs and entry checks of the functions that take image / caption sets.
Every tensor function of this package requires float32 tensors on an AMD GPU ("cuda" device of PyTorch-ROCm) and raises
otherwise; there is no CPU or eager-PyTorch fallback."""
import ctypes as C

import torch

from . import _lib

_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """hipStream_t of PyTorch's current stream (reference kernels run there too).  The raw getter is
    ~10x cheaper than torch.cuda.current_stream(), which matters for the small-batch, launch-bound step."""
    if _RAW_STREAM is not None:
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _require_tensors(*tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError('aladin_amd: expected a torch.Tensor, got %r' % type(t))


def _require_gpu(*tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError('aladin_amd: expected a torch.Tensor, got %r' % type(t))
        if not t.is_cuda:
            raise RuntimeError('aladin_amd: the alignment/matching path runs in HIP kernels on an MI355X only; '
                               'got a %s tensor (no CPU fallback exists)' % t.device)
        if t.dtype != torch.float32:
            raise TypeError('aladin_amd: float32 expected, got %s' % t.dtype)
        if t.device.index is not None and t.device.index != torch.cuda.current_device():
            # kernels are enqueued on the CURRENT device's current stream (one process per GPU)
            raise RuntimeError('aladin_amd: tensor on %s but the current device is cuda:%d; call torch.cuda.set_device() '
                               '(or use `with torch.cuda.device(...)`) first' % (t.device, torch.cuda.current_device()))


def _rows_inner_contig(t):
    """Keep permuted (S,B,D)->(B,S,D) views (reference alad/alad_model.py:377-378) without a copy
    as long as the feature axis is contiguous and rows stay 16-byte aligned."""
    if t.stride(-1) != 1 or any(st % 4 for st in t.stride()[:-1]) or t.data_ptr() % 16:
        return t.contiguous()
    return t


_LEN_CACHE = {}


def lengths_tensor(lens, device):
    """Python list / tensor of lengths -> int32 device tensor (the reference passes lists).
    Lists are cached by value so that a repeated batch shape costs no host->device copy."""
    if isinstance(lens, torch.Tensor):
        return lens.to(device=device, dtype=torch.int32, non_blocking=True)
    key = (tuple(lens), device)
    t = _LEN_CACHE.get(key)
    if t is None:
        if len(_LEN_CACHE) >= 256:
            _LEN_CACHE.clear()
        t = torch.tensor([int(x) for x in key[0]], dtype=torch.int32).to(device, non_blocking=True)
        _LEN_CACHE[key] = t
    return t


def _ld(t):
    """Leading dimension of a 2-D tensor whose rows are contiguous (stride(0) is arbitrary when there is one row)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _unit_cols(x):
    """A 2-D tensor as the kernels read it through _ld: unit column stride and, with more than one row, rows that do not overlap
    (an expanded row has row stride 0); anything else is copied."""
    return x if x.stride(1) == 1 and (x.shape[0] == 1 or x.stride(0) >= x.shape[1]) else x.contiguous()


def _require_square(scores, what, hint=''):
    if scores.dim() != 2 or scores.shape[0] != scores.shape[1] or scores.shape[0] < 1:
        raise ValueError('aladin_amd: %s needs a square score matrix, got %s%s' % (what, tuple(scores.shape), hint))


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _upstream(g):
    """The upstream gradient of a scalar loss as the kernels read it through a pointer: one float32 on the device."""
    return g.to(torch.float32).contiguous()


def _set_view(t, len_t):
    """struct aladin_set of a (B, N, D) tensor with a unit inner stride."""
    return _lib.SetView(t.data_ptr(), t.stride(0), t.stride(1), len_t.data_ptr())


def _grad_view(t):
    return _lib.GradView(t.data_ptr(), t.stride(0), t.stride(1))


def _check_set_shapes(im_set, s_seq, im_len, s_len):
    _require_gpu(im_set, s_seq)
    if im_set.dim() != 3 or s_seq.dim() != 3:
        raise ValueError('aladin_amd: im_set (B,R,D) and s_seq (B,T,D) expected')
    if len(im_len) != im_set.shape[0] or len(s_len) != s_seq.shape[0]:
        raise ValueError('aladin_amd: one length per sample expected')
    if im_set.shape[2] != s_seq.shape[2]:
        raise ValueError('aladin_amd: feature sizes differ (%d vs %d)' % (im_set.shape[2], s_seq.shape[2]))


def _check_sets(im_set, s_seq, im_len, s_len):
    """_check_set_shapes -> the lengths as device tensors (im_len_t, s_len_t)"""
    _check_set_shapes(im_set, s_seq, im_len, s_len)
    return lengths_tensor(im_len, im_set.device), lengths_tensor(s_len, im_set.device)


def _pad_features(im_set, s_seq):
    """The backward kernels move rows as 16-byte float4 columns (D % 4 == 0).  The reference has no such limit: a set whose
    feature size is not a multiple of 4 is padded with zero features here, OUTSIDE the autograd nodes -- zeros change neither
    a norm nor a dot product, and autograd's own backward of the padding drops the extra gradient columns.  One copy of each set,
    paid by odd feature sizes only (every shipped configuration has D = 768)."""
    D = im_set.shape[-1]
    if D % 4 == 0 or im_set.dim() != 3 or s_seq.dim() != 3 or s_seq.shape[-1] != D:
        return im_set, s_seq
    pad = 4 - D % 4
    return torch.nn.functional.pad(im_set, (0, pad)), torch.nn.functional.pad(s_seq, (0, pad))


def _sets_for_node(im_set, s_seq):
    """The sets as a fused loss node takes them: padded (_pad_features) when a gradient can be asked for, detached under
    torch.no_grad() -- a Function's ctx.needs_input_grad follows requires_grad even there: without this the node would prepare
    (and, for a feature size that is no multiple of 4, refuse) a backward nobody can ask for."""
    if not torch.is_grad_enabled():
        return im_set.detach(), s_seq.detach()
    if im_set.requires_grad or s_seq.requires_grad:
        return _pad_features(im_set, s_seq)
    return im_set, s_seq
