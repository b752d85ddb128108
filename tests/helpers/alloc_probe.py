"""Allocation interposer: are an op's outputs and workspaces independent of what their memory held before, and does the op stay
inside them?

Every result tensor and workspace of aladin_amd is torch.empty memory, so each kernel family has to write every element it
returns, zero every accumulator it adds into, read no workspace word that no earlier launch of the call wrote, and stay inside
the promised bytes.  The caching allocator hides all four: a recycled block usually holds the previous, equal answer, and its
rounding to 512 B / 2 MB swallows a small overrun.

AllocProbe is a context manager that replaces torch.empty and torch.empty_like while it is active.  A call made from a module
of the library (decided by the CALLER FRAME's module name; `is_library` is injectable) is carved out of a larger uint8 buffer,
with GUARD bytes of a canary on each side, and returned as a view of the requested dtype, shape and (for empty_like of a dense
permuted tensor) strides.  Every other call falls through to the real function.  Three modes:

  'record'  keep every intercepted allocation, in call order: after the synchronise they hold what a completed call leaves;
  'stale'   the k-th allocation starts as the final bytes of the k-th allocation of `donor` (a finished 'record' probe of the
            same op on another problem of the same shapes); a different shape, dtype or stride raises, as does an allocation
            past the donor's last.  Stale content from a real call keeps every count, offset and index that a kernel might
            wrongly read a valid one for these shapes: a latent bug shows as a wrong value, not as an access out of bounds.
            There are, on purpose, no fills of arbitrary bit patterns;
  'clean'   every allocation is zero-filled.

Leaving the `with` block (without an exception in flight) synchronises the device, checks every guard band front and back, byte
for byte -- the failure names the allocation: call site file:line, shape, dtype -- and, in 'stale' mode, requires
seeded == intercepted >= 1; in every mode it requires that no device allocation of the library was passed through.  The counts
stay readable: intercepted, seeded, passed_through_device (library call sites, e.g. under graph capture) and foreign (calls of
other modules that fell through).  An unsupported keyword (out=, pin_memory, names, a sparse layout, a memory_format other than
contiguous / preserve, requires_grad=True) raises instead of falling through.

same_bits(a, b) / assert_same_outputs(...) compare two passes' outputs bit for bit and name the probed allocation that owns a
differing output.

Out of scope: the probe is not used under graph capture (aladin_amd/graphs.py: a captured graph owns its memory pool, and a
library allocation met while a stream captures is passed through and counted, which fails the probe) nor around
aladin_amd/distributed.py (its buffers are shared with collectives and other ranks).
"""
import os
import sys

import torch

GUARD = 4096
CANARY = 0xA5

_REAL_EMPTY = torch.empty
_REAL_EMPTY_LIKE = torch.empty_like


class ProbeError(AssertionError):
    pass


def library_module(name):
    """the default `is_library`: the package itself or one of its modules"""
    return name == 'aladin_amd' or name.startswith('aladin_amd.')


class Allocation:
    """One intercepted allocation: `buf` = [front guard | data | back guard] bytes, `view` = what the caller got."""
    __slots__ = ('index', 'site', 'shape', 'dtype', 'strides', 'nbytes', 'buf', 'view')

    def __init__(self, index, site, shape, dtype, strides, nbytes, buf, view):
        self.index, self.site, self.shape, self.dtype, self.strides = index, site, shape, dtype, strides
        self.nbytes, self.buf, self.view = nbytes, buf, view

    def data(self):
        return self.buf[GUARD:GUARD + self.nbytes]

    def describe(self):
        return 'allocation #%d at %s, shape %s, dtype %s' % (self.index, self.site, tuple(self.shape), self.dtype)

    def owns(self, t):
        lo = self.buf.data_ptr() + GUARD
        return t.device == self.buf.device and lo <= t.data_ptr() < lo + max(self.nbytes, 1)


def _site(frame):
    return '%s:%d' % (os.path.relpath(frame.f_code.co_filename) if os.path.isabs(frame.f_code.co_filename)
                      else frame.f_code.co_filename, frame.f_lineno)


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    shape = tuple(int(v) for v in size)
    if any(v < 0 for v in shape):
        raise ProbeError('alloc_probe: negative dimension in %r' % (shape,))
    return shape


def _contiguous_strides(shape):
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= max(n, 1)
    return tuple(reversed(st))


class AllocProbe:
    def __init__(self, mode, donor=None, is_library=library_module):
        if mode not in ('record', 'stale', 'clean'):
            raise ValueError("alloc_probe: mode must be 'record', 'stale' or 'clean'")
        if (mode == 'stale') != (donor is not None):
            raise ValueError("alloc_probe: 'stale' takes the finished 'record' probe as donor, the other modes take none")
        if donor is not None and (donor.mode != 'record' or not donor.finished):
            raise ValueError("alloc_probe: the donor must be a finished 'record' probe")
        self.mode, self.donor, self.is_library = mode, donor, is_library
        self.allocations = []
        self.intercepted = self.seeded = self.passed_through_device = self.foreign = 0
        self.finished = False
        self._saved = None

    # -------------------------------------------------------------------------------------------- patching
    def __enter__(self):
        if self._saved is not None or self.finished:
            raise RuntimeError('alloc_probe: a probe is used once')
        if torch.empty is not _REAL_EMPTY or torch.empty_like is not _REAL_EMPTY_LIKE:
            raise RuntimeError('alloc_probe: probes do not nest')
        self._saved = (torch.empty, torch.empty_like)
        probe = self

        def empty(*size, **kw):
            return probe._empty(sys._getframe(1), size, kw)

        def empty_like(t, **kw):
            return probe._empty_like(sys._getframe(1), t, kw)

        torch.empty, torch.empty_like = empty, empty_like
        return self

    def __exit__(self, exc_type, exc, tb):
        torch.empty, torch.empty_like = self._saved
        self._saved = None
        self.finished = True
        if exc_type is None:
            self.verify()
        return False

    # -------------------------------------------------------------------------------------------- the two replacements
    def _from_library(self, frame):
        return bool(self.is_library(frame.f_globals.get('__name__', '')))

    @staticmethod
    def _check_keywords(kw, site, like):
        allowed = {'dtype', 'device', 'requires_grad', 'layout', 'pin_memory', 'memory_format'}
        bad = sorted(set(kw) - allowed)
        if bad:
            raise ProbeError('alloc_probe: unsupported keyword(s) %s at %s' % (', '.join(bad), site))
        if kw.get('pin_memory'):
            raise ProbeError('alloc_probe: pin_memory=True is not supported (%s)' % site)
        if kw.get('requires_grad'):
            raise ProbeError('alloc_probe: requires_grad=True is not supported (%s)' % site)
        if kw.get('layout', torch.strided) is not torch.strided:
            raise ProbeError('alloc_probe: only strided layouts are supported (%s)' % site)
        fmt = kw.get('memory_format', torch.preserve_format if like else torch.contiguous_format)
        if fmt not in ((torch.contiguous_format, torch.preserve_format) if like else (torch.contiguous_format,)):
            raise ProbeError('alloc_probe: unsupported memory_format %s at %s' % (fmt, site))
        return fmt

    def _empty(self, frame, size, kw):
        if not self._from_library(frame):
            self.foreign += 1
            return _REAL_EMPTY(*size, **kw)
        site = _site(frame)
        self._check_keywords(kw, site, like=False)
        shape = _shape_of(size)
        dtype = kw.get('dtype') or torch.get_default_dtype()
        device = torch.device(kw['device']) if kw.get('device') is not None else _REAL_EMPTY(0).device
        return self._carve(site, shape, dtype, _contiguous_strides(shape), device)

    def _empty_like(self, frame, t, kw):
        if not self._from_library(frame):
            self.foreign += 1
            return _REAL_EMPTY_LIKE(t, **kw)
        site = _site(frame)
        fmt = self._check_keywords(kw, site, like=True)
        shape = tuple(t.shape)
        dtype = kw.get('dtype') or t.dtype
        device = torch.device(kw['device']) if kw.get('device') is not None else t.device
        strides = _contiguous_strides(shape)
        if fmt is torch.preserve_format and not t.is_contiguous():
            if not torch.ops.aten.is_non_overlapping_and_dense(t):
                raise ProbeError('alloc_probe: empty_like of a tensor that is neither contiguous nor dense (strides %s) at %s'
                                 % (tuple(t.stride()), site))
            strides = tuple(t.stride())          # what preserve_format gives a dense permutation
        return self._carve(site, shape, dtype, strides, device)

    def _carve(self, site, shape, dtype, strides, device):
        if device.type != 'cpu' and torch.cuda.is_current_stream_capturing():
            self.passed_through_device += 1      # out of scope (see the docstring); verify() reports it
            return _REAL_EMPTY(shape, dtype=dtype, device=device).as_strided(shape, strides)
        k = len(self.allocations)
        numel = 1
        for n in shape:
            numel *= n
        nbytes = numel * _REAL_EMPTY((), dtype=dtype).element_size()
        buf = _REAL_EMPTY(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
        buf[:GUARD].fill_(CANARY)
        buf[GUARD + nbytes:].fill_(CANARY)
        data = buf[GUARD:GUARD + nbytes]
        alloc = Allocation(k, site, shape, dtype, strides, nbytes, buf, None)
        if self.mode == 'clean':
            data.zero_()
        elif self.mode == 'stale':
            if k >= len(self.donor.allocations):
                raise ProbeError('alloc_probe: %s has no counterpart in the donor pass (%d allocations there)'
                                 % (alloc.describe(), len(self.donor.allocations)))
            d = self.donor.allocations[k]
            if (d.shape, d.dtype, d.strides) != (shape, dtype, strides) or d.buf.device != buf.device:
                raise ProbeError('alloc_probe: the allocation sequence changed: %s, but the donor pass made %s'
                                 % (alloc.describe(), d.describe()))
            data.copy_(d.data())
            self.seeded += 1
        view = data.view(dtype) if nbytes else _REAL_EMPTY(0, dtype=dtype, device=device)
        alloc.view = view.as_strided(shape, strides) if nbytes else view.reshape(shape)
        self.allocations.append(alloc)
        self.intercepted += 1
        return alloc.view

    # -------------------------------------------------------------------------------------------- after the op
    def verify(self):
        """Synchronise, then check every guard band and the counts; raises ProbeError naming what failed."""
        if any(a.buf.is_cuda for a in self.allocations):
            torch.cuda.synchronize()
        for a in self.allocations:
            for name, band in (('front', a.buf[:GUARD]), ('back', a.buf[GUARD + a.nbytes:])):
                hit = (band != CANARY).nonzero()
                if hit.numel():
                    reach = '%d byte(s) before its start' % (GUARD - int(hit.min())) if name == 'front' \
                        else '%d byte(s) past its end' % (int(hit.max()) + 1)
                    raise ProbeError('alloc_probe: %s guard band overwritten (%d bytes changed, reaching %s) of %s'
                                     % (name, hit.numel(), reach, a.describe()))
        if self.passed_through_device:
            raise ProbeError('alloc_probe: %d device allocation(s) of the library were not intercepted' % self.passed_through_device)
        if self.mode == 'stale':
            if self.seeded != self.intercepted or self.intercepted < 1:
                raise ProbeError('alloc_probe: %d allocations intercepted, %d seeded' % (self.intercepted, self.seeded))
            if self.intercepted != len(self.donor.allocations):
                raise ProbeError('alloc_probe: the donor pass made %d allocations, this pass %d'
                                 % (len(self.donor.allocations), self.intercepted))

    def owner_of(self, t):
        """the intercepted allocation a tensor's memory lies in, or None (a tensor derived by an ordinary torch op)"""
        for a in self.allocations:
            if a.owns(t):
                return a
        return None


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        t = t.view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)
    return t


def same_bits(a, b):
    """bit-identical?  (float comparison would call NaN != NaN and -0.0 == 0.0)"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def assert_same_outputs(stale, stale_out, clean, clean_out, names=None):
    """The outputs of the 'stale' and the 'clean' pass, output by output, bit for bit; a difference names the output, how many
    elements differ, and the allocation (of the stale pass) that owns it."""
    if len(stale_out) != len(clean_out):
        raise ProbeError('alloc_probe: %d outputs after the stale pass, %d after the clean one' % (len(stale_out), len(clean_out)))
    for i, (a, b) in enumerate(zip(stale_out, clean_out)):
        if (a is None) != (b is None):
            raise ProbeError('alloc_probe: output %d is None in one pass only' % i)
        if a is None or same_bits(a, b):
            continue
        label = names[i] if names else 'output %d' % i
        own = stale.owner_of(a)
        n = int((_bits(a) != _bits(b)).sum()) if a.shape == b.shape and a.dtype == b.dtype else -1
        raise ProbeError('alloc_probe: %s depends on what its memory held before the call: %d differing byte(s)/element(s) between '
                         'the stale and the clean pass; %s' % (label, n, own.describe() if own is not None
                                                               else 'derived from probed allocations by a torch op'))


def run_three_passes(call, donor_inputs, probe_inputs, is_library=library_module, before_pass=None):
    """record on the donor problem, stale and clean on the probed one -> (probes, stale outputs, clean outputs); each pass's
    guards and counts are verified on the way.  before_pass(): resets state that steers the allocation sequence."""
    probes, outs = [], []
    for mode, inputs in (('record', donor_inputs), ('stale', probe_inputs), ('clean', probe_inputs)):
        if before_pass is not None:
            before_pass()
        with AllocProbe(mode, donor=probes[0] if mode == 'stale' else None, is_library=is_library) as p:
            out = call(inputs)
        probes.append(p)
        outs.append(tuple(out))
    return probes, outs[1], outs[2]
