"""A stand-in for the `torch` global of ONE product module that puts every `torch.empty` / `torch.empty_like` of that
module between two guard bands and hands it out poisoned (helper: no test in here).

    g = GuardedTorch(fill=FILL_NAN)
    g.install(monkeypatch, ops, fused)          # monkeypatch.setattr(module, 'torch', g) per module
    ... run the product code ...
    torch.cuda.synchronize()
    g.check_bands()                             # AssertionError naming the call site and the side that was written

An allocation is ONE uint8 buffer of GUARD + nbytes + GUARD bytes from the real torch.empty: both bands hold 0xA5, the middle
holds the run's fill byte, and the caller gets the middle as the dtype and shape it asked for (GUARD is a multiple of every
alignment the allocator gives, so the middle is aligned as the plain allocation would have been).  The base buffers stay
referenced by the records until the proxy goes away, so nothing the allocator hands out later can overlap a band.

Two fills tell a read of scratch nobody wrote from a correct run:
    FILL_NAN   0xFF   every float width reads NaN, every integer -1
    FILL_BIG   0x7E   fp32 8.5e37 (finite): a sum that takes in one stale word overflows or is visibly wrong
A result that is bit-identical under both fills (and under the plain allocator) does not depend on the scratch's prior contents.

A request the proxy cannot guard (a memory format other than contiguous, pinned memory, `out=`, a layout, ...) is passed to the
real torch and counted in `passed_through`; the GPU tests assert that count is zero."""
import os
import sys

import torch as _torch

GUARD = 32768
BAND_BYTE = 0xA5
FILL_NAN = 0xFF
FILL_BIG = 0x7E

_HERE = os.path.abspath(__file__)


class Allocation:
    """one guarded request: where it was made, what was asked for, and the buffer with its two bands"""
    __slots__ = ('site', 'dtype', 'shape', 'nbytes', 'base')

    def __init__(self, site, dtype, shape, nbytes, base):
        self.site, self.dtype, self.shape, self.nbytes, self.base = site, dtype, shape, nbytes, base

    def bands(self):
        return self.base[:GUARD], self.base[GUARD + self.nbytes:]

    def __repr__(self):
        return f'{self.site}: {self.dtype} {tuple(self.shape)}'


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return '<unknown>'
    return f'{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})'


def _shape_of(size):
    """torch.empty's size argument(s): varargs ints, one tuple / list / torch.Size, or () for a scalar"""
    if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
        size = size[0]
    return tuple(int(s) for s in size)


class GuardedTorch:
    """forwards every attribute to the real torch except `empty` and `empty_like`"""

    def __init__(self, fill, real=_torch):
        if fill not in (FILL_NAN, FILL_BIG):
            raise ValueError(f'the fill byte is FILL_NAN (0xFF) or FILL_BIG (0x7E), got {fill!r}')
        self.__dict__['_real'] = real
        self.__dict__['fill'] = fill
        self.__dict__['records'] = []
        self.__dict__['passed_through'] = []

    def __getattr__(self, name):
        return getattr(self.__dict__['_real'], name)

    def __setattr__(self, name, value):
        raise AttributeError('the guarded torch proxy is read-only')

    def install(self, monkeypatch, *modules):
        for m in modules:
            if getattr(m, 'torch', None) is not self._real:
                raise AssertionError(f'{m.__name__} has no module-global `torch` to stand in for')
            monkeypatch.setattr(m, 'torch', self)
        return self

    # ---- the two replaced functions ---------------------------------------------------------------------------------------------
    def empty(self, *size, **kw):
        site = _call_site()
        if 'size' in kw:
            if size:
                raise TypeError('empty() got the size twice')
            size = (kw.pop('size'),)
        return self._guarded(site, _shape_of(size), kw, lambda: self._real.empty(*size, **kw))

    def empty_like(self, t, **kw):
        site = _call_site()
        kw.setdefault('dtype', t.dtype)
        kw.setdefault('device', t.device)
        fmt = kw.get('memory_format', _torch.preserve_format)
        if fmt is _torch.preserve_format:
            if not t.is_contiguous() or t.layout is not _torch.strided:       # (the result would take the input's strides)
                return self._pass(site, kw, lambda: self._real.empty_like(t, **kw))
            kw['memory_format'] = _torch.contiguous_format
        return self._guarded(site, tuple(t.shape), kw, lambda: self._real.empty_like(t, **kw))

    # ---- internals --------------------------------------------------------------------------------------------------------------
    def _pass(self, site, kw, plain):
        self.passed_through.append((site, dict(kw)))
        return plain()

    def _guarded(self, site, shape, kw, plain):
        kw = dict(kw)
        dtype = kw.pop('dtype', None) or self._real.get_default_dtype()
        device = kw.pop('device', None)
        requires_grad = kw.pop('requires_grad', False)
        fmt = kw.pop('memory_format', _torch.contiguous_format)
        layout = kw.pop('layout', _torch.strided)
        pinned = kw.pop('pin_memory', False)
        if kw or pinned or fmt is not _torch.contiguous_format or layout is not _torch.strided or any(s < 0 for s in shape):
            kw.update(dtype=dtype, device=device)
            return self._pass(site, kw, plain)
        numel = 1
        for s in shape:
            numel *= s
        item = _torch.empty((), dtype=dtype).element_size()
        nbytes = numel * item
        base = self._real.empty(GUARD + nbytes + GUARD, dtype=_torch.uint8, device=device)
        base[:GUARD].fill_(BAND_BYTE)
        base[GUARD + nbytes:].fill_(BAND_BYTE)
        if nbytes:
            base[GUARD:GUARD + nbytes].fill_(self.fill)
        strides, run = [], 1
        for s in reversed(shape):
            strides.append(run)
            run *= max(s, 1)
        out = self._real.empty(0, dtype=dtype, device=base.device)
        out.set_(base.untyped_storage(), GUARD // item, shape, tuple(reversed(strides)))   # the middle, not an autograd view
        if requires_grad:
            out.requires_grad_()
        self.records.append(Allocation(site, dtype, shape, nbytes, base))
        return out

    # ---- the check --------------------------------------------------------------------------------------------------------------
    def damaged(self):
        """-> [(Allocation, 'before' | 'after', offset of the damaged byte nearest the buffer relative to its start / end, number of
        damaged bytes)]; call it after torch.cuda.synchronize()"""
        flags = [(band != BAND_BYTE).any().reshape(1) for rec in self.records for band in rec.bands()]
        by_device = {}
        for i, f in enumerate(flags):
            by_device.setdefault(f.device, []).append(i)
        hit = [False] * len(flags)
        for group in by_device.values():                                   # one transfer per device, not one per band
            for i, h in zip(group, _torch.cat([flags[i] for i in group]).cpu().tolist()):
                hit[i] = bool(h)
        out = []
        for r, rec in enumerate(self.records):
            for side, band, h in zip(('before', 'after'), rec.bands(), hit[2 * r:2 * r + 2]):
                if not h:
                    continue
                bad = (band.cpu() != BAND_BYTE).nonzero().flatten()
                first, last = int(bad[0]), int(bad[-1])
                where = (last - GUARD) if side == 'before' else first       # before: -1 is the byte just ahead of the buffer
                out.append((rec, side, where, int(bad.numel())))
        return out

    def check_bands(self):
        bad = self.damaged()
        if bad:
            lines = [f'{n} byte(s) written {side} the buffer allocated at {rec.site} ({rec.dtype}, shape {tuple(rec.shape)}, '
                     f'{rec.nbytes} bytes); nearest damaged byte at offset {where:+d} from its {"start" if side == "before" else "end"}'
                     for rec, side, where, n in bad]
            raise AssertionError('guard band damaged:\n  ' + '\n  '.join(lines))

    def by_site(self):
        """-> {call site: number of guarded allocations}"""
        out = {}
        for rec in self.records:
            out[rec.site] = out.get(rec.site, 0) + 1
        return out
