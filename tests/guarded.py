"""Guarded operands for the launch tests: every tensor a launch reads or writes is a view into a larger allocation whose
margins ("pads") hold a known pattern, and ``Guard.check()`` -- called after the stream is synchronised -- fails, naming the buffer
and the first offending offset, when

* a pad, of an input or an output, is no longer bit-identical to its fill (a write in front of a buffer or past its end);
* the payload of an input changed (a launch scribbled on an operand), unless it was registered as in-out;
* the payload of an output that the operator must write everywhere is not finite: it still holds its NaN fill, or a +inf pad of an
  input entered it.

Reads outside a buffer show up in the comparison the test makes anyway: the pads of FLOAT inputs hold +inf, which survives ``max``
(the fused kernels' max-based ELU and max pooling swallow a NaN), ELU, the InstanceNorm++ affine with positive scales, fp16 rounding
and the two-term fp16 split, and turns into inf or NaN in any sum it enters -- a halo row read past the last sample and "masked" by
a multiply makes the output non-finite.  The pads of INTEGER inputs (labels, index maps, the PACK_WEIGHT table) hold a valid index,
0, so that a stray read cannot become a wild address: for those operands only stray WRITES are detectable.  The pads of outputs
hold a finite sentinel that is exact in fp32.

A pad is 4 KiB (1024 floats) on each side unless asked otherwise: a multiple of 16 bytes, so a payload is aligned as the allocator
would align it, and several rows of any tile.  Scratch buffers and workspaces ask for the larger of that and one per-sample stride,
so that an overrun by a whole sample still lands inside the allocation and is reported.

The helper is device-agnostic (``tests/test_guarded_cpu.py`` runs it on the CPU against stand-in kernels written in torch)."""
import numpy as np

PAD_BYTES = 4096
SENTINEL = -123456.75                    # exact in fp32; the pads of outputs
SENTINEL_BYTE = 0xA5                     # ... of byte outputs
NAN = float('nan')


class GuardError(AssertionError):
    pass


class _Buf:
    __slots__ = ('name', 'kind', 'alloc', 'lo', 'n', 'view', 'padval', 'padbits', 'copy', 'must_write', 'armed')


def _bits(t):
    """The same bytes as integers of the same width: comparisons that see NaN payloads and the sign of zero."""
    import torch
    if t.dtype.is_floating_point:
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def pointer_fields(record):
    """The addresses a ctypes record carries (its ``c_void_p`` fields that are set): what ``Guard.check(touched=...)`` takes."""
    import ctypes
    return {getattr(record, name) for name, ctype, *_ in record._fields_ if ctype is ctypes.c_void_p} - {None}


class Guard:
    def __init__(self, torch, device='cuda'):
        self.torch, self.device = torch, device
        self._bufs = []

    # -- allocation --------------------------------------------------------------------------------------------------------
    def _alloc(self, name, kind, shape, dtype, padval, pad):
        torch = self.torch
        item = torch.empty((), dtype=dtype).element_size()
        per16 = max(1, 16 // item)
        lo = PAD_BYTES // item if pad is None else max(PAD_BYTES // item, -(-int(pad) // per16) * per16)
        n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        b = _Buf()
        b.name, b.kind, b.lo, b.n, b.padval, b.copy, b.must_write, b.armed = name, kind, lo, n, padval, None, False, False
        b.alloc = torch.full((lo + n + lo,), padval, dtype=dtype, device=self.device)
        b.padbits = int(_bits(torch.full((1,), padval, dtype=dtype))[0])     # pads are compared bit for bit
        b.view = b.alloc[lo:lo + n].view(tuple(shape))
        self._bufs.append(b)
        return b

    def inp(self, name, array, inout=False, pad=None):
        """A device copy of ``array`` (numpy array or tensor) between two pads: +inf for float operands, 0 for integer ones.  The
        helper keeps a bit-exact copy of the payload; ``inout`` registers an operand the launch is documented to write as well."""
        torch = self.torch
        src = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        b = self._alloc(name, 'inout' if inout else 'in', tuple(src.shape), src.dtype,
                        float('inf') if src.dtype.is_floating_point else 0, pad)
        b.view.copy_(src)
        if not inout:
            b.copy = b.view.clone()
        return b.view

    def out(self, name, shape, fill=NAN, dtype=None, pad=None, must_write=None):
        """An output of exactly ``shape`` elements, filled with ``fill`` (NaN: the operator must write every element; anything else:
        it accumulates, or needs zeroed counters, or leaves gaps the test checks itself), between two pads of the sentinel."""
        torch = self.torch
        dtype = dtype or torch.float32
        if isinstance(shape, int):
            shape = (shape,)
        padval = SENTINEL if dtype.is_floating_point else (SENTINEL_BYTE if dtype == torch.uint8 else 0x5A5A if dtype == torch.int16 else 0x5A5A5A5A)
        b = self._alloc(name, 'out', tuple(shape), dtype, padval, pad)
        b.view.fill_(fill)
        b.must_write = (dtype.is_floating_point and fill != fill) if must_write is None else must_write
        return b.view

    def _find(self, t):
        for b in self._bufs:
            if b.view.data_ptr() == t.data_ptr() and b.n == t.numel():
                return b
        raise KeyError('not a guarded tensor')

    def freeze(self, t):
        """An output of an earlier launch becomes an input of the next ones: its payload is recorded and must not change any
        more, and its pads now hold what the pads of an input hold."""
        b = self._find(t)
        b.kind, b.must_write, b.copy = 'in', False, b.view.clone()
        if b.alloc.dtype.is_floating_point:
            b.padval = float('inf')
            b.padbits = int(_bits(self.torch.full((1,), b.padval, dtype=b.alloc.dtype))[0])
            b.alloc[:b.lo].fill_(b.padval)
            b.alloc[b.lo + b.n:].fill_(b.padval)
        return t

    def resnap(self, t):
        """The test itself changed an input between two launches: record the new payload."""
        b = self._find(t)
        if b.kind == 'in':
            b.copy = b.view.clone()
        return t

    # -- the check ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _pads_changed(b):
        return _bits(b.alloc[:b.lo]) != b.padbits, _bits(b.alloc[b.lo + b.n:]) != b.padbits

    def _flags(self, b, payloads, written):
        f = [m.any() for m in self._pads_changed(b)]
        if payloads and b.kind == 'in':
            f.append((_bits(b.view) != _bits(b.copy)).any())
        if written and b.must_write and b.armed:
            f.append((~self.torch.isfinite(b.view)).any())
        return f

    def check(self, payloads=True, written=True, touched=None):
        """After the stream is synchronised.  One device reduction when all is well; ``payloads=False`` leaves the comparison of
        the inputs with their copies out (launch loops: the pads are still checked), ``written=False`` the scan of the outputs for non-finite values
        (a call that is not meant to fill them, such as a calibration pass over the first sample).  ``touched``: the addresses the
        launch was given -- an output counts as due from the first launch that was handed it (a test may allocate the outputs of
        its later launches up front); None: every output is due."""
        torch = self.torch
        for b in self._bufs:
            if written and (touched is None or b.view.data_ptr() in touched):
                b.armed = True
        flags = [f for b in self._bufs for f in self._flags(b, payloads, written)]
        if flags and bool(torch.stack(flags).any()):
            self._report(payloads, written)

    def _report(self, payloads, written):
        torch = self.torch

        def first(mask):
            return int(torch.nonzero(mask.reshape(-1))[0])
        for b in self._bufs:
            front, back = self._pads_changed(b)
            if bool(front.any()):
                k = int(torch.nonzero(front)[-1])
                raise GuardError('%s: written in front of the buffer, nearest at offset %d (first at %d), %d elements changed'
                                 % (b.name, k - b.lo, first(front) - b.lo, int(front.sum())))
            if bool(back.any()):
                raise GuardError('%s: written past the end of the buffer, first at offset %d (the buffer has %d elements), %d elements changed'
                                 % (b.name, b.n + first(back), b.n, int(back.sum())))
            if payloads and b.kind == 'in':
                diff = _bits(b.view) != _bits(b.copy)
                if bool(diff.any()):
                    raise GuardError('%s: input modified by the launch, first at offset %d, %d elements changed'
                                     % (b.name, first(diff), int(diff.sum())))
            if written and b.must_write and b.armed:
                un = ~torch.isfinite(b.view)
                if bool(un.any()):
                    raise GuardError('%s: output not finite or left unwritten, first at offset %d, %d elements'
                                     % (b.name, first(un), int(un.sum())))
        raise GuardError('a guard flag was raised that the report cannot find again')


# -- plumbing the launch-test modules share --------------------------------------------------------------------------------------------
class _Current:
    """The Guard of the running test (``begin`` / ``end``, from an autouse fixture of the test module): attribute access goes to it."""
    guard = None

    def __getattr__(self, name):
        return getattr(_Current.guard, name)


current = _Current()


def begin(torch, device='cuda'):
    _Current.guard = Guard(torch, device)
    return _Current.guard


def end():
    _Current.guard = None


def dev(torch, a, name=None, inout=False):
    """Upload ``a`` as a guarded input of the running test's Guard (named by position and shape unless told)."""
    g = _Current.guard
    return g.inp(name or 'operand %d %s' % (len(g._bufs), tuple(a.shape)), a, inout=inout)


def out(shape, name=None, fill=NAN, **kw):
    """A guarded output of exactly ``shape`` elements (an int: a flat buffer) of the running test's Guard."""
    g = _Current.guard
    shape = tuple(shape) if not isinstance(shape, int) else (int(shape),)
    return g.out(name or 'output %d %s' % (len(g._bufs), shape), shape, fill=fill, **kw)


def ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def planes(a):
    """complex64 [...] -> float32 [..., 2], the layout the library reads"""
    a = np.ascontiguousarray(a, np.complex64)
    return a.view(np.float32).reshape(a.shape + (2,))


def cplx(t):
    """a device tensor float32 [..., 2] -> numpy complex64 [...]"""
    return np.ascontiguousarray(t.cpu().numpy()).view(np.complex64)[..., 0]
