"""Guard-band buffers for tests that call a kernel entry point directly.

A fresh ``torch.empty`` hides three kinds of mistake: the caching allocator rounds sizes up, so a store a row past
the end lands in padding; a side buffer sized by a ``*_workspace_bytes`` function is as large as the same function
says it must be; and the second of two runs gets the first run's block back, still holding correct values, so an
element the kernel forgot reads as written.

``Arena(device)`` hands out buffers that sit inside a larger allocation of their own:

    [ pad to 256 B | leading guard, 128 KiB | payload, exactly numel * itemsize bytes | trailing guard, 128 KiB ]

The payload starts on a 256-byte boundary and the trailing guard at the payload's last byte + 1, with no rounding.
Guards and payloads are prefilled with a sentinel that is compared as integers, never as floats: the bytes of the
fp32 quiet NaN 0x7fc5a5a5 (8-byte types: the fp64 quiet NaN 0x7ff8a5a5a5a5a5a5).  Inputs are finite, so no
legitimate result has these bits.  The guard (131,072 B) exceeds the largest footprint one workgroup stores in one
step: the board conv's 4 waves x 16 rows x 1152 B = 73,728 B; a torus workgroup stores 40,960 B.

    out(shape, dtype)   an output the kernel must write completely        payload = sentinel
    ws(nbytes)          a workspace of exactly the bytes a size function returned; may stay partly unwritten
    acc(shape)          an output that accumulates by its header's contract  payload = zeros
    inout(tensor)       a tensor updated in place (running statistics)       payload = a copy of the tensor

``check()`` synchronizes and asserts (a) every guard byte still holds the sentinel (on failure: the buffer's name,
the side, the first and last dirty byte offsets), (b) no word of an ``out`` payload still holds the sentinel;
(c) workspaces, accumulators and in-place tensors are exempt from (b).  ``check_untouched()`` asserts that guards
and payloads alike still hold their prefill (an entry point that must return before any launch).

``Plain(device)`` has the same four methods on ordinary tensors prefilled with zeros: the unguarded run of an A/B
pair.  Nothing here knows about the GPU: the helper's own tests drive it on the CPU.
"""

import torch

GUARD = 128 * 1024
ALIGN = 256
SENTINEL32 = 0x7fc5a5a5
SENTINEL64 = 0x7ff8a5a5a5a5a5a5
_SENTINEL_BYTES = tuple((SENTINEL32 >> (8 * i)) & 0xff for i in range(4))   # little endian


def bits(t):
    """The tensor's elements as integers of the same width (bit-exact comparison: NaNs and signed zeros count)."""
    size = t.element_size()
    if t.dtype.is_floating_point or t.dtype.is_complex:
        return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[size])
    return t


class _Buf:
    def __init__(self, name, kind, raw, start, nbytes, view, keep=None):
        self.name, self.kind, self.raw, self.start, self.nbytes, self.view, self.keep = \
            name, kind, raw, start, nbytes, view, keep

    def guard(self, side):
        lo = self.start - GUARD if side == 'leading' else self.start + self.nbytes
        return self.raw[lo:lo + GUARD]

    def payload(self):
        return self.raw[self.start:self.start + self.nbytes]


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self.bufs = []
        self._pat = torch.tensor(_SENTINEL_BYTES * (GUARD // 4), dtype=torch.uint8).to(self.device)

    # -- allocation
    def _place(self, nbytes, name, kind):
        nbytes = int(nbytes)
        assert nbytes >= 0
        raw = torch.empty(ALIGN + GUARD + nbytes + GUARD, dtype=torch.uint8, device=self.device)
        start = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN
        assert (raw.data_ptr() + start) % ALIGN == 0
        raw[start - GUARD:start].copy_(self._pat)
        raw[start + nbytes:start + nbytes + GUARD].copy_(self._pat)
        name = name or '%s%d' % (kind, len(self.bufs))
        return raw, start, name

    def _typed(self, shape, dtype, name, kind):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        numel = 1
        for s in shape:
            numel *= int(s)
        size = torch.empty(0, dtype=dtype).element_size()
        raw, start, name = self._place(numel * size, name, kind)
        view = raw[start:start + numel * size].view(dtype).view(shape)
        buf = _Buf(name, kind, raw, start, numel * size, view)
        self.bufs.append(buf)
        return buf

    def out(self, shape, dtype=torch.float32, name=None):
        """A payload of exactly numel * itemsize bytes, every word the sentinel: the kernel must write all of it."""
        size = torch.empty(0, dtype=dtype).element_size()
        if size not in (4, 8):
            raise ValueError('out(): 4- and 8-byte types only (the sentinel is a word)')
        buf = self._typed(shape, dtype, name, 'out')
        buf.payload().view(torch.int32 if size == 4 else torch.int64).fill_(SENTINEL32 if size == 4 else SENTINEL64)
        return buf.view

    def ws(self, nbytes, name=None):
        """A workspace of exactly nbytes bytes (uint8), prefilled with the sentinel's bytes."""
        raw, start, name = self._place(nbytes, name, 'ws')
        nbytes = int(nbytes)
        pay = raw[start:start + nbytes]
        reps = (nbytes + GUARD - 1) // GUARD
        for i in range(reps):   # the 4-byte pattern stays in phase: GUARD is a multiple of 4
            piece = pay[i * GUARD:(i + 1) * GUARD]
            piece.copy_(self._pat[:piece.numel()])
        buf = _Buf(name, 'ws', raw, start, nbytes, pay)
        self.bufs.append(buf)
        return buf.view

    def acc(self, shape, dtype=torch.float32, name=None):
        """An output that accumulates by contract: payload zeros, guards the sentinel."""
        buf = self._typed(shape, dtype, name, 'acc')
        buf.view.zero_()
        return buf.view

    def inout(self, tensor, name=None):
        """A tensor the kernel updates in place: payload a copy of `tensor`, guards the sentinel."""
        buf = self._typed(tensor.shape, tensor.dtype, name, 'inout')
        buf.view.copy_(tensor)
        buf.keep = tensor.detach().clone().to(self.device)
        return buf.view

    # -- checks
    def _sync(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)

    def _check_guards(self):
        for b in self.bufs:
            for side in ('leading', 'trailing'):
                dirty = (b.guard(side) != self._pat).nonzero()
                if dirty.numel():
                    first, last = int(dirty[0]), int(dirty[-1])
                    if side == 'leading':
                        where = 'bytes %d .. %d before the payload start' % (GUARD - first, GUARD - last)
                    else:
                        where = 'bytes %d .. %d past the payload end' % (first, last)
                    raise AssertionError('%s (%d-byte payload): %s guard dirty, %d bytes, %s'
                                         % (b.name, b.nbytes, side, dirty.numel(), where))

    def check(self):
        """(a) guards intact, (b) every `out` word written; workspaces, acc and inout exempt from (b)."""
        self._sync()
        self._check_guards()
        for b in self.bufs:
            if b.kind != 'out':
                continue
            size = b.view.element_size()
            words = b.payload().view(torch.int32 if size == 4 else torch.int64)
            left = (words == (SENTINEL32 if size == 4 else SENTINEL64)).nonzero()
            if left.numel():
                raise AssertionError('%s (%d elements): %d never written, first at element %d, last at element %d'
                                     % (b.name, words.numel(), left.numel(), int(left[0]), int(left[-1])))

    def check_untouched(self):
        """Guards and payloads still hold their prefill: nothing was launched."""
        self._sync()
        self._check_guards()
        for b in self.bufs:
            if b.kind == 'out':
                size = b.view.element_size()
                words = b.payload().view(torch.int32 if size == 4 else torch.int64)
                same = bool((words == (SENTINEL32 if size == 4 else SENTINEL64)).all())
            elif b.kind == 'ws':
                same = True
                for i in range((b.nbytes + GUARD - 1) // GUARD):
                    piece = b.view[i * GUARD:(i + 1) * GUARD]
                    same = same and bool((piece == self._pat[:piece.numel()]).all())
            elif b.kind == 'acc':
                same = bool((bits(b.view) == 0).all())
            else:
                same = torch.equal(bits(b.view), bits(b.keep))
            assert same, '%s: payload changed' % b.name


class Plain:
    """The same interface on ordinary tensors prefilled with zeros (the unguarded run of an A/B pair)."""

    def __init__(self, device):
        self.device = torch.device(device)

    def out(self, shape, dtype=torch.float32, name=None):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    acc = out

    def ws(self, nbytes, name=None):
        return torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device)

    def inout(self, tensor, name=None):
        return tensor.detach().clone().to(self.device)

    def check(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)
