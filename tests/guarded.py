"""
Guarded device arrays (imported by tests/test_guarded_cpu.py, tests/test_hip_borrowed.py and tests/test_hip_device_io.py;
not a conftest).

``embed`` lays a list of arrays out inside ONE larger tensor, ``guard | a0 | guard | a1 | ... | guard``, and hands back
contiguous views; ``check`` then proves that nothing outside the views was written (outputs), or nothing at all (inputs).
A kernel that stores one element before or after its array, or reads a neighbour's bytes into its result, leaves a trace
in data the test owns: nothing here relies on a fault, and with guards of ``min_guard`` elements an overrun of up to two
rows still lands inside the tensor.

Guards are compared as integers, so that a NaN guard compares equal to itself and a NaN of another payload does not.
Everything is torch and runs on whichever device the arrays are on.
"""
import numpy as np
import torch

# float64 fills, as bit patterns: a quiet NaN with a recognisable payload, and 1e300 (a finite value that swamps any sum)
NAN_BITS = 0x7FF8DEADBEEF5A5A
BIG_BITS = int(np.float64(1e300).view(np.int64))
INT32_FILL = -0x5A5A5A5B

_BITS = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.int8}


def _signed(bits, itemsize):
    """The bit pattern as the signed integer of that width"""
    n = 8 * itemsize
    bits &= (1 << n) - 1
    return bits - (1 << n) if bits >> (n - 1) else bits


def default_fill(dtype):
    """NaN with the payload for float64 (and its low bits for the narrower floats), INT32_FILL's low bits for integers"""
    if dtype == torch.float64:
        return NAN_BITS
    if dtype == torch.float32:
        return 0x7FC5A5A5
    return INT32_FILL


def min_guard(W):
    """The smallest guard the tests use for arrays of row length W: two rows and a wavefront"""
    return 2 * int(W) + 64


class Handle:
    def __init__(self, buf, views, spans, fill, snapshots, guard):
        self.buf, self.views, self.spans, self.fill, self.snapshots, self.guard = buf, views, spans, fill, snapshots, guard

    def bits(self):
        return self.buf.view(_BITS[self.buf.element_size()])


def embed(arrays, guard, fill=None, device=None, inputs=True, tail=None):
    """Place each array (torch tensors or numpy arrays of ONE dtype) as a contiguous view inside one tensor laid out
    ``guard | a0 | guard | a1 | ... | guard``.  `guard` is a count of elements: the first and the last guard always have
    `tail` elements (default: `guard`, or 64 where `guard` is 0), the ones between the arrays `guard` -- 0 packs the arrays
    back to back, as the rows of a sharding slab are; an odd guard puts consecutive 8-byte bases alternately at 0 and 8
    mod 16 (the allocation itself is 256-byte aligned, so the first array sits at 8 mod 16 when the guard is odd).
    `fill`: the guards' bit pattern.  inputs=True snapshots the arrays, and check() then holds them to the snapshot too.
    Returns (views, handle)."""
    ts = [a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, order="C")) for a in arrays]
    assert ts and all(t.dtype == ts[0].dtype for t in ts), "one dtype per embedding"
    dtype = ts[0].dtype
    device = ts[0].device if device is None else torch.device(device)
    fill = default_fill(dtype) if fill is None else fill
    tail = (guard if guard > 0 else 64) if tail is None else tail
    total = 2 * tail + sum(t.numel() for t in ts) + guard * (len(ts) - 1)
    buf = torch.empty(total, dtype=dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    buf.view(_BITS[buf.element_size()]).fill_(_signed(fill, buf.element_size()))
    views, spans, off = [], [], tail
    for t in ts:
        n = t.numel()
        v = buf[off:off + n].view(t.shape)
        v.copy_(t)
        views.append(v)
        spans.append((off, off + n))
        off += n + guard
    assert off - guard + tail == total
    snaps = [v.clone() for v in views] if inputs else None
    return views, Handle(buf, views, spans, fill, snaps, guard)


def check(handle, what="", frames=True):
    """Every guard still holds its exact bit pattern; for inputs every embedded array equals its snapshot bit for bit
    (frames=False: the guards only, for arrays the test itself has rewritten since).
    Names the first offending guard (0 = before the first array) and the offset inside it, or the array and the offset."""
    bits = handle.bits()
    want = _signed(handle.fill, handle.buf.element_size())
    edges = [0] + [x for span in handle.spans for x in span] + [bits.numel()]
    for g in range(len(handle.spans) + 1):
        lo, hi = edges[2 * g], edges[2 * g + 1]
        if hi <= lo:
            continue
        bad = torch.nonzero(bits[lo:hi] != want)
        if bad.numel():
            at = int(bad[0])
            raise AssertionError("%s: guard %d of %d (%d elements, %s array %d) was written at offset %d (%d from its end): "
                                 "%#x, not the fill %#x; %d elements of it differ" % (
                                     what, g, len(handle.spans) + 1, hi - lo, "before" if g < len(handle.spans) else "after",
                                     min(g, len(handle.spans) - 1), at, hi - lo - at,
                                     int(bits[lo + at]) & ((1 << (8 * handle.buf.element_size())) - 1),
                                     handle.fill & ((1 << (8 * handle.buf.element_size())) - 1), int(bad.numel())))
    if handle.snapshots is not None and frames:
        ib = _BITS[handle.buf.element_size()]
        for k, (v, s) in enumerate(zip(handle.views, handle.snapshots)):
            bad = torch.nonzero(v.reshape(-1).view(ib) != s.reshape(-1).view(ib))
            if bad.numel():
                raise AssertionError("%s: input array %d was written at flat offset %d (%d elements differ from the snapshot)" % (
                    what, k, int(bad[0]), int(bad.numel())))
