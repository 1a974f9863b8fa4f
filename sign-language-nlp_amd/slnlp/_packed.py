"""One packed allocation behind the judging buffers of ``ops``: a layout is ONE ordered table of pieces, and the byte offsets,
the device views and the host cut of a download are all derived from that table."""
import functools
import math

import numpy as np
import torch

_NP = {torch.uint8: np.uint8, torch.int32: np.int32, torch.float32: np.float32, torch.int64: np.int64, torch.float64: np.float64}


def _host(h, off, dtype, shape):
    """the piece at byte ``off`` of the host array ``h`` as a numpy view (a copy where ``off`` is not aligned for ``dtype``)"""
    a = np.ndarray(shape, _NP[dtype], h, off)
    return a.copy() if off % dtype.itemsize else a


@functools.lru_cache(maxsize=1024)
def _table(u, pieces):
    """The one place offsets are computed -> ({name: (byte offset, dtype, shape, byte offset of the end, the elements of flat that
    cover the piece, the piece within those seen as its dtype or None: all of them)}, bytes in all); kept per layout, as a judge
    asks for the same buffers epoch after epoch"""
    at, off = {}, 0
    for name, dtype, shape, align, *reserve in pieces:
        shape, size = shape if isinstance(shape, tuple) else (shape,), dtype.itemsize
        n = math.prod(shape)
        off = -(-off // align) * align
        a, b = off // u, -(-(off + n * size) // u)
        lead = (off - a * u) // size
        at[name] = (off, dtype, shape, off + max([n, *reserve]) * size, slice(a, b), slice(lead, lead + n) if (b - a) * u != n * size else None)
        off = at[name][3]
    return at, off


class Packed:
    """``pieces``: ``(name, dtype, shape, byte alignment[, reserved elements])`` in memory order (``shape`` an int n for (n,)).  A
    piece begins at the next multiple of its alignment and holds max(its elements, the reserved ones); ``flat`` is the whole, in
    elements of ``unit``, rounded up.  ``begin`` / ``end`` of a piece are offsets into ``flat``, in its elements (the end rounded up)."""

    def __init__(self, unit, pieces, device):
        self.u = unit.itemsize
        self.at, total = _table(self.u, tuple(pieces))
        self.flat = torch.empty(-(-total // self.u), dtype=unit, device=device)

    def begin(self, name):
        return self.at[name][0] // self.u

    def end(self, name):
        return -(-self.at[name][3] // self.u)

    def views(self, *names, shaped=True):
        """the pieces ``names`` (default: all) as device views of ``flat`` (``shaped=False``: each in one dimension)"""
        flat, out = self.flat, []
        for name in names or self.at:
            _, dtype, shape, _, cover, inner = self.at[name]
            t = flat[cover] if dtype == flat.dtype else flat[cover].view(dtype)
            if inner is not None:                            # the unit elements around a smaller piece hold more than the piece
                t = t[inner]
            out.append(t.view(shape) if shaped and len(shape) > 1 else t)
        return tuple(out)

    def view(self, name, shaped=True):
        return self.views(name, shaped=shaped)[0]

    def cut(self, first, last):
        """ONE device-to-host copy, ``flat[begin(first):end(last)]``, cut into ``{name: numpy view}`` of the pieces ``first``
        through ``last`` by the table that laid them out"""
        a = self.begin(first)
        h, lo, out = self.flat[a:self.end(last)].cpu().numpy(), a * self.u, {}
        for name, (off, dtype, shape, *_) in self.at.items():
            if out or name == first:
                out[name] = _host(h, off - lo, dtype, shape)
                if name == last:
                    break
        return out


def download(tensors, unit):
    """The numpy arrays of ``tensors``, given in the order they lie in memory: ONE device-to-host copy of the range they span, in
    elements of ``unit``, when they are contiguous slices of one storage that lie in that order with less than one such element of
    padding between them (what ``Packed`` lays out); one copy each otherwise."""
    u, st = unit.itemsize, tensors[0].untyped_storage()
    base, at = st.data_ptr(), [t.data_ptr() for t in tensors]
    end, ok = at[0], (at[0] - base) % u == 0
    for a, t in zip(at, tensors):
        ok = ok and 0 <= a - end < u and t.is_contiguous() and t.untyped_storage().data_ptr() == base
        end = a + t.nbytes
    units = -(-(end - at[0]) // u)
    if ok and at[0] - base + units * u <= st.nbytes():
        h = torch.empty(0, dtype=unit, device=tensors[0].device).set_(st, (at[0] - base) // u, (units,)).cpu().numpy()
        return tuple(_host(h, a - at[0], t.dtype, t.shape) for a, t in zip(at, tensors))
    return tuple(t.cpu().numpy() for t in tensors)
