"""Leak-free splits: the near-duplicate GROUPS of a dataset, formed on the device.

``split_audit`` measures after the fact how many held-out rows have a twin in train; ``duplicate_groups`` is the remedy.  It labels
the connected components of "rows within ``radius`` edits of each other" -- under the unit-cost, the long-row or the
phonology-weighted distance, the metrics of ``split_audit`` -- and ``TokenDataset.with_groups`` lets a dataset carry the labels, which
every splitter then honours: ``TokenDataset.split``, the folds of the grid search and of ``cross_fit``, and each fit's internal valid
split (``data.group_folds``).  A row over-sampled by ``balance_dataset`` keeps its original's group, since slicing carries them.

Components are SINGLE-LINKAGE: A ~ B and B ~ C put A and C together even where d(A, C) > radius.  That is what leak-free requires --
a split that separated A from C would have to separate one of them from B.  At a generous radius the chain can swallow the dataset:
``largest`` says so, and a ``RuntimeWarning`` is raised once a group holds more than half the rows.

The N x N distance matrix is never resident (csrc/dup_groups.hip): the distances are formed one chunk of query rows at a time into
the 256 MiB scratch of the neighbour searches, and each chunk is linked into a device-resident forest before the next overwrites it.
Everything is queued on one stream, nothing waits for the host, and one copy brings the result back."""
import warnings

import numpy as np
import torch

from . import _lib, ops
from .data import TokenDataset
from .edit_knn import SCRATCH_PAIRS, _cuda_device, _on_stream, field_table, field_weights_of, long_max_len, query_chunks


def group_metric(what, ds, radius, field_codes, gap, field_weights, max_len):
    """The metric arguments of ``duplicate_groups`` checked as ``split_audit`` checks its own -> (codes or None, gap, weights or
    None, max_len, radius, the largest distance)"""
    max_len = long_max_len(what, max_len)
    if max_len is not None and field_codes is not None:
        raise ValueError(f"{what}: max_len={max_len} with field_codes: the phonology-weighted search is limited to {_lib.EDIT_MAX_LEN} frames "
                         "(only the unit-cost distance takes max_len)")
    if not isinstance(ds, TokenDataset) or len(ds) < 1:
        raise TypeError(f"{what}: ds must be a non-empty slnlp.data.TokenDataset")
    codes, fweights, unit = None, None, 1
    if field_codes is None and field_weights is not None:
        raise ValueError(f"{what}: field_weights={field_weights!r} without field_codes: the unit-cost distance has no fields")
    if field_codes is not None:
        if field_weights is None:
            codes, gap = field_table(what, field_codes, gap)
            unit = int(codes.shape[1])
        else:
            codes, _ = field_table(what, field_codes, None)
            fweights, unit, gap = field_weights_of(what, field_weights, int(codes.shape[1]), gap)
        vocab = getattr(ds, "vocab_X", None)
        if vocab is not None and codes.shape[0] < len(vocab):
            raise ValueError(f"{what}: field_codes has {codes.shape[0]} rows, the source vocabulary {len(vocab)} tokens: the table must cover "
                             "the vocabulary")
    elif gap is not None:
        raise ValueError(f"{what}: gap={gap!r} without field_codes: the unit-cost distance has no gap cost")
    bound = _lib.EDIT_MAX_LEN * unit if max_len is None else max_len
    return codes, gap, fweights, max_len, ops._int_in(what, "radius", radius, 0, bound), bound


def groups_report(group, degree, head, y, radius, max_distance):
    """The dict ``duplicate_groups`` returns, built on the host from the N group ids and degrees and the head"""
    group, degree = np.asarray(group, dtype=np.int64), np.asarray(degree, dtype=np.int64)
    N = len(group)
    roots, inverse, sizes = np.unique(group, return_inverse=True, return_counts=True)
    y = np.asarray(y)
    lo, hi = np.full(len(roots), np.iinfo(np.int64).max), np.full(len(roots), np.iinfo(np.int64).min)
    np.minimum.at(lo, inverse, y)
    np.maximum.at(hi, inverse, y)
    return {"groups": group, "n_groups": int(head[0]), "sizes": sizes.astype(np.int64), "largest": int(sizes.max()),
            "rows_in_groups": int(sizes[sizes >= 2].sum()), "pairs": int(head[1]), "degree": degree, "flagged": int(head[2]),
            "mixed_label_groups": int((lo != hi).sum()), "radius": int(radius), "max_distance": int(max_distance), "rows": N}


def duplicate_groups(ds, radius=0, *, field_codes=None, gap=None, field_weights=None, max_len=None, device=None, cap=None):
    """The near-duplicate groups of ``ds``: the connected components of the graph over its rows whose edges are the pairs within
    ``radius`` edits of each other, every row labelled with the LOWEST row index of its component.  The metric arguments mean what
    they mean in ``split_audit``: nothing: the unit-cost Levenshtein distance over rows of at most 64 frames, ``radius`` in 0..64;
    ``max_len`` (65..512): the same over rows of up to ``max_len`` frames, ``radius`` in 0..max_len; ``field_codes`` (with ``gap``
    and ``field_weights``): the phonology-weighted distance, ``radius`` in 0..64 F (64 W) in field units.  A row the metric refuses
    (longer than its limit) is a singleton and counted in ``flagged``.  ``cap``: the pairs per chunk (None: the 256 MiB scratch).

    Queued on the fit stream: ``ops.dup_groups_buffers``, per chunk of ``query_chunks`` the metric's ``*_distances`` into the
    scratch and ``ops.dup_groups_link``, then ``ops.dup_groups_finish`` and ONE download.  Returns {``groups`` int64 [N],
    ``n_groups``, ``sizes`` int64 [n_groups] (by ascending group id), ``largest``, ``rows_in_groups`` (rows in groups of two or
    more), ``pairs`` (edges within the radius), ``degree`` int64 [N], ``flagged``, ``mixed_label_groups`` (groups that hold more
    than one label: ``split_audit``'s twin with ANOTHER label, seen from the dataset's side), ``radius``, ``max_distance``,
    ``rows``}; ``ds.with_groups(result)`` carries them.  The same bytes on every run and on any stream."""
    what = "duplicate_groups"
    codes, gap, fweights, max_len, radius, bound = group_metric(what, ds, radius, field_codes, gap, field_weights, max_len)
    cap = SCRATCH_PAIRS if cap is None else ops._int_in(what, "cap", cap, 1, _lib.EDIT_MAX_PAIRS)
    dev = _cuda_device(device)
    _lib.require_gpu()
    N = len(ds)
    width = 1 if codes is None and max_len is None else 2
    got = []

    def body():
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        X, L = up(ds.ids), up(ds.lengths)
        table = None if codes is None else up(codes)
        chunks = query_chunks(N, N, max(1, cap // width))
        scratch = torch.empty((chunks[0][1] - chunks[0][0]) * N, dtype=torch.uint8 if width == 1 else torch.uint16, device=dev)
        buf = ops.dup_groups_buffers(N, dev)
        for a, b in chunks:
            out = scratch[:(b - a) * N].view(b - a, N)
            if table is not None:
                ops.field_distances(X[a:b], L[a:b], X, L, table, gap=gap, out=out, field_weights=fweights)
            elif max_len is not None:
                ops.edit_long_distances(X[a:b], L[a:b], X, L, max_len=max_len, out=out)
            else:
                ops.edit_distances(X[a:b], L[a:b], X, L, out=out)
            ops.dup_groups_link(out, a, radius, buf)
        ops.dup_groups_finish(buf)
        got.append({k: v.copy() for k, v in ops.dup_groups_download(buf).items()})
    _on_stream(dev, body)
    res = groups_report(got[0]["group"], got[0]["degree"], got[0]["head"], ds.y, radius, bound)
    if res["largest"] > N / 2:
        warnings.warn(f"{what}: at radius {radius} the largest group holds {res['largest']} of {N} rows: single-linkage components chain "
                      "(A ~ B ~ C joins A and C); a split can keep at most the other rows apart -- consider a smaller radius",
                      RuntimeWarning, stacklevel=2)
    return res
