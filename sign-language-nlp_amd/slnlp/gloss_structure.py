"""Gloss structure: what the LABELS of a dataset look like under an edit distance, formed on the device.

``EditKNN``, ``split_audit`` and ``duplicate_groups`` ask a question of one row: who are its neighbours, has it a twin across the
split.  ``gloss_structure`` asks it of the labels, before anything is trained: are the glosses clusters under this metric at all
(a silhouette per row, per gloss and overall), which glosses lie on top of each other (the class-to-class mean distances, in the
(a, b) format of ``error_analysis``' most-confused pairs), which row is the typical signing of a gloss (its medoid: the rows
``ds[medoids]`` are the reference set of a nearest-prototype ``EditKNN(k=1)``), and which rows sit nearer to another gloss than to
their own (``misplaced``: candidates for a label error, found without a model).  The silhouette is a neighbour-free way to compare
metrics -- unit cost, phonology-weighted, fitted weights -- beside ``fit_field_weights``' leave-one-out objective.

The N x N distance matrix is never resident (csrc/gloss_structure.hip): the distances are formed one chunk of query rows at a time
into the 256 MiB scratch of the neighbour searches, and each chunk is summed by class before the next overwrites it.  The device
forms integers only -- per row the summed distance to its own class and to the nearest other class, per class pair the summed
distance, per class the medoid -- and the host divides them in fp64, with the conventions of sklearn's ``silhouette_samples``.
Everything is queued on one stream, nothing waits for the host, and one copy brings the O(N + C^2) integers back."""
import sys
import types

import numpy as np
import torch

from . import _lib, ops
from .dup_groups import group_metric
from .edit_knn import SCRATCH_PAIRS, _cuda_device, _on_stream, query_chunks


def structure_values(label, count, own, other, other_class, class_sum):
    """The fp64 values of the definitions (include/slnlp.h) from the device's integers -> (a, b, s, class_distance): a = own / (n
    - 1), b = other / n_other, s = (b - a) / max(a, b); s = 0 where the row's class has one member, where there is no other
    class, or where max(a, b) = 0; a row left out (label -1) has a = b = s = NaN.  class_distance[a, b] = class_sum[a, b] / (n_a
    n_b), its diagonal class_sum[a, a] / (n_a (n_a - 1)); NaN where the divisor is 0."""
    label, count = np.asarray(label, dtype=np.int64), np.asarray(count, dtype=np.int64)
    own, other, other_class = np.asarray(own, dtype=np.int64), np.asarray(other, dtype=np.int64), np.asarray(other_class, dtype=np.int64)
    N = len(label)
    a, b, s = np.full(N, np.nan), np.full(N, np.nan), np.full(N, np.nan)
    lab = label >= 0
    n = count[np.where(lab, label, 0)]
    many, has = lab & (n > 1), lab & (other_class >= 0)
    a[lab], b[lab], s[lab] = 0.0, 0.0, 0.0
    a[many] = own[many].astype(np.float64) / (n[many] - 1).astype(np.float64)
    b[has] = other[has].astype(np.float64) / count[other_class[has]].astype(np.float64)
    top = np.maximum(a, b)
    ok = many & has & (top > 0)
    s[ok] = (b[ok] - a[ok]) / top[ok]
    pairs = np.outer(count, count) - np.diag(count)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.where(pairs > 0, np.asarray(class_sum, dtype=np.int64).astype(np.float64) / pairs.astype(np.float64), np.nan)
    return a, b, s, dist


def structure_report(classes, label, got, max_distance, top=50):
    """The dict ``gloss_structure`` returns, built on the host from ``classes`` (the original label values of the class indices),
    ``label`` int [N] (-1: left out) and ``got``, what ``ops.gloss_structure_download`` hands out"""
    classes, label = np.asarray(classes), np.asarray(label, dtype=np.int64)
    count, medoid = np.asarray(got["count"], dtype=np.int64), np.asarray(got["medoid"], dtype=np.int64)
    other_class = np.asarray(got["other_class"], dtype=np.int64)
    C, N = len(classes), len(label)
    a, b, s, dist = structure_values(label, count, got["own"], got["other"], other_class, got["class_sum"])
    lab = label >= 0
    class_s = np.full(C, np.nan)
    sums = np.bincount(label[lab], weights=s[lab], minlength=C)
    class_s[count > 0] = sums[count > 0] / count[count > 0]
    value = lambda c: classes[c].item()
    nearest = [value(c) if c >= 0 else None for c in other_class]
    ia, ib = np.triu_indices(C, 1)
    keep = ~np.isnan(dist[ia, ib])
    ia, ib = ia[keep], ib[keep]
    order = np.argsort(dist[ia, ib], kind="stable")[:top]
    closest = [(value(x), value(y), float(dist[x, y]), int(count[x]), int(count[y])) for x, y in zip(ia[order], ib[order])]
    wrong = np.flatnonzero(lab & (b < a))
    wrong = wrong[np.argsort(s[wrong], kind="stable")]
    misplaced = [{"row": int(i), "label": value(label[i]), "nearest_class": nearest[i], "a": float(a[i]), "b": float(b[i]),
                  "silhouette": float(s[i])} for i in wrong[:top]]
    labelled = int(lab.sum())
    return {"classes": classes, "counts": count, "silhouette": s, "a": a, "b": b, "nearest_class": nearest, "medoids": medoid,
            "class_silhouette": class_s, "mean_silhouette": float(s[lab].mean()) if labelled else float("nan"), "class_distance": dist,
            "closest_pairs": closest, "misplaced": misplaced, "misplaced_share": len(wrong) / labelled if labelled else float("nan"),
            "flagged": int(N - labelled), "rows": N, "max_distance": int(max_distance)}


def gloss_structure(ds, *, field_codes=None, gap=None, field_weights=None, max_len=None, device=None, cap=None, top=50):
    """The structure of ``ds``'s labels under an edit distance.  The metric arguments mean what they mean in ``duplicate_groups``
    and ``split_audit``: nothing: the unit-cost Levenshtein distance over rows of at most 64 frames; ``max_len`` (65..512): the same
    over rows of up to ``max_len`` frames; ``field_codes`` (with ``gap`` and ``field_weights``): the phonology-weighted distance in
    field units.  The classes are ``np.unique(ds.y)`` (at most 1024).  A row the metric refuses (longer than its limit) is left out
    -- it is nobody's neighbour and has NaN values -- and counted in ``flagged``.  ``cap``: the pairs per chunk (None: the 256 MiB
    scratch); ``top``: the length of ``closest_pairs`` and ``misplaced``.

    Queued on the fit stream: ``ops.gloss_structure_buffers``, per chunk of ``query_chunks`` the metric's ``*_distances`` into the
    scratch and ``ops.gloss_structure_rows``, then ``ops.gloss_structure_finish`` and ONE download.  Returns {``classes`` (the
    original label values), ``counts`` int64 [C], ``silhouette`` / ``a`` / ``b`` fp64 [N] (a: the mean distance to the row's own
    gloss, b: to the nearest other gloss, s = (b - a) / max(a, b), sklearn's conventions), ``nearest_class`` (N original label
    values, None where there is no other gloss), ``medoids`` int64 [C] (row indices, -1 for a gloss without rows), ``class_silhouette``
    fp64 [C], ``mean_silhouette`` (over the labelled rows), ``class_distance`` fp64 [C, C] (the mean distance between two glosses,
    the diagonal over the pairs within one; NaN where undefined), ``closest_pairs`` (the ``top`` pairs a < b of smallest mean
    distance as (label a, label b, mean distance, n_a, n_b)), ``misplaced`` (the rows with b < a, most negative silhouette first,
    each {row, label, nearest_class, a, b, silhouette}), ``misplaced_share``, ``flagged``, ``rows``, ``max_distance``}.  The same
    bytes on every run, on any stream and for any ``cap``."""
    what = "gloss_structure"
    codes, gap, fweights, max_len, _, bound = group_metric(what, ds, 0, field_codes, gap, field_weights, max_len)
    cap = SCRATCH_PAIRS if cap is None else ops._int_in(what, "cap", cap, 1, _lib.EDIT_MAX_PAIRS)
    top = ops._int_in(what, "top", top, 0, 2 ** 31 - 1)
    classes, label = np.unique(np.asarray(ds.y), return_inverse=True)
    if len(classes) > _lib.GLOSS_MAX_CLASSES:
        raise ValueError(f"{what}: {len(classes)} classes, at most {_lib.GLOSS_MAX_CLASSES} are taken")
    N = len(ds)
    if bound * N >= 2 ** 32:
        raise ValueError(f"{what}: {N} rows at distances of up to {bound} reach 2^32: a row's sum over one class must fit 32 bits")
    limit = min(_lib.EDIT_MAX_LEN if max_len is None else max_len, int(ds.ids.shape[1]))
    label = np.where((ds.lengths < 0) | (ds.lengths > limit), -1, label.reshape(-1)).astype(np.int32)
    dev = _cuda_device(device)
    _lib.require_gpu()
    width = 1 if codes is None and max_len is None else 2
    got = []

    def body():
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        X, L = up(ds.ids), up(ds.lengths)
        table = None if codes is None else up(codes)
        chunks = query_chunks(N, N, max(1, cap // width))
        scratch = torch.empty((chunks[0][1] - chunks[0][0]) * N, dtype=torch.uint8 if width == 1 else torch.uint16, device=dev)
        buf = ops.gloss_structure_buffers(N, len(classes), label, bound, dev)
        for a, b in chunks:
            out = scratch[:(b - a) * N].view(b - a, N)
            if table is not None:
                ops.field_distances(X[a:b], L[a:b], X, L, table, gap=gap, out=out, field_weights=fweights)
            elif max_len is not None:
                ops.edit_long_distances(X[a:b], L[a:b], X, L, max_len=max_len, out=out)
            else:
                ops.edit_distances(X[a:b], L[a:b], X, L, out=out)
            ops.gloss_structure_rows(out, a, buf)
        ops.gloss_structure_finish(buf)
        got.append({k: v.copy() for k, v in ops.gloss_structure_download(buf).items()})
    _on_stream(dev, body)
    return structure_report(classes, label, got[0], bound, top)


class _Callable(types.ModuleType):
    """``slnlp.gloss_structure`` names this module AND its function (an imported submodule becomes an attribute of its package):
    calling the module calls the function, so ``slnlp.gloss_structure(ds)`` means the same before and after the first import"""
    __call__ = staticmethod(gloss_structure)


sys.modules[__name__].__class__ = _Callable
