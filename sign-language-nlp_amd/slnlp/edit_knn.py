"""The non-neural baseline and the audit of a split: k nearest neighbours under Levenshtein distance, on the device.

A row of this data is a short sequence of composite phonology tokens, and the obvious method that needs no network is "look up the
most similar training signs".  ``EditKNN`` is that method as one more ``LogProbJudge`` host beside ``VotingEnsemble``, ``PriorShift``
and ``OutOfFold``: ``fit`` uploads the train rows once, and ``_forward_logp(ds, then)`` -- the one hook every consumer goes through
-- forms all-pairs edit distances, the k nearest references of every query and their vote as float32 log-probs [N, V], library
launches only (csrc/edit_knn.hip; no torch arithmetic runs on the device).  ``reliability``, ``ranking``,
``score_interval``, ``label_issues``, ``attribute`` and ``compare`` then work on it unchanged: ``net.compare(knn, X)`` says whether
a network beats the trivial method.  ``leave_one_out()`` gives out-of-sample log-probs of the train rows themselves with no fit at
all.

``split_audit`` asks the other question the same distances answer: do the held-out rows have twins in train?  ASL-Phono holds the
same gloss signed several times; identical or near-identical token sequences on both sides of a split inflate every score, and a
twin with ANOTHER gloss is irreducible error or a label problem no model-based audit can see.

Rows longer than 64 frames are REFUSED by default -- ``fit`` raises, a query is flagged and gets a row of NaN -- never truncated:
the default kernel is Myers' bit-vector recurrence with the query in one 64-bit word.  ``EditKNN(max_len=...)`` and
``split_audit(..., max_len=...)`` with ``max_len`` in 65..512 run the MULTI-WORD recurrence instead (csrc/edit_long.hip: the query
in up to 8 words, a uint16 distance matrix, two bytes a pair): every call of that estimator takes rows of up to ``max_len`` frames
and refuses longer ones in the same way.  It is opt-in: with nothing set every call is the one it was, launch for launch.

``PhonoKNN`` and ``split_audit(field_codes=...)`` answer both questions under the PHONOLOGY-WEIGHTED edit distance instead
(csrc/field_knn.hip): a token is a composition of F fields, and substituting one frame for another costs the number of fields in
which they differ.  Only the search and the vote differ; the unit-cost surface keeps its bytes, messages and defaults.  THE ONE
LIMIT THAT REMAINS: the phonology-weighted search stays at 64 frames (its kernel keeps a thread's column of the dynamic program in
LDS, which does not stretch to 512 positions) -- ``PhonoKNN`` and ``split_audit(field_codes=...)`` refuse ``max_len``.
``field_weights=`` gives every field an integer weight of its own (``slnlp.fit_field_weights`` fits them, slnlp/field_weights.py);
without it every call is the one it was."""
import collections
import copy

import numpy as np
import torch
from sklearn.base import BaseEstimator, ClassifierMixin

from . import _lib, metrics, ops
from .data import DeviceRows, TokenDataset
from .judge import LogProbJudge

WEIGHTS = _lib.EDIT_WEIGHTS
SCRATCH_PAIRS = 1 << 28                      # (query, reference) pairs per launch sequence: one byte each, 256 MiB of scratch


def knn_options(what, k, weights, tau, normalize, smoothing):
    """The options of ``EditKNN`` checked: (k, weights, tau, normalize, smoothing); anything else raises ValueError"""
    k = ops._int_in(what, "k", k, 1, _lib.EDIT_MAX_K)
    if weights not in WEIGHTS:
        raise ValueError(f"{what}: weights={weights!r}, expected one of {WEIGHTS}")
    if not isinstance(normalize, (bool, np.bool_)):
        raise ValueError(f"{what}: normalize={normalize!r}, expected True or False")
    return k, weights, ops._positive(what, "tau", tau), bool(normalize), ops._positive(what, "smoothing", smoothing)


def query_chunks(nq, nr, cap=SCRATCH_PAIRS):
    """The query rows of one pass in chunks ``[(start, stop), ...]`` that keep ``(stop - start) * nr`` under ``cap`` pairs (a single
    query where ``nr`` alone exceeds it): every row exactly once, in order."""
    nq, nr, cap = ops._int_in("query_chunks", "nq", nq, 1, _lib.EDIT_MAX_ROWS), ops._int_in("query_chunks", "nr", nr, 1, _lib.EDIT_MAX_ROWS), \
        ops._int_in("query_chunks", "cap", cap, 1, _lib.EDIT_MAX_PAIRS)
    step = max(1, min(nq, cap // nr))
    return [(a, min(a + step, nq)) for a in range(0, nq, step)]


def long_max_len(what, max_len):
    """``max_len`` checked: None (the 64-frame search) or an integer in 65..512 (the multi-word search); anything else raises
    ValueError"""
    if max_len is None:
        return None
    return ops._int_in(what, "max_len", max_len, _lib.EDIT_MAX_LEN + 1, _lib.EDIT_LONG_MAX_LEN)


def _check_rows(what, ds, max_len=None):
    """A TokenDataset whose every row the kernel takes: lengths in 0..min(64, S) -- or 0..min(max_len, S)"""
    if not isinstance(ds, TokenDataset):
        raise TypeError(f"{what}: expected a slnlp.data.TokenDataset, got {type(ds).__name__}")
    if len(ds) < 1:
        raise ValueError(f"{what}: the dataset has no rows")
    limit = _lib.EDIT_MAX_LEN if max_len is None else max_len
    top = min(limit, int(ds.ids.shape[1]))
    bad = (ds.lengths < 0) | (ds.lengths > top)
    if bad.any():
        raise ValueError(f"{what}: {int(bad.sum())} of {len(ds)} rows have a length outside 0..{top} (first: row {int(np.flatnonzero(bad)[0])}, "
                         f"length {int(ds.lengths[bad][0])}); rows longer than {limit} frames are refused, not truncated")


def _cuda_device(device):
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError(f"device={device!r}: the HIP path is the only compute path, expected a cuda device")
    return dev


def _on_stream(dev, body):
    """``body()`` under the device's gate held shared, on this thread's fit stream; returns once the stream has drained"""
    from .net import device_gate, device_stream, stream_sync
    gate = device_gate(dev)
    gate.enter(False)
    try:
        stream = device_stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.device(dev), torch.cuda.stream(stream), torch.no_grad():
            res = body()
        stream_sync(stream)
    finally:
        gate.leave(False)
    return res


# What ``_search`` needs of a neighbour search: ``width``, the bytes a pair takes in its distance matrix, and
# ``rows(Xq, Lq, Xr, Lr, k, radius, exclude, buf, scratch)``, its ``ops.*_knn_rows`` bound to its metric's arguments
Search = collections.namedtuple("Search", "width rows")


def _bound(width, fn, *metric, **options):
    def rows(Xq, Lq, Xr, Lr, k, radius, exclude, buf, scratch):
        return fn(Xq, Lq, Xr, Lr, *metric, k, radius=radius, exclude=exclude, buf=buf, scratch=scratch, **options)
    return Search(width, rows)


def unit_search(max_len=None):
    """``ops.edit_knn_rows``: one byte a pair -- with ``max_len`` (65..512) ``ops.edit_long_knn_rows``: two"""
    return _bound(1, ops.edit_knn_rows) if max_len is None else _bound(2, ops.edit_long_knn_rows, max_len=max_len)


def field_search(codes, gap, field_weights=None):
    """``ops.field_knn_rows`` over ``codes`` (on the device): two bytes a pair"""
    return _bound(2, ops.field_knn_rows, codes, gap=gap, field_weights=field_weights)


def _search(Xq, Lq, Xr, Lr, k, radius, exclude, each, cap=None, search=None):
    """``search.rows`` (a ``Search``; None: the unit-cost one) over the queries in ``query_chunks``; ``each(start, stop, buf)`` runs
    behind every chunk on the same stream.  One scratch and one buffer serve the chunks of equal size.  A search of two bytes a pair
    (the field metric, the long rows) is chunked at half the pairs: the scratch stays at 256 MiB."""
    search = unit_search() if search is None else search
    nq, nr = int(Xq.shape[0]), int(Xr.shape[0])
    cap = SCRATCH_PAIRS if cap is None else cap
    chunks = query_chunks(nq, nr, max(1, cap // search.width))
    scratch = torch.empty(search.width * (chunks[0][1] - chunks[0][0]) * nr, dtype=torch.uint8, device=Xq.device)
    buf = None
    for a, b in chunks:
        if buf is None or buf["shape"][0] != b - a:
            buf = ops.edit_knn_buffers(b - a, k, Xq.device)
        search.rows(Xq[a:b], Lq[a:b], Xr, Lr, k, radius, None if exclude is None else exclude[a:b], buf, scratch)
        each(a, b, buf)


def field_table(what, field_codes, gap):
    """The code table of the phonology-weighted metric checked, on the host: ``field_codes`` a 2-D integer array [Vt >= 1, F in
    1..16] whose values fit int32, ``gap`` an integer in 1..F (None: F) -> (contiguous int32 array, gap); anything else raises
    ValueError"""
    if torch.is_tensor(field_codes):
        field_codes = field_codes.detach().cpu().numpy()
    codes = np.asarray(field_codes)
    if codes.ndim != 2 or codes.dtype.kind not in "iu" or codes.shape[0] < 1 or not 1 <= codes.shape[1] <= _lib.FIELD_MAX_FIELDS:
        raise ValueError(f"{what}: field_codes must be a 2-D integer array [Vt >= 1, F in 1..{_lib.FIELD_MAX_FIELDS}] (slnlp.ingest.field_codes), "
                         f"got {codes.dtype} {tuple(codes.shape)}")
    if codes.size and (codes.min() < -2 ** 31 or codes.max() >= 2 ** 31):
        raise ValueError(f"{what}: field_codes holds values outside int32")
    F = int(codes.shape[1])
    return np.ascontiguousarray(codes, dtype=np.int32), ops._int_in(what, "gap", F if gap is None else gap, 1, F)


def field_weights_of(what, field_weights, F, gap):
    """The per-field weights of the weighted metric checked, on the host: ``field_weights`` F integers in 0..16 whose sum W lies
    in 1..16, ``gap`` an integer in 1..W (None: W) -> (tuple of ints, W, gap); anything else raises ValueError"""
    _, W, gap = ops._field_weights(what, field_weights, F, gap)
    return tuple(int(v) for v in field_weights), W, gap


class EditKNN(LogProbJudge, ClassifierMixin, BaseEstimator):
    """``k`` nearest train rows under unit-cost Levenshtein distance (1..64; ties at the k-th distance go to the lower train row),
    voting with ``weights`` "uniform" or "distance": w = exp(-d / (tau n)), n = max(len(query), len(neighbour), 1) when
    ``normalize``, else 1.  p_c = (sum of the weights of the neighbours with label c + smoothing prior_c) / (sum of all weights +
    smoothing) with ``prior_`` = (n_c + 1) / (N + V) of the train labels, so no class is at 0 and a query without a neighbour gets
    the prior.  It has no temperature: ``calibration_`` is None, ``temperature_`` 1.0.

    ``max_len`` (None: rows of at most 64 frames, the calls and the bytes it always had): an integer in 65..512 -- every call of
    the estimator (``fit``'s row check, the log-probs, ``kneighbors``, ``leave_one_out``, ``attribute``) takes rows of up to
    ``max_len`` frames through the multi-word search (csrc/edit_long.hip); a longer row is refused as a row beyond 64 is without
    it, and where every row has at most 64 frames the log-probs are bit for bit the ones of ``max_len=None``.  ``get_params``
    lists ``max_len`` only when it is set, so the parameter list of the default estimator is what it was;
    ``set_params(max_len=...)`` is taken either way."""
    calibration_ = None
    temperature_ = 1.0
    predict_nonlinearity = "auto"
    initialized_ = False
    _loo = False
    _cap = None                                              # pairs per launch sequence (None: SCRATCH_PAIRS)
    _max_len = None                                          # what fit checked max_len to: None, the 64-frame search

    def __init__(self, k=5, weights="distance", tau=1.0, normalize=True, smoothing=1.0, device=None, max_len=None):
        knn_options("EditKNN", k, weights, tau, normalize, smoothing)
        long_max_len("EditKNN", max_len)
        if device is not None:
            _cuda_device(device)
        self.k, self.weights, self.tau, self.normalize, self.smoothing, self.device = k, weights, tau, normalize, smoothing, device
        self.max_len = max_len

    def get_params(self, deep=True):
        params = super().get_params(deep=deep)
        if params.get("max_len") is None:
            params.pop("max_len", None)
        return params

    def set_params(self, **params):
        if "max_len" in params:
            self.max_len = params.pop("max_len")
        return super().set_params(**params)

    # ------------------------------------------------------------------ fit
    def fit(self, X, y=None):
        """Check ``X`` (a ``TokenDataset``: lengths in 0..64 -- 0..``max_len`` where that is set --, labels inside the classes:
        ValueError otherwise, before anything touches the GPU) and upload its ids, lengths and labels once.  ``classes_`` as
        ``NeuralNetClassifier`` sets them: the target vocabulary's indices, or 0..max(y) without one."""
        knn_options("EditKNN", self.k, self.weights, self.tau, self.normalize, self.smoothing)
        self._max_len = long_max_len("EditKNN", self.max_len)    # again: set_params goes past __init__
        ds = self._as_dataset(X, y)
        _check_rows("EditKNN.fit", ds, self._max_len)
        classes = np.arange(len(ds.vocab_y)) if ds.vocab_y is not None else np.arange(int(ds.y.max()) + 1)
        V = len(classes)
        self._refuse_labels("EditKNN.fit", ((ds.y < 0) | (ds.y >= V)).sum(), len(ds), V)
        dev = _cuda_device(self.device)
        _lib.require_gpu()
        self.classes_, self.rows_, self.dataset_ = classes, len(ds), ds
        self.prior_ = (np.bincount(np.asarray(ds.y), minlength=V).astype(np.float64) + 1.0) / (len(ds) + V)
        with torch.cuda.device(dev):
            self._ids, self._lengths, self._y = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ds.ids, ds.lengths, np.asarray(ds.y)))
            self._prior = torch.from_numpy(self.prior_).to(dev)
        self._self_index = None
        self.initialized_ = True
        return self

    def leave_one_out(self):
        """A sibling that shares the device rows and judges the FITTED rows themselves: query i skips reference i, so its
        log-probs are out of sample with no fit at all.  It refuses every other dataset (length, labels, lengths and ids are
        compared); the fitted ``EditKNN`` predicts new rows."""
        self._require_initialized()
        sib = copy.copy(self)
        sib._loo = True
        with torch.cuda.device(self._ids.device):
            sib._self_index = torch.from_numpy(np.arange(self.rows_, dtype=np.int64)).to(self._ids.device)
        return sib

    def attribute(self, *args, **kwargs):
        if self._loo:
            raise NotImplementedError("EditKNN.leave_one_out: leave-one-out log-probs exist only for the fitted rows themselves, not for "
                                      "occluded variants of them; attribute with the fitted EditKNN")
        return super().attribute(*args, **kwargs)

    def _refuse_other_data(self, ds):
        own = self.dataset_
        same = isinstance(ds, TokenDataset) and len(ds) == self.rows_ and (ds is own or (np.array_equal(ds.y, own.y) and np.array_equal(ds.lengths, own.lengths)
                                                                                       and np.array_equal(ds.ids, own.ids)))
        if not same:
            raise ValueError(f"EditKNN.leave_one_out: leave-one-out log-probs exist only for the {self.rows_} rows that were fitted on, in their "
                             f"order; got a dataset of {len(ds)} rows" + ("" if len(ds) != self.rows_ else " with other contents")
                             + " (the fitted EditKNN predicts new rows)")

    # ------------------------------------------------------------- the hook
    def _queries(self, ds):
        """(ids, lengths, labels) of the queries on the fitted rows' device, and the exclusion list"""
        if self._loo:
            self._refuse_other_data(ds)
            return self._ids, self._lengths, self._y, self._self_index
        if isinstance(ds, DeviceRows):                       # built on the device (LogProbJudge.attribute): taken as they are
            if ds.ids.device != self._ids.device:
                raise ValueError(f"EditKNN: the rows are on {ds.ids.device}, the fitted rows on {self._ids.device}")
            return ds.ids, ds.lengths, ds.y, None
        if not isinstance(ds, TokenDataset) or len(ds) < 1:
            raise TypeError("EditKNN: expected a non-empty slnlp.data.TokenDataset or slnlp.data.DeviceRows")
        dev = self._ids.device
        return (*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ds.ids, ds.lengths, np.asarray(ds.y))), None)

    def _on_stream(self, body):
        return _on_stream(self._ids.device, body)

    def _searcher(self):
        """What ``_search`` runs: the unit-cost search of the fitted ``max_len``"""
        return unit_search(self._max_len)

    def _vote(self, buf, Lq, **options):
        if self._max_len is not None:
            ops.edit_long_knn_logp(buf, Lq, self._lengths, self._y, self._prior, max_len=self._max_len, **options)
            return
        ops.edit_knn_logp(buf, Lq, self._lengths, self._y, self._prior, **options)

    def _forward_logp(self, ds, then):
        """The float32 log-probs [len(ds), V] of ``ds`` (a ``TokenDataset`` or ``DeviceRows``) on the device, handed to
        ``then(logp, y_dev)``: the hook every consumer of ``LogProbJudge`` goes through.  The queries go in ``query_chunks``; per
        chunk ``ops.edit_knn_rows`` and ``ops.edit_knn_logp`` (with ``max_len``: their ``edit_long_`` siblings) -- five queued launches,
        nothing waits for the host.  A flagged query shows as a row of NaN."""
        self._require_initialized()
        if self._loo:
            self._refuse_other_data(ds)                      # before anything touches the device
        k, weights, tau, normalize, lam = knn_options("EditKNN", self.k, self.weights, self.tau, self.normalize, self.smoothing)

        def body():
            return then(*self._queue_logp(ds, k, weights, tau, normalize, lam))
        return self._on_stream(body)

    def _queue_logp(self, ds, k, weights, tau, normalize, lam):
        """``_forward_logp``'s launches queued on the current stream: (log-probs [len(ds), V], labels), both on the device"""
        Xq, Lq, yq, exclude = self._queries(ds)
        out = torch.empty(int(Xq.shape[0]), len(self.classes_), dtype=torch.float32, device=Xq.device)

        def vote(a, b, buf):
            self._vote(buf, Lq[a:b], weights=weights, tau=tau, normalize=normalize, lam=lam, out=out[a:b])
        _search(Xq, Lq, self._ids, self._lengths, k, 0, exclude, vote, self._cap, self._searcher())
        return out, yq

    # ------------------------------------------------------------ neighbours
    def kneighbors(self, X, k=None):
        """``(distances int32 [N, k], indices int64 [N, k])`` of the ``k`` (None: the estimator's) nearest train rows of every row
        of ``X``, ordered by (distance, train row); (-1, -1) where fewer than k exist or the query's length is outside 0..64
        (0..``max_len`` where that is set).  One download per chunk of queries."""
        self._require_initialized()
        k = ops._int_in("EditKNN.kneighbors", "k", self.k if k is None else k, 1, _lib.EDIT_MAX_K)
        ds = self._as_dataset(X)
        if self._loo:
            self._refuse_other_data(ds)
        got = []

        def body():
            Xq, Lq, _, exclude = self._queries(ds)
            _search(Xq, Lq, self._ids, self._lengths, k, 0, exclude, lambda a, b, buf: got.append(ops.edit_knn_download(buf)["nbr"].copy()), self._cap,
                    self._searcher())
        self._on_stream(body)
        nbr = np.concatenate(got, axis=0)
        return nbr[:, :, 0].astype(np.int32), nbr[:, :, 1].astype(np.int64)


class PhonoKNN(EditKNN):
    """``EditKNN`` under the PHONOLOGY-WEIGHTED edit distance (csrc/field_knn.hip): a token of this data is a composition of F
    fields, and substituting one frame for another costs the number of fields in which they differ -- ``field_codes`` int [Vt, F]
    (``slnlp.ingest.field_codes``) holds token v's per-field value ids in row v; a token outside the table costs F against every
    other -- while inserting or deleting a frame costs ``gap`` (1..F; None: F).  Distances are integers in field units, at most
    64 F; the vote's w = exp(-d / (tau n)) takes n = F max(len(query), len(neighbour), 1) when ``normalize``, else F, so ``tau``
    is in frames as in ``EditKNN``.  ``fit``, ``leave_one_out``, ``kneighbors`` and every ``LogProbJudge`` method are ``EditKNN``'s:
    only the search and the vote differ.  With F = 1, ``field_codes[v, 0] = v`` and ``gap = 1`` it is ``EditKNN``.

    ``field_weights`` (None: the metric above, the calls and the bytes it always had): F integers in 0..16 whose sum W lies in
    1..16 -- field f counts ``field_weights[f]`` instead of 1, a field of weight 0 is ignored, a token outside the table costs W,
    ``gap`` lies in 1..W (None: W), distances are at most 64 W and the vote's unit is W (``unit_``), so ``tau`` stays in frames.
    ``slnlp.fit_field_weights`` fits them.  ``get_params`` lists ``field_weights`` only when it is set, so the parameter list of
    the unweighted estimator is what it was; ``set_params(field_weights=...)`` is taken either way.

    It takes no ``max_len``: the phonology-weighted search is limited to 64 frames, and ``fit`` raises where the attribute was
    set all the same."""

    def __init__(self, field_codes, gap=None, k=5, weights="distance", tau=1.0, normalize=True, smoothing=1.0, device=None, field_weights=None):
        self._check_metric(field_codes, gap, field_weights)
        super().__init__(k=k, weights=weights, tau=tau, normalize=normalize, smoothing=smoothing, device=device)
        self.field_codes, self.gap, self.field_weights = field_codes, gap, field_weights

    @staticmethod
    def _check_metric(field_codes, gap, field_weights):
        """-> (the table, gap, the weights as a tuple or None, the vote's unit: W, or F without weights)"""
        if field_weights is None:
            codes, gap = field_table("PhonoKNN", field_codes, gap)
            return codes, gap, None, int(codes.shape[1])
        codes, _ = field_table("PhonoKNN", field_codes, None)
        w, W, gap = field_weights_of("PhonoKNN", field_weights, int(codes.shape[1]), gap)
        return codes, gap, w, W

    def get_params(self, deep=True):
        params = super().get_params(deep=deep)
        if params.get("field_weights") is None:
            params.pop("field_weights", None)
        return params

    def set_params(self, **params):
        if "field_weights" in params:
            self.field_weights = params.pop("field_weights")
        return super().set_params(**params)

    def fit(self, X, y=None):
        """``EditKNN.fit`` after the table is checked -- again, as ``set_params`` goes past ``__init__`` -- and held to the
        dataset: with a source vocabulary it has a row for every token id (ValueError otherwise, before anything touches the
        GPU).  The table is uploaded once."""
        if getattr(self, "max_len", None) is not None:
            raise ValueError(f"PhonoKNN.fit: max_len={self.max_len!r}: the phonology-weighted search is limited to {_lib.EDIT_MAX_LEN} frames "
                             "(only EditKNN and the unit-cost split_audit take max_len)")
        codes, gap, fweights, unit = self._check_metric(self.field_codes, self.gap, self.field_weights)
        ds = self._as_dataset(X, y)
        vocab = getattr(ds, "vocab_X", None)
        if vocab is not None and codes.shape[0] < len(vocab):
            raise ValueError(f"PhonoKNN.fit: field_codes has {codes.shape[0]} rows, the dataset's source vocabulary {len(vocab)} tokens: "
                             "the table must cover the vocabulary")
        super().fit(ds)
        with torch.cuda.device(self._ids.device):
            self._codes = torch.from_numpy(codes).to(self._ids.device)
        self._gap, self.fields_, self._fweights, self.unit_ = gap, int(codes.shape[1]), fweights, unit
        return self

    def _searcher(self):
        return field_search(self._codes, self._gap, self._fweights)

    def _vote(self, buf, Lq, **options):
        ops.field_knn_logp(buf, Lq, self._lengths, self._y, self._prior, self.unit_, **options)


def split_audit(train, test, radius=2, top=50, judge=None, device=None, *, field_codes=None, gap=None, field_weights=None, max_len=None):
    """Do the rows of ``test`` have twins in ``train``?  One ``ops.edit_knn_rows`` pass with k = 1 (the held-out rows as queries, the
    train rows as references; in chunks where the pairs exceed the scratch cap), one download, then
    ``metrics.split_audit_report``: exact and near (<= ``radius`` edits, 0..64) duplicates, the ones whose twin carries ANOTHER
    label, the histogram of nearest distances, a per-class table and the ``top`` closest pairs.  Labels are the datasets' class
    indices, those of ``classes_`` (the target vocabulary's where there is one).  ``split_audit(train, train)`` -- the same object, or equal
    contents -- skips every row's own copy and audits the training set's own redundancy.  ``judge`` (any ``LogProbJudge``): adds
    ``accuracy_duplicated`` / ``accuracy_clean`` and ``rows_duplicated`` / ``rows_clean`` from ``judge.predict(test)``: how much
    of a reported accuracy sits on rows that have a twin in train (NaN where a side is empty).  Rows whose length lies outside
    0..64 are not audited: ``flagged_queries`` / ``flagged_references`` count them.  ``field_codes`` int [Vt, F] (with ``gap``,
    1..F; None: F): the audit runs under ``PhonoKNN``'s phonology-weighted distance instead -- distances and ``radius`` (0..64 F)
    are in field units, ``nearest_hist`` has 64 F + 2 bins, and a row that differs from a train row in one field of one frame is a
    near duplicate at ``radius=1``.  ``field_weights`` (with ``field_codes``; F integers in 0..16, their sum W in 1..16): the
    audit runs under ``PhonoKNN(field_weights=...)``'s metric -- ``gap`` in 1..W (None: W), ``radius`` (0..64 W) and
    ``nearest_hist`` (64 W + 2 bins) in units of W, ``max_distance`` 64 W -- so a row that differs from a train row only in fields
    of weight 0 is an exact duplicate.  ``max_len`` (None: the audit above, unchanged; an integer in 65..512): the unit-cost audit
    of rows of up to ``max_len`` frames through the multi-word search (csrc/edit_long.hip) -- ``radius`` lies in 0..max_len,
    ``nearest_hist`` has max_len + 2 bins, ``max_distance`` is max_len and only rows beyond max_len frames are flagged.  The
    phonology-weighted search is limited to 64 frames: ``max_len`` beside ``field_codes`` raises ValueError."""
    what = "split_audit"
    max_len = long_max_len(what, max_len)
    if max_len is not None and field_codes is not None:
        raise ValueError(f"{what}: max_len={max_len} with field_codes: the phonology-weighted search is limited to {_lib.EDIT_MAX_LEN} frames "
                         "(only the unit-cost audit takes max_len)")
    for name, ds in (("train", train), ("test", test)):
        if not isinstance(ds, TokenDataset) or len(ds) < 1:
            raise TypeError(f"{what}: {name} must be a non-empty slnlp.data.TokenDataset")
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
        for name, ds in (("train", train), ("test", test)):
            vocab = getattr(ds, "vocab_X", None)
            if vocab is not None and codes.shape[0] < len(vocab):
                raise ValueError(f"{what}: field_codes has {codes.shape[0]} rows, the source vocabulary of {name} {len(vocab)} tokens: the table "
                                 "must cover the vocabulary")
    elif gap is not None:
        raise ValueError(f"{what}: gap={gap!r} without field_codes: the unit-cost distance has no gap cost")
    bound = _lib.EDIT_MAX_LEN * unit if max_len is None else max_len
    radius = ops._int_in(what, "radius", radius, 0, bound)
    top = ops._int_in(what, "top", top, 0, 2 ** 31 - 1)
    if judge is not None and not isinstance(judge, LogProbJudge):
        raise TypeError(f"{what}: judge must be a LogProbJudge (a fit, an ensemble, an EditKNN), got {type(judge).__name__}")
    dev = _cuda_device(device)
    _lib.require_gpu()
    own = test is train or (len(test) == len(train) and np.array_equal(test.ids, train.ids) and np.array_equal(test.lengths, train.lengths)
                            and np.array_equal(test.y, train.y))
    got = []

    def body():
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        Xr, Lr = up(train.ids), up(train.lengths)
        Xq, Lq = (Xr, Lr) if own else (up(test.ids), up(test.lengths))
        exclude = up(np.arange(len(train), dtype=np.int64)) if own else None
        _search(Xq, Lq, Xr, Lr, 1, radius, exclude, lambda a, b, buf: got.append({n: v.copy() for n, v in ops.edit_knn_download(buf).items()}),
                search=unit_search(max_len) if codes is None else field_search(up(codes), gap, fweights))
    _on_stream(dev, body)
    rows, nbr = np.concatenate([g["rows"] for g in got]), np.concatenate([g["nbr"] for g in got])
    head = got[0]["head"].copy()
    head[0] = sum(int(g["head"][0]) for g in got)            # the queries of every chunk; the references are the same in each
    res = metrics.split_audit_report(rows, nbr, np.asarray(test.y), np.asarray(train.y), radius, top, head=head, max_distance=bound)
    res["self"] = bool(own)
    if judge is not None:
        right = np.asarray(judge.predict(test)) == np.asarray(test.y)
        dup = res["duplicated"]
        res.update(rows_duplicated=int(dup.sum()), rows_clean=int((~dup).sum()),
                   accuracy_duplicated=float(right[dup].mean()) if dup.any() else float("nan"),
                   accuracy_clean=float(right[~dup].mean()) if (~dup).any() else float("nan"), accuracy=float(right.mean()))
    return res
