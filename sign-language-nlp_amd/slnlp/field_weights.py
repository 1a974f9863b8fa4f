"""Per-field integer weights of ``PhonoKNN``'s metric, fitted on the device by leave-one-out.

``PhonoKNN`` counts every phonological field 1 when it substitutes one frame for another.  ``fit_field_weights`` replaces that
constant by a cyclic coordinate search over small integer weights: a candidate weight vector is judged by the leave-one-out
log-probs of the train rows under it -- one search, one vote and one ``ops.loo_objective`` launch, nothing of which waits for the
host -- and the candidates of one field fill one device table that is downloaded once.  ``coordinate_search`` is the host side
of it, over any evaluator (tests/field_weight_ref.py restates it)."""
import copy
import math

import numpy as np

from . import _lib, ops

SCORINGS = ("neg_log_loss", "accuracy")
MAX_WEIGHT = _lib.FIELD_MAX_WEIGHT


def search_options(what, F, levels, sweeps, scoring, start):
    """The options of the search checked: ``levels`` a non-empty sequence of distinct integers in 0..16, ``sweeps`` an integer in
    1..64, ``scoring`` "neg_log_loss" or "accuracy", ``start`` None (all ones) or F integers in 0..16 whose sum lies in 1..16 ->
    (levels as a tuple, sweeps, scoring, start as a tuple); anything else raises ValueError"""
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    try:
        lv = list(levels)
    except TypeError:
        lv = []
    if not lv or not all(whole(v) and 0 <= v <= MAX_WEIGHT for v in lv) or len(set(int(v) for v in lv)) != len(lv):
        raise ValueError(f"{what}: levels={levels!r}, expected distinct integers in 0..{MAX_WEIGHT}")
    sweeps = ops._int_in(what, "sweeps", sweeps, 1, 64)
    if scoring not in SCORINGS:
        raise ValueError(f"{what}: scoring={scoring!r}, expected one of {SCORINGS}")
    if start is None:
        start = (1,) * F
    try:
        st = list(start)
    except TypeError:
        st = []
    if len(st) != F or not all(whole(v) and 0 <= v <= MAX_WEIGHT for v in st) or not 1 <= sum(int(v) for v in st) <= MAX_WEIGHT:
        raise ValueError(f"{what}: start={start!r}, expected {F} integers in 0..{MAX_WEIGHT} whose sum lies in 1..{MAX_WEIGHT}")
    return tuple(int(v) for v in lv), sweeps, scoring, tuple(int(v) for v in st)


def rank_key(scoring, weights, right, total):
    """What the candidates of a step are ordered by, smallest first: the objective -- the lower fp64 sum for "neg_log_loss", the
    higher count for "accuracy" -- then the smaller W, then the lexicographically smaller vector.  Exact comparisons."""
    return (float(total) if scoring == "neg_log_loss" else -int(right), sum(weights), tuple(weights))


def coordinate_search(F, evaluate, levels=(0, 1, 2, 4), sweeps=2, scoring="neg_log_loss", start=None, reduce=True, least=1):
    """Cyclic coordinate search over integer weight vectors.  ``evaluate(field, candidates)`` -> [(rows right, sum of -logp), ...]
    for a list of weight tuples (``field`` None: the start alone).  For field f = 0..F-1 every level is tried for w_f with the
    others fixed -- candidates whose sum W lies outside ``least``..16 are skipped, the present vector is always among them -- and the best
    by ``rank_key`` is taken; after ``sweeps`` sweeps, or a sweep that changed nothing, it stops.  ``reduce``: the result is
    divided by the gcd of its weights (c w with gap c W is the same metric).  Returns the report of ``fit_field_weights`` without
    ``rows``."""
    levels, sweeps, scoring, w = search_options("coordinate_search", F, levels, sweeps, scoring, start)
    (right, total), = evaluate(None, [w])
    trace = [{"field": None, "weights": w, "right": int(right), "sum": float(total)}]
    start_right, start_sum = int(right), float(total)
    sweeps_run, converged, steps = 0, False, []
    for _ in range(sweeps):
        changed = False
        for f in range(F):
            values = list(levels) + ([] if w[f] in levels else [w[f]])
            cands = [w[:f] + (v,) + w[f + 1:] for v in values]
            cands = [c for c in cands if least <= sum(c) <= MAX_WEIGHT]
            got = evaluate(f, cands)
            for c, (r, s) in zip(cands, got):
                trace.append({"field": f, "weights": c, "right": int(r), "sum": float(s)})
            best = min(range(len(cands)), key=lambda i: rank_key(scoring, cands[i], got[i][0], got[i][1]))
            changed |= cands[best] != w
            w, right, total = cands[best], int(got[best][0]), float(got[best][1])
            steps.append(w)
        sweeps_run += 1
        if not changed:
            converged = True
            break
    g = 0
    for v in w:
        g = math.gcd(g, v)
    objective = lambda r, s: -s if scoring == "neg_log_loss" else r
    return {"weights": tuple(v // g for v in w) if reduce else w, "weights_unreduced": w, "scoring": scoring,
            "start_objective": objective(start_right, start_sum), "objective": objective(right, total), "rows_right": right, "sum": total,
            "trace": trace, "steps": steps, "evaluations": len(trace), "sweeps_run": sweeps_run, "converged": converged}


def fit_field_weights(train, field_codes, levels=(0, 1, 2, 4), sweeps=2, scoring="neg_log_loss", start=None, gap=None, **knn_options):
    """Per-field integer weights for ``PhonoKNN(field_codes, field_weights=...)`` by cyclic coordinate search on the leave-one-out
    objective of ``PhonoKNN(field_weights=w, **knn_options).fit(train).leave_one_out()``: start at all ones (or ``start``); for
    field f = 0..F-1 try every level of ``levels`` for w_f with the others fixed (candidates whose sum W lies outside 1..16 are
    skipped) and keep the best -- ``scoring="neg_log_loss"``: the lower fp64 sum of -logp[i, y_i]; ``"accuracy"``: the more rows
    right; ties to the smaller W, then to the lexicographically smaller vector, compared exactly on the device's own values --
    and stop after ``sweeps`` sweeps or a sweep that changed nothing.  ``gap`` None: W for every candidate, and the result is
    divided by the gcd of its weights (c w with gap c W is the same metric); an integer: that gap for every candidate (those
    with W below it are skipped) and no division.

    The train rows and the code table are uploaded once.  The candidates of one field are queued back to back on the fit stream
    under the shared device gate -- a search, a vote and ``ops.loo_objective`` into the candidate's own slot each -- and the table
    is downloaded ONCE per field step.

    Returns {``weights``, ``weights_unreduced``, ``scoring``, ``start_objective``, ``objective`` (the negated sum of -logp, or
    the rows right), ``rows_right``, ``rows``, ``sum``, ``trace`` (every evaluated {field, weights, right, sum} in order; field
    None: the start), ``steps`` (the vector behind every field step), ``evaluations``, ``sweeps_run``, ``converged``, ``gap``}.

    WHAT THE NUMBER IS.  It is leave-one-out on the TRAIN split.  This data holds the same gloss signed several times, so a row's
    twins sit among its references and flatter every candidate: ``split_audit(train, train)`` counts them.  Judge the weights on
    held-out rows: ``net.compare(knn, test)`` / ``knn.score_interval(test)`` of the ``PhonoKNN`` fitted with them does that."""
    from .edit_knn import PhonoKNN, field_table, knn_options as check_knn
    what = "fit_field_weights"
    codes, _ = field_table(what, field_codes, None)
    F = int(codes.shape[1])
    levels, sweeps, scoring, w0 = search_options(what, F, levels, sweeps, scoring, start)
    if gap is not None:
        gap = ops._int_in(what, "gap", gap, 1, MAX_WEIGHT)
        if sum(w0) < gap:
            raise ValueError(f"{what}: gap={gap} exceeds the start's W={sum(w0)}")
    unknown = sorted(set(knn_options) - {"k", "weights", "tau", "normalize", "smoothing", "device"})
    if unknown:
        raise ValueError(f"{what}: unknown options {unknown} (known: k, weights, tau, normalize, smoothing, device)")
    base = PhonoKNN(codes, gap=gap, field_weights=w0, **knn_options).fit(train)
    loo = base.leave_one_out()
    options = check_knn("PhonoKNN", base.k, base.weights, base.tau, base.normalize, base.smoothing)
    dev = loo._ids.device

    def evaluate(field, cands):
        def body():
            table = ops.loo_objective_table(len(cands), dev)
            for slot, c in enumerate(cands):
                sib = copy.copy(loo)
                sib._fweights, sib.unit_, sib._gap = tuple(c), sum(c), sum(c) if gap is None else gap
                logp, y = sib._queue_logp(train, *options)
                ops.loo_objective(logp, y, table, slot)
            return ops.loo_objective_download(table)
        got = loo._on_stream(body)
        return [(int(r), float(s)) for r, s in zip(got["right"], got["sum"])]

    res = coordinate_search(F, evaluate, levels, sweeps, scoring, w0, reduce=gap is None, least=1 if gap is None else gap)
    res.update(rows=int(base.rows_), gap=gap)
    return res
