"""The numpy fp64 restatement of occlusion attribution (include/slnlp.h: slnlp_occlude_rows, slnlp_attribution_rows,
slnlp_attribution_summary; slnlp.ops.occlusion_variants), step by step.  Test infrastructure only.

1. ``variants_ref``: the table (row, unit, bin) sorted by (row, unit) and the rows' offsets.  len = clamp(L, 0, S); "mask" / "drop":
   the windows [u stride, min(u stride + width, len)) with u stride < len, bin = min(bins - 1, (bins (lo + hi)) // (2 len));
   "field": one unit per field for a row with len >= 1, bin = unit.
2. ``occlude_ref``: the variants' inputs.  MASK: the window becomes unk.  DROP: the window is deleted and the rest closes up; a
   window over the whole row is masked.  SUBSTITUTE: token v becomes sub[v, unit] when 0 <= v < Vx.  The tail is pad.  An invalid
   variant (row outside [0, n), unit < 0, a window starting at or behind len, a field outside [0, F), len 0) is all pad with length 0
   and label 0.
3. ``rows_ref``: per variant, with the row head of both rows in fp64 -- zmax, a = beta zmax, e_k = exp(beta z_k - a) away from the
   maximum, rest = sum e + (n_max - 1), s0 = 1 + rest, p(k) = 1 / s0 at the maximum and e_k / s0 elsewhere, lp(k) = (beta z_k - a) -
   log1p(rest) -- drop = lp_b(c) - lp_v(c), dp = p_b(c) - p_v(c), kl = fsum of p_b(k) (lp_b(k) - lp_v(k)) over p_b(k) > 0; the
   variant's arg-max and the code: -3 invalid (first), -2 a NaN or no finite maximum in either row, -1 a label outside [0, V), 0.
4. ``summary_ref``: per row the base arg-max, target, code, usable variants, flips, top_unit (largest finite drop, ties to the smaller
   unit), lp_b(c), top_drop, min_drop, sum_drop (``math.fsum``); the (target class, bin) table of count (finite drop and kl), flips,
   nonfinite, and the ``math.fsum`` of drop and of kl; the head."""
import math

import numpy as np

KINDS = {"mask": 0, "drop": 1, "substitute": 2}
NAN = float("nan")


def variants_ref(lengths, S, by, width=1, stride=1, bins=8, n_fields=None):
    out, start = [], [0]
    for i, L in enumerate(np.asarray(lengths).tolist()):
        ln = min(max(int(L), 0), S)
        if by == "field":
            out += [(i, u, u) for u in range(n_fields if ln >= 1 else 0)]
        else:
            u = 0
            while u * stride < ln:
                lo, hi = u * stride, min(u * stride + width, ln)
                out.append((i, u, min(bins - 1, (bins * (lo + hi)) // (2 * ln))))
                u += 1
        start.append(len(out))
    return np.array(out, dtype=np.int32).reshape(-1, 3), np.array(start, dtype=np.int32), (n_fields if by == "field" else bins)


def occlude_ref(X, L, y, variants, kind, width=1, stride=1, pad=1, unk=0, sub=None):
    X, L, y = np.asarray(X, dtype=np.int64), np.asarray(L, dtype=np.int64), np.asarray(y, dtype=np.int64)
    n, S = X.shape
    M = len(variants)
    Xo, Lo, yo = np.full((M, S), pad, dtype=np.int64), np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    for j, (row, unit, _) in enumerate(np.asarray(variants).tolist()):
        if not 0 <= row < n:
            continue
        ln = min(max(int(L[row]), 0), S)
        if kind == "substitute":
            if not (0 <= unit < sub.shape[1] and ln >= 1):
                continue
            src = X[row, :ln]
            inside = (src >= 0) & (src < sub.shape[0])
            new = np.where(inside, sub[np.where(inside, src, 0), unit], src)
        else:
            lo = unit * stride
            if unit < 0 or lo >= ln:
                continue
            hi = min(lo + width, ln)
            src = X[row, :ln]
            if kind == "mask" or (lo == 0 and hi == ln):
                new = src.copy()
                new[lo:hi] = unk
            else:
                new = np.concatenate([src[:lo], src[hi:]])
        Xo[j, :len(new)] = new
        Lo[j], yo[j] = len(new), y[row]
    return Xo, Lo, yo


def row_head(z, beta):
    """(pred, finite, p float64 [V], lp float64 [V]) of one float32 row; p and lp are None for a row without a softmax."""
    z = np.asarray(z, dtype=np.float32)
    zz = z.astype(np.float64)
    pred = int(np.argmax(z))                                 # a NaN first, then the first maximum
    zmax = zz[pred]
    if not np.isfinite(zmax):
        return pred, False, None, None
    with np.errstate(all="ignore"):
        at = zz == zmax
        t = beta * zz - beta * zmax
        e = np.where(at, 0.0, np.exp(t))
        rest = math.fsum(e) + (float(at.sum()) - 1.0)
        s0 = 1.0 + rest
        return pred, True, np.where(at, 1.0 / s0, e / s0), t - math.log1p(rest)


def rows_ref(base, var, y, variants, target, beta=1.0):
    """``var`` float32 [M, V]: row j belongs to variant j.  -> vals float64 [M, 3], ints int64 [M, 2]."""
    N, V = base.shape
    heads = {}
    vals, ints = np.full((len(variants), 3), NAN), np.zeros((len(variants), 2), dtype=np.int64)
    for j, (row, _, _) in enumerate(np.asarray(variants).tolist()):
        if not 0 <= row < N:
            ints[j] = (-1, -3)
            continue
        if row not in heads:
            heads[row] = row_head(base[row], beta)
        pb_, fb, pb, lb = heads[row]
        pv_, fv, pv, lv = row_head(var[j], beta)
        ints[j, 0] = pv_
        if not (fb and fv):
            ints[j, 1] = -2
            continue
        c = pb_
        if target == "label":
            if not 0 <= int(y[row]) < V:
                ints[j, 1] = -1
                continue
            c = int(y[row])
        with np.errstate(all="ignore"):
            on = pb > 0.0
            vals[j] = (lb[c] - lv[c], pb[c] - pv[c], math.fsum((pb[on] * (lb[on] - lv[on])).tolist()))
    return vals, ints


def summary_ref(base, y, variants, row_start, n_bins, target, beta, vals, ints):
    """The summary of a finished table (``vals`` / ``ints``: the restatement's or the device's own) as ``ops.attribution_download``'s
    dict, plus ``row_terms`` / ``cell_terms``: per row and per cell (n, sum |term|) of the float sums, for the tests' bounds."""
    N, V = base.shape
    variants = np.asarray(variants)
    M = len(variants)
    rows_i, rows_d = np.zeros((N, 6), dtype=np.int64), np.full((N, 4), NAN)
    row_terms = np.zeros((N, 2))
    for r in range(N):
        pred, fin, p, lp = row_head(base[r], beta)
        code, c = 0, -1
        if not fin:
            code = -2
        elif target == "label":
            if 0 <= int(y[r]) < V:
                c = int(y[r])
            else:
                code = -1
        else:
            c = pred
        s, e = min(max(int(row_start[r]), 0), M), min(max(int(row_start[r + 1]), 0), M)
        mine = [q for q in range(s, max(s, e)) if variants[q, 0] == r and ints[q, 1] == 0]
        drops = [(float(vals[q, 0]), int(variants[q, 1])) for q in mine if np.isfinite(vals[q, 0])]
        top = min(drops, key=lambda du: (-du[0], du[1])) if drops else None
        rows_i[r] = (pred, c, code, len(mine), sum(1 for q in mine if ints[q, 0] != pred), top[1] if top else -1)
        rows_d[r] = (lp[c] if code == 0 else NAN, top[0] if top else NAN, min(d for d, _ in drops) if drops else NAN,
                     math.fsum(d for d, _ in drops))
        row_terms[r] = (len(drops), math.fsum(abs(d) for d, _ in drops))
    table_i, table_d = np.zeros((V, n_bins, 3), dtype=np.int64), np.zeros((V, n_bins, 2))
    cell_terms = np.zeros((V, n_bins, 3))                    # n, sum |drop|, sum |kl|
    members = {}
    for q in range(M):
        row, _, b = variants[q].tolist()
        if ints[q, 1] == 0 and 0 <= row < N and 0 <= b < n_bins and rows_i[row, 1] >= 0:
            members.setdefault((int(rows_i[row, 1]), b), []).append(q)
    for (c, b), qs in members.items():
        fin = [q for q in qs if np.isfinite(vals[q, 0]) and np.isfinite(vals[q, 2])]
        table_i[c, b] = (len(fin), sum(1 for q in qs if ints[q, 0] != rows_i[variants[q, 0], 0]), len(qs) - len(fin))
        table_d[c, b] = (math.fsum(vals[fin, 0].tolist()), math.fsum(vals[fin, 2].tolist()))
        cell_terms[c, b] = (len(fin), math.fsum(np.abs(vals[fin, 0]).tolist()), math.fsum(np.abs(vals[fin, 2]).tolist()))
    code = ints[:, 1]
    flips = sum(1 for q in range(M) if code[q] == 0 and 0 <= variants[q, 0] < N and ints[q, 0] != rows_i[variants[q, 0], 0])
    head = np.array([(code == 0).sum(), (code == -1).sum(), (code == -2).sum(), ((code != 0) & (code != -1) & (code != -2)).sum(), flips,
                     0, 0, 0], dtype=np.int64)
    return {"head": head, "table_i": table_i, "table_d": table_d, "rows_i": rows_i, "rows_d": rows_d, "row_terms": row_terms,
            "cell_terms": cell_terms}


def attribution_ref(base, var, y, variants, row_start, n_bins, target, beta=1.0):
    """Steps 3 and 4 on given log-probs: ``summary_ref``'s dict plus ``vals`` and ``ints``."""
    vals, ints = rows_ref(base, var, y, variants, target, beta)
    out = summary_ref(base, y, variants, row_start, n_bins, target, beta, vals, ints)
    out.update(vals=vals, ints=ints)
    return out


def smallest_drop_gap(variants, vals, ints):
    """The least distance between two finite drops of usable variants of one row (inf when no row has two)."""
    variants = np.asarray(variants)
    gap = float("inf")
    for r in np.unique(variants[:, 0]):
        d = np.sort(vals[(variants[:, 0] == r) & (ints[:, 1] == 0), 0])
        d = d[np.isfinite(d)]
        if d.size > 1:
            gap = min(gap, float(np.diff(d).min()))
    return gap
