"""The numpy restatement of ``slnlp_train_dynamics_reset`` / ``slnlp_train_dynamics_epoch`` (include/slnlp.h): a fit's training
dynamics -- dataset cartography (Swayamdipta et al. 2020), forgetting events (Toneva et al. 2019), area under the margin (Pleiss
et al. 2020) -- as integers per train row.  Test infrastructure only.

One epoch: z float32 log-probs [n_visit, V] in visit order, y int64 [n_visit] the labels in visit order, order int64 [n_visit]
the dataset row r of every visit (None: r = i), N dataset rows.  Per visit: code -3 for r outside [0, N) (first), -2 for a NaN or a
maximum that is not finite, -1 for a label outside [0, V), else 0; pred the arg-max (a NaN first, larger float32 value first, equal
values by ascending column); correct = (pred == y); q = rint(min(p, 1) 2^20) with p the label's probability on the row head of
label_audit_ref (1 / s0 at the maximum, exp(z - zmax) / s0 elsewhere, fp64); mq = rint(clip(z_y - z_other, -1024, 1024) 2^20) with
`other` the first column other than the label in the arg-max's order, 0 for V = 1.  A usable visit adds into its row; ``fold``
closes the epoch per row."""
import numpy as np

FRAC = 1 << 20
MARGIN_MAX = 1024.0
VISIT_LIMIT = 1 << 23
ROW_INTS = ("visits", "correct_visits", "epochs_seen", "epochs_correct", "forgetting", "first_learned", "last")
HEAD = ("epochs", "visits", "bad_labels", "nan_rows", "bad_rows", "rows_seen", "overflow")


def visits_ref(z, y, order, N):
    """The per-visit values of one epoch: {code, pred, correct, q, mq} int64 [n_visit] and ``row`` (order, or 0 .. n_visit - 1)."""
    z = np.asarray(z, dtype=np.float32)
    y = np.asarray(y).astype(np.int64)
    n, V = z.shape
    row = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    zz = z.astype(np.float64)
    with np.errstate(all="ignore"):
        pred = np.argmax(z, axis=1).astype(np.int64)         # a NaN first, then the first maximum
        zmax = zz.max(axis=1)
        bad = ~np.isfinite(zmax) | np.isnan(zz).any(axis=1)
        at_max = zz == zmax[:, None]
        e = np.where(at_max, 0.0, np.exp(zz - zmax[:, None]))
        s0 = 1.0 + (e.sum(axis=1) + (at_max.sum(axis=1) - 1.0))
        P = np.where(at_max, (1.0 / s0)[:, None], e / s0[:, None])
    code = np.where((row < 0) | (row >= N), -3, np.where(bad, -2, np.where((y < 0) | (y >= V), -1, 0))).astype(np.int64)
    usable = code == 0
    label = np.where(usable, y, 0)
    at = np.arange(n)
    with np.errstate(all="ignore"):
        p = np.where(usable, P[at, label], 0.0)
        q = np.where(usable, np.rint(np.minimum(p, 1.0) * FRAC), 0.0).astype(np.int64)
        rest = np.where(np.arange(V)[None, :] == label[:, None], np.float32(-np.inf), z)     # the row without its label
        other = rest.astype(np.float64).max(axis=1)          # the value of the first column other than the label: the largest
        margin = zz[at, label] - other if V > 1 else np.zeros(n)    # of the rest (usable rows hold no NaN); -inf when none is finite
        margin = np.where(usable, margin, 0.0)               # (an unusable row's difference may be a NaN: never looked at)
        mq = np.rint(np.clip(margin, -MARGIN_MAX, MARGIN_MAX) * FRAC).astype(np.int64)
    correct = (usable & (pred == y)).astype(np.int64)
    return {"code": code, "pred": pred, "correct": correct, "q": q, "mq": mq, "row": row}


def new_state(N):
    st = {name: np.zeros(N, dtype=np.int64) for name in ("sum_q", "sum_q2", "sum_mq") + ROW_INTS}
    st["first_learned"][:] = -1
    st["last"][:] = -1
    st["head"] = np.zeros(8, dtype=np.int64)
    return st


def fold(st, vis, epoch):
    """Add one epoch's per-visit values ``vis`` ({code, correct, q, mq, row}: ``visits_ref``'s, or the device's own with the row
    of every visit) to the state ``st`` in integers and close the epoch per row.  Returns ``st``."""
    N = st["visits"].size
    code = np.asarray(vis["code"]).astype(np.int64)
    use = code == 0
    r = np.asarray(vis["row"]).astype(np.int64)[use]
    q, mq = np.asarray(vis["q"]).astype(np.int64)[use], np.asarray(vis["mq"]).astype(np.int64)[use]
    v_e, c_e = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    np.add.at(v_e, r, 1)
    np.add.at(c_e, r, np.asarray(vis["correct"]).astype(np.int64)[use])
    np.add.at(st["sum_q"], r, q)
    np.add.at(st["sum_q2"], r, q * q)
    np.add.at(st["sum_mq"], r, mq)
    seen = v_e > 0
    a = seen & (c_e == v_e)                                  # right at every visit of the epoch
    st["head"][5] += int((seen & (st["last"] == -1)).sum())
    st["visits"] += v_e
    st["correct_visits"] += c_e
    st["epochs_seen"] += seen
    st["epochs_correct"] += a
    st["forgetting"] += seen & (st["last"] == 1) & ~a
    st["first_learned"][a & (st["first_learned"] == -1)] = epoch
    st["last"][seen] = a[seen]
    st["head"][0] += 1
    st["head"][1] += int(use.sum())
    st["head"][2] += int((code == -1).sum())
    st["head"][3] += int((code == -2).sum())
    st["head"][4] += int((code == -3).sum())
    st["head"][6] |= int((seen & (st["visits"] >= VISIT_LIMIT)).any())
    return st


def epoch_ref(st, z, y, order, epoch):
    """One ``slnlp_train_dynamics_epoch`` call on the state ``st``.  Returns (``st``, the per-visit values)."""
    vis = visits_ref(z, y, order, st["visits"].size)
    return fold(st, vis, epoch), vis


def record_of(st):
    """The state as ``ops.train_dynamics_download``'s dict, for ``metrics.train_dynamics_report``."""
    out = {name: st[name].copy() for name in ("head", "sum_q", "sum_q2", "sum_mq")}
    out.update({name: st[name].astype(np.int32) for name in ROW_INTS})
    return out
