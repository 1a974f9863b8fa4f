"""numpy fp64 restatement of csrc/reliability.hip (``slnlp_reliability_rows``; include/slnlp.h states the definition), line by
line on top of ``calibration_ref._shifted``: the per-row terms, the reliability table in the DEVICE'S summation order (so a table
can be compared bit for bit with one made from the same rows) and the scores formed from a table.  What differs from the device
in the row terms is only the order of the sums over the columns and numpy's exp / log."""
import numpy as np

from calibration_ref import _shifted

MAX_BINS = 64


def bin_of(conf, bins):
    """The bin of a stored confidence: equal-width, right-closed bins (b / B, (b + 1) / B], clamped into 0 .. B - 1."""
    return np.clip(np.ceil(np.asarray(conf, dtype=np.float64) * bins) - 1.0, 0.0, bins - 1.0)


def rows_ref(logp, y, bins, beta=1.0):
    """rows float64 [N, 4] = (conf, brier, nll, code) of ``logp`` float32 [N, V] and ``y`` integer [N] at softmax(beta logp)."""
    logp, y = np.asarray(logp), np.asarray(y).astype(np.int64)
    assert logp.dtype == np.float32 and logp.ndim == 2 and y.shape == (logp.shape[0],) and 1 <= bins <= MAX_BINS
    N, V = logp.shape
    z = logp.astype(np.float64)
    bad = (y < 0) | (y >= V)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        zm = z.max(axis=1, keepdims=True)                   # (a NaN in the row makes it NaN)
        broken = ~bad & ~np.isfinite(zm[:, 0])
        a, e, rest = _shifted(z, beta)
        at_max = z == zm
        k = at_max.sum(axis=1)
        s0 = 1.0 + rest
        pred = np.argmax(logp, axis=1)                      # the first maximum of the float32 values
        by = beta * z[np.arange(N), np.where(bad, 0, y)] - a[:, 0]
        rows = np.zeros((N, 4))
        rows[:, 0] = 1.0 / s0
        rows[:, 1] = (k + np.where(at_max, 0.0, e * e).sum(axis=1)) / (s0 * s0) - 2.0 * np.exp(by) / s0 + 1.0
        rows[:, 2] = np.log1p(rest) - by
        rows[:, 3] = 2.0 * bin_of(rows[:, 0], bins) + (pred == y)
    rows[bad] = (0.0, 0.0, 0.0, -1.0)
    rows[broken] = (np.nan, np.nan, np.nan, -2.0)
    return rows


def _block_sum(values):
    """One block's sum of ``values`` [N] (0.0 where a row does not belong to the block) in the device's order: thread t adds rows
    t, t + 256, ... in increasing order, then the binary tree w = 128 ... 1 over the 256 partial sums."""
    n = len(values)
    padded = np.zeros(((n + 255) // 256) * 256)
    padded[:n] = values
    acc = np.zeros(256)
    for chunk in padded.reshape(-1, 256):
        acc = acc + chunk
    w = 128
    while w >= 1:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w >>= 1
    return acc[0]


def table_ref(rows, bins):
    """table float64 [bins + 1, 4] of ``rows`` [N, 4], summed exactly as ``reliability_table`` sums."""
    rows = np.asarray(rows, dtype=np.float64)
    code = np.where(np.isnan(rows[:, 3]), -2, rows[:, 3]).astype(np.int64)
    scored = code >= 0
    table = np.zeros((bins + 1, 4))
    for b in range(bins):
        mine = scored & ((code >> 1) == b)
        table[b, 0] = _block_sum(np.where(mine, 1.0, 0.0))
        table[b, 1] = _block_sum(np.where(mine, rows[:, 0], 0.0))
        table[b, 2] = _block_sum(np.where(mine, (code & 1).astype(np.float64), 0.0))
    table[bins, 0] = _block_sum(np.where(scored, rows[:, 1], 0.0))
    table[bins, 1] = _block_sum(np.where(scored, rows[:, 2], 0.0))
    table[bins, 2] = _block_sum(np.where(code == -1, 1.0, 0.0))
    table[bins, 3] = _block_sum(np.where(code == -2, 1.0, 0.0))
    return table


def summary_ref(table):
    """The scores of a table, as the issue defines them: M = sum of the counts; ece = sum_b |sum_correct_b - sum_conf_b| / M; mce
    = max over the non-empty bins of |accuracy_b - confidence_b|; brier, nll, accuracy, confidence = means over M.  Any NaN row
    makes ece, mce, brier and nll NaN."""
    bins = len(table) - 1
    M = sum(table[b][0] for b in range(bins))
    out = {"rows": int(M), "bad_labels": int(table[bins][2]), "nan_rows": int(table[bins][3])}
    gaps = [abs(table[b][2] / table[b][0] - table[b][1] / table[b][0]) for b in range(bins) if table[b][0] > 0]
    out["ece"] = sum(abs(table[b][2] - table[b][1]) for b in range(bins)) / M if M else float("nan")
    out["mce"] = max(gaps) if gaps else float("nan")
    out["brier"] = table[bins][0] / M if M else float("nan")
    out["nll"] = table[bins][1] / M if M else float("nan")
    out["accuracy"] = sum(table[b][2] for b in range(bins)) / M if M else float("nan")
    out["confidence"] = sum(table[b][1] for b in range(bins)) / M if M else float("nan")
    if out["nan_rows"]:
        out.update(ece=float("nan"), mce=float("nan"), brier=float("nan"), nll=float("nan"))
    return {k: (v if isinstance(v, int) else float(v)) for k, v in out.items()}


def reliability_ref(logp, y, bins=15, beta=1.0):
    """``summary_ref`` of the restated rows and table: what ``ops.reliability_download(ops.reliability_rows(...))`` holds."""
    return summary_ref(table_ref(rows_ref(logp, y, bins, beta), bins))
