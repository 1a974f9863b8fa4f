"""numpy fp64 restatement of csrc/calibration.hip (``slnlp_fit_temperature`` / ``slnlp_scale_logp``; include/slnlp.h states the
algorithm): the same end-point tests and the same safeguarded Newton iteration in ln(beta), line by line -- not a call to a
library optimiser.  What differs from the device is only the order of the sums and numpy's exp / log."""
import numpy as np

BETA_MIN, BETA_MAX, ITERS = 2.0 ** -6, 2.0 ** 6, 32
GRAD_TOL, STEP_TOL = 2.0 ** -44, 2.0 ** -40


def evaluate(z, y, beta):
    """(f, g, h, s) at ``beta``: the means over the rows of ``z`` float64 [M, V] (labels ``y`` all inside the columns)."""
    a, e, rest = _shifted(z, beta)
    s0 = 1.0 + rest
    mean = (e * z).sum(axis=1) / s0
    zy = z[np.arange(len(y)), y]
    f = np.log1p(rest) - (beta * zy - a[:, 0])
    g = mean - zy
    h = (e * z * z).sum(axis=1) / s0 - mean * mean
    s = np.abs(mean) + np.abs(zy)
    return float(f.mean()), float(g.mean()), float(h.mean()), float(s.mean())


def _shifted(z, beta):
    """(a, e, rest) per row: a = max of beta z [N, 1], e = exp(beta z - a), rest = sum e - 1 -- the columns at the maximum (e = 1
    exactly) are counted, not summed, so that log1p(rest) keeps the digits of a confident row, as the device does."""
    zm = z.max(axis=1, keepdims=True)
    a = beta * zm
    e = np.exp(beta * z - a)
    at_max = z == zm
    return a, e, np.where(at_max, 0.0, e).sum(axis=1) + (at_max.sum(axis=1) - 1.0)


def newton_step(logp, y, beta):
    """|g / (g + beta h)| at ``beta``: the size of the Newton step in ln(beta) the iteration would take from there."""
    z, y = _rows(logp, y)[:2]
    _, g, h, _ = evaluate(z, y, beta)
    return abs(g / (g + beta * h))


def _rows(logp, y):
    logp, y = np.asarray(logp), np.asarray(y).astype(np.int64)
    assert logp.dtype == np.float32 and logp.ndim == 2 and y.shape == (logp.shape[0],)
    ok = (y >= 0) & (y < logp.shape[1])
    return logp[ok].astype(np.float64), y[ok], int((~ok).sum())


def _search(z, y):
    """(beta, reason, iterations)."""
    _, g, _, s = evaluate(z, y, BETA_MIN)
    if abs(g) <= GRAD_TOL * s:
        _, g1, _, s1 = evaluate(z, y, 1.0)
        if abs(g1) <= GRAD_TOL * s1:
            return 1.0, "flat", 0
    if g >= 0.0:
        return BETA_MIN, "bound", 0
    _, g, _, _ = evaluate(z, y, BETA_MAX)
    if g <= 0.0:
        return BETA_MAX, "bound", 0
    lo, hi, beta = BETA_MIN, BETA_MAX, 1.0
    for it in range(1, ITERS + 1):
        _, g, h, s = evaluate(z, y, beta)
        if abs(g) <= GRAD_TOL * s:
            return beta, "gradient", it
        if g < 0.0:
            lo = beta
        else:
            hi = beta
        den = g + beta * h
        nxt = beta * np.exp(-g / den) if den > 0.0 else 0.0
        if not lo < nxt < hi:
            nxt = np.sqrt(lo * hi)
        if abs(np.log(nxt / beta)) <= STEP_TOL:
            return float(nxt), "step", it
        beta = float(nxt)
    return beta, "cap", ITERS


def fit_temperature_ref(logp, y):
    """``ops.temperature_download(ops.fit_temperature(logp, y))`` on the host: ``logp`` float32 [N, V], ``y`` integer [N]."""
    z, yk, bad = _rows(logp, y)
    if len(yk) == 0:
        return {"temperature": 1.0, "beta": 1.0, "nll_before": 0.0, "nll_after": 0.0, "reason": "flat", "iterations": 0, "rows": 0,
                "bad_labels": bad}
    beta, reason, iterations = _search(z, yk)
    return {"temperature": 1.0 / beta, "beta": beta, "nll_before": evaluate(z, yk, 1.0)[0], "nll_after": evaluate(z, yk, beta)[0],
            "reason": reason, "iterations": iterations, "rows": len(yk), "bad_labels": bad}


def scale_logp_ref(logp, beta):
    """The calibrated log-probs beta z - logsumexp(beta z) per row, float64 [N, V] (the device rounds them once to float32)."""
    z = np.asarray(logp).astype(np.float64)
    a, _, rest = _shifted(z, beta)
    return (beta * z - a) - np.log1p(rest)[:, None]
