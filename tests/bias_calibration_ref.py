"""numpy fp64 restatement of csrc/bias_calibration.hip (``slnlp_fit_bias_temperature``; include/slnlp.h states the algorithm): the
same objective, the same damped Newton iteration on the dense (V + 1) x (V + 1) system with the same right-looking Cholesky, the
same Armijo test and the same evaluation count, line by line -- not a call to a library optimiser.  What differs from the device
is only the order of the sums and numpy's exp / log."""
import numpy as np

BETA_MIN, BETA_MAX, EVALS, ARMIJO = 2.0 ** -6, 2.0 ** 6, 48, 1e-4


def _rows(logp, y):
    logp, y = np.asarray(logp), np.asarray(y).astype(np.int64)
    assert logp.dtype == np.float32 and logp.ndim == 2 and y.shape == (logp.shape[0],)
    ok = (y >= 0) & (y < logp.shape[1])
    return logp[ok].astype(np.float64), y[ok], int((~ok).sum())


def evaluate(z, y, theta, bias_sd, hessian=True):
    """``(F, g, H)`` at ``theta`` = (beta, b): ``z`` float64 [M, V] (or float32 log-probs: rows whose label lies outside the
    columns are dropped first), labels ``y``.  F includes the penalty; H is None with ``hessian=False``."""
    if np.asarray(z).dtype != np.float64:
        z, y, _ = _rows(z, y)
    theta = np.asarray(theta, dtype=np.float64)
    M, V = z.shape
    beta, b = theta[0], theta[1:]
    a = beta * z + b
    amax = a.max(axis=1, keepdims=True)
    e = np.exp(a - amax)
    at_max = a == amax                                    # e = 1 exactly there: counted, not summed (log1p keeps the digits)
    rest = np.where(at_max, 0.0, e).sum(axis=1) + (at_max.sum(axis=1) - 1.0)
    s0 = 1.0 + rest
    p = e / s0[:, None]
    m = (e * z).sum(axis=1) / s0
    rows = np.arange(M)
    zy = z[rows, y]
    f = np.log1p(rest) - (a[rows, y] - amax[:, 0])
    lam = 1.0 / (bias_sd * bias_sd * M)
    n = np.bincount(y, minlength=V).astype(np.float64)
    S = p.sum(axis=0)
    F = f.sum() / M + 0.5 * lam * (b * b).sum()
    g = np.concatenate([[(m - zy).sum() / M], (S / M - n / M) + lam * b])
    if not hessian:
        return float(F), g, None
    H = np.empty((V + 1, V + 1))
    H[0, 0] = ((e * z * z).sum(axis=1) / s0 - m * m).sum() / M
    H[1:, 0] = H[0, 1:] = (p * (z - m[:, None])).sum(axis=0) / M
    H[1:, 1:] = np.diag(S / M + lam) - (p.T @ p) / M
    return float(F), g, H


def nll(z, y, theta):
    """The mean log-loss of softmax(beta z + b) WITHOUT the penalty (``nll_before`` / ``nll_after``)."""
    F, _, _ = evaluate(z, y, theta, 1.0, hessian=False)
    return F - 0.5 / len(y) * float((np.asarray(theta)[1:] ** 2).sum())


def newton_direction(H, g):
    """``d = -H^-1 g`` by the device's right-looking Cholesky with the forward solve riding along, or None for a pivot <= 0 (the
    device takes the columns in panels of 8: every element still receives its subtractions in increasing k, as here)."""
    A, w = H.copy(), -g.copy()
    n = len(g)
    for k in range(n):
        if not A[k, k] > 0.0:
            return None
        l = np.sqrt(A[k, k])
        A[k + 1:, k] /= l
        A[k, k] = l
        w[k] /= l
        col = A[k + 1:, k]
        w[k + 1:] -= col * w[k]
        A[k + 1:, k + 1:] -= np.outer(col, col)
    for k in range(n - 1, -1, -1):
        w[k] /= A[k, k]
        w[:k] -= A[k, :k] * w[k]
    return w


def _in_box(beta):
    return BETA_MIN <= beta <= BETA_MAX


def _search(z, y, bias_sd, tol, decisions=None):
    """(theta, reason, evaluations, halvings, F of the accepted points).  ``decisions``: a list that receives, per comparison the
    search takes, ("gradient", max |g|, tol) or ("armijo", F', F + 1e-4 t g^T d): how far each decision was from going the other way."""
    V = z.shape[1]
    theta = np.concatenate([[1.0], np.zeros(V)])
    if len(y) == 0 or V == 1:
        return theta, "flat", 0, 0, []
    F, g, H = evaluate(z, y, theta, bias_sd)
    evals, halvings, trace = 1, 0, [F]
    while True:
        if decisions is not None:
            decisions.append(("gradient", float(np.abs(g).max()), tol))
        if np.abs(g).max() <= tol:
            return theta, "gradient", evals, halvings, trace
        if evals == EVALS:
            return theta, "cap", evals, halvings, trace
        d = newton_direction(H, g)
        if d is None:
            return theta, "pivot", evals, halvings, trace
        gtd, t = float(g @ d), 1.0
        while True:
            while t > 0.0 and not _in_box(theta[0] + t * d[0]):      # the box costs no evaluation
                t *= 0.5
                halvings += 1
            cand = theta + t * d
            Fc, gc, Hc = evaluate(z, y, cand, bias_sd)
            evals += 1
            if decisions is not None:
                decisions.append(("armijo", Fc, F + ARMIJO * t * gtd))
            if Fc <= F + ARMIJO * t * gtd:
                theta, F, g, H = cand, Fc, gc, Hc
                trace.append(F)
                break
            halvings += 1
            if evals == EVALS:
                return theta, "cap", evals, halvings, trace
            t *= 0.5


def fit_bias_temperature_ref(logp, y, bias_sd=2.0, tol=1e-10):
    """``ops.bias_temperature_download(*ops.fit_bias_temperature(logp, y, bias_sd, tol))`` on the host: ``logp`` float32 [N, V], ``y``
    integer [N]; plus ``halvings``, ``trace`` (F at the accepted points) and ``decisions`` (``_search``)."""
    z, yk, bad = _rows(logp, y)
    decisions = []
    theta, reason, evals, halvings, trace = _search(z, yk, float(bias_sd), float(tol), decisions)
    M = len(yk)
    before = nll(z, yk, np.concatenate([[1.0], np.zeros(z.shape[1])])) if M else 0.0
    after = nll(z, yk, theta) if M else 0.0
    return {"temperature": 1.0 / theta[0], "beta": float(theta[0]), "nll_before": before, "nll_after": after, "reason": reason,
            "iterations": evals, "rows": M, "bad_labels": bad, "method": "bias_temperature", "bias_sd": float(bias_sd),
            "bias": theta[1:].copy(), "penalty": 0.5 / (bias_sd * bias_sd * M) * float((theta[1:] ** 2).sum()) if M else 0.0,
            "halvings": halvings, "trace": trace, "decisions": decisions}


def decisions_are_clear(result, factor=2.0, margin=1e-13):
    """Whether no decision of a restatement run was close: every gradient test off ``tol`` by a factor of ``factor`` at least and
    every Armijo comparison decided by more than ``margin`` max(1, |F|) -- hundreds of ulp of F, where the device's other order
    of the sums moves F by a few.  Such a run's decisions are the device's too: same steps, same evaluation count, same reason."""
    for kind, got, bound in result["decisions"]:
        if kind == "gradient" and bound / factor < got <= bound * factor:
            return False
        if kind == "armijo" and abs(got - bound) <= margin * max(1.0, abs(bound)):
            return False
    return True


def shift_logp_ref(logp, beta, bias):
    """The calibrated log-probs (beta z + b) - logsumexp(beta z + b) per row, float64 [N, V]."""
    a = beta * np.asarray(logp).astype(np.float64) + bias
    amax = a.max(axis=1, keepdims=True)
    return (a - amax) - np.log(np.exp(a - amax).sum(axis=1, keepdims=True))


def make_shifted_logp(N, V, seed, sharp=2.0, tail=1.2, absent=None, bad=(), scale=1.7):
    """Log-probs of a model "trained under uniform priors" judged on long-tailed labels: labels drawn from pi_c ~ (c + 1)^-tail,
    scores = scale * (sharp * onehot(label) + noise) with no knowledge of pi (scale > 1: over-confident).  ``absent``: a class no
    row is labelled with; ``bad``: pairs (row, label) to overwrite with labels outside the columns.  Returns ``(logp float32
    [N, V], y int64 [N])``."""
    rng = np.random.default_rng(seed)
    pi = (np.arange(V) + 1.0) ** -tail
    if absent is not None:
        pi[absent] = 0.0
    pi /= pi.sum()
    y = rng.choice(V, size=N, p=pi)
    s = rng.normal(size=(N, V))
    s[np.arange(N), y] += sharp
    s *= scale                                               # over-confident: the temperature has something to do too
    logp = (s - np.log(np.exp(s - s.max(1, keepdims=True)).sum(1, keepdims=True)) - s.max(1, keepdims=True)).astype(np.float32)
    y = y.astype(np.int64)
    for r, label in bad:
        y[r] = label
    return logp, y


def kernel_cases():
    """The inputs tests/test_bias_calibration_gpu.py holds the kernel to: ``(name, logp, y, ld, bias_sd)`` (ld None: no padding) --
    the smallest shapes at which each launch can go wrong.  The data are chosen so that the restatement ends every one of them
    with reason "gradient" inside the cap (5 x 1: "flat") and ``decisions_are_clear``: tests/test_bias_calibration_cpu.py checks
    both, which is what makes the comparison with the device meaningful.  Strongly over-confident scores (scale 6, 12) make the
    first Newton steps leave the box and overshoot, so the box halvings and a rejected candidate are on the path."""
    tiny = np.log(np.array([[0.9, 0.1], [0.9, 0.1], [0.6, 0.4]], dtype=np.float32))
    wide = make_shifted_logp(300, 202, 6, sharp=0.5, scale=6.0, absent=17, bad=((3, -1), (150, 202), (299, -7)))
    return [("N3_V2", tiny, np.array([0, 0, 1]), None, 2.0),                                         # the tiny case
            ("N64_V5_sd0.5", *make_shifted_logp(64, 5, 2, sharp=0.5, scale=6.0), None, 0.5),         # few columns; box halvings
            ("N65_V65", *make_shifted_logp(65, 65, 1), None, 2.0),                                   # a wave plus one column
            # a tile plus one, 256 rows plus one, padded rows; a rejected candidate
            ("N257_V17_ld24_sd8", *make_shifted_logp(257, 17, 2, sharp=0.5, scale=12.0), 24, 8.0),
            ("N40_V16", *make_shifted_logp(40, 16, 6), None, 2.0),                                   # exactly one tile
            ("N300_V202_absent_bad_sd8", *wide, None, 8.0),              # the project's width, excluded rows, rejected candidates
            ("N8193_V3", *make_shifted_logp(8193, 3, 1), None, 2.0),                                 # the rows' stride loop wraps
            ("N5_V1", np.zeros((5, 1), dtype=np.float32), np.zeros(5, dtype=np.int64), None, 2.0)]   # V = 1
