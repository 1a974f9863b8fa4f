"""The numpy fp64 restatement of ``slnlp_fit_priors`` and ``slnlp_shift_logp``, line by line with include/slnlp.h.

``fit_priors`` also returns the traces the device does not keep: ``d_trace[t]`` = d^t and ``gain_trace[t]`` = the gain the rows
would report if the EM stopped after iteration t (at pi^{t+1}'s log-ratio)."""
import numpy as np

FLOOR = 2.0 ** -1022


def counted_rows(z):
    """Rows that hold no NaN and whose maximum is finite."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(z).any(axis=1) & np.isfinite(z.max(axis=1))


def _lse(a):
    amax = a.max(axis=1)
    return amax + np.log(np.exp(a - amax[:, None]).sum(axis=1))


def fit_priors(z, log_source, beta=1.0, max_iter=200, tol=1e-6):
    z = np.asarray(z, dtype=np.float32)
    ls = np.asarray(log_source, dtype=np.float64)
    N, V = z.shape
    keep = counted_rows(z)
    M = int(keep.sum())
    pi0 = np.exp(ls)
    if M == 0:
        return {"mean_proba": pi0.copy(), "priors": pi0.copy(), "log_ratio": np.zeros(V), "gain": 0.0, "d": 0.0, "reason": "empty",
                "iterations": 0, "rows": 0, "nan_rows": N, "d_trace": [], "gain_trace": []}
    bz = np.float64(beta) * z[keep].astype(np.float64)       # beta z, rounded once
    lse0 = _lse(bz + np.zeros(V))
    lw, pi = np.zeros(V), pi0
    d_trace, gain_trace = [], []
    mean = None
    t = 0
    with np.errstate(divide="ignore"):
        while True:
            a = bz + lw[None, :]
            lse = _lse(a)
            S = np.exp(a - lse[:, None]).sum(axis=0)
            new = S / M
            d = float(np.abs(new - pi).max())
            if t == 0:
                mean = new.copy()
            pi = new
            lw_next = np.log(np.maximum(pi, FLOOR)) - ls
            d_trace.append(d)
            gain_trace.append(float((_lse(bz + lw_next[None, :]) - lse0).sum() / M))
            if d <= tol:
                reason = "tol"
                break
            if t == max_iter:
                reason = "cap"
                break
            lw = lw_next
            t += 1
    return {"mean_proba": mean, "priors": pi, "log_ratio": lw_next, "gain": gain_trace[-1], "d": d, "reason": reason,
            "iterations": t + 1, "rows": M, "nan_rows": N - M, "d_trace": d_trace, "gain_trace": gain_trace}


def shift_logp(z, log_w, beta=1.0):
    """float64 [N, V], before the one rounding to float32: (beta z + log_w) - logsumexp, as (a - max) - log1p(sum e - 1) with the
    columns at the maximum counted; NaN in every column of a row without a softmax."""
    z = np.asarray(z, dtype=np.float32)
    lw = np.asarray(log_w, dtype=np.float64)
    out = np.full(z.shape, np.nan, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in np.flatnonzero(counted_rows(z)):
            a = np.float64(beta) * z[i].astype(np.float64) + lw
            amax = a.max()
            if not np.isfinite(amax):
                continue
            at = a == amax
            rest = np.exp(a[~at] - amax).sum() + (at.sum() - 1.0)
            out[i] = (a - amax) - np.log1p(rest)
    return out


def ulp_error(got, want):
    """The largest |got - want| in float32 steps at want (``got`` float32, ``want`` the fp64 restatement), as
    tests/test_calibration_gpu.py measures ``scale_logp``; positions where both are NaN or the same infinity count 0."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float64)
    w32 = want.astype(np.float32)
    same = (np.isnan(got) & np.isnan(w32)) | (np.isinf(w32) & (got == w32))
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(w32)).astype(np.float64)
    err = np.where(same, 0.0, err)
    return float(np.where(np.isnan(err), np.inf, err).max())


def gaussian_shift_problem(V, N, seed, d=8, alpha=0.5):
    """The recovery problem: Gaussian class-conditionals in ``d`` dimensions (unit covariance, means N(0, 2^2) per dimension), a
    uniform source prior, a target prior from Dirichlet(alpha), N target rows.  Returns ``(z float32 [N, V], y int64 [N],
    target prior)``: z the exact source posteriors' log-probs."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(0.0, 2.0, size=(V, d))
    pi_t = rng.dirichlet(np.full(V, alpha))
    y = rng.choice(V, size=N, p=pi_t)
    x = mu[y] + rng.normal(size=(N, d))
    logit = -0.5 * ((x[:, None, :] - mu[None, :, :]) ** 2).sum(axis=2)      # + ln(1 / V): the same in every class
    logp = logit - _lse(logit)[:, None]
    return logp.astype(np.float32), y.astype(np.int64), pi_t


def make_case(N, V, seed):
    """Float32 log-probs [N, V] of a classifier whose rows lean towards a skewed set of classes, and ln of a random source prior:
    ``(z, log_source)``.  What the GPU tests and tools/time_prior_shift.py run the device and the restatement on."""
    rng = np.random.RandomState(seed)
    logits = 2.0 * rng.randn(N, V) + rng.randn(V)[None, :]
    z = (logits - _lse(logits)[:, None]).astype(np.float32)
    source = rng.dirichlet(np.full(V, 2.0)) if V > 1 else np.ones(1)
    return z, np.log(source)


def iterate_bound(want, N):
    """The bound table rows 0 and 1 and the gain are held to: relative 64 N 2^-53 plus an absolute 2^-60 (sums of at most N positive
    terms that differ only in their order, fp64 exp / log that differ by a few ulp; EM amplifies neither)."""
    return 64.0 * N * 2.0 ** -53 * np.abs(want) + 2.0 ** -60


def iterate_errors(got, want, N):
    """The device's result (``ops.priors_download``'s dict) against the restatement's, each error divided by its bound -- at most 1
    when the device holds it: {mean_proba, priors, log_ratio, gain}.  The log-ratio's bound is the priors' times 1 / pi_c."""
    err = {k: float((np.abs(got[k] - want[k]) / iterate_bound(want[k], N)).max()) for k in ("mean_proba", "priors")}
    err["gain"] = float(abs(got["gain"] - want["gain"]) / iterate_bound(want["gain"], N))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(got["log_ratio"] - want["log_ratio"]) / (iterate_bound(want["priors"], N) / want["priors"])
    err["log_ratio"] = float(np.where(got["log_ratio"] == want["log_ratio"], 0.0, rel).max())
    return err
