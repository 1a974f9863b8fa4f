"""numpy fp64 restatement of csrc/ensemble.hip (``slnlp_ensemble_rows``; include/slnlp.h states the definition), on top of
``calibration_ref._shifted``: the members' terms, the mixture, both voting modes and the per-row uncertainty decomposition, and
the generator of the members the CPU and GPU tests share.  What differs from the device is only the order of the sums over the
columns and numpy's exp / log."""
import numpy as np

from calibration_ref import _shifted

MAX_MEMBERS = 32
MODES = {"soft": 0, "log": 1}
# the kernel cases (N, V, K) of the issue, their three input families and the betas member k takes when it has one
SHAPES = [(1, 2, 1), (5, 3, 2), (257, 70, 3), (33, 129, 5), (3, 5, 32), (4, 1, 2), (300, 202, 4)]
STRIDES = {(33, 129, 5): ((136, 129, 200, 136, 129), 136)}          # member strides and ld_out; every other case is dense
FAMILIES = [(8.0, 0.6, 1), (0.3, 0.9, 2), (2.0, 0.6, 3)]
BETAS = (0.16, None, 6.25)


def make_members(N, V, K, scale, boosted, seed):
    """K members float32 [N, V] and the labels: member k is the float32 log-softmax (in fp64, the maximum subtracted) of the
    family's log-probs plus ``0.5 scale randn`` of its own."""
    from test_calibration_cpu import make_logp
    base, y = make_logp(N, V, scale, boosted, seed)
    members = []
    for k in range(K):
        z = base.astype(np.float64) + 0.5 * scale * np.random.RandomState(1000 * seed + k).randn(N, V)
        z -= z.max(axis=1, keepdims=True)
        members.append((z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32))
    return members, y


def case_betas(K, on):
    return [BETAS[k % 3] if on else None for k in range(K)]


def case_weights(K, on):
    return [1.0 + k for k in range(K)] if on else None


def normalised(weights, K):
    """w_k = weights[k] / (their sum in increasing k); None: 1 / K."""
    if weights is None:
        return np.full(K, 1.0 / K)
    total = 0.0
    for w in weights:
        total += float(w)
    return np.array([float(w) / total for w in weights])


def ensemble_ref(members, betas=None, weights=None, mode="soft"):
    """``(out float64 [N, V] -- the value the device rounds once to float32 -- , rows float64 [N, 4])`` of ``members``, a list of
    float32 [N, V]; ``betas``: a list of numbers or None (beta = 1); ``weights``: numbers > 0 or None."""
    K = len(members)
    assert 1 <= K <= MAX_MEMBERS and mode in MODES
    assert all(m.dtype == np.float32 and m.shape == members[0].shape and m.ndim == 2 for m in members)
    N, V = members[0].shape
    w = normalised(weights, K)
    betas = [1.0 if b is None else float(b) for b in (betas if betas is not None else [None] * K)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        bad = np.zeros(N, dtype=bool)
        l = np.empty((K, N, V))
        for k, (m, beta) in enumerate(zip(members, betas)):
            z = m.astype(np.float64)
            bad |= ~np.isfinite(z.max(axis=1))               # a NaN in the row, or a maximum that is not finite
            a, _, rest = _shifted(z, beta)
            l[k] = (beta * z - a) - np.log1p(rest)[:, None]
        p = np.exp(l)
        mx = l.max(axis=0)
        some = mx > -np.inf
        s = np.zeros((N, V))
        for k in range(K):
            s += w[k] * np.where(some, np.exp(l[k] - mx), 0.0)
        mix = np.where(some, mx + np.log(s), -np.inf)
        if mode == "soft":
            out = mix.copy()
        else:
            u = np.zeros((N, V))
            for k in range(K):
                u += w[k] * l[k]
            umax = u.max(axis=1, keepdims=True)
            bad |= ~(umax[:, 0] > -np.inf)
            out = (u - umax) - np.log(np.exp(u - umax).sum(axis=1, keepdims=True))
        pbar = np.where(some, np.exp(mix), 0.0)
        rows = np.zeros((N, 4))
        rows[:, 0] = -np.where(pbar > 0.0, pbar * mix, 0.0).sum(axis=1)
        for k in range(K):
            live = p[k] > 0.0
            rows[:, 1] += w[k] * -np.where(live, p[k] * l[k], 0.0).sum(axis=1)
            rows[:, 2] += w[k] * np.where(live, p[k] * (l[k] - mix), 0.0).sum(axis=1)
        stored = out.astype(np.float32)
        top = np.argmax(stored, axis=1)                      # the first maximum of the row as stored
        for m in members:
            rows[:, 3] += np.argmax(m, axis=1) != top
    out[bad] = np.nan
    rows[bad] = (np.nan, np.nan, np.nan, -2.0)
    return out, rows


def direct_ref(members, betas=None, weights=None):
    """The soft vote and its decomposition computed directly: a plain fp64 softmax per member, the weighted mean, -sum p log p.
    ``(pbar [N, V], H_total [N], H_mean [N])``; finite inputs only."""
    K = len(members)
    w = normalised(weights, K)
    betas = [1.0 if b is None else float(b) for b in (betas if betas is not None else [None] * K)]
    pbar, h_mean = 0.0, 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, (m, beta) in enumerate(zip(members, betas)):
            t = beta * m.astype(np.float64)
            e = np.exp(t - t.max(axis=1, keepdims=True))
            p = e / e.sum(axis=1, keepdims=True)
            pbar = pbar + w[k] * p
            h_mean = h_mean + w[k] * -np.where(p > 0.0, p * np.log(p), 0.0).sum(axis=1)
        h_total = -np.where(pbar > 0.0, pbar * np.log(pbar), 0.0).sum(axis=1)
    return pbar, h_total, h_mean


def spacing32(r):
    """The distance from float32(|r|) to the next float32 above it."""
    return np.spacing(np.abs(np.asarray(r)).astype(np.float32)).astype(np.float64)


def out_bound(r):
    """The issue's bound on |out - r| for the restatement's fp64 value r: one correct rounding plus the fp64 bound."""
    return 0.5 * spacing32(r) + 1e-9 * np.maximum(1.0, np.abs(r))


def top_gap(out):
    """Per row the gap between the two largest values of ``out`` [N, V >= 2]."""
    s = np.sort(out, axis=1)
    return s[:, -1] - s[:, -2]


def uncertainty_ref(rows):
    """``metrics.uncertainty_summary`` restated: means over the scored rows (code >= 0)."""
    rows = np.asarray(rows, dtype=np.float64)
    ok = rows[:, 3] >= 0
    n = int(ok.sum())
    mean = (lambda v: float(np.sum(v) / n)) if n else (lambda v: float("nan"))
    return {"total_entropy": mean(rows[ok, 0]), "expected_entropy": mean(rows[ok, 1]), "mutual_information": mean(rows[ok, 2]),
            "disagreement_rate": mean(rows[ok, 3] > 0), "mean_disagreement": mean(rows[ok, 3]), "rows": n, "nan_rows": int((~ok).sum())}
