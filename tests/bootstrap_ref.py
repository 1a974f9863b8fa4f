"""numpy restatement of the bootstrap of the scores (``slnlp_bootstrap_scores``; csrc/bootstrap.hip, include/slnlp.h, DESIGN.md
section 4).  Test infrastructure only: tests/test_bootstrap_cpu.py holds it to sklearn on explicitly resampled arrays,
tests/test_bootstrap_gpu.py compares the kernel with it.

The draw: replicate ``b``, draw ``j`` in [0, N): Threefry-4x32 with the dropout masks' 12 rounds under key ``(seed_lo, seed_hi, 0,
0)`` at counter ``(j >> 2, b, STAGE, 0)``; of the output words ``X0..X3`` the draw takes ``X[j & 3]`` and the row is
``(X * N) >> 32``.

The scores of a replicate are the PROJECT'S OWN host scoring, ``metrics.scores_from_rows``, on the gathered rows and their
recounted class sums -- no second formula -- and ``np.mean`` of the gathered value columns."""
import numpy as np

from slnlp import metrics
from threefry_ref import threefry4x32

ROUNDS = 12                # SLNLP_THREEFRY_ROUNDS, the dropout masks' (csrc/common.hpp)
STAGE = 0x626F6F74         # SLNLP_BOOT_STAGE
FIXED = 9                  # SLNLP_BOOT_FIXED


def draws(N, B, seed):
    """int64 [B, N]: the row every draw of every replicate takes."""
    seed = int(seed) % (1 << 64)
    q, b = np.meshgrid(np.arange((N + 3) // 4, dtype=np.uint32), np.arange(B, dtype=np.uint32), indexing="xy")      # [B, calls]
    zero = np.zeros_like(q)
    key = [zero + np.uint32(seed & 0xFFFFFFFF), zero + np.uint32(seed >> 32), zero, zero]
    X = threefry4x32([q, b, zero + np.uint32(STAGE), zero], key, ROUNDS)
    words = np.stack(X, axis=2).reshape(B, -1)[:, :N]                            # word w of call q is draw 4 q + w
    return ((words.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def recount(y, pred, V):
    """``score_rows``' counts of the rows given: true_sum | pred_sum | tp_sum | n_bad; a value outside [0, V) is never an index."""
    ok, pok = (y >= 0) & (y < V), (pred >= 0) & (pred < V)
    return np.concatenate([np.bincount(y[ok], minlength=V), np.bincount(pred[pok], minlength=V),
                           np.bincount(y[ok & (pred == y)], minlength=V), [int((~ok).sum())]]).astype(np.int64)


def column_names(top_k):
    """The names ``metrics.scores_from_rows`` knows the fixed columns by (the top-k column: None when ``top_k`` is 0)."""
    return [*metrics.BOOT_COLUMNS[:8], f"top{top_k}_accuracy" if top_k else None]


def replicate_scores(y, pred, rank, V, top_k):
    """The nine fixed columns of ONE replicate whose gathered rows are given, and its counts."""
    counts = recount(y, pred, V)
    ok = (y >= 0) & (y < V)
    rank = None if rank is None else np.where(ok, rank, V)                       # a row whose label is no class is never a hit
    names = [n for n in column_names(top_k) if n is not None]
    # the header's accuracy is sum tp_sum / N: a label and a prediction outside the classes never make a correct row, even when
    # they are the same value -- so what is no class is handed over as two values that cannot be equal
    pok = (pred >= 0) & (pred < V)
    with np.errstate(invalid="ignore", divide="ignore"):
        got = metrics.scores_from_rows(names, np.where(ok, y, -1), np.where(pok, pred, V), None, rank, counts, V)
    return [got.get(n, float("nan")) for n in column_names(top_k)], counts


def bootstrap_ref(y, pred, rank, values, V, top_k, B, seed):
    """-> (stats float64 [B, 9 + Q], counts int64 [B, 3 V + 1]); ``values`` float64 [N, Q] or None."""
    y, pred = np.asarray(y, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    rank = None if rank is None else np.asarray(rank, dtype=np.int64)
    Q = 0 if values is None else values.shape[1]
    rows = draws(len(y), B, seed)
    stats, counts = np.empty((B, FIXED + Q)), np.empty((B, 3 * V + 1), dtype=np.int64)
    for b in range(B):
        r = rows[b]
        stats[b, :FIXED], counts[b] = replicate_scores(y[r], pred[r], None if rank is None else rank[r], V, top_k)
        if Q:
            stats[b, FIXED:] = np.mean(values[r], axis=0)
    return stats, counts


def make_case(N, V, seed, hit=0.7, Q=3):
    """Per-row results of N predictions over V classes as the device calls leave them: labels ``y`` int64 [N] (uniform: with N
    near V many classes hold one row), ``pred`` int32 [N] (the label in a share ``hit`` of the rows, else any class), ``rank``
    int32 [N] (0 where the prediction is right, else anything in [1, V]) and ``values`` float64 [N, Q]."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, V, size=N).astype(np.int64)
    pred = np.where(rs.rand(N) < hit, y, rs.randint(0, V, size=N)).astype(np.int32)
    rank = np.where(pred == y, 0, rs.randint(1, V + 1, size=N)).astype(np.int32)
    values = rs.randn(N, Q) * np.array([1.0, 10.0, 0.1, 3.0, 1.0, 1.0, 1.0, 1.0])[:Q] + 0.5
    return y, pred, rank, values
