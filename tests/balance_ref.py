"""numpy restatement of the class-balanced epoch draw (``iterator_train__balance``; csrc/balance.hip).
Test infrastructure only: tests/test_balance_gpu.py compares ``slnlp_balanced_order`` with ``balanced_order`` element for element.

Labels ``y`` [n], classes in ascending id order with counts ``n_c`` (absent classes take no part).  Targets from
``slnlp.balance.sampling_targets``: keep ``u_c = under[c]`` members, visit ``t_c = over[c]``; ``n_bal = sum t_c``.

Random words: Threefry-4x32 with the dropout masks' 12 rounds, key ``(seed_lo, seed_hi, 0, 0)``, counter
``(index, epoch, stage, 0)``.  Of the four output words ``X0..X3``: a 64-bit key is ``X1 << 32 | X0`` (stages 0 and 2), the
over-sampling word is ``X0`` (stage 1); ``X2`` and ``X3`` are not used.

* stage 0, index = row ``i``: within its class, rows ranked by ``(key, i)``; the ``u_c`` lowest ranks are kept,
  ``kept_c[r]`` = the row of rank ``r``;
* stage 1, index = ``base_c + j`` for extra ``j`` in ``[0, t_c - u_c)`` (``base_c``: the class's first slot): the extra takes
  ``kept_c[mulhi32(X0, u_c)]``;
* stage 2, index = slot: slots laid out class after class (kept rows, then extras), ranked by ``(key, slot)``;
  ``order[rank] = row of the slot``.
"""
import collections

import numpy as np

from slnlp.balance import sampling_targets
from threefry_ref import threefry4x32

ROUNDS = 12           # SLNLP_THREEFRY_ROUNDS, the dropout masks' (csrc/common.hpp)


def words(index, epoch, stage, seed):
    """The four Threefry output words for every entry of ``index`` (uint32 arrays)."""
    index = np.asarray(index, dtype=np.uint32)
    zero = np.zeros_like(index)
    seed = int(seed) % (1 << 64)
    key = [zero + np.uint32(seed & 0xFFFFFFFF), zero + np.uint32(seed >> 32), zero, zero]
    return threefry4x32([index, zero + np.uint32(epoch), zero + np.uint32(stage), zero], key, ROUNDS)


def key64(index, epoch, stage, seed):
    X = words(index, epoch, stage, seed)
    return (X[1].astype(np.uint64) << np.uint64(32)) | X[0].astype(np.uint64)


def targets(y):
    """(classes ascending, under [C], over [C]) of the labels' present classes."""
    counts = dict(collections.Counter(np.asarray(y).tolist()))
    under, over = sampling_targets(counts)
    classes = sorted(counts)
    return classes, [under[c] for c in classes], [over[c] for c in classes]


def balanced_rows(y):
    return int(sum(targets(y)[2]))


def balanced_order(y, seed, epoch):
    """-> (order int64 [n_bal], y[order])"""
    y = np.asarray(y, dtype=np.int64)
    classes, under, over = targets(y)
    k0 = key64(np.arange(len(y)), epoch, 0, seed)
    slot_rows, base = [], 0
    for c, u, t in zip(classes, under, over):
        members = np.flatnonzero(y == c)
        ranked = members[np.lexsort((members, k0[members]))]          # by (key, row) ascending
        kept = ranked[:u]
        w = words(base + np.arange(t - u), epoch, 1, seed)[0]
        r = (w.astype(np.uint64) * np.uint64(u)) >> np.uint64(32)     # mulhi32
        slot_rows.append(np.concatenate([kept, kept[r.astype(np.int64)]]))
        base += t
    slot_rows = np.concatenate(slot_rows).astype(np.int64)
    k2 = key64(np.arange(base), epoch, 2, seed)
    order = slot_rows[np.lexsort((np.arange(base), k2))]
    return order, y[order]
