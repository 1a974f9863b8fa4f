"""numpy restatement of the train-time input augmentation draw (``iterator_train__augment``; csrc/augment.hip, DESIGN.md
section 4).  Test infrastructure only: tests/test_augment_gpu.py compares ``slnlp_augment_rows`` with ``augment_rows`` element
for element, and trains on datasets augmented by it on the host.

``X`` int64 [n, S], ``L`` int64 [n]; row ``i`` has ``len = clamp(L[i], 0, S)``.  Every position ``t < len`` makes one
Threefry-4x32 call with the dropout masks' 12 rounds, key ``(seed_lo, seed_hi, 0, 0)``, counter ``(i, epoch, t, 0)``; of the
output words only ``X0`` is used:

* the position draws **drop** iff ``(X0 & 0xFFFF) < thr16(p_drop)``, **mask** iff ``(X0 >> 16) < thr16(p_mask)``
  (``thr16``: ``threefry_ref.threshold``, the dropout masks' rule);
* a row whose every position ``t < len`` drew drop drops none;
* the kept positions, in ascending ``t``, go to ``X_out[i, 0 .. len')`` -- ``unk`` where the position drew mask, ``X[i, t]``
  otherwise -- ``X_out[i, len' .. S) = pad`` and ``L_out[i] = len'``.  Positions ``>= len`` of ``X`` are never read.
"""
import numpy as np

from threefry_ref import threefry4x32, threshold

ROUNDS = 12           # SLNLP_THREEFRY_ROUNDS, the dropout masks' (csrc/common.hpp)


def word0(rows, epoch, S, seed):
    """``X0`` for every (row index in ``rows``, t < S): uint32 [len(rows), S]."""
    i, t = np.meshgrid(np.asarray(rows, dtype=np.uint32), np.arange(S, dtype=np.uint32), indexing="ij")
    zero = np.zeros_like(i)
    seed = int(seed) % (1 << 64)
    key = [zero + np.uint32(seed & 0xFFFFFFFF), zero + np.uint32(seed >> 32), zero, zero]
    return threefry4x32([i, zero + np.uint32(epoch), t, zero], key, ROUNDS)[0]


def draws(L, S, p_drop, p_mask, seed, epoch, rows=None):
    """(live, drop, mask) bool [n, S]: the positions ``t < len`` and what each drew, before the no-empty-row rule.  ``rows``:
    the row indices the counters use (default ``0 .. n - 1``)."""
    L = np.asarray(L, dtype=np.int64)
    rows = np.arange(len(L)) if rows is None else np.asarray(rows)
    w = word0(rows, epoch, S, seed)
    live = np.arange(S)[None, :] < np.clip(L, 0, S)[:, None]
    drop = live & ((w & np.uint32(0xFFFF)) < np.uint32(threshold(p_drop)))
    mask = live & ((w >> np.uint32(16)) < np.uint32(threshold(p_mask)))
    return live, drop, mask


def augment_rows(X, L, pad, unk, p_drop, p_mask, seed, epoch, rows=None):
    """-> (X_out int64 [n, S], L_out int64 [n])"""
    X = np.asarray(X, dtype=np.int64)
    n, S = X.shape
    live, drop, mask = draws(L, S, p_drop, p_mask, seed, epoch, rows)
    drop &= ~(drop == live).all(axis=1)[:, None]          # every position of the row drew drop: none is dropped
    keep = live & ~drop
    L_out = keep.sum(axis=1).astype(np.int64)
    # a stable sort on "not kept" lists every row's kept positions first, in ascending t (what lies at a position that is
    # not live is garbage to this function: np.where evaluates it, nothing of it reaches the output)
    first_kept = np.argsort(~keep, axis=1, kind="stable")
    vals = np.take_along_axis(np.where(mask, np.int64(unk), X), first_kept, axis=1)
    X_out = np.where(np.arange(S)[None, :] < L_out[:, None], vals, np.int64(pad)).astype(np.int64)
    return X_out, L_out
