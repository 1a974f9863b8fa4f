"""The visit order of a fit's train rows: torch's own ``RandomSampler`` / ``BatchSampler``, wrapped.

skorch hands ``iterator_train__shuffle`` / ``iterator_train__drop_last`` to ``torch.utils.data.DataLoader``, which builds a
``BatchSampler(RandomSampler(dataset, generator=...), batch_size, drop_last)``.  ``EpochOrder`` owns exactly those two objects
(over ``range(n)``), so every index of every epoch is torch's own draw -- nothing about how ``RandomSampler`` uses its
generator is restated here.  The fit loop asks for a whole epoch's order ahead of the epoch (``next_epoch``), because a
lockstep unit runs the epoch without coming back to the host: the order travels to the device as a table (slnlp.lockstep),
and every other path stages its batches through the same table (``slnlp_gather_batch``).

``iterator_train__balance=True`` replaces that order by a class-balanced resample of the fit's own train rows, drawn afresh
every epoch ON THE DEVICE (``slnlp_balanced_order``, csrc/balance.hip; targets: ``slnlp.balance.sampling_targets``) straight into
the same table: the epoch then visits ``balanced_rows(y)`` rows, some of them more than once, and nothing is uploaded.  The draw
is a function of (labels, ``balance_seed``, epoch number), so a resumed fit needs no fast-forward; it already permutes, which
leaves ``iterator_train__shuffle`` nothing to do beside it (accepted, no effect).  ``HONOURED`` keeps naming the two keys this
module draws for on the host; ``BALANCE`` is the third honoured key.

``iterator_train__augment={"frame_drop": p, "token_mask": p}`` regularises the INPUTS instead of the order: every train epoch
sees a freshly augmented copy of the fit's own train rows, drawn ON THE DEVICE (``slnlp_augment_rows``, csrc/augment.hip) into
the two buffers every consumer of the train split already reads -- frame dropping deletes random timesteps (the row closes up
and gets shorter, never empty), token masking replaces random tokens by ``<unk>``.  The draw is a function of (rows,
``augment_seed``, epoch number), per dataset row: a resumed fit needs no fast-forward, it composes with shuffling and balancing
(which only choose the rows' order), and a row a balanced epoch visits twice is seen in the same augmented form both times
within that epoch.  Valid, test and predict data are never augmented.  ``AUGMENT`` is the fourth honoured key,
``augment_options`` its validation.

As for schedules (slnlp/schedule.py), the position is a function of the fit's history: a new fit run builds the sampler from
the seed and draws the epochs the history accounts for (``fast_forward``), so a resumed fit needs no extra checkpoint file --
the seed rides every epoch row of a shuffled fit (``"shuffle_seed"``).
"""
import numpy as np
import torch
from torch.utils.data import BatchSampler, RandomSampler

# the ``iterator_train__*`` keys the fit loop honours beside ``balance`` and ``augment`` below (every other ``iterator_*`` key is
# accepted and has no effect, as the reference's ``collate_fn``)
HONOURED = ("shuffle", "drop_last")


def draw_seed():
    """A fresh seed from torch's global CPU generator, the way ``RandomSampler`` draws one when it is given no generator."""
    return int(torch.empty((), dtype=torch.int64).random_().item())


def seed_from_history(history):
    """The ``shuffle_seed`` of the last epoch row that carries one, or None."""
    for row in reversed(history or []):
        if row.get("shuffle_seed") is not None:
            return int(row["shuffle_seed"])
    return None


BALANCE = "balance"


def seed_of(history, key):
    """The ``key`` ("shuffle_seed" / "balance_seed" / "augment_seed") of the last epoch row that carries one, or None."""
    for row in reversed(history or []):
        if row.get(key) is not None:
            return int(row[key])
    return None


AUGMENT = "augment"
AUGMENT_KEYS = ("frame_drop", "token_mask")


def augment_options(setting):
    """The ``iterator_train__augment`` setting with its defaults filled in -- {frame_drop, token_mask}, each a probability in
    [0, 1), 0 when omitted -- or None (off: None, False or absent).  Anything else raises ValueError."""
    if setting is None or setting is False:
        return None
    if not isinstance(setting, dict):
        raise ValueError(f"iterator_train__augment={setting!r}: expected a dict with keys among {AUGMENT_KEYS}, None or False")
    unknown = sorted(set(setting) - set(AUGMENT_KEYS), key=repr)
    if unknown:
        raise ValueError(f"iterator_train__augment: unknown keys {unknown} (known: {AUGMENT_KEYS})")
    out = {}
    for k in AUGMENT_KEYS:
        p = setting.get(k, 0.0)
        # the library takes the probability as a float32 (the dropout masks' threshold rule): that value must stay below 1
        if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(np.float32(p)) < 1.0:
            raise ValueError(f"iterator_train__augment: {k}={p!r}, expected a real number in [0, 1)")
        out[k] = float(p)
    return out


def balanced_rows(y):
    """Rows a class-balanced epoch over the labels ``y`` visits: the sum of the over-sampling targets (what
    ``slnlp_balance_plan_rows`` returns for the same labels)."""
    import collections
    from .balance import sampling_targets
    return int(sum(sampling_targets(dict(collections.Counter(np.asarray(y).tolist())))[1].values()))


def n_visit(n, batch_size, drop_last=False):
    """Rows one epoch visits."""
    return (n // batch_size) * batch_size if drop_last else n


def check_order(order, rows, n_visit=None):
    """A host order as contiguous int64, after the checks the device side leaves to its caller: one dimension, the expected
    length, every index a row of the dataset."""
    order = np.ascontiguousarray(order, dtype=np.int64)
    if order.ndim != 1 or order.size < 1 or (n_visit is not None and order.size != n_visit):
        raise ValueError(f"order table of shape {order.shape}, expected ({n_visit},)")
    if int(order.min()) < 0 or int(order.max()) >= rows:
        raise ValueError(f"order table indexes rows {int(order.min())}..{int(order.max())} of a dataset of {rows}")
    return order


class EpochOrder:
    """Epoch ``e`` (0-based) of the object is the ``e``-th iteration of
    ``BatchSampler(RandomSampler(range(n), generator=torch.Generator().manual_seed(seed)), batch_size, drop_last)``, flattened."""

    def __init__(self, n, batch_size, seed, drop_last=False):
        n, batch_size = int(n), int(batch_size)
        if n < 1 or batch_size < 1:
            raise ValueError(f"EpochOrder: n={n}, batch_size={batch_size}")
        self.n, self.batch_size, self.seed, self.drop_last = n, batch_size, int(seed), bool(drop_last)
        self.n_visit = n_visit(n, batch_size, self.drop_last)
        if self.n_visit < 1:
            raise ValueError(f"iterator_train__drop_last=True with {n} train rows and batch_size {batch_size}: no full batch, "
                             "nothing to train on")
        self.epochs_drawn = 0
        self._gen = torch.Generator().manual_seed(self.seed)
        self._batches = BatchSampler(RandomSampler(range(n), generator=self._gen), batch_size, self.drop_last)

    def next_epoch(self):
        """The coming epoch's visit order: int64 numpy array of ``n_visit`` row indices."""
        # the iteration is run to its end, as a DataLoader would: what RandomSampler draws after its last index is part of the stream
        order = np.array([i for batch in self._batches for i in batch], dtype=np.int64)
        assert order.shape == (self.n_visit,)
        self.epochs_drawn += 1
        return order

    def fast_forward(self, epochs_done):
        """Draw (and drop) the epochs a history of ``epochs_done`` rows accounts for."""
        for _ in range(int(epochs_done)):
            self.next_epoch()
        return self
