"""In-memory token dataset with the tensor layout the reference hands to the
model (/root/reference/helper.py:293-304 ``collate_data``): ``X int64[N,S]``
padded with ``<pad>``, ``lengths int64[N]``, ``y int64[N]``.

Stands in for the reference's ``AslDataset`` / ``AslSliceDataset``
(dataset/asl_dataset.py:13-303) only as far as the hot path needs: it is
indexable by integer arrays (so sklearn CV splitters and ``_safe_indexing``
work, asl_dataset.py:261-271), carries the labels with the inputs (the
Transformer consumes ``y`` as decoder input even at predict time,
asl_dataset.py:48-55 / transformer.py:65) and exposes ``vocab_X`` / ``vocab_y``.
"""
import numpy as np


class LabelArray(np.ndarray):
    """``dataset.y`` as the int64 array everything here indexes -- and callable, so the reference's spelling
    ``train_data.y().to_array()`` (main.py:77, asl_dataset.py:200-208) reads the same labels."""

    def __call__(self):
        return self

    def to_array(self):
        return np.asarray(self)


def group_ids(what, groups, n):
    """``groups`` checked: an integer array [n] (or the dict ``slnlp.duplicate_groups`` returns: its ``"groups"``) -> a contiguous
    int64 copy; anything else raises ValueError"""
    if isinstance(groups, dict):
        if "groups" not in groups:
            raise ValueError(f"{what}: a dict without \"groups\" (expected what slnlp.duplicate_groups returns)")
        groups = groups["groups"]
    g = np.asarray(groups)
    if g.dtype.kind not in "iu" or g.shape != (n,):
        raise ValueError(f"{what}: groups must be an integer array [{n}] (one id per row), got {g.dtype} {tuple(g.shape)}")
    return np.array(g, dtype=np.int64)


class TokenDataset:
    """``groups`` (None: no groups, every split is the one it always was): int64 [N], rows with one id are near-duplicates of each
    other (``slnlp.duplicate_groups``) and every splitter -- ``split``, the grid's and ``cross_fit``'s folds, a fit's internal
    valid split -- keeps them on one side.  Slicing carries them with the rows."""
    groups = None                                            # (a dataset unpickled from before the attribute existed has none)

    def __init__(self, X, lengths, y, vocab_X=None, vocab_y=None, groups=None):
        self.ids = np.ascontiguousarray(X, dtype=np.int64)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int64)
        self.y = np.ascontiguousarray(y, dtype=np.int64).view(LabelArray)
        assert self.ids.ndim == 2 and len(self.ids) == len(self.lengths) == len(self.y)
        self.vocab_X, self.vocab_y = vocab_X, vocab_y
        self.batch_first = True
        self.groups = None if groups is None else group_ids("TokenDataset", groups, len(self.y))

    def with_groups(self, groups):
        """This dataset carrying ``groups``: an integer array [N], or the dict ``slnlp.duplicate_groups`` returns (None: without
        any).  The rows are shared, not copied."""
        return TokenDataset(self.ids, self.lengths, self.y, self.vocab_X, self.vocab_y,
                            None if groups is None else group_ids("with_groups", groups, len(self)))

    def __len__(self):
        return len(self.y)

    @property
    def shape(self):          # makes sklearn index with X[ndarray] instead of a python loop
        return (len(self.y),)

    def __getitem__(self, idx):
        if isinstance(idx, (int, np.integer)):
            return (self.ids[idx].tolist(), int(self.lengths[idx])), int(self.y[idx])   # asl_dataset item layout
        if isinstance(idx, tuple):        # sklearn's _array_indexing passes (indices, Ellipsis)
            idx = idx[0]
        idx = np.asarray(idx) if not isinstance(idx, slice) else idx
        if self.groups is None:
            return TokenDataset(self.ids[idx], self.lengths[idx], self.y[idx], self.vocab_X, self.vocab_y)
        return TokenDataset(self.ids[idx], self.lengths[idx], self.y[idx], self.vocab_X, self.vocab_y, self.groups[idx])

    def X(self):
        return self

    def to_array(self):
        return np.asarray(self.y)

    def labels(self):
        """Every index of the target vocabulary, specials included (asl_dataset.py:210-213 returns
        ``vocab_y.stoi.values()``); it feeds sklearn's log_loss ``labels=`` and must match the
        model's V output columns."""
        if self.vocab_y is not None:
            return list(range(len(self.vocab_y)))
        return sorted(set(self.y.tolist()))

    def truncated(self, n):
        return self[np.arange(min(n, len(self)))]

    def split(self, test_size=0.15, seed=1):
        """(test, train) like ``AslDataset.split(lengths=0.15, seed)`` (asl_dataset.py:220-253): that is
        ``torch.utils.data.random_split`` with ``Generator().manual_seed(seed)``, i.e. one ``torch.randperm`` whose
        first ``round(test_size * N)`` entries are the test set and the rest the train set, both in permutation order.

        With ``groups`` the same permutation is walked: while the test side holds fewer than ``n_test`` rows, a row whose group is
        not yet placed brings its WHOLE group to the test side (members in permutation order); everything else goes to train, in
        permutation order.  No group straddles the sides, the test side overshoots ``n_test`` by less than the largest group, and
        all-singleton groups give exactly the ungrouped split."""
        import torch
        n_test = int(round(len(self) * test_size)) if isinstance(test_size, float) else int(test_size)
        gen = torch.Generator().manual_seed(seed) if seed else None
        perm = torch.randperm(len(self), generator=gen).numpy()
        if self.groups is None:
            return self[perm[:n_test]], self[perm[n_test:]]
        test, train = grouped_split(perm, self.groups, n_test)
        return self[test], self[train]


def grouped_split(perm, groups, n_test):
    """``TokenDataset.split``'s walk over ``perm`` with ``groups`` -> (test indices, train indices), both in permutation order"""
    perm, groups = np.asarray(perm), np.asarray(groups)
    members = {}
    for i in perm.tolist():
        members.setdefault(int(groups[i]), []).append(i)
    side, test = {}, []                                      # group id -> True: on the test side
    for i in perm.tolist():
        g = int(groups[i])
        if g not in side:
            side[g] = len(test) < n_test
            if side[g]:
                test.extend(members[g])
    train = [i for i in perm.tolist() if not side[int(groups[i])]]
    return np.asarray(test, dtype=np.int64), np.asarray(train, dtype=np.int64)


def group_folds(what, option, y, groups, n_splits):
    """The folds of every splitter that honours groups, ``[(train indices, held-out indices), ...]``: ``StratifiedGroupKFold(
    n_splits)`` without shuffle on (``y``, ``groups``); where that raises ValueError (no class has as many members as there are
    folds) ``GroupKFold(n_splits)``; where there are fewer groups than folds a ValueError that names ``option`` and the counts --
    never an ungrouped split."""
    from sklearn.model_selection import GroupKFold, StratifiedGroupKFold
    y, groups = np.asarray(y), np.asarray(groups)
    n_groups = len(np.unique(groups))

    def refuse(why):
        return ValueError(f"{what}: {option}={n_splits} folds over {n_groups} groups of near-duplicate rows ({len(y)} rows): {why}; "
                          f"lower {option}, lower the radius of the groups or drop them (with_groups(None))")
    if n_groups < n_splits:
        raise refuse("a group stays on one side, so there cannot be more folds than groups")
    idx = np.zeros(len(y))
    try:
        return list(StratifiedGroupKFold(n_splits=n_splits).split(idx, y, groups))
    except ValueError:
        pass
    try:
        return list(GroupKFold(n_splits=n_splits).split(idx, y, groups))
    except ValueError as e:
        raise refuse(str(e)) from None


class DeviceRows:
    """Rows that are already on the device -- ``ids`` int64 [n, S], ``lengths`` int64 [n], ``y`` int64 [n], contiguous tensors on
    one device -- for the forward passes of a fitted estimator: ``NeuralNetClassifier._device_data`` hands the three tensors on as
    they are instead of uploading a ``TokenDataset`` (``LogProbJudge.attribute`` builds its occluded variants on the device)."""

    def __init__(self, ids, lengths, y):
        import torch
        for name, t, dim in (("ids", ids, 2), ("lengths", lengths, 1), ("y", y, 1)):
            if not (torch.is_tensor(t) and t.dtype == torch.int64 and t.dim() == dim and t.is_contiguous() and t.device == ids.device):
                raise ValueError(f"DeviceRows: {name} must be a contiguous int64 tensor of {dim} dimension(s) on the device of ids")
        if not len(ids) == len(lengths) == len(y):
            raise ValueError(f"DeviceRows: {len(ids)} rows of ids, {len(lengths)} lengths and {len(y)} labels")
        self.ids, self.lengths, self.y = ids, lengths, y

    def __len__(self):
        return int(self.y.shape[0])


def collate_data(data):
    """helper.py:293-304: list of ((ids, len), label) -> ({"X","lengths","y"}, y) int64 tensors."""
    import torch
    X, y = zip(*data)
    if len(X[0]) == 3:
        X, X_lengths, _ = zip(*X)
    elif len(X[0]) == 2:
        X, X_lengths = zip(*X)
    X = torch.tensor(X, dtype=torch.long)
    X_lengths = torch.tensor(X_lengths, dtype=torch.long)
    y = torch.tensor(y, dtype=torch.long)
    return {"X": X, "lengths": X_lengths, "y": y}, y


def synthetic_dataset(n, seq_len=48, src_vocab=3000, n_labels=200, seed=1, min_len=8, with_vocab=True):
    """Synthetic ASL-Phono-shaped dataset: ``n_labels`` glosses (+ <unk>, <pad>) and learnable
    structure -- each label draws its tokens from a label-specific slice of the vocabulary.
    ``with_vocab=False``: arrays only (tools/gen_golden.py runs with the reference's ``model`` package imported)."""
    from . import synth
    if with_vocab:
        from model.util import Vocab
    else:
        Vocab = lambda size: None
    rs = np.random.RandomState(seed)
    tgt_vocab = n_labels + 2
    X, lengths, _ = synth.make_batch(n, seq_len, src_vocab, tgt_vocab, seed=seed, min_len=min_len)
    y = rs.randint(2, tgt_vocab, size=n).astype(np.int64)
    span = max(4, (src_vocab - 2) // 8)
    base = 2 + (y * 37) % (src_vocab - 2 - span)
    sig = base[:, None] + rs.randint(0, span, size=X.shape)
    use = rs.random_sample(X.shape) < 0.6
    X = np.where((X != synth.PAD_IDX) & use, sig, X)
    return TokenDataset(X, lengths, y, Vocab(src_vocab), Vocab(tgt_vocab))
