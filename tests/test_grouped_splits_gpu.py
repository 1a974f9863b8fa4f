"""GPU: leak-free splits end to end on the planted 300-row set (tests/dup_groups_ref.py: rows 100..159 are copies of rows 0..59, every
second copy altered in one token) -- ``split_audit`` finds the twins across an ungrouped split and none across the split of the
dataset that carries ``duplicate_groups``' labels; a tiny Transformer ``cross_fit`` keeps every group whole in its folds and in each
fit's internal valid split; the CLI key writes ``duplicate_groups.json`` and its run's own split audit comes out clean."""
import json
import os

import numpy as np
import pytest
import torch

import dup_groups_ref as ref

pytestmark = pytest.mark.gpu

SEED, RADIUS = 1, 1
CFG = dict(module__embedding_size=32, module__num_heads=4, module__num_layers=2, module__hidden_size=64)       # tests/test_net_gpu.py's


@pytest.fixture(scope="module")
def planted():
    """(the dataset, the restatement's distances, the restatement's groups at radius 1), formed once"""
    from model.util import Vocab
    from slnlp.data import TokenDataset
    X, L, y = ref.planted_rows()
    dist, none = ref.distances(X, L)
    return TokenDataset(X, L, y, Vocab(48), Vocab(14)), dist, ref.groups(dist, none, RADIUS)


@pytest.fixture(scope="module")
def grouped(planted):
    import slnlp
    ds, dist, want = planted
    res = slnlp.duplicate_groups(ds, RADIUS)
    assert np.array_equal(res["groups"], want["group"]) and (res["n_groups"], res["largest"], res["pairs"], res["rows_in_groups"]) == (240, 2, 60, 120)
    assert res["mixed_label_groups"] == 0 and res["flagged"] == 0
    return ds.with_groups(res)


def test_split_audit_finds_no_twin_across_the_grouped_split(planted, grouped):
    import slnlp
    ds, dist, want = planted
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(SEED)).numpy()
    te, tr = perm[:60], perm[60:]
    twins = int((dist[np.ix_(te, tr)] <= RADIUS).any(1).sum())                   # by the restatement: test rows with a twin in train
    pairs = int((dist[np.ix_(te, tr)] <= RADIUS).sum())
    print(f"seed {SEED}: the ungrouped split leaves {pairs} twin pairs across the sides ({twins} test rows)")
    assert pairs >= 5
    test, train = ds.split(0.2, SEED)
    leaky = slnlp.split_audit(train, test, radius=RADIUS)
    assert leaky["near_duplicates"] == twins and leaky["near_duplicates"] >= 5 and len(leaky["pairs"]) == twins
    test_g, train_g = grouped.split(0.2, SEED)
    assert not set(test_g.groups.tolist()) & set(train_g.groups.tolist()) and 60 <= len(test_g) < 62 and len(test_g) + len(train_g) == 300
    clean = slnlp.split_audit(train_g, test_g, radius=RADIUS)
    assert clean["near_duplicates"] == 0 and clean["exact_duplicates"] == 0 and clean["pairs"] == [] and not clean["duplicated"].any()
    assert clean["rows"] == len(test_g)


def test_cross_fit_keeps_groups_whole_in_folds_and_valid_splits(planted, grouped):
    import slnlp
    from slnlp.net import NeuralNetClassifier
    ds, dist, want = planted
    g = want["group"]
    net = NeuralNetClassifier(module="model.Transformer", module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                              module__batch_first=True, **CFG, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1,
                              optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05, max_epochs=1, batch_size=20, device="cuda",
                              gradient_clipping={"gradient_clip_value": 0.5})
    oof = slnlp.cross_fit(net, grouped, cv=3, seed=5)
    assert len(oof.members) == 3 and sorted(np.concatenate(oof.folds).tolist()) == list(range(300))
    everything = np.arange(300)
    for member, held_out in zip(oof.members, oof.folds):
        train = np.setdiff1d(everything, held_out)
        assert not set(g[train].tolist()) & set(g[held_out].tolist())            # the fold keeps every group whole
        part = grouped[train]
        assert np.array_equal(part.groups, g[train])
        tr, va = member._train_split(part)                                       # the split the member's fit took
        assert len(member.history) == 1 and np.isfinite(member.history[0]["valid_loss"])
        assert len(tr) + len(va) == len(train) and not set(part.groups[tr].tolist()) & set(part.groups[va].tolist())
        assert abs(len(va) - len(train) / 5) <= 2
    from slnlp.out_of_fold import cross_fit_folds
    assert any(set(g[t].tolist()) & set(g[h].tolist()) for t, h in cross_fit_folds(ds, 3))                                                            # the ungrouped folds of the same rows do cut groups
    proba = oof.predict_proba(grouped)
    assert proba.shape == (300, 14) and np.isfinite(proba).all()


def test_cli_writes_the_groups_and_a_clean_split_audit(tmp_path):
    import slnlp
    from slnlp import cli
    base = {"seed": 1, "cv": 2, "max_epochs": 1, "batch_size": 16, "test_size": 0.25, "scoring": ["neg_log_loss"],
            "model": "model.Transformer", "model_args": {"embedding_size": 16, "hidden_size": 32, "num_layers": 1, "dropout": 0.1, "num_heads": 2},
            "optimizer_args": {"momentum": 0.9}, "gradient_clipping": {"gradient_clip_value": 0.5}, "grid_args": {"lr": [0.05]},
            "dataset_args": {"synthetic": {"n": 96, "seq_len": 10, "src_vocab": 40, "n_labels": 5, "seed": 4, "min_len": 3}}}
    work = tmp_path / "run"
    cli.run(cli.load_config(None, dict(base, workdir=str(work), grouped_splits={"radius": 2}, baseline={"radius": 2, "top": 10})))
    assert {"duplicate_groups.json", "test_split_audit.json", "test_output.json"} <= set(os.listdir(work))
    got = json.load(open(work / "duplicate_groups.json"))
    ds = cli.load_dataset(base)
    want = ref.duplicate_groups(ds.ids, ds.lengths, 2)
    sizes = np.bincount(np.unique(want["group"], return_counts=True)[1])         # how many groups of every size
    assert got["options"] == {"radius": 2, "metric": "unit", "max_len": None}
    assert (got["rows"], got["radius"], got["max_distance"], got["n_groups"], got["pairs"], got["flagged"]) == (96, 2, 64, *(int(v) for v in want["head"][:3]))
    assert got["largest"] == len(sizes) - 1 > 1 and got["size_hist"] == {str(s): int(c) for s, c in enumerate(sizes) if c}
    assert "groups" not in got and "degree" not in got                           # the report without the per-row arrays
    audit = json.load(open(work / "test_split_audit.json"))                      # the end-to-end proof: no twin within the radius is left
    assert audit["radius"] == 2 and audit["near_duplicates"] == 0 and audit["exact_duplicates"] == 0 and audit["pairs"] == []
    test, train = ds.with_groups(want["group"]).split(0.25, 1)
    assert audit["rows"] == len(test) >= 24
    perm = torch.randperm(96, generator=torch.Generator().manual_seed(1)).numpy()            # ... which the ungrouped split does leave
    dist, _ = ref.distances(ds.ids, ds.lengths)
    twins = int((dist[np.ix_(perm[:24], perm[24:])] <= 2).any(1).sum())
    leaky_test, leaky_train = ds.split(0.25, 1)
    assert slnlp.split_audit(leaky_train, leaky_test, radius=2)["near_duplicates"] == twins > 0
