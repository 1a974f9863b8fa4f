"""GPU: weight averaging (SWA / EMA) kept on the device -- the two kernels through the C ABI against the fp64 restatement
(tests/average_ref.py, itself held to torch's ``AveragedModel`` on the CPU), the plans' averaging launches in eager, captured
and recorded steps, and the estimator option: bit-identity with the option off, the average against the model's own
snapshots, ``start_epoch``, predicting with the average, save / resume, lockstep groups, and the rejection of torch-stepped fits.

Every bound is ``average_ref.bound``: updates x 8 x 2^-24 x the largest magnitude fed in -- derived there, not tuned."""
import numpy as np
import pytest
import torch

import gold
from average_ref import average_ref, average_ref_dicts, bound

pytestmark = pytest.mark.gpu

# the accumulator launches at most 2048 blocks x 256 threads x one float4 (csrc/average.hip): three float4 past one full pass
WRAP_N = 4 * (2048 * 256 + 3)
# launches of ONE recorded train step (a one-fit lockstep group) at the two golden shapes below, counted on the commit before
# the averaging launches existed: a step without averaging must still issue exactly these
PARENT_LAUNCHES = {"tf": 96, "gru": 150}
ADDED_LAUNCHES = 2                      # the accumulator, then its one-thread count


def _randn(n, seed, scale=2.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


# ------------------------------------------------------------------------------------------------- kernels, C ABI ----
@pytest.mark.parametrize("kind", ["swa", "ema"])
@pytest.mark.parametrize("n,skip", [(4, (0, 0)), (4 * 257, (0, 0)), (WRAP_N, (0, 0)), (4 * 257, (16, 64))])
def test_average_step_against_the_fp64_reference(kind, n, skip):
    from slnlp import ops
    avg = torch.full((n,), float("nan"), device="cuda")           # the first update must overwrite whatever is there
    count = torch.zeros(1, device="cuda")
    snaps, M = [], 0.0
    for u in range(8):
        p = _randn(n, 100 * u + n % 97)
        ops.average_step(avg, p, count, kind=kind, decay=0.9, skip=skip)
        snaps.append(p.cpu().numpy())
        M = max(M, float(np.abs(snaps[-1]).max()))
        if u == 0:
            assert torch.equal(avg, p), "the first update is a bit copy"
        assert float(count) == u + 1
        if skip[1] > skip[0]:
            assert torch.equal(avg[skip[0]:skip[1]], p[skip[0]:skip[1]]), "skipped floats are copied, never averaged"
    want = average_ref(snaps, kind, 0.9, skip=skip)
    err = float(np.abs(avg.cpu().numpy().astype(np.float64) - want).max())
    print(f"[{kind} n={n} skip={skip}] max |avg - fp64| = {err:.3e} (bound {bound(8, M):.3e})")
    assert err <= bound(8, M)
    if skip[1] > skip[0]:                                          # ... and the floats around the range were averaged
        assert not torch.equal(avg[:skip[0]], p[:skip[0]]) and not torch.equal(avg[skip[1]:], p[skip[1]:])


@pytest.mark.parametrize("n", [4, WRAP_N])
def test_swap_arenas_exchanges_and_restores(n):
    from slnlp import ops
    a, b = _randn(n, 1), _randn(n, 2)
    a0, b0 = a.clone(), b.clone()
    ops.swap_arenas(a, b)
    assert torch.equal(a, b0) and torch.equal(b, a0)
    ops.swap_arenas(a, b)
    assert torch.equal(a, a0) and torch.equal(b, b0)


def test_bad_arguments_return_codes():
    from slnlp import ops
    a, b, c = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(1, device="cuda")
    with pytest.raises(RuntimeError, match="decay"):
        ops.average_step(a, b, c, kind="ema", decay=1.0)
    with pytest.raises(RuntimeError, match="skip range"):
        ops.average_step(a, b, c, kind="swa", skip=(4, 12))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.average_step(a[:6], b[:6], c, kind="swa")
    with pytest.raises(RuntimeError, match="overlap"):
        ops.swap_arenas(a, a)


# ---------------------------------------------------------------------------------------------------------- plans ----
def _plan_engine(kind):
    """A fresh engine at the ``tf_tiny`` / ``rnn_gru_tiny`` golden shape (dropout on) and five batches of its data."""
    from slnlp import synth
    if kind == "tf":
        from slnlp import tf_engine as te
        g, c, sd, X, L, y = gold.tf_case("tiny")
        eng = te.TransformerEngine(te.make_config(c["E"], c["H"], c["N"], c["F"], c["Vs"], c["Vt"], c["B"], c["S"], 1, 1, 0.1, 3), seed=7)
    else:
        from slnlp import rnn_engine as re_
        g, c, sd, X, L, y = gold.rnn_case("gru", "tiny")
        eng = re_.RnnEngine(re_.make_config("gru", c["E"], c["Hd"], c["N"], c["Vs"], c["Vt"], c["B"], c["S"], dropout=0.1), seed=7)
    eng.load_state(sd)
    eng.set_lr(0.05)
    Xn, Ln, yn = synth.make_batch(5 * c["B"], c["S"], c["Vs"], c["Vt"], seed=3, min_len=c["min_len"])
    X, L, y = (torch.from_numpy(a).cuda() for a in (Xn, Ln, yn))
    B = c["B"]
    batches = [((X[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) + ((L[i * B:(i + 1) * B],) if kind != "tf" else ())) for i in range(5)]
    return eng, batches, (X, y, L)


def _launch_count(eng, data, B):
    """Launches of one recorded train step of ``eng`` (a lockstep group of this one fit)."""
    from slnlp.lockstep import LockstepGroup
    X, y, L = data
    with torch.cuda.stream(torch.cuda.Stream()):
        grp = LockstepGroup([eng])
        grp.set_data(0, [X[:B]], [y[:B]], B, [L[:B]])
        grp.epoch(0, B, True, 0.9, 0.5)
        torch.cuda.synchronize()
        n = grp.num_launches(0, B, True)
        grp.close()
    return n


@pytest.mark.parametrize("kind", ["tf", "gru"])
def test_plan_averaging_eager_graph_and_recorded(kind):
    eng, batches, data = _plan_engine(kind)
    new = lambda: (torch.zeros_like(eng.params), torch.zeros(1, device="cuda"))
    avg, count = new()
    eng.set_averaging(avg, count, kind="ema", decay=0.9)
    snaps = []
    for b in batches:                                              # five eager steps, the arena copied out after each
        eng.train_step(*b)
        snaps.append(eng.params.clone())
    torch.cuda.synchronize()
    assert float(count) == 5
    snaps = [s.cpu().numpy() for s in snaps]
    M = max(float(np.abs(s).max()) for s in snaps)
    # (the RNN's dead pre_output_layer is copied by the plan: it never moves, so copy and average agree)
    err = float(np.abs(avg.cpu().numpy().astype(np.float64) - average_ref(snaps, "ema", 0.9)).max())
    print(f"[{kind}] eager: max |avg - fp64| = {err:.3e} (bound {bound(5, M):.3e})")
    assert err <= bound(5, M)
    # the same five steps as a captured graph: the same bits
    eng2, batches2, _ = _plan_engine(kind)
    avg2, count2 = new()
    eng2.set_averaging(avg2, count2, kind="ema", decay=0.9)
    with torch.cuda.stream(torch.cuda.Stream()):
        for b in batches2:
            eng2.train_step_graph(*b)
        torch.cuda.synchronize()
    assert torch.equal(eng2.params, eng.params) and torch.equal(avg2, avg) and float(count2) == 5
    # switched off again: the plan steps on, the average stands still
    eng2.set_averaging(None)
    before = avg2.clone()
    eng2.train_step(*batches2[0])
    torch.cuda.synchronize()
    assert torch.equal(avg2, before) and float(count2) == 5
    # launches of a recorded step: the parent's without averaging, two more with it
    eng3, _, data3 = _plan_engine(kind)
    B = batches[0][0].shape[0]
    off = _launch_count(eng3, data3, B)
    eng3.set_averaging(*new(), kind="ema", decay=0.9)
    on = _launch_count(eng3, data3, B)
    print(f"[{kind}] launches per recorded train step: {off} without averaging, {on} with")
    assert off == PARENT_LAUNCHES[kind]
    assert on == off + ADDED_LAUNCHES


# ------------------------------------------------------------------------------------------------------ estimator ----
CFG = dict(module__embedding_size=32, module__num_heads=4, module__num_layers=2, module__hidden_size=64)
BS = 20
SWA = {"kind": "swa", "every": "epoch"}


def dataset(n=80):
    from slnlp.data import synthetic_dataset
    return synthetic_dataset(n, seq_len=12, src_vocab=64, n_labels=6, seed=6, min_len=3)


def make_net(ds, seed=11, **kw):
    """An estimator on the ``tf_tiny``-sized module, initialised under ``seed`` (the weights are drawn there)."""
    from slnlp.net import NeuralNetClassifier
    args = dict(module="model.Transformer", module__dropout=0.1, module__src_vocab=ds.vocab_X, module__tgt_vocab=ds.vocab_y,
                module__batch_first=True, **CFG, criterion="torch.nn.CrossEntropyLoss", criterion__ignore_index=1,
                optimizer="torch.optim.SGD", optimizer__momentum=0.9, lr=0.05, max_epochs=3, batch_size=BS, device="cuda",
                gradient_clipping={"gradient_clip_value": 0.5})
    args.update(kw)
    net = NeuralNetClassifier(**args)
    torch.manual_seed(seed)
    return net.initialize()


def _sd(net):
    return {k: v.detach().cpu().clone() for k, v in net.module_.state_dict().items()}


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(torch.as_tensor(a[k]).cpu(), torch.as_tensor(b[k]).cpu()) for k in a)


def _param_names(net):
    return [n for n, _, _ in net.module_._entries]


@pytest.fixture(scope="module")
def ds():
    return dataset()


@pytest.fixture(scope="module")
def snapshots(ds):
    """The model after each of four epochs of the plain fit (no option), epoch by epoch through ``partial_fit``."""
    net = make_net(ds, max_epochs=1)
    out = []
    for _ in range(4):
        net.partial_fit(ds)
        out.append(_sd(net))
    return out, net.history


@pytest.fixture(scope="module")
def swa_fit(ds):
    return make_net(ds, weight_averaging=SWA).partial_fit(ds)


def _check_against_snapshots(net, snaps, kind="swa", decay=0.0):
    got = net.averaged_state_dict()
    names = _param_names(net)
    want = average_ref_dicts([{k: s[k].numpy() for k in names} for s in snaps], kind, decay)
    M = max(float(s[k].abs().max()) for s in snaps for k in names)
    err = max(float(np.abs(got[k].cpu().numpy().astype(np.float64) - want[k]).max()) for k in names)
    print(f"max |averaged_state_dict - fp64 of {len(snaps)} snapshots| = {err:.3e} (bound {bound(len(snaps), M):.3e})")
    assert err <= bound(len(snaps), M)
    for k in got:                                                  # buffers stay as they are
        if k not in names:
            assert torch.equal(got[k].cpu(), net.module_.state_dict()[k].cpu()), k


def test_option_on_keeps_the_fits_bits(ds, swa_fit, snapshots):
    off = make_net(ds).partial_fit(ds)
    assert _same(_sd(off), _sd(swa_fit))
    for a, b in zip(off.history, swa_fit.history):
        assert a["train_loss"] == b["train_loss"] and a["valid_loss"] == b["valid_loss"]
        assert [x.get("train_loss", x.get("valid_loss")) for x in a["batches"]] == [x.get("train_loss", x.get("valid_loss")) for x in b["batches"]]
        assert "n_averaged" not in a and set(b) - set(a) == {"n_averaged"}
    assert [r["n_averaged"] for r in swa_fit.history] == [1, 2, 3]
    assert _same(_sd(off), snapshots[0][2]), "three epochs through partial_fit, one at a time, are the three-epoch fit"


def test_epoch_cadence_average_is_the_average_of_the_epochs(swa_fit, snapshots):
    _check_against_snapshots(swa_fit, snapshots[0][:3])


def test_start_epoch(ds, snapshots):
    net = make_net(ds, weight_averaging=dict(SWA, start_epoch=2)).partial_fit(ds)
    assert [r["n_averaged"] for r in net.history] == [0, 1, 2] and net.n_averaged_ == 2
    _check_against_snapshots(net, snapshots[0][1:3])


def test_predict_uses_the_average_and_restores_the_weights(ds, swa_fit):
    before = _sd(swa_fit)
    proba = swa_fit.predict_proba(ds)
    assert _same(_sd(swa_fit), before), "the live weights come back bit for bit"
    fresh = make_net(ds, seed=99)                                  # the averaged weights as a module's own: a plain forward
    fresh.module_.load_state_dict(swa_fit.averaged_state_dict())
    assert np.array_equal(proba, fresh.predict_proba(ds))
    assert not np.array_equal(proba, make_net(ds, seed=99).predict_proba(ds))
    assert np.array_equal(swa_fit.predict(ds), swa_fit.classes_[proba.argmax(-1)])
    assert swa_fit.score(ds) == float((swa_fit.predict(ds) == ds.y).mean())
    assert _same(_sd(swa_fit), before)
    # swap_averaged on the module is the same route by hand: the average becomes the weights, twice restores them
    averaged = {k: v.cpu() for k, v in swa_fit.averaged_state_dict().items()}
    swa_fit.module_.swap_averaged()
    try:
        assert _same(_sd(swa_fit), averaged)
    finally:
        swa_fit.module_.swap_averaged()
    torch.cuda.synchronize()
    assert _same(_sd(swa_fit), before) and _same({k: v.cpu() for k, v in swa_fit.averaged_state_dict().items()}, averaged)


def test_predict_false_leaves_prediction_alone(ds, swa_fit):
    net = make_net(ds, weight_averaging=dict(SWA, predict=False)).partial_fit(ds)
    plain = make_net(ds)
    plain.module_.load_state_dict(net.module_.state_dict())
    assert np.array_equal(net.predict_proba(ds), plain.predict_proba(ds))
    assert not np.array_equal(net.predict_proba(ds), swa_fit.predict_proba(ds))
    assert _same(net.averaged_state_dict(), swa_fit.averaged_state_dict())      # the average is kept all the same


def test_save_load_resume_continues_the_average(ds, tmp_path):
    """save_params -> a fresh estimator -> load_params -> one more epoch == the uninterrupted four-epoch fit, weights and
    average bit for bit.  Dropout is off here: a checkpoint does not carry the dropout mask stream's position, so with dropout
    a resumed fit's WEIGHTS already differ from the uninterrupted fit's (with or without averaging) and there is no common
    fourth model to average."""
    import os
    kw = dict(module__dropout=0.0, weight_averaging=SWA)
    whole = make_net(ds, max_epochs=4, **kw).partial_fit(ds)
    three = make_net(ds, **kw).partial_fit(ds)
    three.save_params(str(tmp_path / "ck"))
    saved = torch.load(str(tmp_path / "ck" / "averaged.pt"))
    assert saved["n_averaged"] == 3 and all(not v.is_cuda for v in saved["state_dict"].values())
    assert _same(saved["state_dict"], three.averaged_state_dict())
    resumed = make_net(ds, seed=5, max_epochs=1, **kw)
    resumed.load_params(str(tmp_path / "ck"))
    assert _same(resumed.averaged_state_dict(), three.averaged_state_dict()) and resumed.n_averaged_ == 3
    resumed.partial_fit(ds)
    assert [r["n_averaged"] for r in resumed.history] == [1, 2, 3, 4]
    assert _same(_sd(resumed), _sd(whole)), "the resumed fit itself"
    assert _same(resumed.averaged_state_dict(), whole.averaged_state_dict())
    assert np.array_equal(resumed.predict_proba(ds), whole.predict_proba(ds))
    # without the option no such file is written
    make_net(ds).save_params(str(tmp_path / "plain"))
    assert "averaged.pt" not in os.listdir(tmp_path / "plain") and "params.pt" in os.listdir(tmp_path / "plain")


def test_batch_cadence_is_the_average_of_every_step(ds):
    """``every="batch"``: the launches ride each train step from ``start_epoch`` on.  One batch per epoch makes the epoch
    snapshots the step snapshots."""
    kw = dict(batch_size=200, max_epochs=1, train_split=None)
    plain = make_net(ds, **kw)
    snaps = []
    for _ in range(3):
        plain.partial_fit(ds)
        snaps.append(_sd(plain))
    net = make_net(ds, **dict(kw, max_epochs=3), weight_averaging={"kind": "ema", "decay": 0.9, "every": "batch", "start_epoch": 2})
    net.partial_fit(ds)
    assert [r["n_averaged"] for r in net.history] == [0, 1, 2] and _same(_sd(net), snaps[-1])
    _check_against_snapshots(net, snaps[1:], "ema", 0.9)


def test_lockstep_group_matches_solo_fits(ds):
    from slnlp.lockstep import fit_lockstep, predict_proba_lockstep
    ema = {"kind": "ema", "decay": 0.9, "every": "batch"}
    settings = [ema, dict(ema, start_epoch=2), ema]                # the second fit rides with a null entry for an epoch
    lrs = [0.05, 0.02, 0.1]
    solo = [make_net(ds, seed=20 + f, lr=lr, weight_averaging=s).partial_fit(ds) for f, (lr, s) in enumerate(zip(lrs, settings))]
    lock = [make_net(ds, seed=20 + f, lr=lr, weight_averaging=s) for f, (lr, s) in enumerate(zip(lrs, settings))]
    fit_lockstep(lock, [ds] * 3)
    strip = lambda h: [{k: v for k, v in r.items() if k != "dur"} for r in h]
    for f, (a, b) in enumerate(zip(solo, lock)):
        assert strip(a.history) == strip(b.history), f
        assert _same(_sd(a), _sd(b)), f
        assert _same(a.averaged_state_dict(), b.averaged_state_dict()), f
    assert [r["n_averaged"] for r in lock[1].history] == [0, 4, 8] and [r["n_averaged"] for r in lock[0].history] == [4, 8, 12]
    before = [_sd(n) for n in lock]
    probas = predict_proba_lockstep(lock, [ds] * 3)
    for f, (n, p) in enumerate(zip(lock, probas)):
        assert np.array_equal(p, n.predict_proba(ds)), f
        assert np.array_equal(p, solo[f].predict_proba(ds)), f
        assert _same(_sd(n), before[f]), f


def test_torch_stepped_fit_is_rejected(ds):
    with pytest.raises(ValueError, match="fused fits only"):
        make_net(ds, optimizer="torch.optim.RMSprop", optimizer__momentum=0.0, weight_averaging=SWA)
