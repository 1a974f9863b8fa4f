"""CPU: the host side of ``weight_averaging`` -- the fp64 restatement the GPU tests lean on against torch's own
``AveragedModel``, the option's validation, and the ``n_averaged`` bookkeeping of the history rows."""
import numpy as np
import pytest
import torch

from average_ref import average_ref, bound


class _Three(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(7, 5))
        self.b = torch.nn.Parameter(torch.zeros(11))
        self.c = torch.nn.Parameter(torch.zeros(3, 2))


@pytest.mark.parametrize("kind", ["swa", "ema"])
def test_average_ref_is_torchs_averaged_model(kind):
    """Six updates of a 3-tensor module through ``torch.optim.swa_utils.AveragedModel`` (fp32) -- default ``avg_fn`` and
    ``get_ema_multi_avg_fn(0.9)`` -- against ``average_ref``: the formulas are torch's, not our reading of them."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    g = torch.Generator().manual_seed(3)
    model = _Three()
    averaged = AveragedModel(model) if kind == "swa" else AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    snaps, M = [], 0.0
    for _ in range(6):
        with torch.no_grad():
            for p in model.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 3.0)
        averaged.update_parameters(model)
        snaps.append(torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy().copy())
        M = max(M, float(np.abs(snaps[-1]).max()))
    assert int(averaged.n_averaged) == 6
    got = torch.cat([p.detach().reshape(-1) for p in averaged.module.parameters()]).numpy().astype(np.float64)
    want = average_ref(snaps, kind, 0.9)
    err = float(np.abs(got - want).max())
    print(f"[{kind}] max |torch fp32 - average_ref| = {err:.3e} (bound {bound(6, M):.3e})")
    assert err <= bound(6, M)
    # and it is an average at all: swa of six models is their mean
    if kind == "swa":
        assert np.allclose(want, np.mean(np.stack(snaps).astype(np.float64), axis=0), rtol=0, atol=1e-12)


def test_average_ref_copies_the_skip_range():
    rs = np.random.RandomState(0)
    snaps = [rs.randn(32).astype(np.float32) for _ in range(4)]
    out = average_ref(snaps, "ema", 0.5, skip=(8, 16))
    assert np.array_equal(out[8:16], snaps[-1][8:16].astype(np.float64))
    assert not np.array_equal(out[:8], snaps[-1][:8].astype(np.float64))


@pytest.mark.parametrize("bad", [{"kind": "polyak"}, {"kind": "ema", "decay": 1.0}, {"kind": "ema", "decay": 0.0},
                                 {"kind": "ema", "decay": -0.1}, {"kind": "ema", "decay": "0.9"}, {"kind": "swa", "start_epoch": 0},
                                 {"kind": "swa", "start_epoch": 1.5}, {"kind": "swa", "every": "step"}, {"kind": "swa", "cadence": "epoch"},
                                 {"kind": "swa", "predict": "yes"}, "swa"])
def test_bad_options_raise_value_error(bad):
    from slnlp.net import NeuralNetClassifier, averaging_options
    with pytest.raises(ValueError, match="weight_averaging"):
        averaging_options(bad)
    # ... and from initialize(), before anything else of the fit is set up (so also on a machine without a GPU)
    with pytest.raises(ValueError, match="weight_averaging"):
        NeuralNetClassifier(module="model.Transformer", weight_averaging=bad).initialize()


def test_options_defaults_and_sklearn_surface():
    from slnlp.net import NeuralNetClassifier, averaging_options
    assert averaging_options(None) is None
    assert averaging_options({"kind": "swa"}) == {"kind": "swa", "decay": 0.0, "every": "epoch", "start_epoch": 1, "predict": True}
    assert averaging_options({"kind": "ema", "every": "batch", "start_epoch": 3, "predict": False}) == \
        {"kind": "ema", "decay": 0.999, "every": "batch", "start_epoch": 3, "predict": False}
    net = NeuralNetClassifier(module="model.Transformer")
    assert net.get_params()["weight_averaging"] is None              # default off
    net.set_params(weight_averaging={"kind": "ema", "decay": 0.5})
    assert net.get_params()["weight_averaging"] == {"kind": "ema", "decay": 0.5} and net.weight_averaging["decay"] == 0.5


def _rows(opts, epochs, n_batches, history=None):
    from slnlp.net import next_n_averaged
    history = list(history or [])
    for _ in range(epochs):
        history.append({"epoch": len(history) + 1, "n_averaged": next_n_averaged(opts, history, n_batches)})
    return history


@pytest.mark.parametrize("every,start,want", [("epoch", 1, [1, 2, 3, 4, 5]), ("epoch", 3, [0, 0, 1, 2, 3]),
                                               ("batch", 1, [4, 8, 12, 16, 20]), ("batch", 3, [0, 0, 4, 8, 12])])
def test_n_averaged_from_the_history(every, start, want):
    from slnlp.net import averaging_options
    opts = averaging_options({"kind": "swa", "every": every, "start_epoch": start})
    assert [r["n_averaged"] for r in _rows(opts, 5, 4)] == want
    # across a resume: the loaded history's last row carries the count, the resumed fit goes on from it
    first = _rows(opts, 2, 4)
    resumed = _rows(opts, 3, 4, history=[dict(r) for r in first])
    assert [r["n_averaged"] for r in resumed] == want
    # a history written without the option (no such key) counts as nothing averaged so far
    bare = [{"epoch": 1}, {"epoch": 2}]
    assert _rows(opts, 1, 4, history=bare)[-1]["n_averaged"] == (0 if start > 3 else (1 if every == "epoch" else 4))


def test_lockstep_key_separates_what_a_group_cannot_share():
    from slnlp.lockstep import _avg_key
    from slnlp.net import averaging_options

    class Net:
        def __init__(self, setting):
            self._avg_opts = averaging_options(setting)
    ema = {"kind": "ema", "decay": 0.9, "every": "batch"}
    assert _avg_key(Net(None)) is None
    assert _avg_key(Net(ema)) == _avg_key(Net(dict(ema, start_epoch=4, predict=False)))     # per-fit settings
    assert len({_avg_key(Net(ema)), _avg_key(Net(dict(ema, decay=0.99))), _avg_key(Net(dict(ema, every="epoch"))),
                _avg_key(Net({"kind": "swa", "every": "batch"})), _avg_key(Net(None))}) == 5
