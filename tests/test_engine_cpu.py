"""The two engine classes are one base plus what is theirs (slnlp/_engine.py).  Host only: no engine is constructed."""
import inspect

from slnlp import _engine, _lib, rnn_engine, tf_engine

# what a subclass may define although the base defines it (the base's version is a no-op or the family-neutral form)
OWN = {"TransformerEngine": {"__init__", "sync_params_version"}, "RnnEngine": set()}
# what is a subclass's alone: its batch signature and its plan type's switches
THEIRS = {
    "TransformerEngine": {"set_dmem_batched", "forward", "train_step_adam", "train_step", "train_step_graph", "step"},
    "RnnEngine": {"set_fused_backward", "set_persistent", "health", "forward", "train_step_adam", "train_step", "train_step_graph",
                  "step"},
}
EXTRA_CALLS = {"tf": {"params_changed", "set_dmem_batched"}, "rnn": {"set_fused_backward", "set_persistent", "health"}}


def _defined(cls):
    return {k for k, v in vars(cls).items() if inspect.isfunction(v) or isinstance(v, property)}


def test_both_engines_derive_from_plan_engine():
    assert issubclass(tf_engine.TransformerEngine, _engine.PlanEngine) and tf_engine.TransformerEngine.prefix == "tf"
    assert issubclass(rnn_engine.RnnEngine, _engine.PlanEngine) and rnn_engine.RnnEngine.prefix == "rnn"
    assert tf_engine.TransformerEngine.__mro__[1] is _engine.PlanEngine and rnn_engine.RnnEngine.__mro__[1] is _engine.PlanEngine


def test_every_call_of_the_base_exists_for_both_prefixes():
    src = inspect.getsource(_engine)
    import re
    named = set(re.findall(r'_call\("(\w+)"', src)) | set(re.findall(r'slnlp_\{(?:self\.)?prefix\}_(\w+)', src))
    assert named and named <= set(_engine.CALLS) | set(_engine.LAYOUT_CALLS), named - set(_engine.CALLS) - set(_engine.LAYOUT_CALLS)
    for prefix in ("tf", "rnn"):
        for name in _engine.CALLS + _engine.LAYOUT_CALLS:
            assert f"slnlp_{prefix}_{name}" in _lib.SIGNATURES, (prefix, name)
    for cls, prefix in ((tf_engine.TransformerEngine, "tf"), (rnn_engine.RnnEngine, "rnn")):
        own = set(re.findall(r'_call\("(\w+)"', inspect.getsource(cls)))
        assert own == EXTRA_CALLS[prefix], (prefix, own)
        for name in own:
            assert f"slnlp_{prefix}_{name}" in _lib.SIGNATURES, (prefix, name)


def test_subclasses_keep_only_what_is_theirs():
    base = _defined(_engine.PlanEngine)
    for cls in (tf_engine.TransformerEngine, rnn_engine.RnnEngine):
        mine = _defined(cls)
        assert mine & base == OWN[cls.__name__], (cls.__name__, sorted(mine & base))
        assert mine - base == THEIRS[cls.__name__], (cls.__name__, sorted(mine - base))
    # the settings every recent feature touched exist once
    for name in ("set_criterion", "set_update", "set_param_groups", "set_lr", "views", "load_state", "optim", "optim_adam", "backward",
                 "seed_dlogp", "tap", "staging", "loss", "grad_norm", "__del__"):
        assert name in base, name


def test_layout_helpers_stay_importable():
    cfg = tf_engine.make_config(32, 4, 2, 64, 64, 16, 4, 12)
    assert tf_engine.layout(cfg) == _engine.layout("tf", cfg)
    rcfg = rnn_engine.make_config("gru", 32, 32, 1, 64, 16, 4, 12)
    assert rnn_engine.layout(rcfg) == _engine.layout("rnn", rcfg)
