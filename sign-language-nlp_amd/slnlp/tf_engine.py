"""Host-side owner of one Transformer plan (libslnlp ``slnlp_tf_*``): ``_engine.PlanEngine`` plus what is the
Transformer's own -- the positional table, the arena's version counter, the two-argument batch.
"""
import math

import torch

from . import _engine, _lib
from ._lib import TfConfig


def positional_table(max_len, d_model):
    """Sinusoidal table, same arithmetic (torch fp32 ops) as
    /root/reference/model/component/positional_encoding.py:27-35 -> bit-identical
    to the reference's ``pe`` buffer.  Shape [max_len, d_model]."""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def make_config(E, H, N, F, Vs, Vt, B, S, pad_src=1, pad_tgt=1, dropout=0.0, precision=3):
    return TfConfig(E, H, N, F, Vs, Vt, B, S, pad_src, pad_tgt, float(dropout), precision)


def layout(cfg):
    """[(name, shape tuple, offset in floats)] in reference state_dict order + arena size.
    Pure host query: works without a GPU."""
    return _engine.layout("tf", cfg)


class TransformerEngine(_engine.PlanEngine):
    prefix = "tf"

    def __init__(self, cfg, device="cuda", seed=0, max_len=5000, params=None, grads=None, momentum=None, pe=None, rng=None, lr=None, scalars=None):
        """``pe``: adopt the caller's positional table [>= S, E] as the arenas are adopted."""
        _lib.require_gpu()
        self.pe = positional_table(max_len, cfg.E).to(torch.device(device)) if pe is None else pe   # [max_len, E]
        self._pv = None
        super().__init__(cfg, device, seed, params, grads, momentum, rng, lr, scalars)

    def sync_params_version(self):
        """The fused update keeps the bf16 weight planes current; a write to the arena from the torch side (load_state_dict,
        a torch optimizer, an in-place edit -- all of which move the tensor's version counter, which kernel launches through
        raw pointers do not) makes them stale: tell the plan before the next launch."""
        v = self.params._version
        if v != self._pv:
            self._call("params_changed")
            self._pv = v

    def set_dmem_batched(self, on=True):
        """d memory of all decoder layers in one launch behind the decoder's backward loop (default) or a launch per layer
        inside it: same bits, an A / B switch."""
        self._call("set_dmem_batched", int(bool(on)))
        self._graph_keys = {}

    # ---- compute: the Transformer ignores ``lengths`` (transformer.py:60) ------------------------------------------
    def forward(self, X, y, train=False):
        """X int64 [B,S], y int64 [B] on the device -> log-probs [B,Vt] (a view
        of the engine's output buffer, valid until the next call)."""
        return self._forward((X, y), train)

    def train_step_adam(self, X, y, exp_avg_sq, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.5, lengths=None):
        return self._train_step_adam((X, y), exp_avg_sq, betas, eps, weight_decay, max_norm)

    def train_step(self, X, y, momentum=0.9, max_norm=0.5):
        return self._train_step((X, y), momentum, max_norm)

    def train_step_graph(self, X, y, momentum=0.9, max_norm=0.5):
        return self._train_step_graph((X, y), momentum, max_norm)

    def step(self, X, y, lengths=None, momentum=0.9, max_norm=0.5, graph="auto"):
        """Uniform fused-step entry (estimator)."""
        return self._step((X, y), momentum, max_norm, graph)
