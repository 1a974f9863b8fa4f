"""Host-side owner of one EncoderDecoder{LSTM,GRU}Attn plan (libslnlp ``slnlp_rnn_*``): ``_engine.PlanEngine`` plus what
is the RNN plan's own -- the backward / persistent switches, the health flag, the three-argument batch."""
import ctypes as C

from . import _engine
from ._lib import RnnConfig


def make_config(rnn_type, E, Hd, N, Vs, Vt, B, S, pad_src=1, pad_tgt=1, bos_idx=0, dropout=0.0, precision=3):
    assert rnn_type in ("lstm", "gru"), "Invalid `rnn_type`."       # bkp.py:347
    return RnnConfig(int(rnn_type == "lstm"), E, Hd, N, Vs, Vt, B, S, pad_src, pad_tgt, bos_idx, float(dropout), precision)


def layout(cfg):
    """[(name, shape, offset)] in reference state_dict order + arena size; host-only query."""
    return _engine.layout("rnn", cfg)


class RnnEngine(_engine.PlanEngine):
    prefix = "rnn"

    def forward(self, X, y, lengths, train=False):
        return self._forward((X, y, lengths), train)

    def train_step_adam(self, X, y, exp_avg_sq, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.5, lengths=None):
        return self._train_step_adam((X, y, lengths), exp_avg_sq, betas, eps, weight_decay, max_norm)

    def train_step(self, X, y, lengths, momentum=0.9, max_norm=0.5):
        return self._train_step((X, y, lengths), momentum, max_norm)

    def train_step_graph(self, X, y, lengths, momentum=0.9, max_norm=0.5):
        return self._train_step_graph((X, y, lengths), momentum, max_norm)

    def step(self, X, y, lengths, momentum=0.9, max_norm=0.5, graph="auto"):
        """Uniform fused-step entry (estimator)."""
        return self._step((X, y, lengths), momentum, max_norm, graph)

    def set_fused_backward(self, on):
        """False: backward through time as the cell kernel + K-sliced grouped GEMM pair (the comparison path of the tests)."""
        self._call("set_fused_backward", int(bool(on)))

    def set_persistent(self, on):
        """True: each encoder layer's timesteps in one persistent launch (opt-in; one fit per GPU only)."""
        self._call("set_persistent", int(bool(on)))

    def health(self):
        """0 = every device-wide barrier of the persistent layer kernels completed; synchronises."""
        st = C.c_int32(-1)
        self._call("health", C.byref(st))
        return st.value
