"""Host-side owner of one plan of libslnlp, whatever its type: what ``tf_engine.TransformerEngine`` (``slnlp_tf_*``) and
``rnn_engine.RnnEngine`` (``slnlp_rnn_*``) share.

PyTorch is plumbing here: it allocates the flat parameter / gradient / momentum arenas and the activation workspace in HBM
and provides the stream; the layout, the launch sequence and all arithmetic live in the HIP library.  The two C families
take the same arguments but for the batch -- ``X, y`` or ``X, y, lengths`` -- so the subclasses keep their own forward /
step signatures and hand the batch on as a tuple.
"""
import ctypes as C

import torch

from . import _lib
from .launch import LaunchPolicy
from ._lib import TfBuffers, check, load, ptr

# every slnlp_<prefix>_<name> a PlanEngine calls through _call (tests/test_engine_cpu.py holds them against _lib.SIGNATURES)
CALLS = ("create", "destroy", "set_destroy_sync", "set_criterion", "set_update", "set_param_groups", "set_averaging", "forward", "seed_dlogp",
         "backward", "optim", "optim_adam", "train_step", "graph_capture_train", "graph_launch", "tap")
LAYOUT_CALLS = ("num_params", "param_info", "arena_floats", "workspace_bytes")


def layout(prefix, cfg):
    """[(name, shape tuple, offset in floats)] in reference state_dict order + arena size.
    Pure host query: works without a GPU."""
    lib = load()
    n = getattr(lib, f"slnlp_{prefix}_num_params")(C.byref(cfg))
    if n < 0:
        check(1, f"{prefix}_num_params")
    out = []
    for i in range(n):
        name = C.create_string_buffer(128)
        shape = (C.c_int64 * 2)()
        ndim, off = C.c_int32(0), C.c_int64(0)
        check(getattr(lib, f"slnlp_{prefix}_param_info")(C.byref(cfg), i, name, C.byref(shape), C.byref(ndim), C.byref(off)),
              f"{prefix}_param_info")
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(ndim.value)), int(off.value)))
    return out, int(getattr(lib, f"slnlp_{prefix}_arena_floats")(C.byref(cfg)))


class PlanEngine:
    """One plan = one (config, max batch) on one GPU / one stream."""
    prefix = None       # "tf" / "rnn": the C family
    pe = None           # positional table [max_len, E] (the Transformer's)

    def __init__(self, cfg, device="cuda", seed=0, params=None, grads=None, momentum=None, rng=None, lr=None, scalars=None):
        """``params`` / ``grads`` / ``momentum``: adopt arenas owned by the caller (the drop-in modules keep their
        nn.Parameters as views of ``params``)."""
        _lib.require_gpu()
        self._alloc_stream = self._last_stream = torch.cuda.current_stream(torch.device(device))   # whose pool the buffers come from
        self.cfg = cfg
        self.device = dev = torch.device(device)
        self.entries, self.arena_floats = layout(self.prefix, cfg)
        mk = lambda t: torch.zeros(self.arena_floats, dtype=torch.float32, device=dev) if t is None else t
        self.params, self.grads, self.momentum = mk(params), mk(grads), mk(momentum)
        for t in (self.params, self.grads, self.momentum):
            assert t.is_cuda and t.dtype == torch.float32 and t.numel() == self.arena_floats and t.is_contiguous()
        ws = int(getattr(load(), f"slnlp_{self.prefix}_workspace_bytes")(C.byref(cfg)))
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=dev)
        # rng = {seed, dropout step counter}; lr: read from device memory by the update kernel.  A module with several
        # plans (one per sequence length) hands every plan the same two tensors
        self.rng = torch.tensor([seed, 0], dtype=torch.int64, device=dev) if rng is None else rng
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev) if lr is None else lr
        self.scalars = torch.zeros(4, dtype=torch.float32, device=dev) if scalars is None else scalars   # {loss, grad norm, Adam step count, -}
        self.logp = torch.empty(cfg.B, cfg.Vt, dtype=torch.float32, device=dev)
        bufs = TfBuffers(ptr(self.params), ptr(self.grads), ptr(self.momentum), ptr(self.pe), ptr(self.workspace),
                         ptr(self.rng), ptr(self.lr), ptr(self.scalars))
        handle = C.c_void_p()
        check(getattr(load(), f"slnlp_{self.prefix}_create")(C.byref(cfg), C.byref(bufs), C.byref(handle)), f"{self.prefix}_create")
        self.handle = handle
        # every buffer of this plan is a torch tensor from the stream-ordered caching allocator, and __del__ waits for the
        # plan's last stream when that is not the allocating one: the plan itself needs no device-wide wait when it goes
        # away (which would stall the other host threads' queued work each time a fit ends).  Per plan, not process-wide.
        self._call("set_destroy_sync", 0)
        self._graph_keys = {}
        self._launch = LaunchPolicy()
        self._xbuf = self._ybuf = self._lbuf = None

    def _call(self, name, *args):
        """slnlp_<prefix>_<name>(handle, ...), its status checked."""
        check(getattr(load(), f"slnlp_{self.prefix}_{name}")(self.handle, *args), f"{self.prefix}_{name}")

    def _sp(self):
        """Pointer of the stream this call runs on; remembered for the destructor."""
        st = self._last_stream = torch.cuda.current_stream(self.device)
        return st.cuda_stream

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                # the buffers return to the pool of the stream they were allocated on: if the plan last ran on another
                # stream, that work must be over first (same stream: the allocator's stream order covers it)
                ls, al = getattr(self, "_last_stream", None), getattr(self, "_alloc_stream", None)
                if ls is not None and al is not None and ls != al:
                    ls.synchronize()
                getattr(load(), f"slnlp_{self.prefix}_destroy")(h)
            except Exception:
                pass
            self.handle = None

    _pv = None

    def sync_params_version(self):
        """Before a launch that reads data derived from the arena (the Transformer's weight planes); nothing to do here."""

    # ---- parameter access ------------------------------------------------
    def views(self, arena=None):
        """name -> tensor view into ``arena`` (default: the parameter arena)."""
        arena = self.params if arena is None else arena
        out = {}
        for name, shape, off in self.entries:
            n = 1
            for s in shape:
                n *= s
            out[name] = arena[off:off + n].view(*shape)
        return out

    def load_state(self, sd):
        for k, t in self.views().items():
            t.copy_(torch.as_tensor(sd[k]).to(self.device, torch.float32))

    def set_criterion(self, weight=None, label_smoothing=0.0, reduction="mean"):
        """CrossEntropyLoss settings of every later forward (train and eval): ``weight`` [Vt] or None, ``label_smoothing``,
        ``reduction`` "mean" / "sum".  A change drops the plan's captured graphs (re-captured on the next graph step)."""
        w = None if weight is None else torch.as_tensor(weight).detach().to("cpu", torch.float32).contiguous()   # host memory
        if w is not None and w.shape != (self.cfg.Vt,):
            raise ValueError(f"set_criterion: weight of shape {tuple(w.shape)}, expected ({self.cfg.Vt},) -- one per target class")
        self._call("set_criterion", ptr(w), float(label_smoothing), _lib.REDUCTIONS[reduction], self._sp())
        self._graph_keys = {}

    def set_update(self, kind="sgd", dampening=0.0, weight_decay=0.0, nesterov=False):
        """Update rule of the fused step: "sgd" (``optim`` / ``step`` run torch.optim.SGD with these settings), "adam" or
        "adamw" (``optim_adam`` runs Adam / AdamW with the weight decay of that call; ``weight_decay`` here is the fit's own in
        a lockstep group, slnlp.lockstep)."""
        self._call("set_update", _lib.UPDATE_KINDS[kind], float(dampening), float(weight_decay), int(bool(nesterov)))
        self._graph_keys = {}

    def set_param_groups(self, table=None, lr=None):
        """Per-parameter-group lr / weight decay of the fused update (``optimizer__param_groups``): ``table`` {seg_begin,
        seg_group, weight_decay} as ``slnlp.param_groups.segments`` builds it, ``lr`` the float32 device tensor [groups] the
        update reads every step (the caller writes the rates there; ``set_lr`` is then not read by the update).  None clears
        the table: the one-group update again.  A change drops the plan's captured graphs."""
        if not table:
            self._call("set_param_groups", 0, None, None, 0, None, None, self._sp())
            self._group_lr = None
        else:
            begin, group, wd = list(table["seg_begin"]), list(table["seg_group"]), list(table["weight_decay"])
            if lr is None or not lr.is_cuda or lr.dtype != torch.float32 or lr.numel() != len(wd) or not lr.is_contiguous():
                raise ValueError(f"set_param_groups: lr must be a contiguous float32 device tensor of {len(wd)} rates")
            self._call("set_param_groups", len(begin), (C.c_int64 * len(begin))(*begin), (C.c_int32 * len(group))(*group),
                       len(wd), (C.c_float * len(wd))(*wd), ptr(lr), self._sp())
            self._group_lr = lr                  # kept alive: the update kernels read it
        self._graph_keys = {}

    def set_averaging(self, avg=None, count=None, kind="swa", decay=0.0):
        """Weight averaging riding the train step: every update of this plan is followed by the accumulator's two launches on
        ``avg`` (arena-shaped float32 device tensor) and ``count`` ([1] float32, the models averaged so far) -- "swa" or "ema"
        with ``decay`` (``ops.average_step``).  ``avg`` None removes them.  A change drops the plan's captured graphs."""
        if avg is None:
            self._call("set_averaging", None, None, 0, 0.0)
        else:
            if not (avg.is_cuda and avg.dtype == torch.float32 and avg.numel() == self.arena_floats and avg.is_contiguous()):
                raise ValueError("set_averaging: avg must be a contiguous float32 device tensor of the arena's size")
            self._call("set_averaging", ptr(avg), ptr(count), _lib.AVERAGE_KINDS[kind], float(decay))
        self._averaging = (avg, count)       # kept alive: the step's launches write them
        self._graph_keys = {}

    def params_changed(self):
        """The arena was rewritten by a launch through its raw pointer (``ops.swap_arenas``), which moves no tensor version
        counter: the next ``sync_params_version`` tells the plan whatever the counter says."""
        self._pv = None

    def set_lr(self, lr):
        self.lr.fill_(float(lr))

    # ---- compute: `ids` is the batch as the C family takes it, (X, y) or (X, y, lengths), int64 on the device ------
    def _forward(self, ids, train):
        """-> log-probs [B, Vt] (a view of the engine's output buffer, valid until the next call)."""
        self.sync_params_version()
        ids = self._keep = tuple(t.contiguous() for t in ids)  # backward reads the ids again
        B = ids[0].shape[0]
        self._call("forward", *map(ptr, ids), B, int(train), ptr(self.logp), self._sp())
        return self.logp[:B]

    def seed_dlogp(self, dlogp):
        self._call("seed_dlogp", ptr(dlogp.contiguous()), self._sp())

    def backward(self):
        self._call("backward", self._sp())

    def optim(self, momentum=0.9, max_norm=0.5):
        self._call("optim", momentum, max_norm, self._sp())

    def optim_adam(self, exp_avg_sq, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.5):
        """clip_grad_norm_ + torch.optim.Adam fused (exp_avg = the momentum arena, exp_avg_sq = ``exp_avg_sq``, step count in
        ``scalars[2]``)."""
        self._call("optim_adam", ptr(exp_avg_sq), betas[0], betas[1], eps, weight_decay, max_norm, self._sp())

    def _train_step_adam(self, ids, exp_avg_sq, betas, eps, weight_decay, max_norm):
        logp = self._forward(ids, True)
        self.backward()
        self.optim_adam(exp_avg_sq, betas, eps, weight_decay, max_norm)
        return logp

    def _train_step(self, ids, momentum, max_norm):
        """Eager fwd + criterion + bwd + clip + SGD; returns log-probs view.
        loss / grad-norm stay on the device in ``scalars[0:2]``."""
        self.sync_params_version()
        ids = self._keep = tuple(t.contiguous() for t in ids)
        B = ids[0].shape[0]
        self._call("train_step", *map(ptr, ids), B, momentum, max_norm, ptr(self.logp), self._sp())
        return self.logp[:B]

    def staging(self):
        """The plan's fixed staging buffers ``(X [B, S], lengths [B], y [B])``: what a captured graph reads.  A shuffled fit
        gathers its batches straight into them (``ops.gather_batch(..., out=engine.staging())``) and steps on the views it gets
        back; the lengths buffer is there for the uniform call, the Transformer never reads it."""
        if self._xbuf is None:
            dev = self.device
            self._xbuf = torch.empty(self.cfg.B, self.cfg.S, dtype=torch.int64, device=dev)
            self._ybuf = torch.empty(self.cfg.B, dtype=torch.int64, device=dev)
            self._lbuf = torch.empty(self.cfg.B, dtype=torch.int64, device=dev)
        return self._xbuf, self._lbuf, self._ybuf

    def _train_step_graph(self, ids, momentum, max_norm):
        """Same step replayed from a captured hipGraph (one per batch size):
        the batch is copied into fixed staging buffers (unless it was gathered there), then one graph launch."""
        self.sync_params_version()
        B = ids[0].shape[0]
        key = (B, float(momentum), float(max_norm))
        self.staging()
        bufs = [b[:B] for b in (self._xbuf, self._ybuf, self._lbuf)[:len(ids)]]
        for dst, src in zip(bufs, ids):
            if src.data_ptr() != dst.data_ptr():          # a shuffled fit's batch was gathered here already
                dst.copy_(src)
        st = self._sp()
        if st == 0:
            raise RuntimeError("train_step_graph needs a non-default stream (use torch.cuda.stream(...))")
        if self._graph_keys.get(B) != key:       # one captured graph per batch size, kept by the plan
            self._call("graph_capture_train", *map(ptr, bufs), B, momentum, max_norm, ptr(self.logp), st)
            self._graph_keys[B] = key
        self._call("graph_launch", B, st)
        return self.logp[:B]

    def _step(self, ids, momentum, max_norm, graph):
        """graph: True (hipGraph replay) / False (eager launches) / "auto" (time both, keep the faster; launch.py)."""
        if graph == "auto" and self._sp() == 0:
            graph = False                    # graph capture needs a non-default stream
        if graph == "auto":
            return self._launch.run((ids[0].shape[0], float(momentum), float(max_norm)),
                                    lambda: self._train_step_graph(ids, momentum, max_norm),
                                    lambda: self._train_step(ids, momentum, max_norm))
        return (self._train_step_graph if graph else self._train_step)(ids, momentum, max_norm)

    def tap(self, name, rows, cols):
        out = torch.empty(rows, cols, dtype=torch.float32, device=self.device)
        n = C.c_int64(0)
        self._call("tap", name.encode(), ptr(out), out.numel(), C.byref(n), self._sp())
        assert n.value == rows * cols, (name, n.value, rows, cols)
        return out

    @property
    def loss(self):
        return float(self.scalars[0])

    @property
    def grad_norm(self):
        return float(self.scalars[1])
