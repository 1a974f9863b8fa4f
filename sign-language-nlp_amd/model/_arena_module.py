"""Shared machinery of the HIP-backed drop-in modules: every nn.Parameter is a view of ONE flat
fp32 arena whose layout the HIP library defines, and the forward is a ``torch.autograd.Function``
whose backward launches the HIP backward and hands each parameter its gradient."""
import torch
import torch.nn as nn


class _Holder(nn.Module):
    """Name-space node so parameters get the reference's dotted key names."""


def _register(root, dotted, tensor, is_param=True):
    parts = dotted.split(".")
    node = root
    for p in parts[:-1]:
        if not hasattr(node, p):
            node.add_module(p, _Holder())
        node = getattr(node, p)
    if is_param:
        node.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=True))
    else:
        node.register_buffer(parts[-1], tensor)


class _HipFn(torch.autograd.Function):
    """log-probs = HIP forward; backward = HIP backward into the gradient arena."""

    @staticmethod
    def forward(ctx, module, inputs, *params):
        eng = module._engine_for(inputs[0].shape[0], inputs[0].shape[1])
        logp = eng.forward(*inputs, train=True).clone()
        ctx.module, ctx.eng = module, eng
        return logp

    @staticmethod
    def backward(ctx, dlogp):
        eng = ctx.eng
        eng.seed_dlogp(dlogp)
        eng.backward()
        # the fused clip+SGD kernel advances the dropout step counter; on this path (stock torch.optim / skorch loop)
        # nothing else would, and every step would redraw the SAME masks
        eng.rng[1:2].add_(1)
        gv = eng.views(eng.grads)
        dead = ctx.module._dead_params
        grads = tuple(None if name in dead else gv[name].clone() for name in ctx.module._param_names)
        return (None, None) + grads


class ArenaModule(nn.Module):
    """Subclasses set ``_entries`` [(name, shape, offset)], ``_arena_floats`` and implement
    ``_state_order(views)`` (registration order incl. buffers) and ``_make_engine(B, S, old)``."""

    _dead_params = frozenset()

    def _setup_arena(self, entries, total, init_values, recipe=None, recipe_seed=0):
        """init_values: {name: tensor} drawn by the caller (the reference-identical CPU stream), or None with a `recipe`
        {name: (kind, scale[, zero_row])}: the same distributions drawn by ``_materialize`` on whatever device the arena lands
        on, from a generator seeded with `recipe_seed` -- no CPU modules are built and no global RNG is consumed."""
        self._entries = entries
        self._param_names = [n for n, _, _ in entries]
        self._engines = {}
        self._opt_state = None      # (grads, momentum, rng, lr) on the device: ONE set per module, shared by every plan
        self._pending_recipe = None
        if init_values is None:
            assert recipe is not None, "either initial values or an init recipe"
            self._pending_recipe = (dict(recipe), int(recipe_seed))
            self._build(torch.empty(total, dtype=torch.float32))      # untouched pages until it is materialised
        else:
            self._build(torch.zeros(total, dtype=torch.float32), init_values)

    def _materialize(self):
        """Draw the pending init recipe into the arena, on the arena's device (one generator, tensors in layout order)."""
        pend = getattr(self, "_pending_recipe", None)
        if pend is None:
            return
        recipe, seed = pend
        self._pending_recipe = None
        arena = self._arena
        g = torch.Generator(device=arena.device)
        g.manual_seed(seed)
        with torch.no_grad():
            for name, shape, off in self._entries:
                n = 1
                for d in shape:
                    n *= d
                v = arena[off:off + n].view(*shape)
                kind, scale, *rest = recipe[name]
                if kind == "normal":
                    v.normal_(0.0, scale, generator=g)
                elif kind == "uniform":
                    v.uniform_(-scale, scale, generator=g)
                elif kind == "const":
                    v.fill_(scale)
                else:
                    raise ValueError(f"init recipe: unknown kind {kind!r} for {name}")
                if rest and rest[0] is not None:
                    v[rest[0]].zero_()                   # nn.Embedding(padding_idx=...) keeps that row at zero

    def state_dict(self, *args, **kwargs):
        self._materialize()
        return super().state_dict(*args, **kwargs)

    def _shared_state(self):
        """Gradient / momentum arenas, dropout rng {seed, step} and lr live on the module, not on a plan: training with
        more than one sequence length (per-batch padding) must not split the momentum or restart the mask stream."""
        dev = self._arena.device
        st = self._opt_state
        if st is None or st["grads"].device != dev:
            n = self._arena.numel()
            st = self._opt_state = {
                "grads": torch.zeros(n, dtype=torch.float32, device=dev), "momentum": torch.zeros(n, dtype=torch.float32, device=dev),
                "rng": torch.tensor([self.seed, 0], dtype=torch.int64, device=dev), "lr": torch.zeros(1, dtype=torch.float32, device=dev),
                "scalars": torch.zeros(4, dtype=torch.float32, device=dev)}
        return st

    def adam_second_moment(self):
        """Arena-shaped exp_avg_sq buffer of the fused Adam update (allocated on first use)."""
        st = self._shared_state()
        if "exp_avg_sq" not in st:
            st["exp_avg_sq"] = torch.zeros_like(st["momentum"])
        return st["exp_avg_sq"]

    def averaged_arena(self):
        """(avg, count): the arena-shaped running average of the weights and the number of models averaged so far, a device
        float (allocated on first use, zero: the first update copies)."""
        st = self._shared_state()
        if "averaged" not in st:
            st["averaged"] = torch.zeros_like(st["momentum"])
            st["n_averaged"] = torch.zeros(1, dtype=torch.float32, device=st["momentum"].device)
        return st["averaged"], st["n_averaged"]

    def has_averaged(self):
        st = self._opt_state
        return st is not None and "averaged" in st and st["averaged"].device == self._arena.device

    def set_averaging(self, kind=None, decay=0.0):
        """Weight averaging riding every train step (``kind`` "swa" / "ema"; None: off), for every plan of the module, now and
        created later -- as ``set_train_options``."""
        new = None if kind is None else (str(kind), float(decay))
        if new == getattr(self, "_averaging", None):
            return
        self._averaging = new
        for eng in self._engines.values():
            self._apply_averaging(eng)

    def _apply_averaging(self, eng):
        av = getattr(self, "_averaging", None)
        if av is None:
            if getattr(eng, "_averaging", (None, None))[0] is not None:
                eng.set_averaging(None)
        else:
            eng.set_averaging(*self.averaged_arena(), kind=av[0], decay=av[1])

    def average_skip(self):
        """Floats [begin, end) of the arena the accumulator copies instead of averaging: the parameters torch never steps
        (``_dead_params``), when they lie in one run -- what the plans' own averaging launches skip."""
        dead = [(off, shape) for name, shape, off in self._entries if name in self._dead_params]
        if not dead:
            return 0, 0
        end = 0
        for off, shape in dead:
            n = 1
            for d in shape:
                n *= d
            end = max(end, off + n)
        return min(off for off, _ in dead), (end + 3) // 4 * 4

    def average_now(self, kind, decay=0.0):
        """One update of the running average from the weights as they stand (the epoch cadence): two launches on the current
        stream, no host wait."""
        from slnlp import ops
        self._materialize()
        avg, count = self.averaged_arena()
        ops.average_step(avg, self._arena, count, kind=kind, decay=decay, skip=self.average_skip())

    def swap_averaged(self):
        """Exchange the weights with their running average in place (one launch) and tell the plans, so the next forward reads
        planes of the weights it is given.  Twice restores every bit."""
        from slnlp import ops
        self._materialize()
        ops.swap_arenas(self._arena, self.averaged_arena()[0])
        for eng in self._engines.values():
            eng.params_changed()

    def _state_order(self, views):
        raise NotImplementedError

    def _make_engine(self, B, S, old):
        raise NotImplementedError

    def _build(self, arena, values=None):
        for name in list(self._modules):
            del self._modules[name]
        self._arena = arena
        views = {}
        for name, shape, off in self._entries:
            n = 1
            for s in shape:
                n *= s
            views[name] = arena[off:off + n].view(*shape)
            if values is not None:
                with torch.no_grad():
                    views[name].copy_(values[name])
        for name, tensor, is_param in self._state_order(views):
            _register(self, name, tensor, is_param)

    def to(self, device):
        """Reference contract (transformer.py:50-58, bkp.py:383-386): move, remember the device, return self."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device != self._arena.device:
            grads = {n: p.grad for n, p in self.named_parameters() if p.grad is not None}
            self._move_buffers(device)
            if getattr(self, "_pending_recipe", None) is not None:      # nothing drawn yet: allocate there, draw there
                self._build(torch.empty(self._arena.numel(), dtype=torch.float32, device=device))
            else:
                self._build(self._arena.detach().to(device))
            for n, p in self.named_parameters():
                if n in grads:
                    p.grad = grads[n].to(device)
            self._engines = {}
        self.device = device
        self._materialize()
        return self

    def _move_buffers(self, device):
        pass

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    def cpu(self):
        return self.to("cpu")

    def _engine_for(self, B, S):
        """One HIP plan per sequence length, grown when a larger batch arrives; all share the arenas."""
        if not self._arena.is_cuda:
            raise RuntimeError("%s: the module is on %s -- the HIP path is the only compute path "
                               "(no CPU fallback); call .to('cuda') first" % (type(self).__name__, self._arena.device))
        self._materialize()
        eng = self._engines.get(S)
        if eng is None or eng.cfg.B < B:
            old = eng
            eng = self._make_engine(max(B, old.cfg.B if old is not None else 0), S, self._shared_state())
            self._apply_train_options(eng)
            self._apply_averaging(eng)
            self._engines[S] = eng
        return eng

    def engine(self, B, S):
        """Public handle for the fused-step estimator (slnlp.net)."""
        return self._engine_for(B, S)

    def set_train_options(self, criterion=None, update=None, param_groups=None):
        """Criterion and update settings of the fused step, for every plan of the module (now and created later):
        ``criterion`` {weight, label_smoothing, reduction}, ``update`` {kind, dampening, weight_decay, nesterov} -- the
        keywords of the engines' ``set_criterion`` / ``set_update``; ``param_groups`` {seg_begin, seg_group, weight_decay}
        (``slnlp.param_groups.segments``; the engines' ``set_param_groups``) or False: no groups.  None leaves that part as
        it is."""
        opts = dict(getattr(self, "_train_opts", None) or {})
        if param_groups is not None:
            opts["param_groups"] = dict(param_groups) if param_groups else False
            self._group_lr_host = None
        if criterion is not None:
            opts["criterion"] = dict(criterion)
        if update is not None:
            opts["update"] = dict(update)
        self._train_opts = opts
        for eng in self._engines.values():
            self._apply_train_options(eng)

    def _apply_train_options(self, eng):
        opts = getattr(self, "_train_opts", None) or {}
        if "criterion" in opts:
            eng.set_criterion(**opts["criterion"])
        if "update" in opts:
            eng.set_update(**opts["update"])
        if "param_groups" in opts:
            tab = opts["param_groups"]
            eng.set_param_groups(tab or None, self._group_lr(len(tab["weight_decay"])) if tab else None)

    def _group_lr(self, n):
        """The groups' learning rates on the device, [n] float32: ONE tensor per module, read by every plan's update."""
        st = self._shared_state()
        t = st.get("group_lr")
        if t is None or t.numel() != n:
            t = st["group_lr"] = torch.zeros(n, dtype=torch.float32, device=self._arena.device)
            self._group_lr_host = None
        return t

    def set_group_lrs(self, lrs):
        """Write the groups' current rates: a fill launch per rate that moved, queued on the fit's stream like the one-group
        ``lr.fill_`` -- the host never waits for the stream, so a per-batch schedule costs no synchronisation."""
        lrs = [float(v) for v in lrs]
        t = self._group_lr(len(lrs))
        have = getattr(self, "_group_lr_host", None)
        for i, v in enumerate(lrs):
            if have is None or have[i] != v:
                t[i:i + 1].fill_(v)
        self._group_lr_host = lrs

    def forget_group_lrs(self):
        """The device copy of the rates is about to be written from elsewhere (a lockstep group's rate tables): the next
        ``set_group_lrs`` writes every rate."""
        self._group_lr_host = None

    def _run(self, inputs):
        if self.training and torch.is_grad_enabled():
            named = dict(self.named_parameters())
            return _HipFn.apply(self, inputs, *[named[n] for n in self._param_names])
        eng = self._engine_for(inputs[0].shape[0], inputs[0].shape[1])
        return eng.forward(*inputs, train=self.training).clone()

    # engines hold ctypes handles: rebuild lazily after copy / pickle (sklearn.clone, checkpoints).  copy.deepcopy
    # and pickle restore every tensor separately, so the parameters would stop aliasing ``_arena`` (the memory the HIP
    # plans compute from): ``__setstate__`` re-creates them as views of the restored arena.
    def __getstate__(self):
        self._materialize()
        d = self.__dict__.copy()
        d["_engines"] = {}
        d["_opt_state"] = None
        d["_param_grads"] = {n: p.grad for n, p in self.named_parameters() if p.grad is not None}
        return d

    def __setstate__(self, state):
        grads = state.pop("_param_grads", {})
        super().__setstate__(state)
        self._engines, self._opt_state = {}, None
        self._build(self._arena.detach())
        for n, p in self.named_parameters():
            if n in grads:
                p.grad = grads[n]

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__setstate__(copy.deepcopy(self.__getstate__(), memo))
        return new
