"""Optimizers for the G+D step, each executed as ONE fused HIP launch over a flat fp32 parameter arena, with the reference's
`add_weight_decay` filter (no decay on 1-D tensors and *.bias -- optim/optim_factory.py:25-37; D: model/model_handler.py:107).

Parameters, gradients and both state tensors live in four contiguous buffers; every nn.Parameter is a
view into the arena, every .grad a view into the gradient arena (so a bag-parallel step all-reduces one
tensor per network). The L1 regulariser of loss/utils.py:6-14 is applied inside the same kernel as
coef*sign(w).

  FlatAdam    torch.optim.Adam (L2-in-grad weight decay); state_dict() has torch.optim.Adam's layout, so reference checkpoints resume
  FlatOptim   the other elementwise names create_optimizer can be given from a handler's config: adamw, nadam, radam, adadelta, and
              any of them (or adam) behind the `lookahead_` prefix -- csrc/optim.hip::optim_kernel; state_dict() has the layout of the
              class the reference would have built."""
import torch

from . import ops

# names of optim/optim_factory.py:70-118 without a path here, and why
_NO_PATH = {
    "adamp": "needs a per-tensor projection", "sgdp": "needs a per-tensor projection",
    "novograd": "needs per-tensor gradient norms", "nvnovograd": "needs per-tensor gradient norms",
    "adafactor": "keeps factored second moments", "adahessian": "is second order (Hessian-vector products)",
    **{n: "is unreachable from a handler (the handlers pass momentum=None, a TypeError in the reference)"
       for n in ("sgd", "nesterov", "momentum", "rmsprop", "rmsproptf")},
    **{n: "needs apex in the reference" for n in ("fusedsgd", "fusedmomentum", "fusedadam", "fusedadamw", "fusedlamb", "fusednovograd")},
}
_KINDS = ("adam", "adamw", "nadam", "radam", "adadelta")


def parse_opt_name(opt):
    """The reference's reading of `opt` (optim_factory.py:46,68-69,123-125): lower-case, split on '_', the last token names the
    optimizer, a first token `lookahead` (of more than one) wraps it. -> (name, lookahead)"""
    parts = str(opt).lower().split("_")
    return parts[-1], len(parts) > 1 and parts[0] == "lookahead"


def create_optimizer(args, model, filter_bias_and_bn=True):
    """Reference signature (optim/optim_factory.py:40)."""
    name, lookahead = parse_opt_name(args.opt)
    if name in _NO_PATH:
        raise NotImplementedError(f"opt={args.opt}: `{name}` {_NO_PATH[name]}; the fused arena step covers "
                                  f"{', '.join(_KINDS)} and their lookahead_ forms")
    if name not in _KINDS:
        raise ValueError(f"opt={args.opt}: invalid optimizer `{name}`")
    wd = args.weight_decay or 0.0
    kw = {}
    if getattr(args, "opt_eps", None) is not None:
        kw["eps"] = args.opt_eps
    if getattr(args, "opt_betas", None) is not None:
        if name == "adadelta":
            raise TypeError("opt=adadelta takes no betas (opt_betas must be None)")
        kw["betas"] = tuple(args.opt_betas)
    filt = bool(wd and filter_bias_and_bn)
    if name == "adam" and not lookahead:
        return FlatAdam(model, lr=args.lr, weight_decay=wd, filter_bias_and_bn=filt, **kw)
    return FlatOptim(model, name, lr=args.lr, weight_decay=wd, filter_bias_and_bn=filt, lookahead=lookahead, **kw)


class FlatArenaOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: the arenas (parameters, gradients, two state tensors, per-element weight decay), the views the
    parameters become, the bf16x3 weight planes, the clean-gradient protocol, and state_dict()/load_state_dict() through the arenas.
    A subclass names its two state tensors (STATE_NAMES) and implements step()."""
    STATE_NAMES = ("exp_avg", "exp_avg_sq")
    KERNEL_NAME = "optimizer"
    INT_STEP = False              # state["step"]: a float tensor (torch.optim classes) or a Python int (the vendored ones)

    def __init__(self, model, defaults, weight_decay=0.0, filter_bias_and_bn=False, l1_coef=0.0):
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if not named:
            raise ValueError("no parameters")
        dev = named[0][1].device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs the fused HIP {self.KERNEL_NAME} kernel: move the model to the GPU first")
        if filter_bias_and_bn:
            no_decay = [(n, p) for n, p in named if p.dim() == 1 or n.endswith(".bias")]
            decay = [(n, p) for n, p in named if not (p.dim() == 1 or n.endswith(".bias"))]
            groups = [{"params": [p for _, p in no_decay], "weight_decay": 0.0},
                      {"params": [p for _, p in decay], "weight_decay": weight_decay}]
        else:
            groups = [{"params": [p for _, p in named], "weight_decay": weight_decay}]
        # Arena layout (independent of the param_groups / state_dict order above): vectors first, then matrices, each in named
        # order. That puts the two branch weights (and the two branch biases) of every gated-attention scorer side by side, which
        # is what lets the pooling kernels read them as one stacked [2D, D] view and accumulate their gradients in one launch.
        ordered = ([(n, p) for n, p in named if p.dim() == 1 or n.endswith(".bias")]
                   + [(n, p) for n, p in named if not (p.dim() == 1 or n.endswith(".bias"))])
        super().__init__(groups, dict(defaults, weight_decay=weight_decay))
        self.l1_coef = float(l1_coef)
        self.names = [n for n, _ in ordered]
        # ---- arenas (each tensor 8-element aligned: fp32 views are 32 B aligned, the bf16 operand planes' views 16 B aligned)
        offs, total = [], 0
        for _, p in ordered:
            offs.append(total)
            total += (p.numel() + 7) // 8 * 8
        self.flat_param = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        ops.ARENA_STORAGES.add(self.flat_grad.untyped_storage().data_ptr())     # (a deferred split-K fold may only land here: ops.gemm)
        self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)       # state tensor STATE_NAMES[0]
        self.flat_v = torch.zeros(total, dtype=torch.float32, device=dev)       # state tensor STATE_NAMES[1]
        self.flat_wd = torch.zeros(total, dtype=torch.float32, device=dev)
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)

        # bf16x3 operand planes of the weights (hi = bf16(w), lo = bf16(w - hi)), same layout as the arena: written by the optimizer
        # kernel with every update, so no contraction ever re-splits a weight (ops.weight_planes)
        # (both planes in ONE allocation, lo behind hi: a weight's two planes are then one strided view -- ops.gemm_two_layers stacks the
        # planes of two layers with one launch)
        self.planes = ops.Planes.alloc((total,), dev)
        self.planes.hi.zero_(); self.planes.lo.zero_()
        self._views = []
        s1, s2 = self.STATE_NAMES
        with torch.no_grad():
            for (n, p), o in zip(ordered, offs):
                k = p.numel()
                self.flat_param[o:o + k].copy_(p.reshape(-1))
                p.data = self.flat_param[o:o + k].view(p.shape)
                p.grad = self.flat_grad[o:o + k].view(p.shape)
                p._arena_grad = p.grad                     # backward kernels accumulate here directly (ops._arena_grad)
                p._arena_owner = self                      # ... and tell this optimizer that its arena is being written (grad_is_clean)
                self._views.append((p, o, k))
            for g in self.param_groups:
                for p in g["params"]:
                    o, k = next((o, k) for q, o, k in self._views if q is p)
                    self.flat_wd[o:o + k] = g["weight_decay"]
                    self.state[p] = {"step": self._step_value(0), s1: self.flat_m[o:o + k].view(p.shape),
                                     s2: self.flat_v[o:o + k].view(p.shape)}
        self._has_wd = bool(self.flat_wd.abs().max().item() > 0)
        self.refresh_planes()

    def _step_value(self, n):
        return int(n) if self.INT_STEP else torch.tensor(float(n))

    def refresh_planes(self):
        """Re-derive the weight planes from the arena (construction, load_state_dict, any torch-side write to a parameter) and
        stamp every parameter with its current version counter."""
        ops.split_planes(self.flat_param, out=self.planes)
        for p, o, k in self._views:
            p._advmil_planes = (self, p._version, ops.Planes(self.planes.hi[o:o + k].view(p.shape), self.planes.lo[o:o + k].view(p.shape)))

    # ---- "is the gradient arena known to be all zero?" A step(clear_grad=True) zeroes the arena behind its read, so the zero_grad()
    # that follows has nothing to fill. The knowledge is HOST state about DEVICE memory, so every writer must be seen:
    #   * kernels that accumulate into arena slots get them from ops._arena_grad, which calls mark_grad_dirty();
    #   * torch-side writes (autograd's AccumulateGrad, p.grad.add_(), ...) move flat_grad's version counter (views share it);
    #   * nothing is recorded while a stream is being CAPTURED (no kernel runs then): a captured step's zero_grad() launches no fill
    #     when the capturer said the graph starts from a clean arena (`capture_assumes_clean`, set by graphed.GraphedStep, whose
    #     replay() makes that true), and the flag is set again by replay() -- never by the captured calls themselves.
    _grad_clean = False
    _clean_version = -1
    capture_assumes_clean = False

    def mark_grad_dirty(self):
        self._grad_clean = False

    def mark_grad_clean(self):
        self._grad_clean, self._clean_version = True, self.flat_grad._version

    def grad_is_clean(self):
        return bool(self._grad_clean and self.flat_grad._version == self._clean_version)

    def zero_grad(self, set_to_none: bool = False):
        if torch.cuda.is_current_stream_capturing():
            if not self.capture_assumes_clean:
                self.flat_grad.zero_()
        elif self.grad_is_clean():
            self._grad_clean = False         # the last step cleared the arena behind its read (step(clear_grad=True)): nothing to fill
        else:
            self.flat_grad.zero_()
            self._grad_clean = False
        for p, o, k in self._views:          # re-attach if someone replaced .grad
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * o:
                p.grad = self.flat_grad[o:o + k].view(p.shape)
                p._arena_grad = p.grad

    def _stepped(self, clear_grad):
        """Host bookkeeping behind a step launch."""
        if not torch.cuda.is_current_stream_capturing():
            if clear_grad:
                self.mark_grad_clean()
            else:
                self._grad_clean = False

    def state_dict(self):
        n = int(self.step_t.item())
        for st in self.state.values():
            st["step"] = self._step_value(n)
        return super().state_dict()

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        s1, s2 = self.STATE_NAMES
        step = 0
        with torch.no_grad():
            for p, o, k in self._views:       # pull the loaded state tensors back into the arenas
                st = self.state[p]
                self.flat_m[o:o + k].copy_(st[s1].reshape(-1))
                self.flat_v[o:o + k].copy_(st[s2].reshape(-1))
                st[s1] = self.flat_m[o:o + k].view(p.shape)
                st[s2] = self.flat_v[o:o + k].view(p.shape)
                step = int(st["step"])
            self.step_t.fill_(step)
            for g in self.param_groups:
                for p in g["params"]:
                    o, k = next((o, k) for q, o, k in self._views if q is p)
                    self.flat_wd[o:o + k] = g["weight_decay"]
        self._has_wd = bool(self.flat_wd.abs().max().item() > 0)
        self.refresh_planes()


class FlatAdam(FlatArenaOptimizer):
    KERNEL_NAME = "Adam"

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, filter_bias_and_bn=False, l1_coef=0.0):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps), weight_decay=weight_decay, filter_bias_and_bn=filter_bias_and_bn,
                         l1_coef=l1_coef)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, tick=True, abs_partial=None, clear_grad=False):
        """tick = False: the device step counter is left to the caller (ops.step_seed_tick(self.step_t, seed): the captured step folds it
        into the RNG seed's advance). abs_partial: receives the per-workgroup shares of sum |p| BEFORE the update (the logged L1 term).
        clear_grad: the kernel zeroes the gradient arena behind its read and the next zero_grad() launches nothing -- p.grad then reads
        zero after step(), so only the captured step (nobody looks at gradients between replays) asks for it."""
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        self.n_updates = getattr(self, "n_updates", 0) + 1      # host-side version of the parameters (forward memo key)
        ops.adam_step(self.flat_param, self.flat_grad, self.flat_m, self.flat_v, self.flat_wd if self._has_wd else None,
                      self.step_t, g0["lr"], b1, b2, g0["eps"], grad_scale, self.l1_coef, planes=self.planes, tick=tick,
                      abs_partial=abs_partial, clear_grad=clear_grad)
        self._stepped(clear_grad)


class FlatOptim(FlatArenaOptimizer):
    """adamw | nadam | radam | adadelta (and adam, as a lookahead base) with FlatAdam's interface; lookahead=True adds the slow arena
    of optim/lookahead.py (alpha 0.5, k 6), synced inside the same launch on every k-th step as counted by the DEVICE step counter, so
    a replayed graph syncs where the eager loop would.

    state_dict(): torch.optim.AdamW / Adadelta / Adam keys, or `step, m_schedule, exp_avg, exp_avg_sq` (optim/nadam.py) and
    `step, exp_avg, exp_avg_sq` (optim/radam.py::RAdam) with their Python-number steps. Behind lookahead the dict is
    `state / slow_state / param_groups` with lookahead_alpha / lookahead_k / lookahead_step in every group; slow_state is keyed by the
    parameter's INDEX in the packed state (the reference keys it by id(), which no other process can resolve). A dict without such a
    slow_state resumes with no slow buffer: the next sync creates it as a copy of the fast weights, which is where the reference's own
    load ends up."""

    def __init__(self, model, kind, lr=1e-3, betas=(0.9, 0.999), eps=None, weight_decay=0.0, filter_bias_and_bn=False, l1_coef=0.0,
                 lookahead=False, lookahead_alpha=0.5, lookahead_k=6, rho=0.9, schedule_decay=4e-3):
        if kind not in _KINDS:
            raise ValueError(f"FlatOptim: kind `{kind}` is none of {_KINDS}")
        if not 0.0 <= lookahead_alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {lookahead_alpha}")
        if not 1 <= lookahead_k:
            raise ValueError(f"Invalid lookahead steps: {lookahead_k}")
        self.kind, self.lookahead = kind, bool(lookahead)
        self.INT_STEP = kind in ("nadam", "radam")
        if kind == "adadelta":
            self.STATE_NAMES = ("square_avg", "acc_delta")
            defaults = dict(lr=lr, rho=rho, eps=1e-6 if eps is None else eps)
        else:
            defaults = dict(lr=lr, betas=tuple(betas), eps=1e-8 if eps is None else eps)
            if kind == "nadam":
                defaults["schedule_decay"] = schedule_decay
            if kind == "adamw":
                defaults["amsgrad"] = False
        if self.lookahead:
            defaults.update(lookahead_alpha=lookahead_alpha, lookahead_k=int(lookahead_k), lookahead_step=0)
        super().__init__(model, defaults, weight_decay=weight_decay, filter_bias_and_bn=filter_bias_and_bn, l1_coef=l1_coef)
        dev = self.flat_param.device
        # NAdam's running product of the momentum schedule: two device doubles, the step-t launch reads slot (t-1)&1 and writes slot t&1
        self.m_sched = torch.ones(2, dtype=torch.float64, device=dev) if kind == "nadam" else None
        if kind == "nadam":
            for st in self.state.values():
                st["m_schedule"] = 1.0
        self.flat_slow = self.la_state = None
        if self.lookahead:
            self.flat_slow = torch.zeros_like(self.flat_param)
            self.la_state = torch.zeros(2, dtype=torch.int32, device=dev)
            self._set_lookahead(first=int(lookahead_k), offset=0)
        # the arenas never move (load_state_dict copies into them): checked and bound once, a step only rewrites the scalars
        self._call = ops.OptimCall(kind, self.flat_param, self.flat_grad, self.flat_m, self.flat_v, self.flat_wd, self.step_t,
                                   planes=self.planes, m_sched=self.m_sched, slow=self.flat_slow, la_state=self.la_state)

    def _set_lookahead(self, first, offset):
        """first: the lookahead step whose sync creates the slow buffer (0: it exists); offset: base step - lookahead step."""
        self._la_first, self._la_off = int(first), int(offset)
        self.la_state.copy_(torch.tensor([self._la_first, self._la_off], dtype=torch.int32))

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, tick=True, abs_partial=None, clear_grad=False):
        """Same contract as FlatAdam.step."""
        g0 = self.param_groups[0]
        b1, b2 = (g0["rho"], 0.0) if self.kind == "adadelta" else g0["betas"]
        self.n_updates = getattr(self, "n_updates", 0) + 1      # host-side version of the parameters (forward memo key)
        self._call(g0["lr"], b1, b2, g0["eps"], grad_scale, self.l1_coef, tick=tick, abs_partial=abs_partial, clear_grad=clear_grad,
                   schedule_decay=g0.get("schedule_decay", 0.0), la_alpha=g0.get("lookahead_alpha", 0.5), la_k=g0.get("lookahead_k", 6),
                   use_wd=self._has_wd)
        self._stepped(clear_grad)

    def _param_index(self):
        """parameter -> its index in the packed state_dict (torch.optim.Optimizer.state_dict numbers them across the groups)."""
        return {id(p): i for i, p in enumerate(q for g in self.param_groups for q in g["params"])}

    def state_dict(self):
        n = int(self.step_t.item())
        if self.kind == "nadam":
            ms = float(self.m_sched[n & 1].item())
            for st in self.state.values():
                st["m_schedule"] = ms
        if not self.lookahead:
            return super().state_dict()
        lt = n - self._la_off
        for g in self.param_groups:
            g["lookahead_step"] = lt
        sd = super().state_dict()
        slow_state = {}
        if self._la_first == 0 or lt >= self._la_first:          # the slow buffer exists
            idx = self._param_index()
            slow_state = {idx[id(p)]: {"slow_buffer": self.flat_slow[o:o + k].view(p.shape)} for p, o, k in self._views}
        return {"state": sd["state"], "slow_state": slow_state, "param_groups": sd["param_groups"]}

    def load_state_dict(self, sd):
        super().load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})
        n = int(self.step_t.item())
        if self.kind == "nadam":
            self.m_sched.fill_(float(next(iter(self.state.values()))["m_schedule"]))
        if not self.lookahead:
            return
        g0 = self.param_groups[0]
        for g in self.param_groups:              # a checkpoint of the bare base optimizer: the wrapper starts counting here
            g.setdefault("lookahead_alpha", self.defaults["lookahead_alpha"])
            g.setdefault("lookahead_k", self.defaults["lookahead_k"])
            g.setdefault("lookahead_step", 0)
        lt, k = int(g0["lookahead_step"]), int(g0["lookahead_k"])
        idx = self._param_index()
        slow = sd.get("slow_state") or {}
        usable = all(isinstance(slow.get(idx[id(p)]), dict) and torch.is_tensor(slow[idx[id(p)]].get("slow_buffer"))
                     and slow[idx[id(p)]]["slow_buffer"].numel() == kk for p, _, kk in self._views)
        with torch.no_grad():
            if usable:
                for p, o, kk in self._views:
                    self.flat_slow[o:o + kk].copy_(slow[idx[id(p)]]["slow_buffer"].reshape(-1))
            else:
                self.flat_slow.zero_()
        self._set_lookahead(first=0 if usable else (lt // k + 1) * k, offset=n - lt)
