"""Adam and SGD over flat parameter buffers (torch.optim semantics, train.py:232-261).

One vae2_adam_step_dev / vae2_sgd_step_dev launch per flat buffer; the math follows
torch.optim.Adam (lerp first moment, L2 weight decay folded into the gradient, bias
corrections in double) and torch.optim.SGD (L2 weight decay, momentum buffer = gradient on
the first step, dampening, Nesterov).  The step counter and learning rate live in device
memory (vae2_adam_coeffs / vae2_sgd_coeffs advance them), so the whole step can be captured
in a HIP graph and replayed (vae2.graph.StepGraph); change the learning rate through
param_groups[0]["lr"] and the next eager step() — or set_lr() between replays.
state_dict() / load_state_dict() use torch.optim's formats (per-parameter exp_avg /
exp_avg_sq / step for Adam, momentum_buffer for SGD) so optimizer checkpoints interchange.

max_grad_norm (both optimizers; None = off, the launches are then exactly the unclipped
ones) clips the global 2-norm of all flat gradients of the optimizer to that threshold, with
the semantics of torch.nn.utils.clip_grad_norm_: one vae2_grad_sumsq per flat buffer (fp64
partial sums, fixed order), one vae2_clip_coeffs, and the *_clip form of the step, which
multiplies each gradient element by the device-resident coefficient while it reads it (no
extra write pass; the gradient buffer is not modified).  Norm and coefficient are recomputed
on the device by every step, so a captured step replays them; grad_norm() returns the
device value of the last step without synchronising.  In the distributed loop
allreduce_grads runs before step(), so the norm is that of the reduced gradient and is
identical on every rank.  clip_grad_norm_ below is the stand-alone, torch-shaped form.

ema_decay (both optimizers; None = off: no buffers, and the launches are exactly those
without it) keeps an exponential moving average of the weights in `ema`, one buffer per flat
parameter buffer, with the semantics of torch.optim.swa_utils.AveragedModel +
get_ema_multi_avg_fn(decay): the first update copies the weights, later ones do
ema += (1 - decay) * (p - ema).  step() launches one vae2_ema_coeffs and one
vae2_ema_update_dev per flat buffer after the parameter update; the update count lives on
the device (ema_updates), so "first update" is decided there and a captured step replays it.
swap_ema() exchanges the contents of the weights and their average (and re-packs the conv
weights) for evaluation.  BatchNorm running statistics are buffers, not parameters: they are
not averaged, and under swap_ema() the model runs with the live ones.  ema_decay is
configuration, not optimizer state: param_groups and state_dict() do not carry it.
"""
import contextlib
import math

import torch

from . import ops, streams
from ._lib import call, load
from .params import flatten


def _clip_threshold(max_norm, what="max_grad_norm"):
    """None (off) or a float > 0 (inf allowed), else ValueError."""
    if max_norm is None:
        return None
    v = float(max_norm)
    if math.isnan(v) or v <= 0.0:
        raise ValueError(f"Invalid {what}: {max_norm} (None, or a float > 0)")
    return v


def _ema_decay(decay):
    """None (off) or a float in [0, 1), else ValueError."""
    if decay is None:
        return None
    v = float(decay)
    if not 0.0 <= v < 1.0:  # NaN fails both comparisons
        raise ValueError(f"Invalid ema_decay: {decay} (None, or a float in [0, 1))")
    return v


class _GradNorm:
    """The device side of global-norm clipping over a list of FlatParams: the fp64 partials
    of all buffers laid end to end in one workspace, and clip = {norm, coefficient, -, -}.
    Everything is allocated here, so launch() may run inside a graph capture."""

    def __init__(self, flats):
        self.flats = flats
        sizes = [int(load().vae2_grad_norm_ws_size(f.numel)) for f in flats]
        self.offsets = [sum(sizes[:k]) for k in range(len(sizes))]
        self.count = sum(sizes)
        dev = flats[0].data.device
        self.ws = torch.empty(self.count, dtype=torch.float64, device=dev)
        self.clip = torch.zeros(4, dtype=torch.float32, device=dev)

    def launch(self, max_norm, s):
        for f, off in zip(self.flats, self.offsets):
            call("vae2_grad_sumsq", ops.ptr(f.grad), f.numel, ops.ptr(self.ws[off:]), s)
        call("vae2_clip_coeffs", ops.ptr(self.ws), self.count, max_norm, ops.ptr(self.clip), s)


class _FusedFlat:
    """What the fused optimizers share: the flat buffers and weight packs of their modules,
    the device-resident {step, lr} state, learning-rate sync and zero_grad."""

    def _init_flat(self, modules, lr, n_coeffs, max_grad_norm=None, ema_decay=None):
        self.max_grad_norm = _clip_threshold(max_grad_norm)
        self.ema_decay = _ema_decay(ema_decay)
        if not isinstance(modules, (list, tuple)):
            modules = [modules]
        self.flats = [flatten(m) for m in modules]
        # packed conv weights, refreshed in one launch per model after every update
        self.packs = [ops.PackPlan(m) for m in modules]
        self.lr = float(lr)
        dev = self.flats[0].data.device
        self._state = torch.zeros(2, dtype=torch.float64, device=dev)  # {step, lr}
        self._coeffs = torch.zeros(n_coeffs, dtype=torch.float32, device=dev)
        self._dev_lr = None
        # allocated here, never in step(): the step may be the one a graph captures
        self._norm = _GradNorm(self.flats) if self.max_grad_norm is not None else None
        self.ema = None
        if self.ema_decay is not None:
            # not read before the first update (the kernel copies then), so left uninitialised
            self.ema = [torch.empty_like(f.data) for f in self.flats]
            self._ema_state = torch.zeros(2, dtype=torch.float64, device=dev)  # {updates, -}
            self._ema_coeffs = torch.zeros(4, dtype=torch.float32, device=dev)

    def _finish_step(self, s):
        """After the parameter update of all flats: the EMA update, then the re-pack."""
        if self.ema is not None:
            call("vae2_ema_coeffs", ops.ptr(self._ema_state), self.ema_decay,
                 ops.ptr(self._ema_coeffs), s)
            for f, e in zip(self.flats, self.ema):
                call("vae2_ema_update_dev", ops.ptr(e), ops.ptr(f.data), f.numel,
                     ops.ptr(self._ema_coeffs), s)
        for plan in self.packs:
            plan.bump_versions()

    @property
    def ema_updates(self):
        """The number of EMA updates so far (the device counter: one synchronising read)."""
        if self.ema is None:
            return 0
        return int(self._ema_state[0].item())

    @ema_updates.setter
    def ema_updates(self, n):
        if self.ema is None:
            raise RuntimeError("ema_updates: the optimizer was built with ema_decay=None")
        self._ema_state[0].fill_(float(n))

    def _exchange_ema(self):
        for f, e in zip(self.flats, self.ema):
            tmp = f.data.clone()
            f.data.copy_(e)
            e.copy_(tmp)
        for plan in self.packs:
            plan.bump_versions()

    @contextlib.contextmanager
    def swap_ema(self):
        """Run the model with the averaged weights: the contents of each flat parameter buffer
        and its `ema` buffer are exchanged (parameter views and pointers keep their identity)
        and the conv weights re-packed; on exit, also on an exception, they are exchanged
        back.  BatchNorm running statistics stay the live ones.  An epoch-boundary operation
        (plain copies, one synchronising read), not for use inside a captured step."""
        if self.ema is None:
            raise RuntimeError("swap_ema(): the optimizer was built with ema_decay=None")
        if self.flats[0].data.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("swap_ema(): not inside a graph capture")
        streams.join_all()
        if self.ema_updates == 0:
            raise RuntimeError("swap_ema(): no EMA update has happened yet (ema_updates == 0: "
                               "the ema buffers are uninitialised)")
        with torch.no_grad():
            self._exchange_ema()
        try:
            yield self
        finally:
            streams.join_all()
            with torch.no_grad():
                self._exchange_ema()

    def grad_norm(self):
        """The total gradient 2-norm of the last step(): a 0-dim device tensor (a view of
        the device-resident value, no synchronisation).  Needs max_grad_norm."""
        if self._norm is None:
            raise RuntimeError("grad_norm(): the optimizer was built with max_grad_norm=None "
                               "(pass float('inf') to measure without clipping)")
        return self._norm.clip[0]

    def _params(self):
        return [p for f in self.flats for p in f.params]

    def zero_grad(self, set_to_none=False):
        streams.join_all()
        for f in self.flats:
            f.zero_grad()

    @property
    def step_count(self):
        return int(self._state[0].item())

    @step_count.setter
    def step_count(self, n):
        self._state[0].fill_(float(n))

    def set_lr(self, lr):
        self.param_groups[0]["lr"] = float(lr)
        self._sync_lr()

    def _sync_lr(self):
        lr = float(self.param_groups[0]["lr"])
        self.lr = lr
        if lr != self._dev_lr:  # eager: graphs read the device copy on replay
            self._state[1].fill_(lr)
            self._dev_lr = lr

    def _slices(self, *bufs):
        """(index, parameter, its slice of each flat-shaped buffer list) in state_dict order."""
        idx = 0
        for k, f in enumerate(self.flats):
            for p, off in zip(f.params, f.offsets):
                yield idx, p, [b[k][off:off + p.numel()] for b in bufs]
                idx += 1

    def _group_dict(self):
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(sum(len(f.params) for f in self.flats)))
        return group


def _check_kind(st, want, other, name):
    """A clear error for a checkpoint of the other optimizer (torch would fail on a key)."""
    for s in st.values():
        if other in s and want not in s:
            raise ValueError(f"{name}.load_state_dict: the state holds '{other}' entries and no "
                             f"'{want}' (a checkpoint of another optimizer); set "
                             "TRAIN.OPTIMIZER to the one that wrote it")


class FusedAdam(_FusedFlat):
    def __init__(self, modules, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm=None, ema_decay=None):
        self._init_flat(modules, lr, 2, max_grad_norm, ema_decay)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.weight_decay = float(weight_decay)
        self.exp_avg = [torch.zeros_like(f.data) for f in self.flats]
        self.exp_avg_sq = [torch.zeros_like(f.data) for f in self.flats]
        self.param_groups = [{"params": self._params(), "lr": self.lr,
                              "betas": self.betas, "eps": self.eps,
                              "weight_decay": self.weight_decay, "amsgrad": False,
                              "maximize": False, "foreach": None, "capturable": False,
                              "differentiable": False, "fused": None}]

    @torch.no_grad()
    def step(self):
        self._sync_lr()
        streams.join_all()
        s = ops.stream_ptr()
        if self._norm is not None:
            self._norm.launch(self.max_grad_norm, s)
        call("vae2_adam_coeffs", ops.ptr(self._state), self.betas[0], self.betas[1],
             ops.ptr(self._coeffs), s)
        for f, m, v in zip(self.flats, self.exp_avg, self.exp_avg_sq):
            if self._norm is not None:
                call("vae2_adam_step_dev_clip", ops.ptr(f.data), ops.ptr(f.grad), ops.ptr(m),
                     ops.ptr(v), f.numel, ops.ptr(self._coeffs), ops.ptr(self._norm.clip),
                     self.betas[0], self.betas[1], self.eps, self.weight_decay, s)
            else:
                call("vae2_adam_step_dev", ops.ptr(f.data), ops.ptr(f.grad), ops.ptr(m),
                     ops.ptr(v), f.numel, ops.ptr(self._coeffs), self.betas[0], self.betas[1],
                     self.eps, self.weight_decay, s)
        self._finish_step(s)

    # ---- torch.optim.Adam-compatible checkpoint format ----
    def state_dict(self):
        state = {}
        step = float(self.step_count)
        for idx, p, (m, v) in self._slices(self.exp_avg, self.exp_avg_sq):
            state[idx] = {"step": torch.tensor(step),
                          "exp_avg": m.view_as(p).clone(),
                          "exp_avg_sq": v.view_as(p).clone()}
        return {"state": state, "param_groups": [self._group_dict()]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        st = sd["state"]
        _check_kind(st, "exp_avg", "momentum_buffer", "FusedAdam")
        steps = []
        for idx, p, (m, v) in self._slices(self.exp_avg, self.exp_avg_sq):
            if idx in st:
                m.copy_(st[idx]["exp_avg"].reshape(-1))
                v.copy_(st[idx]["exp_avg_sq"].reshape(-1))
                steps.append(int(float(st[idx]["step"])))
        if steps:
            self.step_count = max(steps)
        g = sd["param_groups"][0]
        self.param_groups[0]["lr"] = g.get("lr", self.lr)
        self._sync_lr()
        self.betas = tuple(g.get("betas", self.betas))
        self.eps = g.get("eps", self.eps)
        self.weight_decay = g.get("weight_decay", self.weight_decay)


class FusedSGD(_FusedFlat):
    """torch.optim.SGD (reference train.py:232-250: lr, momentum, weight_decay, nesterov).

    param_groups[0] carries torch's SGD keys for checkpoints and schedulers, but only "lr"
    is live (re-read at every eager step(), as in FusedAdam): momentum, dampening,
    weight_decay and nesterov are fixed at construction or by load_state_dict(), and a later
    edit of those keys is ignored.  load_state_dict() takes momentum buffers for all
    parameters or for none: one device step counter decides "first step" for every parameter,
    so a torch state that lacks the buffer of some parameters (ones that never received a
    gradient) is refused with a ValueError."""

    def __init__(self, modules, lr, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False, max_grad_norm=None, ema_decay=None):
        # torch.optim.SGD's own checks and messages, before any buffer is built
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._init_flat(modules, lr, 4, max_grad_norm, ema_decay)
        self.momentum = float(momentum)
        self.dampening = float(dampening)
        self.weight_decay = float(weight_decay)
        self.nesterov = bool(nesterov)
        # allocated here, not at the first step: that step may be the one a graph captures, and
        # an allocation inside a capture would be zero-filled again by every replay.  The
        # kernel does not read it on the first step, and state_dict() shows it only after one
        # (torch's momentum_buffer appears then)
        self.momentum_buffer = None
        if self.momentum != 0:
            self._buffers()
        self.param_groups = [{"params": self._params(), "lr": self.lr,
                              "momentum": self.momentum, "dampening": self.dampening,
                              "weight_decay": self.weight_decay, "nesterov": self.nesterov,
                              "maximize": False, "foreach": None, "differentiable": False,
                              "fused": None}]
        self._sync_lr()  # the device lr is set before a capture of the very first step

    def _buffers(self):
        if self.momentum_buffer is None:
            self.momentum_buffer = [torch.zeros_like(f.data) for f in self.flats]
        return self.momentum_buffer

    @torch.no_grad()
    def step(self):
        self._sync_lr()
        streams.join_all()
        s = ops.stream_ptr()
        bufs = self._buffers() if self.momentum != 0 else [None] * len(self.flats)
        if self._norm is not None:
            self._norm.launch(self.max_grad_norm, s)
        call("vae2_sgd_coeffs", ops.ptr(self._state), self.momentum, self.dampening,
             int(self.nesterov), ops.ptr(self._coeffs), s)
        for f, b in zip(self.flats, bufs):
            if self._norm is not None:
                call("vae2_sgd_step_dev_clip", ops.ptr(f.data), ops.ptr(f.grad),
                     ops.ptr(b) if b is not None else None, f.numel, ops.ptr(self._coeffs),
                     ops.ptr(self._norm.clip), self.momentum, self.weight_decay,
                     int(self.nesterov), s)
            else:
                call("vae2_sgd_step_dev", ops.ptr(f.data), ops.ptr(f.grad),
                     ops.ptr(b) if b is not None else None, f.numel, ops.ptr(self._coeffs),
                     self.momentum, self.weight_decay, int(self.nesterov), s)
        self._finish_step(s)

    # ---- torch.optim.SGD-compatible checkpoint format ----
    def state_dict(self):
        state = {}
        if self.momentum_buffer is not None and self.step_count > 0:
            for idx, p, (b,) in self._slices(self.momentum_buffer):
                state[idx] = {"momentum_buffer": b.view_as(p).clone()}
        return {"state": state, "param_groups": [self._group_dict()]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        st = sd["state"]
        _check_kind(st, "momentum_buffer", "exp_avg", "FusedSGD")
        loaded = [i for i, s in st.items() if s.get("momentum_buffer") is not None]
        n_params = sum(len(f.params) for f in self.flats)
        if loaded and len(loaded) != n_params:
            # one device step counter decides "first step" for every parameter
            raise ValueError(f"FusedSGD.load_state_dict: momentum buffers for {len(loaded)} of "
                             f"{n_params} parameters (all or none are supported)")
        if loaded:
            for idx, p, (b,) in self._slices(self._buffers()):
                b.copy_(st[idx]["momentum_buffer"].reshape(-1))
            self.step_count = max(self.step_count, 1)  # the next step is not the first
        else:
            self.step_count = 0
        g = sd["param_groups"][0]
        grp = self.param_groups[0]
        for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"):
            grp[k] = g.get(k, grp[k])
        self._sync_lr()
        self.momentum = float(grp["momentum"])
        self.dampening = float(grp["dampening"])
        self.weight_decay = float(grp["weight_decay"])
        self.nesterov = bool(grp["nesterov"])
        if self.momentum != 0:
            self._buffers()


@torch.no_grad()
def clip_grad_norm_(target, max_norm):
    """torch.nn.utils.clip_grad_norm_ (2-norm) over flat gradients, for callers with their own
    loop (for instance expose_grads() + a torch.optim optimizer): `target` is a fused
    optimizer or a list of FlatParams.  The gradients are scaled in place by
    min(1, max_norm / (norm + 1e-6)) (vae2_scale_dev); returns the total norm before
    clipping as a 0-dim device tensor, without synchronising.  Allocates its small workspace
    per call: inside a captured step use the optimizers' max_grad_norm instead."""
    max_norm = _clip_threshold(max_norm, "max_norm")
    if max_norm is None:
        raise ValueError("Invalid max_norm: None")
    flats = list(target.flats) if hasattr(target, "flats") else list(target)
    if not flats:
        raise ValueError("clip_grad_norm_: no flat gradients")
    streams.join_all()
    s = ops.stream_ptr()
    norm = _GradNorm(flats)
    norm.launch(max_norm, s)
    for f in flats:
        call("vae2_scale_dev", ops.ptr(f.grad), f.numel, ops.ptr(norm.clip), s)
    return norm.clip[0]
