"""Optimizers of the reference's training scripts on the multi-tensor HIP kernel (csrc/optim.hip).

``FusedAdam`` == torch.optim.Adam(params, lr, betas, eps, weight_decay) as used by seg18/train_swin.py:122;
``FusedSGD``  == torch.optim.SGD(params, lr, momentum, weight_decay) with per-group lr / weight_decay
                 (train_CL_ft_mswin_sgd_minput.py:147-162); the LARS wrapper of the contrastive stage is
                 stswincl_amd/contrast/lars.py (``make_contrast_optimizer`` builds main_pretrain_swinv5.py:37-47's stack);
``ema_update``== PixPro._momentum_update_key_encoder (PixPro_swin_v5.py:258-289) in ~8 launches instead of ~370x2.
"""
from __future__ import annotations

import math
import weakref
from typing import Iterable, Sequence

import torch

import os

from . import hip

_EAGER_REPACK = os.environ.get("STSWIN_LAZY_REPACK") != "1"       # (A/B switch: per-weight re-packing at the next use)


def _mark_updated(params: Sequence[torch.Tensor]) -> None:
    """The multi-tensor kernel writes through raw pointers, which autograd's version counters do not see - and the bf16
    weight cache of the GEMM path (ops.wcast) is keyed on `_version`, exactly like anything else that memoises on a
    parameter.  Bump the counters of the tensors just written (no kernel launch)."""
    if not params:
        return
    setter = getattr(torch._C._autograd, "_unsafe_set_version_counter", None)
    if setter is not None:
        setter(list(params), [int(p._version) + 1 for p in params])
    else:                                  # older torch: an in-place no-op through the dispatcher
        torch._foreach_add_(list(params), 0)
    if _EAGER_REPACK:                      # ... and re-make their cached GEMM operands now, batched (two launches instead of ~90)
        from . import ops
        ops.repack(params)


_generation = 0            # replay generation: moves when device counters advanced without the host side of the step (graph.GraphedStep)
_CAPTURED = weakref.WeakSet()     # optimizers a GraphedStep captured: their state tensors and clocks are operands of a live graph


def bump_generation() -> None:
    """A captured step ran on the device, or a capture ran its host side without executing it: every host mirror of a device
    counter (_Clock.step, hence EmaSchedule.k / PixPro.k and FusedAdam's per-parameter `step`) is re-read at its next read."""
    global _generation
    _generation += 1


def note_captured(optimizers) -> None:
    """(graph.GraphedStep) these optimizers are captured: a load_state_dict that cannot be written in place raises from now on."""
    _CAPTURED.update(optimizers)


def _refuse_in_capture(what: str, advice: str) -> None:
    if torch.cuda.is_current_stream_capturing():
        raise hip.StswinHipError(f"{what} inside a hipGraph capture: {advice}")


class _Clock:
    """Device-resident step state: `counter` int32 [1] (steps taken) and `hyper` fp32 [4] = {lr, 1 - b1^t, sqrt(1 - b2^t), EMA
    momentum} (csrc/optim.hip, stswin_optim_tick).  The update kernels read their step-dependent scalars from `hyper`, so a hipGraph
    replay of the step advances them exactly like eager steps do.  `step` is the host mirror of the counter: exact after eager steps,
    re-read from the device at its first read after the replay generation moved."""

    def __init__(self, device, step: int = 0):
        _refuse_in_capture("a new device step clock (a parameter's first gradient, the first key-encoder update, a new parameter group)",
                           "run the step eagerly once before capturing it")
        self.counter = torch.full((1,), int(step), dtype=torch.int32, device=device)
        self.hyper = torch.zeros(4, dtype=torch.float32, device=device)
        self._step, self._gen = int(step), _generation
        self.lr = None                       # the value hyper[0] holds
        self.members = []                    # optimizer state dicts of the parameters that took the last step on this clock

    @property
    def step(self) -> int:
        return self._step if self._gen == _generation else self.sync()

    def sync(self) -> int:
        """Host mirror <- device counter (one device read)."""
        _refuse_in_capture("a host step mirror that graph replays left stale is read", "read it before the capture")
        self._step, self._gen = int(self.counter.item()), _generation
        return self._step

    def tick(self, kind: int, a: float, b: float) -> None:
        hip.optim_tick(kind, self.counter, self.hyper, a, b)
        if self._gen == _generation:         # (a stale mirror stays stale: its next read sees this tick on the device)
            self._step += 1

    def load(self, step: int) -> None:
        """Re-seed the counter in place (a captured graph keeps ticking this one); hyper is re-derived from it at the next tick."""
        _refuse_in_capture("a device step clock is re-seeded", "load before the capture or between replays")
        self.counter.fill_(int(step))
        self._step, self._gen = int(step), _generation

    def push_lr(self, lr: float) -> None:
        """Stream-ordered fill of hyper[0] when the host's learning rate differs from what the device holds (schedulers); a no-op
        otherwise.  Inside a capture the fill would become a graph node that overwrites every later push: refused."""
        lr = float(lr)
        if self.lr != lr:
            _refuse_in_capture(f"learning rate changed ({self.lr} -> {lr})", "change it in before_step, outside the captured step")
            self.hyper[0:1].fill_(lr)
            self.lr = lr


class LrClocks:
    """The device-resident learning rate of each parameter group of an SGD-like optimizer (lr is its only step-dependent scalar),
    by group POSITION: torch's load_state_dict replaces the group dicts, while a captured graph keeps reading these clocks."""

    def __init__(self):
        self.clocks = {}

    def hyper(self, i: int, lr: float, device) -> torch.Tensor:
        c = self.clocks.get(i)
        if c is None or c.hyper.device != device:
            c = self.clocks[i] = _Clock(device)
        c.push_lr(lr)
        return c.hyper

    def push(self, param_groups) -> None:
        """Before a graph replay: the groups' current learning rates -> device (graph.GraphedStep)."""
        for i, c in self.clocks.items():
            c.push_lr(param_groups[i]["lr"])


def load_in_place(opt, state_dict, owner) -> None:
    """torch's Optimizer.load_state_dict on `opt`, then the loaded values written INTO the state tensors and Adam clocks `opt` held
    before - a captured graph keeps their addresses, so replays after the load continue like eager steps after it.  A load that
    cannot be written so (another shape / dtype / device, no loaded tensor for one the graph reads, parameters of one clock loading
    different counts) raises when `owner` (opt or its wrapper) was captured, and leaves `opt` as it was; otherwise it keeps torch's
    new objects and the clocks are re-made at the next step."""
    old_state, old_groups = opt.state, opt.param_groups
    torch.optim.Optimizer.load_state_dict(opt, state_dict)
    copies, clocks, bad = [], {}, None
    for p, old in old_state.items():
        new = opt.state.get(p, {})
        for key, o in old.items():
            v = new.get(key)
            if key == "_clock":
                if old.get("step") == o.step:           # (one that sat the clock's last step out is not on it any more)
                    clocks.setdefault(id(o), (o, []))[1].append(new)
            elif torch.is_tensor(o):
                if torch.is_tensor(v) and v.shape == o.shape and v.dtype == o.dtype and v.device == o.device:
                    copies.append((new, key, o, v))
                else:
                    bad = f"state '{key}' of a parameter loads as {None if v is None else (tuple(v.shape), v.dtype, v.device)}"
    for c, sts in clocks.values():
        if bad is None and len({int(st.get("step", -1)) for st in sts}) != 1:
            bad = "parameters that share a device clock load different step counts"
    if bad is not None:
        if owner in _CAPTURED:
            opt.state, opt.param_groups = old_state, old_groups
            raise hip.StswinHipError(f"load_state_dict after a hipGraph capture cannot be written into what the graph reads: {bad}")
        return
    for new, key, o, v in copies:
        o.copy_(v)
        new[key] = o
    for c, sts in clocks.values():
        c.load(int(sts[0]["step"]))
        c.members = sts
        for st in sts:
            st["step"], st["_clock"] = c.step, c


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._gen = _generation
        self._clock_groups = []

    def _clocks(self):
        seen = {}
        for st in self.state.values():
            c = st.get("_clock")
            if c is not None:
                seen[id(c)] = c
        return list(seen.values())

    def push_hyper(self) -> None:
        """Before a graph replay: hand the groups' current learning rates to the device (stswincl_amd.graph.GraphedStep calls this)."""
        for clock, i in self._clock_groups:              # (clock, group position) pairs of the last step() - the one that was captured
            clock.push_lr(self.param_groups[i]["lr"])

    def sync_steps(self) -> None:
        """Host step counts <- device counters: a device read only at the first call after the replay generation moved
        (step() and state_dict() call it)."""
        if self._gen != _generation:
            for c in self._clocks():
                for st in c.members:        # (a parameter that shares the clock but sat the last step out keeps its own count)
                    st["step"] = c.step
            self._gen = _generation

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:                    # (torch.optim re-enables grad for the closure: it runs forward + backward)
            with torch.enable_grad():
                loss = closure()
        self.sync_steps()
        self._clock_groups = []
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            by_clock = {}         # torch.optim.Adam keeps the step count PER PARAMETER (bias corrections differ when a branch
            touched = []          # had no gradient on some steps, or a parameter was unfrozen later): one launch per count.
            fresh = {}            # Parameters at the same count share a device clock.
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if not isinstance(st["step"], int):          # a state loaded from torch.optim.Adam holds tensor steps: one host
                    st["step"] = int(st["step"])             # read, here, before any capture (see load_state_dict)
                clock = st.get("_clock")
                if clock is not None and clock.step != st["step"]:
                    clock = None                             # it sat out steps the clock's other parameters took: its own count, its own clock
                if clock is None:                            # first gradient (or a loaded state): join the clock of this count
                    key = (st["step"], p.device)
                    clock = fresh.get(key)
                    if clock is None:
                        clock = fresh[key] = next((c for (c, *_r) in by_clock.values() if c.step == st["step"] and c.counter.device == p.device),
                                                  None) or _Clock(p.device, st["step"])
                    st["_clock"] = clock
                _c, ps, gs, ms, vs, sts = by_clock.setdefault(id(clock), (clock, [], [], [], [], []))
                ps.append(p.data)
                touched.append(p)
                gs.append(p.grad.contiguous() if not p.grad.is_contiguous() else p.grad)
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
                sts.append(st)
            for clock, ps, gs, ms, vs, sts in by_clock.values():
                self._clock_groups.append((clock, gi))
                clock.push_lr(group["lr"])
                clock.tick(0, float(b1), float(b2))
                clock.members = sts
                for st in sts:
                    st["step"] = clock.step
                hip.multi_tensor(0, ps, gs, ms, vs, b1=b1, b2=b2, eps=group["eps"], wd=group["weight_decay"], hyper=clock.hyper)
            _mark_updated(touched)
        return loss

    def state_dict(self):
        """(the device clocks stay out of the checkpoint: `step` per parameter is what torch.optim.Adam writes, too)"""
        self.sync_steps()
        sd = super().state_dict()
        sd["state"] = {k: {kk: vv for kk, vv in v.items() if kk != "_clock"} for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """torch.optim.Adam checkpoints keep `step` as a (possibly GPU) tensor per parameter; the counts become Python ints here -
        once, outside any hipGraph capture.  The loaded state is written into the existing tensors and clocks (load_in_place)."""
        self.sync_steps()
        load_in_place(self, state_dict, self)
        for st in self.state.values():
            if "step" in st and not isinstance(st["step"], int):
                st["step"] = int(st["step"])


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self._lr = LrClocks()

    def push_hyper(self) -> None:
        self._lr.push(self.param_groups)

    def load_state_dict(self, state_dict):
        load_in_place(self, state_dict, self)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:                    # (torch.optim re-enables grad for the closure: it runs forward + backward)
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            first, later, touched = ([], [], []), ([], [], []), []
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                g = p.grad.contiguous() if not p.grad.is_contiguous() else p.grad
                if st.get("momentum_buffer") is None:      # (a loaded state may hold None: first step)
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    tgt = first
                else:
                    tgt = later
                tgt[0].append(p.data)
                touched.append(p)
                tgt[1].append(g)
                tgt[2].append(st["momentum_buffer"])
            for (ps, gs, ms), c1 in ((first, 1.0), (later, 0.0)):
                if ps:
                    hip.multi_tensor(1, ps, gs, ms, None, b1=group["momentum"], wd=group["weight_decay"], c1=c1,
                                     hyper=self._lr.hyper(gi, group["lr"], ps[0].device))
            _mark_updated(touched)
        return loss


@torch.no_grad()
def ema_update(keys: Sequence[torch.Tensor], queries: Sequence[torch.Tensor], momentum: float, hyper=None) -> None:
    """key <- key * momentum + query * (1 - momentum) for every pair.  Pass the key PARAMETERS (not their .data aliases):
    their version counters are bumped so that caches keyed on them see the update.  hyper (device fp32 [4]): the momentum is read
    from hyper[3] (EmaSchedule) instead of the argument."""
    hip.multi_tensor(2, [k.data for k in keys], [q.data for q in queries], b1=momentum, hyper=hyper)
    _mark_updated(list(keys))


class EmaSchedule:
    """The key-encoder momentum schedule of PixPro_swin_v5.py:258-262 - m = 1 - (1 - m0)(cos(pi k / K) + 1) / 2, k += 1 per update -
    with k and m in device memory (stswin_optim_tick kind 1), so that eager steps and hipGraph replays of the step walk the same
    schedule.  `k` is the clock's host mirror (_Clock.step)."""

    def __init__(self, device, base_momentum: float, K: int, k: int = 0):
        self.clock = _Clock(device, k)
        self.m0, self.K = float(base_momentum), float(K)

    def tick(self) -> torch.Tensor:
        self.clock.tick(1, self.m0, self.K)
        return self.clock.hyper

    @property
    def k(self) -> int:
        return self.clock.step

    def sync(self) -> int:
        return self.clock.sync()


def make_contrast_optimizer(params, batch_size: int, base_learning_rate: float = 1.0, momentum: float = 0.9,
                            weight_decay: float = 1e-5, optimizer: str = "lars"):
    """The optimizer stack of main_pretrain_swinv5.py:32-47 on the fused kernels: lr = global batch / 256 * base lr;
    'lars': add_weight_decay groups (1-D parameters: no decay, no trust ratio) + SGD momentum under LARS; 'sgd': plain
    SGD momentum with weight decay.  -> (optimizer, short name for reports)."""
    from .contrast.lars import LARS
    params = list(params)
    lr = batch_size / 256.0 * base_learning_rate
    if optimizer == "sgd":
        return FusedSGD(params, lr, momentum=momentum, weight_decay=weight_decay), "SGD"
    groups = [{"params": [p for p in params if p.dim() == 1], "weight_decay": 0, "ignore": True},
              {"params": [p for p in params if p.dim() != 1], "weight_decay": weight_decay, "ignore": False}]
    return LARS(FusedSGD(groups, lr, momentum=momentum)), "LARS(SGD)"
