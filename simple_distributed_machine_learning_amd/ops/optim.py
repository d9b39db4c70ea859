"""Per-stage fused SGD with momentum over the rank's flat parameter buffer.

Replaces ``DistributedOptimizer(optim.SGD, param_rrefs, lr=0.1, momentum=0.5)``
(/root/reference/simple_distributed.py:100-104, :113), which creates one TorchScript
``_FunctionalSGD`` per parameter owner and drives each step by RPC. Here each rank updates
the parameters it owns with ONE kernel launch over its flat buffer (utils/flat.py); the
update rule is torch.optim.SGD's (dampening 0, no nesterov, no weight decay by default):
``buf = momentum * buf + g`` (``buf = g`` on the first step), ``p -= lr * buf``.
"""
from __future__ import annotations

import os

import torch

from . import (ADAMW_PREP_FLOATS, DECAY_GRANULE, PREP_LR, PREP_NORM, SQNORM_MAX_BLOCKS, adamw_, adamw_mixed_,
               adamw_prep, grad_sqnorm, sgd_momentum_, sgd_momentum_mixed_)
from .reference import lr_at
from ..utils.flat import ALIGN, FlatParams


def make_schedule(kind: str = "constant", warmup: int = 0, decay_steps: int = 0, min_lr: float = 0.0):
    """The learning-rate schedule as the optimizers take it (``reference.lr_at``'s keywords), or None when the
    learning rate never changes (constant, no warmup)."""
    if kind not in ("constant", "cosine"):
        raise ValueError(f"unknown lr schedule {kind!r} (constant, cosine)")
    if warmup < 0 or decay_steps < 0:
        raise ValueError("lr schedule: warmup and decay_steps must be >= 0")
    if warmup == 0 and (kind == "constant" or decay_steps == 0):
        return None
    return {"kind": kind, "warmup": int(warmup), "decay_steps": int(decay_steps), "min_lr": float(min_lr)}


class FusedSGD:
    kind = "sgd"

    def __init__(self, flat: FlatParams, lr: float, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, schedule=None):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.flat = flat
        # host-side schedule (reference.lr_at): ``lr`` is set from it before each eager step; a captured step would
        # freeze one value, so the engine keeps the fused / one-launch / graphed SGD paths off with a schedule
        self.schedule, self.base_lr = schedule, lr
        self.lr, self.momentum, self.dampening = lr, momentum, dampening
        self.weight_decay, self.nesterov = weight_decay, nesterov
        # low-precision models (bf16 GPT-2) keep fp32 master weights + fp32 momentum here
        self.master = flat.params.float().clone() if flat.params.dtype != torch.float32 else None
        ref = self.master if self.master is not None else flat.params
        self.momentum_buffer = torch.zeros_like(ref) if momentum != 0 else ref.new_zeros(64)
        self.steps = 0
        self.plane_cache = None  # (PlaneCache, weight, flat offset): written by the step kernel

    def add_plane_cache(self, cache, weight: torch.Tensor) -> bool:
        """Have the fp32 step kernel also write ``cache`` (ops.PlaneCache) from ``weight``'s updated
        values. One cache per optimizer (the kernel takes one); returns False if not taken."""
        if self.master is not None or self.plane_cache is not None or not self.flat.params.is_cuda:
            return False
        off = (weight.data_ptr() - self.flat.params.data_ptr()) // self.flat.params.element_size()
        if not (0 <= off < self.flat.numel) or off % 4 or weight.shape[1] % 4:
            return False
        self.plane_cache = (cache, weight, off)
        return True

    def step(self, zero_grad: bool = True):
        """One update. ``zero_grad`` clears the gradients inside the same kernel (the engine
        then skips its own zero_grad at the next step: one launch, one pass over memory)."""
        if self.schedule is not None:
            self.lr = lr_at(self.steps + 1, self.base_lr, **self.schedule)
        if self.master is not None:
            sgd_momentum_mixed_(self.master, self.flat.params, self.flat.grads, self.momentum_buffer, self.lr,
                                self.momentum, self.dampening, self.weight_decay, self.nesterov, self.steps == 0,
                                zero_grad)
        else:
            planes = None
            if self.plane_cache is not None:
                cache, w, off = self.plane_cache
                planes = (cache.planes, off, w.shape[0], w.shape[1])
            sgd_momentum_(self.flat.params, self.flat.grads, self.momentum_buffer, self.lr, self.momentum,
                          self.dampening, self.weight_decay, self.nesterov, self.steps == 0, zero_grad, planes)
        if zero_grad:
            self.flat.grads_zero = True
        self.steps += 1
        self.flat.param_epoch += 1
        _weights_rewritten()
        if self.plane_cache is not None:
            from . import PlaneCache

            cache, w, _ = self.plane_cache
            cache.token = PlaneCache.token_of(w, self.flat.param_epoch)

    def fused_args(self, spans, zero_grad: bool = True):
        """Arguments for applying this optimizer's step inside the reduction that produces the step's
        last gradients (ops.linear_wgrad_u8_dl ``sgd``), or None when that cannot cover the whole step:
        ``spans`` = [(first grad tensor, numel)] of the flat gradient ranges that reduction writes;
        every parameter segment must lie inside them (the padding between segments stays zero)."""
        if self.master is not None or not self.flat.params.is_cuda or os.environ.get("SDML_FUSED_STEP", "1") == "0":
            return None
        base, es = self.flat.grads.data_ptr(), self.flat.grads.element_size()
        ranges = [((t.data_ptr() - base) // es, n) for t, n in spans]
        for seg in self.flat.segments:
            if not any(o <= seg.offset and seg.offset + seg.numel <= o + n for o, n in ranges):
                return None
        planes, poff, prows, pk = None, 0, 0, 0
        if self.plane_cache is not None:
            cache, w, poff = self.plane_cache
            planes, prows, pk = cache.planes, w.shape[0], w.shape[1]
        return (self.flat.params, self.flat.grads, self.momentum_buffer, float(self.lr), float(self.momentum),
                float(self.dampening), float(self.weight_decay), bool(self.nesterov), self.steps == 0,
                bool(zero_grad), planes, int(poff), int(prows), int(pk))

    def commit_fused(self, zero_grad: bool = True, planes_current: bool = True):
        """Book-keeping of a step that a fused kernel applied (what step() does after its kernel):
        ``fused_args``' reductions, or the whole-step kernel (``planes_current=False``: it did not
        write the weight-plane cache, which the next uint8 forward then re-splits)."""
        if zero_grad:
            self.flat.grads_zero = True
        self.steps += 1
        self.flat.param_epoch += 1
        _weights_rewritten()
        if self.plane_cache is not None:
            from . import PlaneCache

            cache, w, _ = self.plane_cache
            cache.token = PlaneCache.token_of(w, self.flat.param_epoch) if planes_current else None

    def buffer_view(self, param: torch.Tensor):
        """The momentum buffer's view aligned with ``param`` (a view into the flat parameter buffer), or
        None without momentum."""
        if self.momentum == 0:
            return None
        off = (param.data_ptr() - self.flat.params.data_ptr()) // self.flat.params.element_size()
        return self.momentum_buffer[off:off + param.numel()].view(param.shape)

    def zero_grad(self):
        self.flat.zero_grad()

    # ---- checkpoint (per-parameter names, reference-compatible keys) ----------------------
    def state_dict_for_stage(self, stage: int) -> dict:
        bufs = {}
        for seg in self.flat.segments:
            if seg.stage == stage and self.momentum != 0:
                bufs[seg.name] = self.momentum_buffer[seg.offset:seg.offset + seg.numel].view(seg.shape).detach().cpu().clone()
        out = {"momentum_buffer": bufs, "steps": self.steps, "lr": self.lr, "momentum": self.momentum,
               "dampening": self.dampening, "weight_decay": self.weight_decay, "nesterov": self.nesterov}
        if self.master is not None:
            out["master"] = {seg.name: self.master[seg.offset:seg.offset + seg.numel].view(seg.shape).detach().cpu().clone()
                             for seg in self.flat.segments if seg.stage == stage}
        return out

    def load_state_dict_for_stage(self, stage: int, sd: dict):
        for seg in self.flat.segments:
            if seg.stage == stage and seg.name in sd.get("momentum_buffer", {}):
                self.momentum_buffer[seg.offset:seg.offset + seg.numel].copy_(
                    sd["momentum_buffer"][seg.name].reshape(-1).to(self.momentum_buffer))
        if self.master is not None:
            for seg in self.flat.segments:
                if seg.stage != stage:
                    continue
                src = sd.get("master", {}).get(seg.name)
                dst = self.master[seg.offset:seg.offset + seg.numel]
                # without saved master weights fall back to the (rounded) model weights
                dst.copy_(src.reshape(-1) if src is not None else
                          self.flat.params[seg.offset:seg.offset + seg.numel].float())
        self.steps = max(self.steps, int(sd.get("steps", 0)))


class FusedAdamW:
    """torch.optim.AdamW over the flat buffer, with global-norm gradient clipping (``clip_grad`` = the maximum norm,
    0: off; ``clip_grad_norm_``'s coefficient) and a learning-rate schedule (``make_schedule``).

    Weight decay is decoupled and applies to parameters with ``dim >= 2`` only (biases, LayerNorm and BatchNorm
    vectors are not decayed); a table with one entry per 64-element granule of the flat buffer carries that mask
    to the kernel. The step counter, and everything that depends on it (bias corrections, learning rate, clip
    coefficient), live on the device: a step is [sum g^2 ->] prep -> update with no host synchronisation, and a
    captured step (parallel/graphs.py) replays correctly. ``norm_reduce`` (set by the engine when a pipeline's
    stages live on different ranks) sums the squared norm across ranks in between.
    """

    kind = "adamw"

    def __init__(self, flat: FlatParams, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 clip_grad: float = 0.0, schedule=None):
        b1, b2 = float(betas[0]), float(betas[1])
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"AdamW: betas must be in [0, 1), got {betas}")
        if lr < 0 or eps < 0 or weight_decay < 0 or clip_grad < 0:
            raise ValueError("AdamW: lr, eps, weight_decay and clip_grad must be >= 0")
        assert ALIGN == DECAY_GRANULE
        self.flat = flat
        self.lr, self.betas, self.eps = float(lr), (b1, b2), float(eps)
        self.weight_decay, self.clip_grad, self.schedule = float(weight_decay), float(clip_grad), schedule
        dev = flat.params.device
        self.master = flat.params.float().clone() if flat.params.dtype != torch.float32 else None
        ref = self.master if self.master is not None else flat.params
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(ref), torch.zeros_like(ref)
        self.decay = self._decay_table(flat).to(dev)
        self.steps = 0
        self.step_ctr = torch.zeros(1, dtype=torch.int64, device=dev)  # steps taken, as the kernels see it
        self.prep = torch.zeros(ADAMW_PREP_FLOATS, device=dev, dtype=torch.float32 if dev.type == "cuda" else torch.float64)
        self.norm2 = torch.zeros(1, dtype=torch.float64, device=dev)
        self.partials = torch.zeros(SQNORM_MAX_BLOCKS, dtype=torch.float32, device=dev) if dev.type == "cuda" else None
        self.norm_reduce = None  # callable(float64 [1] tensor): in-place sum over the ranks that hold the other stages
        self.plane_cache = None

    @staticmethod
    def _decay_table(flat: FlatParams) -> torch.Tensor:
        """uint8, one entry per 64-element granule: 1 where the granule belongs to a parameter with dim >= 2
        (offsets are padded to 64 elements, so no granule spans two parameters)."""
        t = torch.zeros((flat.numel + DECAY_GRANULE - 1) // DECAY_GRANULE, dtype=torch.uint8)
        for seg in flat.segments:
            if len(seg.shape) >= 2:
                t[seg.offset // DECAY_GRANULE:(seg.offset + seg.numel + DECAY_GRANULE - 1) // DECAY_GRANULE] = 1
        return t

    # the SGD step kernel's extras (weight-plane cache, the step fused into a reduction) are not available here
    def add_plane_cache(self, cache, weight: torch.Tensor) -> bool:
        return False

    def fused_args(self, spans, zero_grad: bool = True):
        return None

    @property
    def last_grad_norm(self):
        """The global gradient norm of the last step as a device scalar (no synchronisation); None with clipping
        off (the norm is not computed then)."""
        return self.prep[PREP_NORM] if self.clip_grad > 0 else None

    @property
    def last_lr(self):
        """The learning rate of the last step as a device scalar (no synchronisation)."""
        return self.prep[PREP_LR]

    def step(self, zero_grad: bool = True):
        b1, b2 = self.betas
        g = self.flat.grads
        if self.clip_grad > 0 and self.norm_reduce is not None:
            grad_sqnorm(g, out=self.norm2, partials=self.partials)
            self.norm_reduce(self.norm2)
            adamw_prep(self.step_ctr, self.prep, self.lr, b1, b2, self.clip_grad, self.schedule, norm2=self.norm2)
        elif self.clip_grad > 0:
            adamw_prep(self.step_ctr, self.prep, self.lr, b1, b2, self.clip_grad, self.schedule, g=g,
                       partials=self.partials, norm2=self.norm2)
        else:
            adamw_prep(self.step_ctr, self.prep, self.lr, b1, b2, 0.0, self.schedule)
        if self.master is not None:
            adamw_mixed_(self.master, self.flat.params, g, self.exp_avg, self.exp_avg_sq, self.decay, self.prep, b1, b2,
                         self.eps, self.weight_decay, zero_grad)
        else:
            adamw_(self.flat.params, g, self.exp_avg, self.exp_avg_sq, self.decay, self.prep, b1, b2, self.eps,
                   self.weight_decay, zero_grad)
        self.commit_fused(zero_grad)

    def commit_fused(self, zero_grad: bool = True, planes_current: bool = True):
        """Book-keeping of a step the kernels applied: step() after its launches, and a replayed graph (whose
        launches advanced the device counter themselves)."""
        if zero_grad:
            self.flat.grads_zero = True
        self.steps += 1
        self.flat.param_epoch += 1
        _weights_rewritten()

    def zero_grad(self):
        self.flat.zero_grad()

    # ---- checkpoint (per-parameter names; tensors and numbers only: weights_only loading) --------
    def _views(self, buf, stage: int) -> dict:
        return {seg.name: buf[seg.offset:seg.offset + seg.numel].view(seg.shape).detach().cpu().clone()
                for seg in self.flat.segments if seg.stage == stage}

    def state_dict_for_stage(self, stage: int) -> dict:
        out = {"exp_avg": self._views(self.exp_avg, stage), "exp_avg_sq": self._views(self.exp_avg_sq, stage),
               "steps": self.steps, "lr": self.lr, "beta1": self.betas[0], "beta2": self.betas[1], "eps": self.eps,
               "weight_decay": self.weight_decay, "clip_grad": self.clip_grad}
        if self.master is not None:
            out["master"] = self._views(self.master, stage)
        return out

    def load_state_dict_for_stage(self, stage: int, sd: dict):
        for seg in self.flat.segments:
            if seg.stage != stage:
                continue
            sl = slice(seg.offset, seg.offset + seg.numel)
            for key, buf in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                if seg.name in sd.get(key, {}):
                    buf[sl].copy_(sd[key][seg.name].reshape(-1).to(buf))
            if self.master is not None:
                src = sd.get("master", {}).get(seg.name)
                # without saved master weights fall back to the (rounded) model weights
                self.master[sl].copy_(src.reshape(-1) if src is not None else self.flat.params[sl].float())
        self.steps = max(self.steps, int(sd.get("steps", 0)))
        self.step_ctr.fill_(self.steps)


def _weights_rewritten():
    """The step kernels rewrote parameters through raw pointers: drop weight-derived caches keyed on tensor
    versions (ops/conv.py's kernel weight layouts)."""
    from .conv import bump_weight_generation

    bump_weight_generation()
