"""Optimizers.

Replaces the reference's DistributedOptimizer-over-RPC
(reference: experiment/launch.py:152-156, runner.py:139): in the SPMD world
each rank steps its OWN stage's parameters locally after its backward —
there is no cross-rank optimizer traffic at all.

FusedSGD keeps optional fp32 master weights for bf16 parameters and uses
the multi-tensor HIP SGD kernel on GPU (single launch over all chunks);
on CPU it applies the same math eagerly.

FusedAdamW is the fine-tuning optimizer: the multi-tensor HIP AdamW kernel
with the gradient clip folded in, per-tensor weight-decay exemption, and its
step count, clip factor and lr kept on the device so that a captured step
stays live under graph replay. build_optimizer picks between the two by
config (the reference's ``getattr(torch.optim, optim_type)``).
"""

from __future__ import annotations

import torch

from . import ops
from .ops import hiplib


class FusedSGD:
    def __init__(
        self,
        params,
        lr: float = 1e-3,
        momentum: float = 0.0,
        weight_decay: float = 0.0,
        master_weights: bool | None = None,
    ):
        self.params = [p for p in params if p.requires_grad]
        self.lr = lr
        self.momentum = momentum
        self.weight_decay = weight_decay
        if master_weights is None:
            master_weights = any(p.dtype == torch.bfloat16 for p in self.params)
        self.masters = (
            [p.detach().clone().float() for p in self.params] if master_weights else None
        )
        # momentum buffers are ALWAYS fp32: the HIP multi-tensor path reads
        # them as float* (ops/hip/sgd.hip) regardless of the param dtype,
        # and fp32 accumulation is the numerically right choice for bf16
        # params even without master weights.
        self.momentum_bufs = (
            [torch.zeros(p.shape, dtype=torch.float32, device=p.device)
             for p in self.params]
            if momentum != 0.0
            else None
        )
        self._gpu_plan = None  # lazy multi-tensor launch plan

    @torch.no_grad()
    def sync_masters(self):
        """Refresh fp32 masters (and reset momentum) from the CURRENT param
        values. Must be called after any out-of-band weight mutation
        (checkpoint restore, ParameterServer scatter) or the next step()
        would write ``stale_master - lr*grad`` back over the restored
        weights."""
        if self.masters is not None:
            for m, p in zip(self.masters, self.params):
                m.copy_(p.detach().float())
        if self.momentum_bufs is not None:
            for b in self.momentum_bufs:
                b.zero_()

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().zero_()

    @torch.no_grad()
    def step(self):
        grads = [p.grad for p in self.params]
        use_hip = (
            hiplib.available()
            and self.params
            and self.params[0].is_cuda
            and all(g is not None for g in grads)
        )
        if use_hip:
            self._hip_step(grads)
        else:
            ops.sgd_step(
                self.params, grads, self.lr, self.momentum, self.weight_decay,
                self.momentum_bufs, self.masters,
            )

    def _hip_step(self, grads):
        from .ops.multi_tensor import multi_tensor_sgd

        multi_tensor_sgd(
            self.params, grads, self.masters, self.momentum_bufs,
            self.lr, self.momentum, self.weight_decay,
        )

    def state_dict(self) -> dict:
        return {
            "lr": self.lr, "momentum": self.momentum, "weight_decay": self.weight_decay,
            "masters": self.masters, "momentum_bufs": self.momentum_bufs,
        }

    def load_state_dict(self, sd: dict):
        self.lr = sd["lr"]
        self.momentum = sd["momentum"]
        self.weight_decay = sd["weight_decay"]
        if sd.get("masters") is not None and self.masters is not None:
            for m, s in zip(self.masters, sd["masters"]):
                m.copy_(s.to(m.device))
        if sd.get("momentum_bufs") is not None and self.momentum_bufs is not None:
            for m, s in zip(self.momentum_bufs, sd["momentum_bufs"]):
                m.copy_(s.to(m.device))


# word indices of the device hyper block (layout: ops/hip/adamw.hip)
_H_LR, _H_CLIP, _H_GNORM, _H_STEP, _H_WORDS = 0, 1, 2, 6, 8


class FusedAdamW:
    """AdamW (decoupled weight decay, torch.optim.AdamW's semantics) with
    the gradient clip folded into the update, over the same surface as
    FusedSGD.

    On GPU one step is four launches of ops/hip/adamw.hip: the gradient
    norm in two kernels (only with ``max_grad_norm``), the step counter's
    tick, and the multi-tensor update, which multiplies the clip factor in
    as it loads each gradient (gradients are never rewritten). Everything
    that changes from step to step — the step count and its bias
    corrections, the clip factor, ``lr`` — lives in a small device tensor,
    the hyper block, so a ``step()`` captured in a hipGraph keeps counting,
    clipping and following an lr schedule under replay. ``step()`` makes no
    allocation and no synchronisation after its first call, which builds the
    launch plan.

    ``no_decay``: a predicate on the parameter tensor, a list of bools (one
    per entry of ``params``), or ``"1d"`` for every tensor with
    ``ndim <= 1`` (biases and LayerNorm parameters); those tensors get no
    weight decay. Clipping is per rank, over this optimizer's parameters.
    Moments are always fp32."""

    def __init__(
        self,
        params,
        lr: float = 1e-3,
        betas: tuple[float, float] = (0.9, 0.999),
        eps: float = 1e-8,
        weight_decay: float = 0.01,
        master_weights: bool | None = None,
        max_grad_norm: float | None = None,
        no_decay=None,
    ):
        params = list(params)
        if no_decay is None:
            exempt = [False] * len(params)
        elif no_decay == "1d":
            exempt = [p.ndim <= 1 for p in params]
        elif callable(no_decay):
            exempt = [bool(no_decay(p)) for p in params]
        else:
            exempt = [bool(x) for x in no_decay]
            if len(exempt) != len(params):
                raise ValueError(
                    f"no_decay has {len(exempt)} entries for {len(params)} params")
        self.no_decay = [e for e, p in zip(exempt, params) if p.requires_grad]
        self.params = [p for p in params if p.requires_grad]
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.weight_decay = float(weight_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if master_weights is None:
            master_weights = any(p.dtype == torch.bfloat16 for p in self.params)
        self.masters = (
            [p.detach().clone().float() for p in self.params] if master_weights else None
        )
        self.exp_avgs = [torch.zeros(p.shape, dtype=torch.float32, device=p.device)
                         for p in self.params]
        self.exp_avg_sqs = [torch.zeros(p.shape, dtype=torch.float32, device=p.device)
                            for p in self.params]
        device = self.params[0].device if self.params else torch.device("cpu")
        self._lr = float(lr)
        host = torch.zeros(_H_WORDS, dtype=torch.float32)
        host[_H_LR] = self._lr
        host[_H_CLIP] = 1.0
        self._hyper = host.to(device)
        self._lr_slot = self._hyper[_H_LR:_H_LR + 1]
        self._step_slot = self._hyper.view(torch.int32)[_H_STEP:_H_STEP + 1]

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float):
        # a stream-ordered write of the device copy, and only on a change:
        # the next step reads it, captured or not
        value = float(value)
        if value != self._lr:
            self._lr = value
            self._lr_slot.fill_(value)

    @property
    def grad_norm(self) -> torch.Tensor:
        """The unclipped gradient norm of the last step that clipped, as a
        0-dim device tensor. Reading its value synchronises; fetching it
        does not."""
        return self._hyper[_H_GNORM]

    @property
    def step_count(self) -> int:
        """The number of steps taken (reads the device counter: synchronises)."""
        return int(self._step_slot.item())

    @torch.no_grad()
    def sync_masters(self):
        """Refresh fp32 masters from the CURRENT param values, zero both
        moments and reset the step counter to 0. Must be called after any
        out-of-band weight mutation (checkpoint restore, ParameterServer
        scatter). Optimizer state is not part of those checkpoints, so a
        restore restarts the moments and the bias correction: the next step
        is a fresh optimizer's first step."""
        if self.masters is not None:
            for m, p in zip(self.masters, self.params):
                m.copy_(p.detach().float())
        for b in self.exp_avgs + self.exp_avg_sqs:
            b.zero_()
        self._step_slot.zero_()

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().zero_()

    @torch.no_grad()
    def step(self):
        grads = [p.grad for p in self.params]
        use_hip = (
            hiplib.available()
            and self.params
            and self.params[0].is_cuda
            and all(g is not None for g in grads)
        )
        if use_hip:
            from .ops.multi_tensor import multi_tensor_adamw

            multi_tensor_adamw(
                self.params, grads, self.masters, self.exp_avgs,
                self.exp_avg_sqs, self._hyper, self.betas[0], self.betas[1],
                self.eps, self.weight_decay, self.no_decay, self.max_grad_norm,
            )
            return
        t = self.step_count + 1
        norm, clip = ops.adamw_step(
            self.params, grads, self.exp_avgs, self.exp_avg_sqs, t, self._lr,
            self.betas[0], self.betas[1], self.eps, self.weight_decay,
            self.masters, self.max_grad_norm, self.no_decay,
        )
        self._step_slot.fill_(t)
        if norm is not None:
            self._hyper[_H_GNORM].copy_(norm)
            self._hyper[_H_CLIP].copy_(clip)

    def state_dict(self) -> dict:
        return {
            "lr": self._lr, "betas": self.betas, "eps": self.eps,
            "weight_decay": self.weight_decay, "max_grad_norm": self.max_grad_norm,
            "no_decay": list(self.no_decay), "step": self.step_count,
            "masters": self.masters, "exp_avgs": self.exp_avgs,
            "exp_avg_sqs": self.exp_avg_sqs,
        }

    @torch.no_grad()
    def load_state_dict(self, sd: dict):
        self.lr = sd["lr"]
        self.betas = tuple(sd["betas"])
        self.eps = sd["eps"]
        self.weight_decay = sd["weight_decay"]
        self.max_grad_norm = sd["max_grad_norm"]
        self.no_decay = list(sd["no_decay"])
        self._step_slot.fill_(int(sd["step"]))
        if sd.get("masters") is not None and self.masters is not None:
            for m, s in zip(self.masters, sd["masters"]):
                m.copy_(s.to(m.device))
        for mine, key in ((self.exp_avgs, "exp_avgs"), (self.exp_avg_sqs, "exp_avg_sqs")):
            for m, s in zip(mine, sd[key]):
                m.copy_(s.to(m.device))


def _classification_loss():
    def loss_fn(logits, labels):
        return torch.nn.functional.cross_entropy(logits.float(), labels)

    return loss_fn


def _masked_lm_loss(num_classes: int | None = None, ignore_index: int = -100,
                    inplace_backward: bool = False):
    def loss_fn(logits, labels):
        return ops.softmax_cross_entropy(
            logits, labels, ignore_index=ignore_index, num_classes=num_classes,
            inplace_backward=inplace_backward)

    return loss_fn


LOSSES = {"CrossEntropy": _classification_loss, "MaskedLM": _masked_lm_loss}


def build_loss(cfg: dict | None = None):
    """Build ``loss_fn(logits, labels)`` from a config dict: ``type`` names
    it, every other key goes to its builder.

    ``"CrossEntropy"`` (also when ``cfg`` is empty or None) is the
    classification loss, ``cross_entropy(logits.float(), labels)``.
    ``"MaskedLM"`` takes ``num_classes`` (the vocabulary size; the logits'
    further columns are padding), ``ignore_index`` and ``inplace_backward``
    and calls ops.softmax_cross_entropy: the mean over the labelled tokens.

    With microbatches the engines average these per-microbatch means, and
    scale each backward by 1/M. For MaskedLM the step loss is therefore the
    mean of per-microbatch valid-token means, which weights a token of a
    sparsely labelled microbatch more than the mean over all of the step's
    labelled tokens would; a microbatch with no labelled token counts as 0."""
    kwargs = dict(cfg or {})
    kind = kwargs.pop("type", "CrossEntropy")
    if kind not in LOSSES:
        raise ValueError(
            f"unknown loss type {kind!r}; known types: {sorted(LOSSES)}")
    return LOSSES[kind](**kwargs)


OPTIMIZERS = {"SGD": FusedSGD, "AdamW": FusedAdamW}


def build_optimizer(cfg: dict, params):
    """Build an optimizer from a config dict: ``type`` names it ("SGD" when
    absent), every other key goes to its constructor."""
    kwargs = dict(cfg)
    kind = kwargs.pop("type", "SGD")
    if kind not in OPTIMIZERS:
        raise ValueError(
            f"unknown optimizer type {kind!r}; known types: {sorted(OPTIMIZERS)}")
    return OPTIMIZERS[kind](params, **kwargs)
