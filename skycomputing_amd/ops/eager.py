"""Eager (plain PyTorch) implementations of every fused op.

These serve two purposes:
  * the CPU execution path (tests, gloo multi-process plumbing), and
  * the fp32 numerics reference that every HIP kernel is tested against
    (tests/test_ops_gpu.py compares HIP bf16 kernels vs these in fp32).

The op set mirrors the reference's BERT hot path (reference:
scaelum/model/bert_layers.py:21-168 — gelu/bias_gelu/swish/bias_tanh,
LayerNorm, LinearActivation; :249-275 masked softmax) but is organized as a
fusion-shaped functional API so the HIP kernels slot in 1:1.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def gelu(x: torch.Tensor) -> torch.Tensor:
    """erf-formula GELU (the reference's formula, not tanh-approx)."""
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def bias_gelu(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return gelu(x + bias)


def swish(x: torch.Tensor) -> torch.Tensor:
    return x * torch.sigmoid(x)


def bias_tanh(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return torch.tanh(x + bias)


ACT_FNS = {"gelu": gelu, "relu": F.relu, "swish": swish, "tanh": torch.tanh}


def layer_norm(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    eps: float = 1e-12,
    residual: torch.Tensor | None = None,
) -> torch.Tensor:
    """LayerNorm over the last dim with optional fused residual add.

    Accumulates in fp32 regardless of input dtype (what the HIP kernel does).
    """
    if residual is not None:
        x = x + residual
    orig_dtype = x.dtype
    y = F.layer_norm(x.float(), (x.shape[-1],), weight.float(), bias.float(), eps)
    return y.to(orig_dtype)


def masked_softmax(scores: torch.Tensor, mask: torch.Tensor | None) -> torch.Tensor:
    """softmax(scores + mask) over the last dim, fp32 accumulation.

    ``mask`` is the additive extended attention mask ((1-m) * -10000,
    broadcastable to ``scores``), as built by the embeddings layer.
    """
    orig_dtype = scores.dtype
    s = scores.float()
    if mask is not None:
        s = s + mask.float()
    return F.softmax(s, dim=-1).to(orig_dtype)


def attention_context(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    mask: torch.Tensor | None,
    dropout_p: float = 0.0,
    training: bool = False,
) -> torch.Tensor:
    """Full attention: softmax(QK^T/sqrt(d) + mask) V.

    q/k/v: [B, h, S, d]. Returns [B, h, S, d].
    """
    d = q.shape[-1]
    scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(d)
    probs = masked_softmax(scores, mask)
    if dropout_p > 0.0 and training:
        probs = F.dropout(probs, p=dropout_p, training=True)
    return torch.matmul(probs, v)


def linear_act(
    x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, act: str = "gelu"
) -> torch.Tensor:
    """Linear + bias + activation in one op (GEMM-epilogue fusion target).

    Mirrors the reference's LinearActivation fused module
    (reference: scaelum/model/bert_layers.py:60-108)."""
    y = F.linear(x, weight)
    if bias is not None:
        if act == "gelu":
            return bias_gelu(y, bias)
        if act == "tanh":
            return bias_tanh(y, bias)
        y = y + bias
    return ACT_FNS[act](y) if act != "none" else y


def embedding_fused(
    input_ids: torch.Tensor,
    token_type_ids: torch.Tensor,
    position_ids: torch.Tensor,
    word_emb: torch.Tensor,
    pos_emb: torch.Tensor,
    type_emb: torch.Tensor,
    ln_weight: torch.Tensor,
    ln_bias: torch.Tensor,
    eps: float = 1e-12,
) -> torch.Tensor:
    """3-way embedding gather + add + LayerNorm (dropout applied by caller)."""
    e = (
        F.embedding(input_ids, word_emb)
        + F.embedding(position_ids, pos_emb)
        + F.embedding(token_type_ids, type_emb)
    )
    return layer_norm(e, ln_weight, ln_bias, eps)


def softmax_cross_entropy(
    logits: torch.Tensor,
    labels: torch.Tensor,
    ignore_index: int = -100,
    num_classes: int | None = None,
) -> torch.Tensor:
    """Mean cross-entropy over the valid rows of logits [..., ld], fp32,
    0-dim; the semantics of the HIP kernels (ops/hip/xent.hip):

      * columns num_classes..ld-1 are padding: sliced off, gradient 0;
      * a row is valid iff 0 <= label < num_classes and
        label != ignore_index; any other label ignores the row (torch
        raises on an out-of-range label);
      * no valid row gives loss 0 and zero gradients (torch gives NaN);
      * ignored rows contribute nothing whatever they hold.
    """
    ld = logits.shape[-1]
    V = ld if num_classes is None else int(num_classes)
    if not 1 <= V <= ld:
        raise ValueError(f"num_classes {V} outside 1..{ld}")
    if labels.shape != logits.shape[:-1]:
        raise ValueError(
            f"labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
    z = logits.reshape(-1, ld)[:, :V].float()
    lab = labels.reshape(-1).to(torch.int64)
    valid = (lab >= 0) & (lab < V) & (lab != ignore_index)
    # ignored rows are replaced, not multiplied by 0: a NaN there stays out
    # of the loss and of the gradient
    z = z.masked_fill(~valid[:, None], 0.0)
    rowloss = F.cross_entropy(z, torch.where(valid, lab, torch.zeros_like(lab)),
                              reduction="none")
    rowloss = torch.where(valid, rowloss, torch.zeros_like(rowloss))
    count = valid.sum()
    return rowloss.sum() / count.clamp(min=1).to(rowloss.dtype)


@torch.no_grad()
def sgd_step(
    params: list[torch.Tensor],
    grads: list[torch.Tensor],
    lr: float,
    momentum: float = 0.0,
    weight_decay: float = 0.0,
    momentum_bufs: list[torch.Tensor] | None = None,
    master_params: list[torch.Tensor] | None = None,
):
    """Multi-tensor SGD. With ``master_params`` (fp32), the update is applied
    to the master copy and the (possibly bf16) param is refreshed from it."""
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            continue
        target = master_params[i] if master_params is not None else p
        # the update is computed in fp32 (momentum buffers are fp32 even
        # when the params are bf16 without masters — see FusedSGD)
        gf = g.float()
        if weight_decay != 0.0:
            gf = gf.add(target.float(), alpha=weight_decay)
        if momentum != 0.0:
            buf = momentum_bufs[i]
            buf.mul_(momentum).add_(gf)
            gf = buf
        if target.dtype == torch.float32:
            target.add_(gf, alpha=-lr)
        else:
            target.copy_((target.float().add_(gf, alpha=-lr)).to(target.dtype))
        if master_params is not None:
            p.copy_(target.to(p.dtype))


@torch.no_grad()
def adamw_step(
    params: list[torch.Tensor],
    grads: list[torch.Tensor],
    exp_avgs: list[torch.Tensor],
    exp_avg_sqs: list[torch.Tensor],
    step: int,
    lr: float,
    beta1: float = 0.9,
    beta2: float = 0.999,
    eps: float = 1e-8,
    weight_decay: float = 0.01,
    master_params: list[torch.Tensor] | None = None,
    max_grad_norm: float | None = None,
    no_decay: list[bool] | None = None,
):
    """Multi-tensor AdamW (decoupled decay, eps outside the square root) in
    fp32 torch ops; ``step`` is this step's number, counted from 1.

    With ``max_grad_norm`` the gradients are read through the factor
    ``min(1, max_grad_norm / (norm + 1e-6))`` of
    ``torch.nn.utils.clip_grad_norm_`` without being rewritten. Tensors
    flagged in ``no_decay`` get no weight decay. ``exp_avgs`` and
    ``exp_avg_sqs`` are fp32; with ``master_params`` (fp32) the update is
    applied to the master and the param is refreshed from it. Returns
    ``(norm, clip)`` as 0-dim fp32 tensors, or ``(None, None)`` without
    clipping."""
    live = [i for i, g in enumerate(grads) if g is not None]
    norm = clip = None
    if max_grad_norm is not None and live:
        sq = torch.stack([grads[i].float().square().sum() for i in live]).sum()
        norm = sq.sqrt()
        clip = (max_grad_norm / (norm + 1e-6)).clamp(max=1.0)
    step_size = lr / (1.0 - beta1 ** step)
    rsqrt_bc2 = 1.0 / math.sqrt(1.0 - beta2 ** step)
    for i in live:
        p = params[i]
        target = master_params[i] if master_params is not None else p
        m, v = exp_avgs[i], exp_avg_sqs[i]
        g = grads[i].float()
        if clip is not None:
            g = g * clip
        wd = 0.0 if (no_decay is not None and no_decay[i]) else weight_decay
        t32 = target.float().mul(1.0 - lr * wd)
        m.mul_(beta1).add_(g, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
        t32.addcdiv_(m, v.sqrt().mul_(rsqrt_bc2).add_(eps), value=-step_size)
        target.copy_(t32.to(target.dtype))
        if master_params is not None:
            p.copy_(target.to(p.dtype))
    return norm, clip
