"""Public functional op API with device dispatch.

CPU tensors (tests, gloo plumbing) run the eager fp32-reference path; CUDA
tensors run the hand-written gfx950 HIP kernels. On a GPU box with the
extension missing the core ops FAIL LOUDLY (hiplib.require) instead of
silently falling back to eager — set SKY_ALLOW_EAGER_GPU=1 to override for
debugging only.

Op inventory maps 1:1 onto the reference's BERT hot path
(SURVEY.md §2c table); plain unfused GEMMs go through torch (hipBLASLt on
ROCm), fused GEMM+epilogue paths are progressively replaced by MFMA kernels.
"""

from __future__ import annotations

import math
import os

import torch

from . import eager, hiplib
from .eager import ACT_FNS, gelu, swish  # re-export

__all__ = [
    "layer_norm", "bias_gelu", "bias_tanh", "masked_softmax", "dropout",
    "attention_context", "attention_block", "ffn_block", "linear_act",
    "linear_residual_layer_norm",
    "embedding_fused", "softmax_cross_entropy", "sgd_step", "adamw_step",
    "gelu", "swish", "ACT_FNS", "hip_available",
]


def hip_available() -> bool:
    return hiplib.available()


def _use_hip(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    if hiplib.available():
        return True
    if os.environ.get("SKY_ALLOW_EAGER_GPU") == "1":
        return False
    hiplib.require()  # raises with a build hint
    return False


def layer_norm(x, weight, bias, eps: float = 1e-12, residual=None,
               dropout_p: float = 0.0, training: bool = False):
    """LayerNorm with optional fused residual add and fused PRE-add dropout
    on x: LN(dropout(x) + residual)."""
    p = dropout_p if training else 0.0
    if _use_hip(x):
        from .functions import LayerNormFn

        if p > 0.0 and x.shape[-1] % 8 != 0:
            x = dropout(x, p, True)
            p = 0.0
        return LayerNormFn.apply(x, weight, bias, eps, residual, p)
    if p > 0.0:
        x = torch.nn.functional.dropout(x, p=p, training=True)
    return eager.layer_norm(x, weight, bias, eps, residual)


def bias_gelu(x, bias):
    if _use_hip(x):
        from .functions import BiasGeluFn

        return BiasGeluFn.apply(x, bias)
    return eager.bias_gelu(x, bias)


def bias_tanh(x, bias):
    # tiny (pooler-sized) op: torch native on both devices
    return eager.bias_tanh(x, bias)


def masked_softmax(scores, mask, scale: float = 1.0):
    """softmax(scores*scale + mask) over the last dim of [B,h,Sq,Sk]."""
    if _use_hip(scores):
        from .functions import MaskedSoftmaxFn

        return MaskedSoftmaxFn.apply(scores, mask, scale)
    return eager.masked_softmax(scores * scale if scale != 1.0 else scores, mask)


def dropout(x, p: float, training: bool = True):
    if p <= 0.0 or not training:
        return x
    if _use_hip(x):
        from .functions import DropoutFn

        return DropoutFn.apply(x, p)
    return torch.nn.functional.dropout(x, p=p, training=True)


def attention_context(q, k, v, mask, dropout_p: float = 0.0, training: bool = False):
    """softmax(QK^T/sqrt(d) + mask) V for q/k/v [B,h,S,d].

    GPU path: batched GEMMs via torch (hipBLASLt) + fused HIP masked-softmax
    + seed-regenerated dropout. (A flash-style fused kernel replaces this
    path for long sequences; at the reference workload S=128 the score
    matrix is L2-resident and the batched-GEMM path is the right shape.)
    """
    d = q.shape[-1]
    scale = 1.0 / math.sqrt(d)
    if _use_hip(q):
        scores = torch.matmul(q, k.transpose(-1, -2))
        probs = masked_softmax(scores, mask, scale)
        probs = dropout(probs, dropout_p, training)
        return torch.matmul(probs, v)
    return eager.attention_context(q, k, v, mask, dropout_p, training)


def attention(qkv, mask, dropout_p: float = 0.0, training: bool = False):
    """Multi-head attention over a packed qkv tensor [B, S, 3, h, d];
    returns [B, S, h*d].

    GPU fast path (bf16, d=64, S<=128): ONE fused MFMA kernel
    (FusedAttentionFn). Otherwise: strided-view batched GEMMs + fused
    masked softmax (HIP on GPU, eager on CPU)."""
    from .functions import _split_heads

    B, S, three, h, d = qkv.shape
    scale = 1.0 / math.sqrt(d)
    if (
        qkv.is_cuda and qkv.dtype == torch.bfloat16 and d == 64
        and hiplib.available() and os.environ.get("SKY_NO_FUSED_ATTN") != "1"
    ):
        from .functions import FlashAttentionFn, FusedAttentionFn

        if S <= 128:
            out = FusedAttentionFn.apply(qkv, mask, scale, dropout_p, training)
            return out.reshape(B, S, h * d)
        if S <= 4096 and os.environ.get("SKY_FLASH_ATTN") == "1":
            # our experimental flash-style forward (online softmax, no
            # S x S tensor in forward; backward decomposes). Kept
            # env-selectable; the sdpa path below beats it at every
            # measured S (tools/flash_bench.py), so it is not the default.
            out = FlashAttentionFn.apply(qkv, mask, scale, dropout_p, training)
            return out.reshape(B, S, h * d)
        # long-sequence default: torch-ROCm's flash scaled_dot_product
        # _attention (fwd AND bwd tiled — no S x S tensor in either
        # direction, unlike the decomposed path whose backward
        # materializes scores). Same standing as hipBLASLt for plain
        # GEMMs: library kernels where they win, hand kernels where ours
        # do (S<=128 is the fused MFMA kernel above). Measured at S=512:
        # sdpa ~26 us core vs 108 us decomposed / 176 us flash-v1.
        if os.environ.get("SKY_NO_SDPA") != "1":
            q, k, v = _split_heads(qkv)
            am = mask
            if am is not None:
                am = am.to(qkv.dtype)  # additive [B,1,1,S], broadcast
            ctx = torch.nn.functional.scaled_dot_product_attention(
                q, k, v, attn_mask=am,
                dropout_p=dropout_p if training else 0.0,
            )
            return ctx.permute(0, 2, 1, 3).reshape(B, S, h * d)
    q, k, v = _split_heads(qkv)
    ctx = attention_context(q, k, v, mask, dropout_p, training)
    return ctx.permute(0, 2, 1, 3).reshape(B, S, h * d)


def linear(x, weight, bias=None):
    """Linear with HIP-colsum dbias backward on GPU (GEMMs via hipBLASLt)."""
    if _use_hip(x):
        from .functions import LinearBiasFn

        return LinearBiasFn.apply(x, weight, bias)
    return torch.nn.functional.linear(x, weight, bias)


def linear_residual_layer_norm(x, weight, bias, ln_weight, ln_bias,
                               eps: float = 1e-12, residual=None,
                               dropout_p: float = 0.0, training: bool = False):
    """LN(dropout(linear(x)) + residual).

    GPU (bias present, fp32/bf16, LayerNorm width supported by the
    three-sum backward): one autograd node whose backward takes the
    linear's dbias from the LayerNorm backward pass and runs the weight
    gradient as a plain GEMM (LinearResidualLayerNormFn). Everything else
    — CPU, no bias, other widths, SKY_NO_LN_DBIAS=1 — is the composition
    of ops.linear and ops.layer_norm."""
    if (
        bias is not None
        and x.dtype in (torch.float32, torch.bfloat16)
        and _use_hip(x)
    ):
        from .functions import (
            LinearResidualLayerNormFn, ln_dbias_enabled, ln_xsum_width_ok,
        )

        if ln_dbias_enabled() and ln_xsum_width_ok(weight.shape[0]):
            p = dropout_p if training else 0.0
            return LinearResidualLayerNormFn.apply(
                x, weight, bias, ln_weight, ln_bias, eps, residual, p
            )
    return layer_norm(linear(x, weight, bias), ln_weight, ln_bias, eps,
                      residual, dropout_p, training)


def attention_block(hidden, mask, qkv_weight, qkv_bias, num_heads: int,
                    attn_dropout_p: float, out_weight, out_bias, ln_weight,
                    ln_bias, eps: float = 1e-12, hidden_dropout_p: float = 0.0,
                    training: bool = False):
    """The attention third of an encoder block:
    LN(dropout(attention(hidden @ Wqkv^T + bqkv) @ Wo^T + bo) + hidden)
    for hidden [B, S, H], mask [B, 1, 1, S] additive or None.

    GPU, bf16, head dim 64, S <= 128, both biases present and the
    LayerNorm width supported by the three-sum backward: one autograd node
    (AttentionBlockFn) whose backward takes the qkv dbias from the
    attention backward kernels and sums hidden's two gradients inside the
    qkv dgrad GEMM. Everything else — CPU, fp32, long sequences,
    SKY_NO_ATTN_BLOCK=1, SKY_NO_LN_DBIAS=1 and the env-selected attention
    paths — is the composition of ops.linear, ops.attention and
    ops.linear_residual_layer_norm."""
    B, S, H = hidden.shape
    d = H // num_heads
    if (
        hidden.is_cuda and hidden.dtype == torch.bfloat16 and d == 64
        and S <= 128 and qkv_bias is not None and out_bias is not None
        and hiplib.available()
        and os.environ.get("SKY_NO_FUSED_ATTN") != "1"
        and os.environ.get("SKY_NO_FUSED_ATTN_BWD") != "1"
        and os.environ.get("SKY_ATTN_FUSED_BWD") != "1"
    ):
        from .functions import (
            AttentionBlockFn, attn_block_enabled, ln_dbias_enabled,
            ln_xsum_width_ok,
        )

        if attn_block_enabled() and ln_dbias_enabled() and ln_xsum_width_ok(H):
            ap = attn_dropout_p if (training and attn_dropout_p > 0) else 0.0
            hp = hidden_dropout_p if training else 0.0
            return AttentionBlockFn.apply(
                hidden, qkv_weight, qkv_bias, mask, num_heads, ap,
                out_weight, out_bias, ln_weight, ln_bias, eps, hp
            )
    qkv = linear(hidden, qkv_weight, qkv_bias).view(B, S, 3, num_heads, d)
    attn = attention(qkv, mask, attn_dropout_p, training)
    return linear_residual_layer_norm(
        attn, out_weight, out_bias, ln_weight, ln_bias, eps, hidden,
        hidden_dropout_p, training)


def _linear_gelu_node_ok(x, weight) -> bool:
    """Whether ops.linear_act runs gelu(linear(x)) as LinearGeluFn (one GEMM
    with the bias + gelu + pre-activation epilogue) for a GPU x with bias."""
    from .functions import _g2_enabled, _g2_fit, _use_hblt

    # GELU_AUX_BIAS epilogue: this hipBLASLt build only supports it for
    # fp32 D (bf16 returns HIPBLAS_STATUS_NOT_SUPPORTED — probed on HW,
    # tools/hblt_probe.py), so the fused linear+gelu is fp32-only and
    # opt-in; the bf16 hot path keeps GEMM + the HIP bias+gelu kernel.
    if (_use_hblt() and os.environ.get("SKY_HBLT_GELU") == "1"
            and x.dtype == torch.float32 and weight.shape[0] % 8 == 0):
        return True
    # v2 hand-GEMM path: one 256^2 8-phase kernel with the bias+gelu
    # epilogue fused (and the pre-activation stored for backward)
    if x.dtype == torch.bfloat16:
        rows = x.numel() // x.shape[-1]
        return (_g2_enabled("fwd", rows, weight.shape[0], weight.shape[1])
                and _g2_fit(rows, weight.shape[0], weight.shape[1]))
    return False


def linear_act(x, weight, bias, act: str = "gelu"):
    """Linear + bias + activation (the reference's LinearActivation).

    GPU: ONE hipBLASLt GEMM with the GELU_AUX_BIAS epilogue (bias + gelu +
    pre-activation save fused into the GEMM); SKY_NO_HBLT=1 falls back to
    GEMM + the standalone HIP bias+gelu kernel."""
    if _use_hip(x) and act == "gelu" and bias is not None:
        if _linear_gelu_node_ok(x, weight):
            from .functions import LinearGeluFn

            return LinearGeluFn.apply(x, weight, bias)
        y = torch.nn.functional.linear(x, weight)
        return bias_gelu(y, bias)
    return eager.linear_act(x, weight, bias, act)


def ffn_block(x, up_weight, up_bias, down_weight, down_bias, ln_weight,
              ln_bias, eps: float = 1e-12, hidden_dropout_p: float = 0.0,
              training: bool = False, act: str = "gelu"):
    """The FFN two-thirds of an encoder block:
    LN(dropout(act(x @ Wup^T + bup) @ Wdown^T + bdown) + x)
    for x [..., H].

    Where ops.linear_act would run its one-GEMM gelu node AND
    ops.linear_residual_layer_norm its node — GPU, gelu, both biases
    present, a shape the fused ffn-up forward takes, the LayerNorm width
    supported by the three-sum backward: one autograd node (FfnBlockFn)
    whose backward sums x's two gradients inside the ffn-up dgrad GEMM and
    finishes its four column sums in one launch. Everything else — CPU,
    other activations, dtypes and shapes, SKY_NO_FFN_BLOCK=1,
    SKY_NO_LN_DBIAS=1 — is the composition of ops.linear_act and
    ops.linear_residual_layer_norm."""
    if (
        act == "gelu" and up_bias is not None and down_bias is not None
        and x.dtype in (torch.float32, torch.bfloat16) and _use_hip(x)
    ):
        from .functions import (
            FfnBlockFn, ffn_block_enabled, ln_dbias_enabled, ln_xsum_width_ok,
        )

        if (ffn_block_enabled() and ln_dbias_enabled()
                and ln_xsum_width_ok(down_weight.shape[0])
                and _linear_gelu_node_ok(x, up_weight)):
            p = hidden_dropout_p if training else 0.0
            return FfnBlockFn.apply(x, up_weight, up_bias, down_weight,
                                    down_bias, ln_weight, ln_bias, eps, p)
    inter = linear_act(x, up_weight, up_bias, act)
    return linear_residual_layer_norm(
        inter, down_weight, down_bias, ln_weight, ln_bias, eps, x,
        hidden_dropout_p, training)


def embedding_fused(
    input_ids, token_type_ids, position_ids,
    word_emb, pos_emb, type_emb, ln_weight, ln_bias, eps: float = 1e-12,
):
    if _use_hip(word_emb):
        from .functions import EmbeddingFusedFn

        return EmbeddingFusedFn.apply(
            input_ids, token_type_ids, position_ids,
            word_emb, pos_emb, type_emb, ln_weight, ln_bias, eps,
        )
    return eager.embedding_fused(
        input_ids, token_type_ids, position_ids,
        word_emb, pos_emb, type_emb, ln_weight, ln_bias, eps,
    )


def softmax_cross_entropy(logits, labels, ignore_index: int = -100,
                          num_classes: int | None = None,
                          inplace_backward: bool = False):
    """Mean softmax cross-entropy over the valid rows: a 0-dim fp32 loss.

    logits [..., ld] and labels [...] are flattened to rows. Columns
    num_classes..ld-1 are padding (None: ld classes): never part of the
    softmax, gradient 0. A row is valid iff 0 <= label < num_classes and
    label != ignore_index; EVERY other label ignores its row, an
    out-of-range one included (nothing validates labels on the host, which
    would synchronise). With no valid row the loss is 0 and the gradient
    zero, where torch returns NaN.

    GPU, fp32/bf16: SoftmaxCrossEntropyFn, two row kernels and a one-block
    finish (ops/hip/xent.hip). The logits are read once forward and once
    backward, ignored rows not at all; by byte count that is 0.75 GB where
    cross_entropy(logits.float(), labels) moves at least 3.5 GB at
    [4096, 30522] bf16; measured there on an MI355X, forward + backward
    take 245 us against 1160 us, with 250 MB instead of 1500 MB above the
    logits (profiles/r10_notes.md). The valid count stays on the device: no
    synchronisation, and a captured step follows new labels under replay.

    inplace_backward=True writes the gradient over the logits' own storage
    instead of allocating a second [N, ld] buffer. That is safe only when
    nothing else reads the logits after this loss — true for the output of a
    linear layer, whose backward needs its input and weight but not its
    output; false if the logits are also returned, logged, or fed to another
    op that saves them. Off by default.

    CPU, other dtypes and SKY_ALLOW_EAGER_GPU=1 run ops/eager.py with the
    same semantics."""
    if logits.dtype in (torch.float32, torch.bfloat16) and _use_hip(logits):
        from .functions import SoftmaxCrossEntropyFn

        V = logits.shape[-1] if num_classes is None else int(num_classes)
        return SoftmaxCrossEntropyFn.apply(
            logits, labels, V, int(ignore_index), bool(inplace_backward))
    if logits.is_cuda:
        _use_hip(logits)  # a missing extension still fails loudly
    return eager.softmax_cross_entropy(logits, labels, ignore_index, num_classes)


def sgd_step(params, grads, lr, momentum=0.0, weight_decay=0.0,
             momentum_bufs=None, master_params=None):
    """Multi-tensor SGD step; fused HIP path lives in optim.FusedSGD."""
    eager.sgd_step(params, grads, lr, momentum, weight_decay, momentum_bufs, master_params)


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1=0.9,
               beta2=0.999, eps=1e-8, weight_decay=0.01, master_params=None,
               max_grad_norm=None, no_decay=None):
    """Multi-tensor AdamW step with the clip folded in; fused HIP path
    lives in optim.FusedAdamW."""
    return eager.adamw_step(params, grads, exp_avgs, exp_avg_sqs, step, lr,
                            beta1, beta2, eps, weight_decay, master_params,
                            max_grad_norm, no_decay)
