"""ops.attention_block on CPU is the composition of the eager ops, and
routing BertLayerHead through it leaves the module tree (and so state
dicts and checkpoints) as it was."""

from __future__ import annotations

import torch

from skycomputing_amd import ops
from skycomputing_amd.models.bert_layers import BertLayerHead
from skycomputing_amd.ops import eager


def test_cpu_wrapper_matches_eager():
    torch.manual_seed(0)
    B, S, h, d = 2, 10, 2, 8
    H = h * d
    hidden = torch.randn(B, S, H, requires_grad=True)
    wqkv = (torch.randn(3 * H, H) * 0.1).requires_grad_(True)
    bqkv = torch.randn(3 * H).requires_grad_(True)
    wo = (torch.randn(H, H) * 0.1).requires_grad_(True)
    bo = torch.randn(H).requires_grad_(True)
    ln_w = (torch.rand(H) + 0.5).requires_grad_(True)
    ln_b = torch.randn(H).requires_grad_(True)
    mask = torch.zeros(B, 1, 1, S)
    mask[:, :, :, -3:] = -10000.0
    leaves = [hidden, wqkv, bqkv, wo, bo, ln_w, ln_b]

    y = ops.attention_block(hidden, mask, wqkv, bqkv, h, 0.1, wo, bo, ln_w, ln_b,
                            1e-12, 0.1, False)
    dy = torch.randn_like(y)
    got = torch.autograd.grad(y, leaves, dy)

    qkv = torch.nn.functional.linear(hidden, wqkv, bqkv).view(B, S, 3, h, d)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ctx = eager.attention_context(q, k, v, mask).permute(0, 2, 1, 3).reshape(B, S, H)
    yr = eager.layer_norm(torch.nn.functional.linear(ctx, wo, bo), ln_w, ln_b, 1e-12, hidden)
    want = torch.autograd.grad(yr, leaves, dy)

    assert torch.allclose(y, yr, atol=1e-6, rtol=1e-6)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)


def test_head_state_dict_keys_unchanged():
    cfg = dict(hidden_size=32, num_attention_heads=4, intermediate_size=64)
    head = BertLayerHead(cfg)
    assert list(head.state_dict().keys()) == [
        "attention.qkv.weight", "attention.qkv.bias",
        "output.dense.weight", "output.dense.bias",
        "output.layer_norm.weight", "output.layer_norm.bias",
    ]
    # and the module still runs end to end on CPU
    x = torch.randn(2, 6, 32)
    out, m = head(x, None)
    assert out.shape == x.shape and m is None
