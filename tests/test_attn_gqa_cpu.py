"""Grouped-query attention off the GPU: ops.attention(num_kv_heads=) against an fp64
repeat_interleave reference, its ValueErrors, and BertLayer_Head with num_key_value_heads."""

import math

import pytest
import torch

from skycomputing_amd import ops
from skycomputing_amd.models.bert_layers import BertLayerHead
from skycomputing_amd.ops import eager
from tests.test_attn_segments_cpu import ids_from_runs

B, S, H, D = 2, 12, 4, 8


def _ref64(qkv, h_kv, mask, ids, causal):
    q, k, v = (t.permute(0, 2, 1, 3) for t in qkv.split((H, h_kv, h_kv), dim=2))
    k, v = (t.repeat_interleave(H // h_kv, dim=1) for t in (k, v))
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    if mask is not None:
        s = s + mask.double()
    vis = eager.causal_mask(S) if causal else torch.ones(1, 1, S, S, dtype=torch.bool)
    if ids is not None:
        vis = vis & eager.segment_mask(ids)
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, S, H * D)


@pytest.mark.parametrize("mode", ["mask", "causal", "segments", "causal+segments"])
@pytest.mark.parametrize("h_kv", [1, 2, 4])
def test_attention_matches_fp64(h_kv, mode):
    torch.manual_seed(10 * h_kv)
    qkv = torch.randn(B, S, H + 2 * h_kv, D, requires_grad=True)
    dout = torch.randn(B, S, H * D)
    mask = ids = None
    if mode == "mask":
        mask = torch.zeros(B, 1, 1, S)
        mask[1, ..., 9:] = -10000.0
    if "segments" in mode:
        ids = ids_from_runs(S, [([0, 5], False), ([0, 4, 9], True)])
    out = ops.attention(qkv, mask, segment_ids=ids, causal="causal" in mode, num_kv_heads=h_kv)
    out.backward(dout)
    q64 = qkv.detach().double().requires_grad_(True)
    ref = _ref64(q64, h_kv, mask, ids, "causal" in mode)
    ref.backward(dout.double())
    for name, got, want in (("out", out, ref), ("dqkv", qkv.grad, q64.grad)):
        assert torch.allclose(got.double(), want.detach(), atol=1e-6, rtol=0), name


@pytest.mark.parametrize("heads", [None, 5, 7])  # 5-D multi-head tensor; h = 1 < 2; h = 3 on 2
def test_value_errors(heads):
    qkv = torch.randn(B, S, 3, H, D) if heads is None else torch.randn(B, S, heads, D)
    with pytest.raises(ValueError):
        ops.attention(qkv, None, num_kv_heads=2)


def test_layer_head_with_kv_heads():
    bc = dict(vocab_size=50, hidden_size=H * D, num_attention_heads=H, intermediate_size=64,
              hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(3)
    gqa, mha = BertLayerHead(dict(bc, num_key_value_heads=2)), BertLayerHead(bc)
    assert gqa.attention.qkv.weight.shape == ((H + 2 * 2) * D, H * D)
    assert gqa.layer_flops(B, S) < mha.layer_flops(B, S)
    mha.output.load_state_dict(gqa.output.state_dict())
    with torch.no_grad():
        for dst, src in ((mha.attention.qkv.weight, gqa.attention.qkv.weight),
                         (mha.attention.qkv.bias, gqa.attention.qkv.bias)):
            dst.copy_(eager.expand_kv(src.view(1, 1, H + 4, D, -1), 2).reshape(dst.shape))
    x, mask = torch.randn(B, S, H * D), torch.zeros(B, 1, 1, S)
    mask[0, ..., 10:] = -10000.0
    res = []
    for layer in (gqa, mha):
        xi = x.clone().requires_grad_(True)
        y, _ = layer(xi, mask)
        y.backward(torch.ones_like(y) * torch.arange(H * D))
        res.append((y.detach(), xi.grad))
    for got, want in zip(res[0], res[1]):  # the same fp32 mathematics: 16 ulp of the largest value
        assert (got - want).abs().max() <= 2.0 ** -20 * want.abs().max()
