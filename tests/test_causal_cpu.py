"""Causal attention off the GPU: the eager path of ops.attention(causal=True), the prefix
property of a causal_lm_pipeline_config model and the "CausalLM" loss."""

import pytest
import torch

from skycomputing_amd import ops
from skycomputing_amd.builder import build_module_from_cfg
from skycomputing_amd.models import bert_pretraining_pipeline_config, causal_lm_pipeline_config
from skycomputing_amd.ops import eager
from skycomputing_amd.optim import build_loss
from tests.test_attn_segments_cpu import ids_from_runs


@pytest.mark.parametrize("rows", [None, [([0, 7], False), ([0, 12, 15], True)]])
def test_attention_equals_dense_mask(rows):
    torch.manual_seed(0)
    qkv = torch.randn(2, 20, 3, 2, 8)
    ids = ids_from_runs(20, rows) if rows else None
    vis = eager.causal_mask(20)
    if rows:
        vis = vis & eager.segment_mask(ids)
    dense = torch.zeros(vis.shape).masked_fill_(~vis, float("-inf"))
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    want = eager.attention_context(q, k, v, dense).permute(0, 2, 1, 3).reshape(2, 20, 16)
    assert torch.equal(ops.attention(qkv, None, segment_ids=ids, causal=True), want)
    assert torch.equal(ops.attention(qkv, None, segment_ids=ids, causal=False),
                       ops.attention(qkv, None, segment_ids=ids))
    assert not torch.equal(ops.attention(qkv, None, segment_ids=ids), want)


def test_prefix_property():
    """Tokens after position t change no logit at positions <= t; without causal they do."""
    bc = dict(vocab_size=50, hidden_size=32, num_attention_heads=4, intermediate_size=64,
              max_position_embeddings=16)
    torch.manual_seed(1)
    tok = torch.randint(0, 50, (2, 12))
    other = tok.clone()
    other[:, 7:] = (tok[:, 7:] + 1) % 50
    for cfg, causal in ((causal_lm_pipeline_config(2, bc), True),
                        (bert_pretraining_pipeline_config(2, bc), False)):
        model = build_module_from_cfg(cfg, device="cpu", dtype=torch.float32).eval()
        a, b = model(tok), model(other)
        assert torch.equal(a[:, :7], b[:, :7]) == causal
        assert not torch.equal(a[:, 7:], b[:, 7:])


def test_causal_lm_loss():
    torch.manual_seed(2)
    logits = torch.randn(3, 6, 16, requires_grad=True)
    labels = torch.randint(0, 11, (3, 6))
    labels[0, 3] = -100
    labels[1, 1:] = -100  # a row whose only targets are ignored
    loss = build_loss(dict(type="CausalLM", num_classes=11, ignore_index=-100))(logits, labels)
    want = torch.nn.functional.cross_entropy(
        logits[:, :-1, :11].reshape(-1, 11), labels[:, 1:].reshape(-1), ignore_index=-100)
    assert torch.allclose(loss, want, atol=1e-6, rtol=0)
    loss.backward()
    assert logits.grad[1].abs().max() == 0 and logits.grad[:, -1].abs().max() == 0
