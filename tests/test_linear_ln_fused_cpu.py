"""ops.linear_residual_layer_norm off the GPU: it is the composition of
ops.linear and ops.layer_norm, and the modules that call it keep their
parameter names."""

from __future__ import annotations

import torch

from skycomputing_amd import ops
from skycomputing_amd.models.bert import BertConfig
from skycomputing_amd.models.bert_layers import BertLayerTail, BertSelfOutput


def _args(rows=6, K=24, N=40):
    torch.manual_seed(0)
    return (torch.randn(rows, K), torch.randn(N, K) * 0.1, torch.randn(N),
            torch.rand(N) + 0.5, torch.randn(N), 1e-12, torch.randn(rows, N))


def test_cpu_equals_composition_eval():
    x, w, b, lw, lb, eps, res = _args()
    got = ops.linear_residual_layer_norm(x, w, b, lw, lb, eps, res, 0.3, False)
    want = ops.layer_norm(ops.linear(x, w, b), lw, lb, eps, res, 0.3, False)
    assert torch.equal(got, want)
    got = ops.linear_residual_layer_norm(x, w, None, lw, lb, eps, None)
    want = ops.layer_norm(ops.linear(x, w), lw, lb, eps)
    assert torch.equal(got, want)


def test_cpu_equals_composition_training():
    x, w, b, lw, lb, eps, res = _args()
    torch.manual_seed(5)
    got = ops.linear_residual_layer_norm(x, w, b, lw, lb, eps, res, 0.3, True)
    torch.manual_seed(5)
    want = ops.layer_norm(ops.linear(x, w, b), lw, lb, eps, res, 0.3, True)
    assert torch.equal(got, want)


def test_cpu_gradients_equal_composition():
    base = _args()

    def run(fn):
        leaves = [t.clone().requires_grad_(True) if torch.is_tensor(t) else t for t in base]
        fn(*leaves).sum().backward()
        return [t.grad for t in leaves if torch.is_tensor(t)]

    got = run(lambda x, w, b, lw, lb, eps, res:
              ops.linear_residual_layer_norm(x, w, b, lw, lb, eps, res))
    want = run(lambda x, w, b, lw, lb, eps, res:
               ops.layer_norm(ops.linear(x, w, b), lw, lb, eps, res))
    for g, r in zip(got, want):
        assert torch.equal(g, r)


def test_state_dict_keys_unchanged():
    cfg = BertConfig.from_dict(dict(hidden_size=64, num_attention_heads=4,
                                    intermediate_size=128, vocab_size=100))
    want = ["dense.weight", "dense.bias", "layer_norm.weight", "layer_norm.bias"]
    assert list(BertSelfOutput(cfg).state_dict().keys()) == want
    tail = BertLayerTail(cfg)
    assert list(tail.state_dict().keys()) == want
    assert tuple(tail.dense.weight.shape) == (64, 128)


def test_modules_forward_on_cpu():
    cfg = BertConfig.from_dict(dict(hidden_size=64, num_attention_heads=4,
                                    intermediate_size=128, vocab_size=100))
    torch.manual_seed(1)
    so = BertSelfOutput(cfg).eval()
    h, r = torch.randn(2, 5, 64), torch.randn(2, 5, 64)
    want = so.layer_norm(so.dense(h), residual=r)
    assert torch.equal(so(h, r), want)
    tail = BertLayerTail(cfg).eval()
    inter = torch.randn(2, 5, 128)
    want = tail.layer_norm(tail.dense(inter), residual=r)
    out, mask = tail(r, inter, None)
    assert torch.equal(out, want) and mask is None
