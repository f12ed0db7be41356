"""SequentialWrapper's pairing protocol and BertLayerBody's use of it: a
Body followed by its Tail in the same wrapper runs as one ops.ffn_block call
(on CPU: the composition), with the module tree, parameter order and
state-dict keys as they were; a pipeline cut between the two, a hook on
either, or SKY_NO_FFN_BLOCK=1 keep them separate."""

from __future__ import annotations

import pytest
import torch

from skycomputing_amd import ops
from skycomputing_amd.builder import SequentialWrapper
from skycomputing_amd.models.bert_layers import (
    BertLayerBody, BertLayerHead, BertLayerTail,
)

CFG = dict(hidden_size=32, num_attention_heads=4, intermediate_size=64,
           hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
B, S = 2, 6


@pytest.fixture()
def block():
    torch.manual_seed(0)
    mods = [BertLayerHead(CFG), BertLayerBody(CFG), BertLayerTail(CFG)]
    for m in mods:  # the default LN weight/bias (1, 0) would hide a swap
        for p in m.parameters():
            if p.dim() == 1:
                torch.nn.init.normal_(p, std=0.5)
    x = torch.randn(B, S, CFG["hidden_size"])
    mask = torch.zeros(B, 1, 1, S)
    mask[:, :, :, -2:] = -10000.0
    dy = torch.randn(B, S, CFG["hidden_size"])
    return mods, x, mask, dy


@pytest.fixture()
def ffn_calls(monkeypatch):
    """Counts the calls of ops.ffn_block, which still runs."""
    calls = []
    real = ops.ffn_block

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "ffn_block", counted)
    return calls


def _params(mods):
    return [p for m in mods for p in m.parameters()]


def _run(fn, mods, x, dy):
    """Output and gradients (input first, then every parameter)."""
    xin = x.clone().requires_grad_(True)
    for p in _params(mods):
        p.grad = None
    out, m = fn(xin)
    out.backward(dy)
    return out.detach(), m, [xin.grad] + [p.grad.clone() for p in _params(mods)]


def _sequence(mods, mask):
    def fn(x):
        out = (x, mask)
        for m in mods:
            out = m(*out)
        return out
    return fn


def _same(got, want):
    y, m, g = got
    yr, mr, gr = want
    assert torch.equal(m, mr)  # a backward hook re-wraps it: not `is`
    assert torch.equal(y, yr)
    assert len(g) == len(gr)
    for a, b in zip(g, gr):
        assert torch.equal(a, b)


def test_wrapper_pairs_body_and_tail(block, ffn_calls):
    mods, x, mask, dy = block
    want = _run(_sequence(mods, mask), mods, x, dy)
    assert not ffn_calls  # the modules one by one never pair
    wrapper = SequentialWrapper(*mods)
    got = _run(lambda t: wrapper(t, mask), mods, x, dy)
    assert len(ffn_calls) == 1
    _same(got, want)


def test_eval_mode_pairs_too(block, ffn_calls):
    mods, x, mask, dy = block
    wrapper = SequentialWrapper(*mods).eval()
    want = _run(_sequence(mods, mask), mods, x, dy)
    got = _run(lambda t: wrapper(t, mask), mods, x, dy)
    assert len(ffn_calls) == 1
    _same(got, want)


def test_cut_between_body_and_tail_does_not_pair(block, ffn_calls):
    mods, x, mask, dy = block
    want = _run(_sequence(mods, mask), mods, x, dy)
    first, second = SequentialWrapper(*mods[:2]), SequentialWrapper(mods[2])
    got = _run(lambda t: second(*first(t, mask)), mods, x, dy)
    assert not ffn_calls
    _same(got, want)


@pytest.mark.parametrize("which", [1, 2], ids=["body", "tail"])
@pytest.mark.parametrize("kind", ["forward", "forward_pre", "full_backward"])
def test_hook_fires_and_keeps_them_separate(block, ffn_calls, which, kind):
    mods, x, mask, dy = block
    want = _run(_sequence(mods, mask), mods, x, dy)
    fired = []
    register = getattr(mods[which], f"register_{kind}_hook")
    handle = register(lambda *a: fired.append(1) and None)
    wrapper = SequentialWrapper(*mods)
    got = _run(lambda t: wrapper(t, mask), mods, x, dy)
    assert fired == [1]
    assert not ffn_calls
    _same(got, want)
    handle.remove()
    _run(lambda t: wrapper(t, mask), mods, x, dy)
    assert len(ffn_calls) == 1  # pairs again once the hook is gone


def test_env_switch_keeps_them_separate(block, ffn_calls, monkeypatch):
    mods, x, mask, dy = block
    want = _run(_sequence(mods, mask), mods, x, dy)
    monkeypatch.setenv("SKY_NO_FFN_BLOCK", "1")
    wrapper = SequentialWrapper(*mods)
    got = _run(lambda t: wrapper(t, mask), mods, x, dy)
    assert not ffn_calls
    _same(got, want)


def test_body_not_followed_by_tail_runs_alone(block, ffn_calls):
    mods, x, mask, dy = block
    wrapper = SequentialWrapper(mods[0], mods[1])
    a, inter, m = wrapper(x, mask)
    assert inter.shape == (B, S, CFG["intermediate_size"]) and m is mask
    assert not ffn_calls


def test_wrapper_protocol_is_generic():
    """Any module can make the offer; the wrapper only checks adjacency."""
    class Twice(torch.nn.Module):
        def forward(self, x):
            return x * 2

    class Offers(torch.nn.Module):
        def forward(self, x):
            return x + 1

        def fuse_with_next(self, nxt):
            if isinstance(nxt, Twice):
                return lambda x: (x + 1) * 2 + 1000  # tell-tale
            return None

    x = torch.ones(3)
    assert torch.equal(SequentialWrapper(Offers(), Twice())(x), x * 1004)
    assert torch.equal(SequentialWrapper(Offers(), Offers(), Twice())(x), x * 1006)
    assert torch.equal(SequentialWrapper(Twice(), Offers())(x), x * 3)


def test_names_and_state_dict_keys_unchanged(block):
    mods, *_ = block
    wrapper = SequentialWrapper(*mods)
    want = [
        "0.attention.qkv.weight", "0.attention.qkv.bias",
        "0.output.dense.weight", "0.output.dense.bias",
        "0.output.layer_norm.weight", "0.output.layer_norm.bias",
        "1.intermediate.weight", "1.intermediate.bias",
        "2.dense.weight", "2.dense.bias",
        "2.layer_norm.weight", "2.layer_norm.bias",
    ]
    assert [n for n, _ in wrapper.named_parameters()] == want
    assert list(wrapper.state_dict().keys()) == want
