"""The attention third of an encoder block as one autograd node
(AttentionBlockFn behind ops.attention_block): qkv dbias from the attention
backward kernels, the residual-gradient add folded into the qkv dgrad GEMM.
Checked against the three-node composition it replaces
(SKY_NO_ATTN_BLOCK=1), against an fp32 eager reference, and under graph
capture.
"""

from __future__ import annotations

import os

import pytest
import torch

from tests.test_attn_bwd_dbias_gpu import SHAPES, make_mask
from tests.test_ops_gpu import _tols

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd import ops
    from skycomputing_amd.ops import eager, hiplib
    from skycomputing_amd.ops import functions as F

NAMES = ["d_hidden", "dWqkv", "dbqkv", "dWo", "dbo", "ln_dw", "ln_db"]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _inputs(B, S, h, masked, seed):
    H = 64 * h
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=g) * scale).to(torch.bfloat16)

    hidden = rn(B, S, H)
    wqkv = rn(3 * H, H, scale=0.03)
    bqkv = rn(3 * H, scale=0.1)
    wo = rn(H, H, scale=0.03)
    bo = rn(H, scale=0.1)
    ln_w = (torch.rand(H, device="cuda", generator=g) + 0.5).to(torch.bfloat16)
    ln_b = rn(H)
    dy = rn(B, S, H)
    mask = make_mask(B, S, g) if masked else None
    return [hidden, wqkv, bqkv, wo, bo, ln_w, ln_b], mask, dy


def _run(base, mask, dy, h, p, training=True):
    """ops.attention_block forward + backward on fresh leaves; returns y,
    the gradients in NAMES order and the output's grad_fn name."""
    F.set_dropout_seed(4321)
    hidden, wqkv, bqkv, wo, bo, ln_w, ln_b = [
        t.clone().requires_grad_(True) for t in base]
    y = ops.attention_block(hidden, mask, wqkv, bqkv, h, p, wo, bo, ln_w, ln_b,
                            1e-12, p, training)
    node = type(y.grad_fn).__name__
    y.backward(dy)
    grads = [t.grad for t in (hidden, wqkv, bqkv, wo, bo, ln_w, ln_b)]
    return y.detach(), grads, node


def _composition(base, mask, dy, h, p):
    assert os.environ.get("SKY_NO_ATTN_BLOCK") is None
    os.environ["SKY_NO_ATTN_BLOCK"] = "1"
    try:
        return _run(base, mask, dy, h, p)
    finally:
        del os.environ["SKY_NO_ATTN_BLOCK"]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,S,h", SHAPES)
def test_node_vs_composition(B, S, h, masked):
    """Same seeds, p = 0.1: y bit-identical (same forward kernels, same
    salts in the same order); every gradient inside atol = rtol = 2e-2."""
    p = 0.1
    base, mask, dy = _inputs(B, S, h, masked, seed=50 + S)
    y_n, g_n, node_n = _run(base, mask, dy, h, p)
    y_c, g_c, node_c = _composition(base, mask, dy, h, p)
    assert node_n == "AttentionBlockFnBackward"
    assert node_c == "LinearResidualLayerNormFnBackward"
    assert torch.equal(y_n, y_c)
    bad = []
    for name, a, c in zip(NAMES, g_n, g_c):
        assert a.dtype == c.dtype and a.shape == c.shape
        a, c = a.float(), c.float()
        err = (a - c).abs().max().item()
        nbad = ((a - c).abs() > 2e-2 + 2e-2 * c.abs()).sum().item()
        print(f"{name}: max abs diff {err:.3e}, {nbad} of {a.numel()} outside the bound")
        if not torch.allclose(a, c, atol=2e-2, rtol=2e-2):
            bad.append((name, err, nbad))
    assert not bad, bad


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,S,h", SHAPES)
def test_node_vs_fp32_reference(B, S, h, masked):
    """No dropout. y and d hidden at _tols(bf16); the row-accumulated
    gradients at atol*100, rtol = 0.05."""
    base, mask, dy = _inputs(B, S, h, masked, seed=60 + S)
    y, grads, node = _run(base, mask, dy, h, 0.0)
    assert node == "AttentionBlockFnBackward"

    ref = [t.float().clone().requires_grad_(True) for t in base]
    hf, wq, bq, wof, bof, lw, lb = ref
    H = 64 * h
    qkv = torch.nn.functional.linear(hf, wq, bq).view(B, S, 3, h, 64)
    q, k, v = F._split_heads(qkv)
    ctx = eager.attention_context(q, k, v, mask.float() if mask is not None else None)
    ctx = ctx.permute(0, 2, 1, 3).reshape(B, S, H)
    yr = eager.layer_norm(torch.nn.functional.linear(ctx, wof, bof), lw, lb, 1e-12, hf)
    yr.backward(dy.float())

    t = _tols(torch.bfloat16)
    bad = []
    for name, got, want, tol in (
        [("y", y, yr.detach(), t), ("d_hidden", grads[0], hf.grad, t)]
        + [(n, g, r.grad, dict(atol=t["atol"] * 100, rtol=0.05))
           for n, g, r in zip(NAMES[1:], grads[1:], ref[1:])]
    ):
        err = (got.float() - want).abs().max().item()
        print(f"{name}: max abs err {err:.3e}")
        assert got.dtype == torch.bfloat16
        if not torch.allclose(got.float(), want, **tol):
            bad.append((name, err))
    assert not bad, bad


def test_eval_mode_and_env_paths_compose():
    """Not training: the node runs without dropout and matches the
    composition exactly in y. Each env-selected attention path and
    SKY_NO_LN_DBIAS keep the composition."""
    B, S, h = 2, 64, 2
    base, mask, dy = _inputs(B, S, h, True, seed=70)
    y_n, _, node = _run(base, mask, dy, h, 0.1, training=False)
    assert node == "AttentionBlockFnBackward"
    os.environ["SKY_NO_ATTN_BLOCK"] = "1"
    try:
        y_c, _, _ = _run(base, mask, dy, h, 0.1, training=False)
    finally:
        del os.environ["SKY_NO_ATTN_BLOCK"]
    assert torch.equal(y_n, y_c)
    for var in ("SKY_NO_FUSED_ATTN", "SKY_NO_FUSED_ATTN_BWD", "SKY_ATTN_FUSED_BWD",
                "SKY_NO_LN_DBIAS"):
        assert os.environ.get(var) is None
        os.environ[var] = "1"
        try:
            hidden = base[0].clone().requires_grad_(True)
            y = ops.attention_block(hidden, mask, base[1], base[2], h, 0.1, base[3],
                                    base[4], base[5], base[6], 1e-12, 0.1, True)
        finally:
            del os.environ[var]
        assert type(y.grad_fn).__name__ != "AttentionBlockFnBackward", var


def test_node_under_graph_capture():
    """Forward and backward of the node captured in one graph (p = 0.1,
    salts frozen at capture, no step-counter tick) and replayed twice:
    every replay equals the eager run made with the same dropout seed."""
    B, S, h = 2, 100, 2
    base, mask, dy = _inputs(B, S, h, True, seed=80)
    F.rng_state()  # allocate before any capture
    y_e, g_e, node = _run(base, mask, dy, h, 0.1)  # also tunes the GEMM plans
    assert node == "AttentionBlockFnBackward"

    leaves = [t.clone().requires_grad_(True) for t in base]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = ops.attention_block(leaves[0], mask, leaves[1], leaves[2], h, 0.1,
                                leaves[3], leaves[4], leaves[5], leaves[6],
                                1e-12, 0.1, True)
        y.backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    for t in leaves:
        t.grad = None
    F.set_dropout_seed(4321)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = ops.attention_block(leaves[0], mask, leaves[1], leaves[2], h, 0.1,
                                  leaves[3], leaves[4], leaves[5], leaves[6],
                                  1e-12, 0.1, True)
        y_g.backward(dy)
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_g.detach(), y_e), replay
        for name, t, want in zip(NAMES, leaves, g_e):
            assert torch.equal(t.grad, want), (replay, name)
