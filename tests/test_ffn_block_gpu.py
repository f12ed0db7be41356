"""The FFN two-thirds of an encoder block as one autograd node (FfnBlockFn
behind ops.ffn_block): x's two gradients summed inside the ffn-up dgrad GEMM,
the four column sums finished in one launch. Checked against the two-node
composition it replaces (SKY_NO_FFN_BLOCK=1), against an fp32 eager
reference, and under graph capture.

The fused ffn-up forward is enabled by default only at the benchmark's shape;
the tests enable its site for their small shapes the way
test_gemm2_linear_fwd_bwd_matches_reference does.
"""

from __future__ import annotations

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd import ops
    from skycomputing_amd.ops import eager, hiplib
    from skycomputing_amd.ops import functions as F

NAMES = ["d_x", "dWup", "dbup", "dWdown", "dbdown", "d_ln_w", "d_ln_b"]
NODE = "FfnBlockFnBackward"

# (B, S, H, I): rows 256 with I = 2048 is the smallest problem both the
# fused forward (M, N % 256) and the streaming gelu backward (cols % 2048)
# accept; rows 512 with I = 4096 has the benchmark's widths.
SHAPES = [(2, 128, 1024, 2048), (4, 128, 1024, 4096)]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


@pytest.fixture()
def g2_sites():
    """Sets the v2 hand-GEMM sites for a test and restores them after."""
    old = (F._G2_SITES, F._G2_SITES_SET)

    def use(*sites):
        F._G2_SITES, F._G2_SITES_SET = set(sites), True

    yield use
    F._G2_SITES, F._G2_SITES_SET = old


@pytest.fixture()
def env():
    """Sets environment switches for a test and removes them after."""
    names = []

    def use(name):
        assert os.environ.get(name) is None
        os.environ[name] = "1"
        names.append(name)

    yield use
    for n in names:
        del os.environ[n]


def _inputs(B, S, H, I, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=g) * scale).to(torch.bfloat16)

    x = rn(B, S, H)
    wup = rn(I, H, scale=0.03)
    bup = rn(I, scale=0.1)
    wdown = rn(H, I, scale=0.03)
    bdown = rn(H, scale=0.1)
    ln_w = (torch.rand(H, device="cuda", generator=g) + 0.5).to(torch.bfloat16)
    ln_b = rn(H)
    dy = rn(B, S, H)
    return [x, wup, bup, wdown, bdown, ln_w, ln_b], dy


def _call(leaves, p):
    x, wup, bup, wdown, bdown, ln_w, ln_b = leaves
    return ops.ffn_block(x, wup, bup, wdown, bdown, ln_w, ln_b, 1e-12, p, True)


def _run(base, dy, p):
    """ops.ffn_block forward + backward on fresh leaves; returns y, the
    gradients in NAMES order and the output's grad_fn name."""
    F.set_dropout_seed(4321)
    leaves = [t.clone().requires_grad_(True) for t in base]
    y = _call(leaves, p)
    node = type(y.grad_fn).__name__
    y.backward(dy)
    return y.detach(), [t.grad for t in leaves], node


def _composition(base, dy, p):
    assert os.environ.get("SKY_NO_FFN_BLOCK") is None
    os.environ["SKY_NO_FFN_BLOCK"] = "1"
    try:
        return _run(base, dy, p)
    finally:
        del os.environ["SKY_NO_FFN_BLOCK"]


_REF = {}


def _fp32_dx(shape):
    """d x of the block in fp32 eager from the same bf16 inputs, no dropout;
    computed once per shape and shared."""
    if shape not in _REF:
        base, dy = _inputs(*shape, seed=60 + shape[3])
        x, wup, bup, wdown, bdown, ln_w, ln_b = [
            t.float().clone().requires_grad_(True) for t in base]
        pre = torch.nn.functional.linear(x, wup, bup)
        inter = pre * 0.5 * (1 + torch.erf(pre / 2 ** 0.5))
        y = eager.layer_norm(torch.nn.functional.linear(inter, wdown, bdown),
                             ln_w, ln_b, 1e-12, x)
        y.backward(dy.float())
        _REF[shape] = (base, dy, x.grad.detach())
    return _REF[shape]


@pytest.mark.parametrize("sites", [("fwd",), ("fwd", "dgrad")], ids=["addmm", "g2dgrad"])
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("shape", SHAPES, ids=["r256", "r512"])
def test_node_vs_composition(shape, p, sites, g2_sites):
    """Same seeds: y bit-identical (same forward kernels, same salt); the
    six parameter gradients differ by exactly 0 (same kernels on the same
    bits, only the finals merged); d x, rounded once instead of twice,
    inside atol = rtol = 2e-2. ids: addmm = the benchmark's path
    (hipBLASLt dgrad with beta = 1), g2dgrad = add_ of the hand dgrad."""
    g2_sites(*sites)
    base, dy = _inputs(*shape, seed=50 + shape[3])
    y_n, g_n, node_n = _run(base, dy, p)
    y_c, g_c, node_c = _composition(base, dy, p)
    assert node_n == NODE
    assert node_c == "LinearResidualLayerNormFnBackward"
    assert torch.equal(y_n, y_c)
    bad = []
    for name, a, c in zip(NAMES, g_n, g_c):
        assert a.dtype == c.dtype and a.shape == c.shape
        assert torch.isfinite(a).all() and torch.isfinite(c).all(), name
        a, c = a.float(), c.float()
        err = (a - c).abs().max().item()
        print(f"{name}: max abs diff {err:.3e}")
        if name == "d_x":
            ratio = ((a - c).abs() / (2e-2 + 2e-2 * c.abs())).max().item()
            print(f"d_x: worst err/bound {ratio:.3f}")
            if not torch.allclose(a, c, atol=2e-2, rtol=2e-2):
                bad.append((name, err))
        elif err != 0.0:
            bad.append((name, err))
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES, ids=["r256", "r512"])
def test_dx_error_vs_fp32_not_above_compositions(shape, g2_sites):
    """No dropout. Both d x share every error upstream of the last GEMM (the
    same dpre and dres bits); the composition then rounds dpre @ Wup to bf16
    and rounds again after autograd's add, the node rounds the fp32 sum
    once. The shared part is the same in both, so the whole-tensor RMS error
    against fp32 eager must not be larger for the node: that is the
    assertion. The max-abs errors sit on single elements where the shared
    part decides, and are printed only."""
    g2_sites("fwd")
    base, dy, want = _fp32_dx(shape)
    _, g_n, node = _run(base, dy, 0.0)
    _, g_c, _ = _composition(base, dy, 0.0)
    assert node == NODE
    e_n = g_n[0].float() - want
    e_c = g_c[0].float() - want
    rms_n, rms_c = e_n.pow(2).mean().sqrt().item(), e_c.pow(2).mean().sqrt().item()
    print(f"d_x rms err vs fp32: node {rms_n:.4e}, composition {rms_c:.4e}; "
          f"max abs: node {e_n.abs().max().item():.4e}, "
          f"composition {e_c.abs().max().item():.4e}")
    assert rms_n <= rms_c


@pytest.mark.parametrize("p", [0.0, 0.4])
def test_separate_finals_give_the_same_bits(p, g2_sites, env):
    """SKY_NO_MERGED_FINISH=1 (one final launch per producer) against the
    merged finish, in the node: every output bit-identical."""
    g2_sites("fwd")
    base, dy = _inputs(*SHAPES[0], seed=71)
    y_m, g_m, node_m = _run(base, dy, p)
    env("SKY_NO_MERGED_FINISH")
    y_s, g_s, node_s = _run(base, dy, p)
    assert node_m == node_s == NODE
    assert torch.equal(y_m, y_s)
    for name, a, b in zip(NAMES, g_m, g_s):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("var", ["SKY_NO_FFN_BLOCK", "SKY_NO_LN_DBIAS"])
def test_env_switches_keep_the_composition(var, g2_sites, env):
    g2_sites("fwd")
    base, _ = _inputs(*SHAPES[0], seed=72)
    leaves = [t.clone().requires_grad_(True) for t in base]
    assert type(_call(leaves, 0.1).grad_fn).__name__ == NODE
    env(var)
    assert type(_call(leaves, 0.1).grad_fn).__name__ != NODE


def test_outside_the_fused_forwards_shapes_is_the_composition(g2_sites):
    """With no site enabled ops.linear_act does not take LinearGeluFn, so
    neither does the block take its node."""
    g2_sites()
    base, dy = _inputs(*SHAPES[0], seed=73)
    y, grads, node = _run(base, dy, 0.0)
    assert node == "LinearResidualLayerNormFnBackward"
    assert all(torch.isfinite(g).all() for g in grads)


@pytest.mark.parametrize("p", [0.0, 0.4])
def test_node_under_graph_capture(p, g2_sites):
    """Forward and backward of the node captured in one graph (salt frozen
    at capture, no step-counter tick) and replayed twice: every replay
    equals the eager run made with the same dropout seed."""
    g2_sites("fwd")
    base, dy = _inputs(*SHAPES[0], seed=80)
    F.rng_state()  # allocate before any capture
    y_e, g_e, node = _run(base, dy, p)  # also tunes the GEMM plans
    assert node == NODE

    leaves = [t.clone().requires_grad_(True) for t in base]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(leaves, p).backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    for t in leaves:
        t.grad = None
    F.set_dropout_seed(4321)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = _call(leaves, p)
        y_g.backward(dy)
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_g.detach(), y_e), replay
        for name, t, want in zip(NAMES, leaves, g_e):
            assert torch.equal(t.grad, want), (replay, name)
