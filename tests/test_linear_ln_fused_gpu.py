"""linear -> dropout -> residual LayerNorm as one autograd node
(LinearResidualLayerNormFn): the linear's dbias comes out of the LayerNorm
backward pass (sky_layernorm_bwd_xsum) and its weight gradient is a plain
hipBLASLt GEMM (sky_hblt_wgrad). Checked against the fp32 eager reference,
against the two-Function composition it replaces, and under graph capture.
"""

from __future__ import annotations

import os

import pytest
import torch

from tests.test_ops_gpu import _tols

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd import ops
    from skycomputing_amd.ops import eager, hiplib
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops.hiplib import check, ptr


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _inputs(rows, K, N, dtype, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)

    x = rn(rows, K)
    w = rn(N, K, scale=0.03)
    b = rn(N)
    ln_w = (torch.rand(N, device="cuda", generator=g) + 0.5).to(dtype)
    ln_b = rn(N)
    res = rn(rows, N)
    dy = rn(rows, N)
    return [x, w, b, ln_w, ln_b, res], dy


def _leaves(ts):
    return [t.clone().requires_grad_(True) for t in ts]


# (rows, K, N): fewer rows than one block's four waves (and not a multiple
# of 4); more than 4*512 rows so the 512-block grid cap makes blocks loop
# with a ragged tail; cols/8 = 65, a partly filled second chunk; CH=4.
_SHAPES = [(5, 64, 1024), (2100, 128, 1024), (256, 256, 520), (128, 64, 2048)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,K,N", _SHAPES)
def test_fused_vs_fp32_reference(rows, K, N, dtype):
    """No dropout. y, dx, dres at _tols(dtype); the five row-accumulated
    gradients at the test_hblt_linear_bias_backward dW/db tolerance."""
    assert F.ln_xsum_width_ok(N)
    base, dy = _inputs(rows, K, N, dtype, seed=40)
    x, w, b, ln_w, ln_b, res = _leaves(base)
    y = F.LinearResidualLayerNormFn.apply(x, w, b, ln_w, ln_b, 1e-12, res, 0.0)
    y.backward(dy)

    ref = _leaves([t.float() for t in base])
    xf, wf, bf, lwf, lbf, rf = ref
    yr = eager.layer_norm(torch.nn.functional.linear(xf, wf, bf), lwf, lbf, 1e-12, rf)
    yr.backward(dy.float())

    t = _tols(dtype)
    for name, got, want in (("y", y, yr), ("dx", x.grad, xf.grad), ("dres", res.grad, rf.grad)):
        err = (got.float() - want).abs().max().item()
        print(f"{name}: max abs err {err:.3e}")
        assert torch.allclose(got.float(), want, **t), (name, err)
    for name, got, want in (("ln_dw", ln_w.grad, lwf.grad), ("ln_db", ln_b.grad, lbf.grad),
                            ("dW", w.grad, wf.grad), ("dbias", b.grad, bf.grad)):
        err = (got.float() - want).abs().max().item()
        print(f"{name}: max abs err {err:.3e}")
        assert got.dtype == dtype
        assert torch.allclose(got.float(), want, atol=t["atol"] * 100, rtol=0.05), (name, err)


def test_unsupported_width_takes_composition():
    """CH=8 widths are not built with the third sum: the entry point
    refuses them and the public wrapper composes linear + layer_norm."""
    N = 4096
    assert not F.ln_xsum_width_ok(N)
    base, dy = _inputs(8, 64, N, torch.bfloat16, seed=41)
    x, w, b, ln_w, ln_b, res = _leaves(base)
    y = ops.linear_residual_layer_norm(x, w, b, ln_w, ln_b, 1e-12, res, 0.0, True)
    assert type(y.grad_fn).__name__ == "LayerNormFnBackward"
    with pytest.raises(RuntimeError, match="sky_layernorm_bwd_xsum"):
        F.LinearResidualLayerNormFn.apply(x, w, b, ln_w, ln_b, 1e-12, res, 0.0).backward(dy)
    y2 = ops.linear_residual_layer_norm(x[:, :64], w[:1024], b[:1024], ln_w[:1024],
                                        ln_b[:1024], 1e-12, res[:, :1024], 0.0, True)
    assert type(y2.grad_fn).__name__ == "LinearResidualLayerNormFnBackward"


def _raw_ln_bwd_xsum(node, dy):
    """Re-run the fused node's LayerNorm backward kernel on its own saved
    tensors and salt: returns the gradient w.r.t. the linear's output,
    which the Function itself never exposes."""
    lib = hiplib.require()
    _, _, h, ln_w, mean, rstd = node.saved_tensors
    cols = h.shape[-1]
    rows = h.numel() // cols
    dh = torch.empty_like(h)
    dres = torch.empty_like(h)
    outs = [torch.empty(cols, dtype=ln_w.dtype, device="cuda") for _ in range(3)]
    scratch = torch.empty(1024 * 3 * cols, dtype=torch.float32, device="cuda")
    check(
        lib.sky_layernorm_bwd_xsum(
            torch.cuda.current_stream().cuda_stream, ptr(dy), ptr(h),
            ptr(node.residual), ptr(ln_w), ptr(mean), ptr(rstd), ptr(dh),
            ptr(outs[0]), ptr(outs[1]), ptr(scratch), rows, cols,
            F._dt(h), node.keep, node.salt, F.rng_state().data_ptr(),
            ptr(dres), ptr(outs[2]),
        ),
        "sky_layernorm_bwd_xsum",
    )
    return dh, outs[2]


@pytest.fixture(scope="module")
def dropout_pair():
    """One fused run and one composition run (LinearBiasFn then
    LayerNormFn) at p = 0.4 with the same dropout seed, shared by the
    comparisons below."""
    rows, K, N = 256, 512, 1024
    p = 0.4
    base, dy = _inputs(rows, K, N, torch.bfloat16, seed=42)

    F.set_dropout_seed(1234)
    fx = _leaves(base)
    y_f = F.LinearResidualLayerNormFn.apply(fx[0], fx[1], fx[2], fx[3], fx[4], 1e-12, fx[5], p)
    node = y_f.grad_fn
    y_f.backward(dy, retain_graph=True)
    dh_f, dxsum = _raw_ln_bwd_xsum(node, dy.contiguous())

    F.set_dropout_seed(1234)
    cx = _leaves(base)
    h = F.LinearBiasFn.apply(cx[0], cx[1], cx[2])
    h.retain_grad()
    y_c = F.LayerNormFn.apply(h, cx[3], cx[4], 1e-12, cx[5], p)
    salts = (node.salt, y_c.grad_fn.salt)
    y_c.backward(dy)
    names = ["dx", "dW", "dbias", "ln_dw", "ln_db", "dres"]
    fused = {n: t.grad for n, t in zip(names, fx)}
    comp = {n: t.grad for n, t in zip(names, cx)}
    fused.update(y=y_f.detach(), dlin=dh_f, dxsum=dxsum)
    comp.update(y=y_c.detach(), dlin=h.grad)
    return fused, comp, salts


def test_dropout_pair_same_forward_and_mask(dropout_pair):
    """Same salt, same forward kernels on the same inputs: y bit-identical;
    the keep-mask seen in d(linear out) is identical, exactly."""
    fused, comp, salts = dropout_pair
    assert salts[0] == salts[1] and salts[0] != 0
    assert torch.equal(fused["y"], comp["y"])
    assert torch.equal(fused["dlin"] != 0, comp["dlin"] != 0)
    dropped = (comp["dlin"] == 0).float().mean().item()
    assert 0.3 < dropped < 0.5, dropped
    # the raw re-run is the Function's own kernel call: its third sum is
    # the dbias the Function returned
    assert torch.equal(fused["dxsum"], fused["dbias"])


@pytest.mark.parametrize("name", ["y", "dlin", "dx", "dW", "dbias", "ln_dw", "ln_db", "dres"])
def test_dropout_pair_agrees(dropout_pair, name):
    """Fused vs composition at atol = rtol = 2e-2, the bound
    test_hblt_matches_fallback_path uses for the same kind of comparison.
    dbias holds it because the LN backward sums d(linear out) as stored
    (rounded to bf16), the same values the BGRADB epilogue sums."""
    fused, comp, _ = dropout_pair
    a, c = fused[name].float(), comp[name].float()
    err = (a - c).abs().max().item()
    nbad = ((a - c).abs() > 2e-2 + 2e-2 * c.abs()).sum().item()
    print(f"{name}: max abs diff {err:.3e}, {nbad} of {a.numel()} outside the bound")
    assert torch.allclose(a, c, atol=2e-2, rtol=2e-2), (name, err, nbad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,K,N", [(256, 512, 1024), (512, 1024, 3072)])
def test_hblt_wgrad_plain(M, K, N, dtype):
    """sky_hblt_wgrad alone vs fp32 dy^T @ x; the first call of a shape
    runs the measured algorithm selection, the second the cached plan."""
    lib = hiplib.require()
    g = torch.Generator(device="cuda")
    g.manual_seed(43)
    x = torch.randn(M, K, device="cuda", generator=g).to(dtype)
    dy = torch.randn(M, N, device="cuda", generator=g).to(dtype)
    ref = dy.float().t() @ x.float()
    t = _tols(dtype)
    for call in range(2):
        dw = torch.full((N, K), float("nan"), dtype=dtype, device="cuda")
        check(
            lib.sky_hblt_wgrad(torch.cuda.current_stream().cuda_stream, ptr(x),
                               ptr(dy), ptr(dw), M, N, K, F._dt(x)),
            "sky_hblt_wgrad",
        )
        err = (dw.float() - ref).abs().max().item()
        print(f"call {call}: max abs err {err:.3e}")
        assert torch.allclose(dw.float(), ref, atol=t["atol"] * 100, rtol=0.05), (call, err)


def _graphed_losses():
    from skycomputing_amd.builder import build_module_from_cfg
    from skycomputing_amd.models import bert_pipeline_config
    from skycomputing_amd.optim import FusedSGD
    from skycomputing_amd.parallel.graph import GraphedTrainStep

    torch.manual_seed(44)
    F.set_dropout_seed(44)
    F.rng_state().zero_()  # the device step counter is mixed into every mask
    cfgs = bert_pipeline_config(
        2, dict(hidden_size=256, num_attention_heads=4, intermediate_size=1024,
                vocab_size=2000, hidden_dropout_prob=0.1,
                attention_probs_dropout_prob=0.1)
    )
    stage = build_module_from_cfg(cfgs, device="cuda:0", dtype=torch.bfloat16,
                                  record_forward_time=False)
    opt = FusedSGD(stage.parameters(), lr=1e-3)
    ids = torch.randint(0, 2000, (4, 32), device="cuda")
    inputs = [ids, torch.zeros_like(ids), torch.ones_like(ids)]
    labels = torch.randint(0, 3, (4,), device="cuda")
    g = GraphedTrainStep(
        stage, opt,
        lambda lg, lb: torch.nn.functional.cross_entropy(lg.float(), lb),
        inputs, labels,
    )
    losses = []
    for _ in range(3):
        g.step(inputs, labels)
        losses.append(g.loss_value())
    return losses


def test_fused_path_under_graph_capture():
    """Three captured steps of a 2-layer stage: finite losses, and the same
    losses as the composition (SKY_NO_LN_DBIAS=1) — same seeds, so same
    init, data and dropout masks."""
    assert os.environ.get("SKY_NO_LN_DBIAS") is None
    fused = _graphed_losses()
    os.environ["SKY_NO_LN_DBIAS"] = "1"
    try:
        comp = _graphed_losses()
    finally:
        del os.environ["SKY_NO_LN_DBIAS"]
    print("fused", fused, "composition", comp)
    assert all(torch.isfinite(torch.tensor(fused)))
    assert torch.allclose(torch.tensor(fused), torch.tensor(comp), rtol=2e-2, atol=0.0)
