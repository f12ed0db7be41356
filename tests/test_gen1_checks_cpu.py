"""The first-generation kernel tests must be able to fail: for each input
family of test_*_gen1_gpu.py, build the fp64 reference and a deliberately,
subtly wrong result on the CPU, and assert that the comparison helper of
tests/kernel_checks.py accepts the faithful result and REJECTS the wrong
one. No GPU, no kernel library.
"""

from __future__ import annotations

import pytest
import torch

from skycomputing_amd.ops import eager

from . import kernel_checks as kc


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _cpu_mask(B, S, gen):
    drop = torch.rand(B, S, generator=gen) < 0.25
    drop[:, 0] = False
    return (drop.float() * -10000.0).to(torch.bfloat16).view(B, 1, 1, S)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_colsum_bound_rejects_a_left_out_slab(out_dtype):
    """10 rows in slabs of 4 + 4 + 2 (SKY_GELU_CS_SLABS=3): the ragged last
    slab's two rows left out."""
    g = _gen(1)
    dy = torch.randn(10, 2048, generator=g).bfloat16()
    x = torch.randn(10, 2048, generator=g).bfloat16()
    b = torch.randn(2048, generator=g).bfloat16()
    terms = kc.bias_gelu_bwd_ref64(dy, x, b)
    kc.assert_colsum(terms.float().sum(0).to(out_dtype), terms, "faithful db")
    with pytest.raises(AssertionError):
        kc.assert_colsum(terms[:8].float().sum(0).to(out_dtype), terms, "db without slab 2")
    # a slab that is never written leaves NaN behind
    bad = terms.float().sum(0).to(out_dtype)
    bad[5] = float("nan")
    with pytest.raises(AssertionError):
        kc.assert_colsum(bad, terms, "db with an unwritten element")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_softmax_bounds_reject_wrong_batch_mask_and_missing_shift(dtype):
    B, h, Sq, Sk = 3, 2, 5, 48
    g = _gen(2)
    scores = (torch.randn(B, h, Sq, Sk, generator=g) * 40.0).to(dtype)
    mask = _cpu_mask(B, Sk, g).to(dtype)
    assert not torch.equal(mask[0], mask[1])
    ref = kc.softmax_ref64(scores, mask, 1.0)
    eager32 = lambda: eager.masked_softmax(scores.float(), mask.float())

    kc.assert_output(eager32().to(dtype), ref, eager32, "faithful probs")
    wrong_mask = kc.softmax_ref64(scores, mask, 1.0, mask_batch=0).float().to(dtype)
    with pytest.raises(AssertionError):
        kc.assert_output(wrong_mask, ref, eager32, "batch 0's mask everywhere")
    no_shift = kc.softmax_noshift_fp32(scores, mask, 1.0)
    assert not torch.isfinite(no_shift).all()  # exp(40 * randn) overflows fp32
    with pytest.raises(AssertionError):
        kc.assert_output(no_shift.to(dtype), ref, eager32, "no max subtraction")


def test_sgd_bounds_reject_ignored_weight_decay():
    g = _gen(3)
    params = [torch.randn(n, generator=g) for n in (7, 1029)]
    grads = [[0.1 * torch.randn(p.numel(), generator=g) for p in params] for _ in range(3)]
    ref_p, ref_b = kc.sgd_ref64(params, grads, 0.1, 0.9, 0.01)
    # the kernel's arithmetic, in fp32
    ps = [p.clone() for p in params]
    bufs = [torch.zeros_like(p) for p in params]
    eager.sgd_step(ps, grads[0], 0.1, 0.9, 0.01, bufs)
    eager.sgd_step(ps, grads[1], 0.1, 0.9, 0.01, bufs)
    eager.sgd_step(ps, grads[2], 0.1, 0.9, 0.01, bufs)
    for k in range(2):
        kc.assert_sgd_close(ps[k], ref_p[k], "faithful param")
        kc.assert_sgd_close(bufs[k], ref_b[k], "faithful momentum")
    no_wd, no_wd_b = kc.sgd_ref64(params, grads, 0.1, 0.9, 0.0)
    with pytest.raises(AssertionError):
        kc.assert_sgd_close(no_wd[1].float(), ref_p[1], "param, wd ignored")
    with pytest.raises(AssertionError):
        kc.assert_sgd_close(no_wd_b[1].float(), ref_b[1], "momentum, wd ignored")


def test_master_weight_checks_reject_a_bf16_only_update():
    n, steps, lr, gval = 16, 50, 0.1, 1e-3
    start = [torch.ones(n, dtype=torch.bfloat16)]
    grads = [[torch.full((n,), gval, dtype=torch.bfloat16)]] * steps
    (ref,), _ = kc.sgd_ref64(start, grads, lr, 0.0, 0.0)
    assert ref.to(torch.bfloat16)[0].item() == 0.99609375
    kc.assert_sgd_close(ref.float(), ref, "faithful master")
    (stalled,), _ = kc.sgd_ref64(start, grads, lr, 0.0, 0.0, bf16_every_step=True)
    assert torch.equal(stalled, torch.ones(n, dtype=torch.float64))
    with pytest.raises(AssertionError):
        kc.assert_sgd_close(stalled.float(), ref, "bf16-only update as master")
    assert not torch.equal(stalled.to(torch.bfloat16), ref.to(torch.bfloat16))


@pytest.mark.parametrize("cols", [1024, 1001])
def test_layernorm_bounds_reject_single_pass_variance_at_mean_64(cols):
    g = _gen(4)
    x = torch.randn(9, cols, generator=g) + 64.0
    w = torch.rand(cols, generator=g) + 0.5
    b = torch.randn(cols, generator=g)
    y64, _, rstd64, _ = kc.layernorm_ref64(x, w, b, 1e-12)
    ey = eager.layer_norm(x, w, b, 1e-12)
    _, _, erstd = torch.native_layer_norm(x, (cols,), w, b, 1e-12)
    erstd = erstd.reshape(-1)
    # centred variance in fp32, as the kernels compute it
    mean = x.sum(-1, keepdim=True) / cols
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / cols + 1e-12)
    kc.assert_within_eager(d * rstd * w + b, ey, y64, "centred y")
    kc.assert_within_eager(rstd.reshape(-1), erstd, rstd64, "centred rstd")
    y1, rstd1 = kc.layernorm_single_pass_fp32(x, w, b, 1e-12)
    with pytest.raises(AssertionError):
        kc.assert_within_eager(y1, ey, y64, "single-pass y")
    with pytest.raises(AssertionError):
        kc.assert_within_eager(rstd1, erstd, rstd64, "single-pass rstd")
    # bf16 output: one rounding bound
    xb, wb, bb = x.bfloat16(), w.bfloat16(), b.bfloat16()
    yb64, _, _, _ = kc.layernorm_ref64(xb, wb, bb, 1e-12)
    kc.assert_bf16_close(yb64.float().bfloat16(), yb64, 1e-6, "faithful bf16 y")
    y1b, _ = kc.layernorm_single_pass_fp32(xb, wb, bb, 1e-12)
    with pytest.raises(AssertionError):
        kc.assert_bf16_close(y1b.bfloat16(), yb64, 1e-6, "single-pass bf16 y")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_embedding_bound_rejects_a_scatter_that_does_not_accumulate(dtype):
    V, P, H, B, S = 10, 12, 72, 5, 12
    g = _gen(5)
    we, pe, te = (torch.randn(V, H, generator=g).to(dtype), torch.randn(P, H, generator=g).to(dtype),
                  torch.randn(2, H, generator=g).to(dtype))
    w = (torch.rand(H, generator=g) + 0.5).to(dtype)
    b = torch.randn(H, generator=g).to(dtype)
    tok = torch.randint(0, V, (B,), generator=g)
    tok[0] = tok[-1] = V - 1
    ids = tok.view(B, 1).expand(B, S).contiguous()
    tids = torch.randint(0, 2, (B, S), generator=g)
    pids = torch.arange(S).view(1, S).expand(B, S).contiguous()
    dy = torch.randn(B, S, H, generator=g).to(dtype)
    _, (gwe, awe), _, _, _, _ = kc.embedding_ref64(ids, tids, pids, we, pe, te, w, b, 1e-12, dy)
    kc.assert_colsum_ref(gwe.float().to(dtype), gwe, awe, "faithful d word_emb")
    _, (bad, _), _, _, _, _ = kc.embedding_ref64(ids, tids, pids, we, pe, te, w, b, 1e-12, dy,
                                                 last_only_id=V - 1)
    assert torch.equal(bad[: V - 1], gwe[: V - 1])
    with pytest.raises(AssertionError):
        kc.assert_colsum_ref(bad.float().to(dtype), gwe, awe, "d word_emb, last row only")
