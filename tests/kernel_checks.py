"""fp64 references and error bounds shared by the first-generation kernel
tests (test_*_gen1_gpu.py) and by test_gen1_checks_cpu.py, which shows that
each bound rejects a subtly wrong result.

Everything here is plain torch on whatever device its inputs live on. Every
assert_* helper prints the figures it compares, treats a NaN as a failure
and leaves no element out of the comparison.

Bounds
  column sums    |err| <= rel*|ref| + 1e-4 * sum|terms|, rel = 2^-7 for a
                 bf16 output (one rounding is at most 2^-8*|ref|) and 1e-5
                 for fp32
  bf16 outputs   |err| <= 2^-8*|ref| + floor: one rounding to bf16 (8
                 significant bits) from an fp32 value is at most
                 2^-8*|ref|, so the floor is all that the fp32 arithmetic
                 before it may use
  fp32 outputs   max|err| <= 8 * max|err| of the fp32 eager op on the same
                 inputs, both against fp64
"""

from __future__ import annotations

import torch

BF16_REL = 2.0 ** -8
COLSUM_REL = {torch.bfloat16: 2.0 ** -7, torch.float32: 1e-5}
COLSUM_TERMS = 1e-4
EAGER_FACTOR = 8.0


def _report(name, err, bound):
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"{name}: max|err| {err.max().item():.3e}, max err/bound {worst:.3f}")
    return worst


def assert_bounded(got, ref64, bound, name="value"):
    """Elementwise |got - ref64| <= bound, NaN in got failing."""
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    err = (got.double() - ref64).abs()
    worst = _report(name, err, bound)
    ok = err <= bound  # False where err is NaN
    assert ok.all(), f"{name}: {int((~ok).sum())} elements over the bound, worst x{worst:.2f}"


def assert_colsum(got, terms64, name="colsum", sum_dim=0):
    """got[c] against the fp64 sum of terms64 over sum_dim."""
    ref = terms64.sum(sum_dim)
    a = terms64.abs().sum(sum_dim)
    assert_colsum_ref(got, ref, a, name)


def assert_colsum_ref(got, ref64, abs_terms64, name="colsum"):
    """Column-sum bound from a precomputed fp64 sum and sum of |terms|."""
    rel = COLSUM_REL[got.dtype]
    assert_bounded(got, ref64, rel * ref64.abs() + COLSUM_TERMS * abs_terms64, name)


def assert_bf16_close(got, ref64, floor=1e-6, name="bf16 value"):
    assert got.dtype == torch.bfloat16, got.dtype
    assert_bounded(got, ref64, BF16_REL * ref64.abs() + floor, name)


def assert_within_eager(got, eager32, ref64, name="fp32 value", factor=EAGER_FACTOR):
    """max|got - ref64| <= factor * max|eager32 - ref64|. Returns the eager
    error so the caller can quote it."""
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    eager_err = (eager32.double() - ref64).abs().max().item()
    err = (got.double() - ref64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    worst = err.max().item()
    print(f"{name}: max|err| {worst:.3e}, fp32 eager max|err| {eager_err:.3e}, "
          f"ratio {worst / eager_err if eager_err else float('inf'):.2f}")
    assert worst <= factor * eager_err, (
        f"{name}: {worst:.3e} > {factor:g} x eager {eager_err:.3e}")
    return eager_err


def assert_output(got, ref64, eager32_fn, name, floor=1e-6):
    """The elementwise rule by dtype: bf16 by its rounding bound, fp32
    against the eager op (eager32_fn() is only evaluated for fp32)."""
    if got.dtype == torch.bfloat16:
        assert_bf16_close(got, ref64, floor, name)
    else:
        assert_within_eager(got, eager32_fn(), ref64, name)


def assert_sgd_close(got, ref64, name="sgd"):
    """fp32 optimizer state against the fp64 loop: 1e-6 relative + 1e-7."""
    assert got.dtype == torch.float32, got.dtype
    assert_bounded(got, ref64, 1e-6 * ref64.abs() + 1e-7, name)


# ---------------------------------------------------------------- references


def gelu_grad64(z):
    cdf = 0.5 * (1.0 + torch.erf(z / 2.0 ** 0.5))
    pdf = torch.exp(-0.5 * z * z) / (2.0 * torch.pi) ** 0.5
    return cdf + z * pdf


def bias_gelu_bwd_ref64(dy, x, b):
    """dx terms of d/dx gelu(x + b) in fp64 from the kernel's own inputs;
    db is their column sum. b may be None (x is the pre-activation)."""
    z = x.double() if b is None else x.double() + b.double()
    return dy.double() * gelu_grad64(z)


def softmax_ref64(scores, mask, scale, mask_batch=None):
    """softmax(scores*scale + mask) in fp64. mask is [B,1,1,Sk] additive or
    None; mask_batch=i uses batch i's mask for every batch (a wrong variant
    for the tests of the tests)."""
    z = scores.double() * scale
    if mask is not None:
        m = mask.double()
        if mask_batch is not None:
            m = m[mask_batch:mask_batch + 1].expand_as(m)
        z = z + m
    return torch.softmax(z, dim=-1)


def softmax_bwd_ref64(dp, probs, scale):
    """ds = scale * p * (dp - sum_k dp*p) from the probabilities the kernel
    was given."""
    p, d = probs.double(), dp.double()
    return scale * p * (d - (d * p).sum(-1, keepdim=True))


def softmax_noshift_fp32(scores, mask, scale):
    """Wrong variant: fp32 softmax without the common shift."""
    z = scores.float() * scale
    if mask is not None:
        z = z + mask.float()
    e = torch.exp(z)
    return e / e.sum(-1, keepdim=True)


def layernorm_ref64(x, w, b, eps, residual=None):
    """(y, mean, rstd, xhat) in fp64."""
    xs = x.double() if residual is None else x.double() + residual.double()
    mean = xs.mean(-1, keepdim=True)
    var = ((xs - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xs - mean) * rstd
    return xhat * w.double() + b.double(), mean.squeeze(-1), rstd.squeeze(-1), xhat


def layernorm_single_pass_fp32(x, w, b, eps):
    """Wrong variant: var = E[x^2] - mean^2 in fp32. Returns (y, rstd)."""
    xf = x.float()
    n = xf.shape[-1]
    mean = xf.sum(-1, keepdim=True) / n
    var = ((xf * xf).sum(-1, keepdim=True) / n - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + eps)
    return (xf - mean) * rstd * w.float() + b.float(), rstd.squeeze(-1)


def layernorm_bwd_ref64(dy, xs64, w, eps):
    """LayerNorm backward in fp64 on the (already dropped-out and
    residual-added) input xs64. Returns (dxs, dw_terms, db_terms): dxs is
    the gradient of xs64, the term tensors sum over rows to dw and db."""
    mean = xs64.mean(-1, keepdim=True)
    var = ((xs64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xs64 - mean) * rstd
    d = dy.double()
    dxhat = d * w.double()
    s1 = dxhat.mean(-1, keepdim=True)
    s2 = (dxhat * xhat).mean(-1, keepdim=True)
    return rstd * (dxhat - s1 - xhat * s2), d * xhat, d


def embedding_ref64(ids, tids, pids, we, pe, te, w, b, eps, dy, last_only_id=None):
    """Fused embedding + LayerNorm forward and the five gradients in fp64.
    Returns y and, for each table, (grad, sum of |terms|), plus the dw/db
    term tensors. last_only_id=t stores only the last row's contribution to
    word row t (a scatter that does not accumulate; wrong variant)."""
    i, t, p = ids.reshape(-1), tids.reshape(-1), pids.reshape(-1)
    xs = we.double()[i] + pe.double()[p] + te.double()[t]
    y, _, _, _ = layernorm_ref64(xs, w, b, eps)
    dy2 = dy.reshape(-1, dy.shape[-1])
    dxs, dw_terms, db_terms = layernorm_bwd_ref64(dy2, xs, w, eps)

    def scatter(table, idx, skip=None):
        g = torch.zeros(table.shape, dtype=torch.float64, device=table.device)
        a = torch.zeros_like(g)
        src = dxs
        if skip is not None:
            rows = (idx == skip).nonzero().flatten()
            keep = torch.ones(idx.numel(), dtype=torch.bool, device=idx.device)
            keep[rows[:-1]] = False
            idx, src = idx[keep], dxs[keep]
        g.index_add_(0, idx, src)
        a.index_add_(0, idx, src.abs())
        return g, a

    return (y.view(*ids.shape, -1), scatter(we, i, last_only_id), scatter(pe, p),
            scatter(te, t), dw_terms, db_terms)


def sgd_ref64(params, grads_per_step, lr, momentum, wd, bf16_every_step=False):
    """Plain SGD loop in fp64: g += wd*p; buf = momentum*buf + g; p -= lr*buf.
    lr, momentum and wd are used as the fp32 values the kernel is handed.
    params: list of tensors (any dtype); grads_per_step: list (one entry
    per step) of lists of tensors. bf16_every_step rounds p to bf16 after
    every step (a run without master weights). Returns (params64, bufs64)."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).double().item()
    lr, momentum, wd = f32(lr), f32(momentum), f32(wd)
    ps = [p.detach().double().clone() for p in params]
    bufs = [torch.zeros_like(p) for p in ps]
    for grads in grads_per_step:
        for k, g in enumerate(grads):
            gg = g.detach().double()
            if wd != 0.0:
                gg = gg + wd * ps[k]
            if momentum != 0.0:
                bufs[k] = bufs[k] * momentum + gg
                gg = bufs[k]
            ps[k] = ps[k] - lr * gg
            if bf16_every_step:
                ps[k] = ps[k].to(torch.bfloat16).double()
    return ps, bufs
