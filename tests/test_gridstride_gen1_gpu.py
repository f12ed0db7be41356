"""Kernels whose grid is capped, at the smallest sizes that make a block take
its grid-stride step: bias-gelu and dropout (2048 blocks of 256 vec8 items),
ln_fwd_vec_kernel (8192 blocks of 4 rows), emb_fwd_kernel (4096 blocks, one
row each; the backward takes 8 rows per block). fp64 references from the
kernels' own inputs, bounds from tests/kernel_checks.py.
"""

from __future__ import annotations

import pytest
import torch

from . import kernel_checks as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import eager, hiplib
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops.hiplib import check, ptr


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


CAP_ITEMS = 2048 * 256  # work items of one full capped elementwise grid

# floors of the bf16 elementwise bound: a few fp32 roundings (2^-24 each) of
# intermediates of magnitude <= 8
GELU_FLOOR = 4 * 8 * 2.0 ** -24
LN_FLOOR = 1e-5


def test_bias_gelu_past_grid_cap(monkeypatch):
    """1040 x 4096 bf16 is 532480 vec8 items > 2048 * 256: the first 8192
    threads of the forward take a second item. The default backward is the
    streaming kernel (512 slabs of 3 rows: 346 full, one of 2 rows, the
    rest empty); with SKY_GELU_SPLIT_DB the capped dx_vec kernel runs."""
    monkeypatch.delenv("SKY_GELU_SPLIT_DB", raising=False)
    monkeypatch.delenv("SKY_GELU_FUSED_BWD", raising=False)
    monkeypatch.delenv("SKY_GELU_CS_SLABS", raising=False)
    rows, cols = 1040, 4096
    assert rows * cols // 8 > CAP_ITEMS
    gen = torch.Generator(device="cuda")
    gen.manual_seed(101)
    x = torch.randn(rows, cols, device="cuda", generator=gen).bfloat16().requires_grad_(True)
    b = torch.randn(cols, device="cuda", generator=gen).bfloat16().requires_grad_(True)
    dy = torch.randn(rows, cols, device="cuda", generator=gen).bfloat16()
    y = F.BiasGeluFn.apply(x, b)
    z = x.detach().double() + b.detach().double()
    kc.assert_bf16_close(y.detach(), z * 0.5 * (1.0 + torch.erf(z / 2.0 ** 0.5)),
                         GELU_FLOOR, "y")
    terms = kc.bias_gelu_bwd_ref64(dy, x.detach(), b.detach())

    y.backward(dy, retain_graph=True)
    kc.assert_bf16_close(x.grad, terms, GELU_FLOOR, "dx (streaming)")
    kc.assert_colsum(b.grad, terms, "db (streaming)")

    x.grad = b.grad = None
    monkeypatch.setenv("SKY_GELU_SPLIT_DB", "1")
    y.backward(dy)
    kc.assert_bf16_close(x.grad, terms, GELU_FLOOR, "dx (dx_vec)")
    kc.assert_colsum(b.grad, x.grad.double(), "db (colsum of stored dx)")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [8 * CAP_ITEMS + 8 * 7, CAP_ITEMS + 3], ids=["vec", "scalar"])
def test_dropout_past_grid_cap(n, dtype):
    """Vector kernel with 7 items past one full grid, scalar kernel with 3.
    Every output is 0 or x/keep; the backward draws the forward's mask;
    and the mask is the one the OTHER kernel (scalar for vector and the
    reverse) draws for the same salt at the same element indices."""
    keep = 0.7
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n)
    x = (torch.rand(n, device="cuda", generator=gen) + 0.5).to(dtype).requires_grad_(True)
    F.set_dropout_seed(n)
    y = F.DropoutFn.apply(x, 1.0 - keep)
    salt = y.grad_fn.salt
    mask = y.detach() != 0
    frac = mask.double().mean().item()
    assert abs(frac - keep) < 5 * (keep * (1 - keep) / n) ** 0.5 + 2.0 ** -16, frac
    ref = x.detach().double() * mask.double() / keep
    if dtype == torch.bfloat16:
        kc.assert_bf16_close(y.detach(), ref, 0.0, "y")
    else:
        # one fp32 multiply by the fp32 value of 1/keep
        kc.assert_bounded(y.detach(), ref, 2.0 ** -22 * ref.abs(), "y")
    y.backward(torch.ones_like(y))
    assert torch.equal(x.grad != 0, mask), "backward mask differs from forward mask"

    # the other kernel: n + 1 is odd for the vector size, n - 3 a multiple of 8
    m = n + 1 if n % 8 == 0 else n - 3
    assert (m % 8 == 0) != (n % 8 == 0)
    ones = torch.ones(m, dtype=dtype, device="cuda")
    other = torch.empty_like(ones)
    check(
        hiplib.require().sky_dropout_fwd(
            torch.cuda.current_stream().cuda_stream, ptr(ones), ptr(other), m,
            keep, salt, F.rng_state().data_ptr(), F._dt(ones)),
        "sky_dropout_fwd",
    )
    k = min(m, n)
    assert torch.equal(other[:k] != 0, mask[:k]), "scalar and vector masks differ"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_layernorm_fwd_past_grid_cap(dtype):
    """4 * 8192 + 5 rows of 64: every block takes a second row group, the
    first two a ragged third. y and the saved mean and rstd."""
    rows, cols = 4 * 8192 + 5, 64
    gen = torch.Generator(device="cuda")
    gen.manual_seed(202)
    x = torch.randn(rows, cols, device="cuda", generator=gen).to(dtype).requires_grad_(True)
    w = (torch.rand(cols, device="cuda", generator=gen) + 0.5).to(dtype)
    b = torch.randn(cols, device="cuda", generator=gen).to(dtype)
    y = F.LayerNormFn.apply(x, w, b, 1e-12, None, 0.0)
    _, _, mean, rstd = y.grad_fn.saved_tensors
    y64, mean64, rstd64, _ = kc.layernorm_ref64(x.detach(), w, b, 1e-12)
    ey, emean, erstd = torch.native_layer_norm(
        x.detach().float(), (cols,), w.float(), b.float(), 1e-12)
    kc.assert_output(y.detach(), y64, lambda: ey, "y", floor=LN_FLOOR)
    kc.assert_within_eager(mean, emean.reshape(-1), mean64, "mean")
    kc.assert_within_eager(rstd, erstd.reshape(-1), rstd64, "rstd")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_embedding_past_grid_cap_shared_ids(dtype):
    """4100 rows (41 x 100): four blocks of the forward take a second row,
    the backward's last block holds 4 of 8 rows. H = 72 leaves most of a
    block's threads idle. Every row of a batch is the same token, so each
    word row sums 100 or more rows through atomics, each position row 41,
    each type row about 2050. All five gradients."""
    V, P, H, B, S = 50, 100, 72, 41, 100
    gen = torch.Generator(device="cuda")
    gen.manual_seed(303)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=gen).to(dtype)

    we, pe, te = (rnd(V, H).requires_grad_(True), rnd(P, H).requires_grad_(True),
                  rnd(2, H).requires_grad_(True))
    w = (torch.rand(H, device="cuda", generator=gen) + 0.5).to(dtype).requires_grad_(True)
    b = rnd(H).requires_grad_(True)
    tok = torch.randint(0, V, (B,), device="cuda", generator=gen)
    tok[0], tok[-1] = V - 1, V - 1  # the last word row, from two batches
    ids = tok.view(B, 1).expand(B, S).contiguous()
    tids = torch.randint(0, 2, (B, S), device="cuda", generator=gen)
    pids = torch.arange(S, device="cuda").view(1, S).expand(B, S).contiguous()
    assert (ids == V - 1).any() and (pids == P - 1).any() and ids.numel() == 4100
    dy = rnd(B, S, H)

    y = F.EmbeddingFusedFn.apply(ids, tids, pids, we, pe, te, w, b, 1e-12)
    y.backward(dy)
    d = lambda t: t.detach()
    y64, (gwe, awe), (gpe, ape), (gte, ate), dw_terms, db_terms = kc.embedding_ref64(
        ids, tids, pids, d(we), d(pe), d(te), d(w), d(b), 1e-12, dy)
    kc.assert_output(
        d(y), y64,
        lambda: eager.embedding_fused(ids, tids, pids, d(we), d(pe), d(te), d(w), d(b), 1e-12),
        "y", floor=LN_FLOOR)
    kc.assert_colsum_ref(we.grad, gwe, awe, "d word_emb")
    kc.assert_colsum_ref(pe.grad, gpe, ape, "d pos_emb")
    kc.assert_colsum_ref(te.grad, gte, ate, "d type_emb")
    kc.assert_colsum(w.grad, dw_terms, "d ln_w")
    kc.assert_colsum(b.grad, db_terms, "d ln_b")
