"""Column reductions of the first-generation kernels at shapes where their
row loops loop: several rows per slab, a ragged last slab, empty slabs,
fewer rows than slabs, and grids past their caps.

  sky_bias_gelu_bwd   streaming dx + db (default), SKY_GELU_SPLIT_DB,
                      SKY_GELU_FUSED_BWD, with and without bias
  functions.colsum    two-stage and atomic fallback
  LayerNormFn         the non-xsum backward: fused dx + partials and the
                      SKY_LN_SPLIT_WB chain

References are fp64, built from the kernel's own inputs; bounds are those of
tests/kernel_checks.py. dx is checked against fp64 first. The terms of a
bias-gelu db are the values the reduction summed:
  * the stored dx (in fp64) where a second kernel sums it (split path), and
    for every fp32 run, where the stored dx IS the fp32 value that the fused
    kernels accumulate;
  * the fp64 dx for the fused kernels in bf16, which accumulate the fp32 dx
    before it is rounded; its error (1e-6) is far inside the bound's 2^-7.
Taking the fp64 dx as terms in fp32 too does not work for a one-row sum: the
bound is then 1.1e-4 * |dx|, and where gelu'(x + b) crosses zero (x + b near
-0.75) dx is small against the 1.5e-7 absolute error of the kernels' erf;
measured on an MI355X, 1 to 6 of 2048 to 4096 columns were 1.5 to 18 times
over, while dx itself stays within about 2 x the fp32 eager op's error.
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


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ("SKY_GELU_CS_SLABS", "SKY_GELU_SPLIT_DB", "SKY_GELU_FUSED_BWD",
                "SKY_LN_CS_GRID", "SKY_LN_SPLIT_WB"):
        monkeypatch.delenv(var, raising=False)


DTYPES = [torch.bfloat16, torch.float32]
NAN = float("nan")

# floor of the bf16 elementwise bound for dx-like outputs: a handful of fp32
# operations on intermediates of magnitude <= 8 (|dy*w| <= 4.5*1.5), each
# rounding to 2^-24 * 8 = 5e-7
DX_FLOOR = 1e-5
# floor for dy * gelu'(x + b): four fp32 roundings of a value <= 8
GELU_FLOOR = 4 * 8 * 2.0 ** -24


def _gelu_inputs(rows, cols, dtype, bias, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    x = torch.randn(rows, cols, device="cuda", generator=gen).to(dtype)
    dy = torch.randn(rows, cols, device="cuda", generator=gen).to(dtype)
    b = torch.randn(cols, device="cuda", generator=gen).to(dtype) if bias else None
    return dy, x, b


def _run_gelu_bwd(dy, x, b):
    """Raw sky_bias_gelu_bwd into NaN-filled dx, db and scratch."""
    rows, cols = x.shape
    dx = torch.full_like(x, NAN)
    db = torch.full((cols,), NAN, dtype=x.dtype, device="cuda")
    scratch = torch.full((F._CS_SLABS * cols,), NAN, dtype=torch.float32, device="cuda")
    check(
        hiplib.require().sky_bias_gelu_bwd(
            torch.cuda.current_stream().cuda_stream, ptr(dy), ptr(x), ptr(b),
            ptr(dx), ptr(db), ptr(scratch), rows, cols, F._dt(x)),
        "sky_bias_gelu_bwd",
    )
    return dx, db


def _eager_gelu_dx(dy, x, b):
    z = (x.float() if b is None else x.float() + b.float()).requires_grad_(True)
    eager.gelu(z).backward(dy.float())
    return z.grad


def _check_gelu_bwd(dy, x, b, db_from_stored_dx):
    db_from_stored_dx = db_from_stored_dx or x.dtype == torch.float32
    dx, db = _run_gelu_bwd(dy, x, b)
    terms = kc.bias_gelu_bwd_ref64(dy, x, b)
    kc.assert_output(dx, terms, lambda: _eager_gelu_dx(dy, x, b), "dx", floor=GELU_FLOOR)
    kc.assert_colsum(db, dx.double() if db_from_stored_dx else terms, "db")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("cols", [2048, 4096])
@pytest.mark.parametrize("rows,slabs", [(10, 3), (9, 3), (4, 3), (1, 3), (1030, None)])
def test_bias_gelu_bwd_streaming(rows, slabs, cols, bias, dtype, monkeypatch):
    """bias_gelu_bwd_cs_kernel. With 3 slabs: 10 rows = 4 + 4 + 2 (several
    rows per slab, ragged last), 9 = 3 + 3 + 3, 4 = 2 + 2 + 0 (an empty
    slab), 1 row (fewer rows than slabs). 1030 rows pass the natural slab
    count (1024 at cols 2048, 512 at 4096). The sums are accumulated from
    the unrounded fp32 dx: terms as the module docstring says."""
    if slabs is not None:
        monkeypatch.setenv("SKY_GELU_CS_SLABS", str(slabs))
    dy, x, b = _gelu_inputs(rows, cols, dtype, bias, 7 * rows + cols)
    _check_gelu_bwd(dy, x, b, db_from_stored_dx=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("cols", [2048, 1024, 72])
@pytest.mark.parametrize("rows", [300, 1500, 10, 1])
@pytest.mark.parametrize("mode", ["split", "fused"])
def test_bias_gelu_bwd_split_and_fused(mode, rows, cols, bias, dtype, monkeypatch):
    """split: dx_vec + two-stage colsum over the stored dx (the reduction's
    input, hence its reference terms). fused: bias_gelu_bwd_part_kernel,
    sums of the unrounded dx. Both cap the slab count at the row count
    until rows pass 1024 slabs: 1500 rows give two rows per slab and empty
    slabs behind them, 300 rows one row per slab."""
    monkeypatch.setenv("SKY_GELU_SPLIT_DB", "1")
    if mode == "fused":
        monkeypatch.setenv("SKY_GELU_FUSED_BWD", "1")
    dy, x, b = _gelu_inputs(rows, cols, dtype, bias, 11 * rows + cols)
    _check_gelu_bwd(dy, x, b, db_from_stored_dx=(mode == "split"))


def test_bias_gelu_bwd_default_narrow_width():
    """cols % 8 == 0 but not % 2048, no environment: dx_vec + colsum_part."""
    dy, x, b = _gelu_inputs(300, 1024, torch.bfloat16, True, 5)
    _check_gelu_bwd(dy, x, b, db_from_stored_dx=True)


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["out_bf16", "out_fp32"])
@pytest.mark.parametrize("cols", [8, 1032, 301])
@pytest.mark.parametrize("rows", [1, 129, 1500])
def test_colsum(rows, cols, out_dtype):
    """Two-stage colsum (cols % 8 == 0; 1500 rows give 2 to 3 rows per slab
    and empty slabs) and the atomic fallback (cols = 301, fp32 result cast
    by the wrapper)."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(rows * 31 + cols)
    src = torch.randn(rows, cols, device="cuda", generator=gen).to(torch.bfloat16)
    out = F.colsum(src, out_dtype)
    assert out.dtype == out_dtype and out.shape == (cols,)
    kc.assert_colsum(out, src.double(), "colsum")


# ------------------------------------------------------- LayerNorm backward


def _ln_bwd_case(rows, cols, dtype, residual, p, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=gen).to(dtype)

    x = rnd(rows, cols).requires_grad_(True)
    res = rnd(rows, cols).requires_grad_(True) if residual else None
    w = (torch.rand(cols, device="cuda", generator=gen) + 0.5).to(dtype).requires_grad_(True)
    b = rnd(cols).requires_grad_(True)
    dy = rnd(rows, cols)
    F.set_dropout_seed(seed)
    y = F.LayerNormFn.apply(x, w, b, 1e-12, res, p)
    y.backward(dy)
    assert w.grad.dtype == dtype and b.grad.dtype == dtype

    keep = 1.0 - p
    if p > 0:
        # the keep mask is where dx is non-zero (dx is mask/keep * dxs)
        mask = (x.grad != 0)
        frac = mask.double().mean().item()
        n = mask.numel()
        assert abs(frac - keep) < 5 * (keep * (1 - keep) / n) ** 0.5 + 2.0 ** -16, frac
        mask64 = mask.double() / keep
    else:
        mask64 = torch.ones_like(x, dtype=torch.float64)
    xs = x.detach().double() * mask64
    if residual:
        xs = xs + res.detach().double()
    dxs, dw_terms, db_terms = kc.layernorm_bwd_ref64(dy, xs, w.detach(), 1e-12)

    def eager_grads():
        xf = x.detach().float().requires_grad_(True)
        rf = res.detach().float().requires_grad_(True) if residual else None
        h = xf * mask64.float()
        eager.layer_norm(h, w.detach().float(), b.detach().float(), 1e-12, rf).backward(
            dy.float())
        return xf.grad, (rf.grad if residual else None)

    eg = eager_grads() if dtype == torch.float32 else (None, None)
    kc.assert_output(x.grad, dxs * mask64, lambda: eg[0], "dx", floor=DX_FLOOR)
    if residual:
        kc.assert_output(res.grad, dxs, lambda: eg[1], "dres", floor=DX_FLOOR)
    kc.assert_colsum(w.grad, dw_terms, "dw")
    kc.assert_colsum(b.grad, db_terms, "db")


LN_CASES = [
    # rows, env: 2100 rows = 525 row groups over the 512-block cap (blocks
    # 0..12 take a second group); 5 rows = two blocks, the second with one
    # wave active; 2 blocks x 37 rows = 4 to 5 rows per wave; the split
    # chain with one row per slab (37) and two rows per slab plus empty
    # slabs (1100 rows over 1024 slabs)
    (2100, {}),
    (5, {}),
    (37, {"SKY_LN_CS_GRID": "2"}),
    (37, {"SKY_LN_SPLIT_WB": "1"}),
    (1100, {"SKY_LN_SPLIT_WB": "1"}),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("rows,env", LN_CASES,
                         ids=["r2100", "r5", "r37_grid2", "r37_split", "r1100_split"])
def test_layernorm_backward_non_xsum(rows, env, residual, p, dtype, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _ln_bwd_case(rows, 1024, dtype, residual, p, seed=rows + 13)
