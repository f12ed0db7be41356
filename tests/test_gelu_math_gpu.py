"""GELU and its derivative as the kernels compute them (ops/hip/common.h:
erf_fast with the hardware reciprocal, one shared exponential in the
derivative), against fp64 on every finite bf16 x with |x| <= 16.

Bound for a bf16 output: |out - ref| <= 2^-8 |ref| + 2e-6. The first term is
half a bf16 ulp (the final rounding); the second covers the fp32 formula
(Abramowitz & Stegun 7.1.26 with v_rcp_f32 / v_exp_f32: emulated at 4.4e-7
for gelu and 3.6e-7 for the derivative, reciprocal pushed +-1 ulp).

The streaming backward also returns db, which must be the column sum of dx:
the bound is the one tests/test_finish_reductions_gpu.py uses for its
off-path case (fp32 slab sums, one rounding to the output dtype).

The fused gemm2 forward is driven with one-hot x rows and zero bias, so each
pre-activation is exactly one weight entry: Z must be that entry bit for bit
and Y must meet the bound above. The weights run over zero and the normal
bf16 range of one sign per call. (Subnormal entries are left out: whether a
subnormal operand survives the MFMA is the matrix unit's denormal mode, not
this epilogue's arithmetic.)
"""

from __future__ import annotations

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.ops.hiplib import check, ptr

BF16, FP32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _from_bits(bits):
    return torch.tensor(bits, dtype=torch.int32).to(torch.int16).view(BF16)


def _all_bf16_upto_16():
    """Every finite bf16 with |x| <= 16: bit patterns 0x0000..0x4180 of each
    sign, 2 * 16769 = 33538 values (both zeros, all subnormals)."""
    pos = list(range(0x0000, 0x4181))
    vals = _from_bits(pos + [0x8000 | p for p in pos])
    assert vals.numel() == 33538 and vals.float().abs().max() == 16.0
    return vals


def _gelu64(x):
    x = x.double()
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_grad64(x):
    x = x.double()
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return cdf + x * pdf


def _assert_within(out, ref, what):
    err = (out.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2e-6
    worst = (err / bound).max().item()
    print(f"{what}: max err/bound {worst:.3f}, max abs err {err.max().item():.3e}")
    assert torch.isfinite(out).all(), what
    assert (err <= bound).all(), what


@pytest.fixture(scope="module")
def grids():
    """The 33538 values, zero-padded, as 17 x 2048 (one 2048-column window)
    and 9 x 4096 (two windows), with their fp64 references."""
    vals = _all_bf16_upto_16()
    out = {}
    for rows, cols in [(17, 2048), (9, 4096)]:
        x = torch.zeros(rows * cols, dtype=BF16)
        x[: vals.numel()] = vals
        x = x.view(rows, cols)
        out[(rows, cols)] = (x.cuda(), _gelu64(x), _gelu_grad64(x))
    return out


# slabs None: the launcher's own choice, one row per slab at these heights
# (the loop's odd-row tail). Otherwise SKY_GELU_CS_SLABS: 17 rows in 4 slabs
# are 5 + 5 + 5 + 2 (two-row trips plus the tail; a ragged last slab), 9 rows
# in 2 slabs are 5 + 4.
@pytest.mark.parametrize("rows,cols,slabs", [
    (17, 2048, None), (17, 2048, 4), (9, 4096, None), (9, 4096, 2)])
def test_gelu_backward_against_fp64(grids, monkeypatch, rows, cols, slabs):
    x, _, ref = grids[(rows, cols)]
    if slabs is not None:
        monkeypatch.setenv("SKY_GELU_CS_SLABS", str(slabs))
    dy = torch.ones_like(x)
    dx = torch.full_like(x, NAN)
    db = torch.full((cols,), NAN, dtype=BF16, device="cuda")
    scratch = torch.full((F._CS_SLABS * cols,), NAN, dtype=FP32, device="cuda")
    check(hiplib.require().sky_bias_gelu_bwd(
        _stream(), ptr(dy), ptr(x), 0, ptr(dx), ptr(db), ptr(scratch),
        rows, cols, F._dt(x)), "gelu_bwd")
    torch.cuda.synchronize()
    _assert_within(dx, ref, f"gelu' {rows}x{cols} slabs={slabs}")
    # db: column sum of the stored dx
    d = dx.double()
    want, a = d.sum(0), d.abs().sum(0)
    err = (db.double() - want).abs()
    bound = 2.0 ** -7 * want.abs() + 1e-4 * a
    print(f"db: max err/bound {(err / bound).max().item():.3f}")
    assert torch.isfinite(db).all()
    assert (err <= bound).all()


@pytest.mark.parametrize("rows,cols", [(17, 2048), (9, 4096)])
def test_gelu_forward_against_fp64(grids, rows, cols):
    x, ref, _ = grids[(rows, cols)]
    b = torch.zeros(cols, dtype=BF16, device="cuda")
    y = torch.full_like(x, NAN)
    check(hiplib.require().sky_bias_gelu_fwd(
        _stream(), ptr(x), ptr(b), ptr(y), rows, cols, F._dt(x)), "gelu_fwd")
    torch.cuda.synchronize()
    _assert_within(y, ref, f"gelu {rows}x{cols}")


def _one_sign_weights(n, sign):
    """n bf16 values of one sign: normal numbers, bit patterns spread evenly
    over 0x0080..0x7f7f (all 32512 of them once n allows it), and +0 in the
    positive set (a -0 entry gives a +0 accumulator, which is the MFMA's
    business: 1 * -0 added to +0)."""
    normals = list(range(0x0080, 0x7F80))
    if n >= len(normals):
        bits = [0x0080] * (n - len(normals)) + normals
    else:
        step = len(normals) / n
        bits = [normals[int(i * step)] for i in range(n)]
        bits[-1] = 0x7F7F  # keep the largest finite value
    if sign == 0:
        bits[0] = 0
    assert len(bits) == n
    return _from_bits([sign | b for b in bits])


@pytest.mark.parametrize("sign", [0x0000, 0x8000], ids=["positive", "negative"])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (512, 256, 128)])
def test_gemm2_fused_forward_on_exact_preactivations(M, N, K, sign):
    w = _one_sign_weights(N * K, sign).view(N, K)
    x = torch.zeros(M, K, dtype=BF16)
    x[torch.arange(M), torch.arange(M) % K] = 1.0
    pre = w[:, torch.arange(M) % K].t().contiguous()  # pre[m][n] = w[n][m % K]
    wd, xd = w.cuda(), x.cuda()
    bias = torch.zeros(N, dtype=BF16, device="cuda")
    y = torch.full((M, N), NAN, dtype=BF16, device="cuda")
    z = torch.full((M, N), NAN, dtype=BF16, device="cuda")
    F._g2_call(xd, wd, y, bias, z, M, N, K, K, K, N, 0, 0, 2, 1)
    torch.cuda.synchronize()
    assert torch.equal(z.cpu().view(torch.int16), pre.view(torch.int16))
    _assert_within(y, _gelu64(pre), f"gemm2 Y {M}x{N}x{K} sign={sign:#x}")
