"""LayerNorm forward on rows whose mean is far from zero.

A single-pass variance (E[x^2] - mean^2) in fp32 loses log2(mean^2 / var)
bits: at cols = 1024, std 1 the error in x-hat against fp64 is 5e-7 at mean
0, 1e-5 at 4, 1.3e-4 at 16 and 2.4e-3 at 64, where the two-pass fp32 eager
op stays within about 1e-5. The kernels compute the variance from centred
values; this test holds them to 8 x the eager op's own error, y and the
saved rstd and mean alike, and bf16 outputs to one rounding
(2^-8 * |ref| + 1e-6).

Measured on an MI355X, fp32, max |err| of y against fp64, kernel / eager:
  mean      vector (cols 1024)       scalar (cols 1001)
   0        4.4e-7 / 4.4e-7          6.0e-7 / 5.3e-7
  16        2.5e-6 / 2.7e-6          5.3e-7 / 2.3e-6
  64        5.0e-6 / 1.2e-5          5.1e-7 / 9.9e-6
and of rstd, 4e-8 to 1.5e-7 against 5e-8 to 6e-7 (worst ratio 1.7).

The bf16 bound leaves 1e-6 for everything before the output rounding, less
than the rounding of an fp32 mean of 64 (up to 4e-6). The vector case meets
it because 1024 bf16 values near 64 have an exactly representable mean; the
scalar fallback (1001 columns) meets it because it takes the residual of the
centred sum off x - mean. With the plain centred variance it was over on 2
of 9009 elements, by a factor of 1.08.
"""

from __future__ import annotations

import pytest
import torch

from . import kernel_checks as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import eager, hiplib
    from skycomputing_amd.ops.functions import LayerNormFn


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


ROWS = 9  # three blocks of the vector kernel, the last with one wave active
EPS = 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mu", [0, 16, 64])
@pytest.mark.parametrize("cols", [1024, 1001], ids=["vector", "scalar"])
def test_layernorm_fwd_offset_row_mean(cols, mu, dtype):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * mu + cols)
    x = (torch.randn(ROWS, cols, device="cuda", generator=gen) + mu).to(dtype)
    x.requires_grad_(True)
    w = (torch.rand(cols, device="cuda", generator=gen) + 0.5).to(dtype)
    b = torch.randn(cols, device="cuda", generator=gen).to(dtype)
    y = LayerNormFn.apply(x, w, b, EPS, None, 0.0)
    _, _, mean, rstd = y.grad_fn.saved_tensors
    xd = x.detach()
    y64, mean64, rstd64, _ = kc.layernorm_ref64(xd, w, b, EPS)

    ey = eager.layer_norm(xd.float(), w.float(), b.float(), EPS)
    _, emean, erstd = torch.native_layer_norm(xd.float(), (cols,), w.float(), b.float(), EPS)
    if dtype == torch.float32:
        kc.assert_within_eager(y.detach(), ey, y64, f"y mu={mu}")
    else:
        kc.assert_bf16_close(y.detach(), y64, 1e-6, f"y mu={mu}")
    kc.assert_within_eager(rstd, erstd.reshape(-1), rstd64, f"rstd mu={mu}")
    kc.assert_within_eager(mean, emean.reshape(-1), mean64, f"mean mu={mu}")
