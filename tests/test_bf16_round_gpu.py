"""The fp32 -> bf16 rounding of ops/hip/common.h, over all 2^32 inputs.

f32_to_bf16 and f32x2_to_bf16x2 use the hardware convert. For every non-NaN
float it must give the bits of the integer round-to-nearest-even formula the
kernels used before; a NaN input must stay a NaN (the formula turned some
payloads into +-0 or +-Inf, the one permitted difference). The probe kernel
(ops/hip/bf16_round_probe.hip) keeps the formula as its reference, checks the
scalar form and both lanes of the packed form, and counts the violations and
the inputs it examined (a launch that counted nothing would also report no
violations).
"""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.ops.hiplib import check, ptr


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def test_hardware_rounding_matches_the_integer_formula_on_every_float():
    counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    check(hiplib.require().sky_probe_bf16_round(
        torch.cuda.current_stream().cuda_stream, ptr(counts)), "bf16_round_probe")
    torch.cuda.synchronize()
    differ, nan_lost, seen = counts.tolist()
    print(f"non-NaN inputs with other bits: {differ}; NaN inputs not NaN: "
          f"{nan_lost}; inputs examined: {seen}")
    assert seen == 2 ** 32
    assert differ == 0
    assert nan_lost == 0
