"""Masked softmax forward and backward where the first-round test could not
tell a wrong kernel from a right one: a different random mask per batch
(the mask row is picked by row / (h*Sq)), logits of scale 40 (overflow
without the max subtraction), 30 rows (no multiple of the 4, 8 or 16 rows a
block takes), one batch whose mask hides every key, and every path by Sk:

  8, 48     16-lane groups        136   32-lane group, partly filled
  264       64-lane group, partly filled        512   64-lane group, full
  100       scalar fallback (Sk % 8 != 0)       520   fallback past 512

fp32 bounds: 8 x the error of eager.masked_softmax in fp32 on the same
inputs against fp64 (forward) and of the fp32 eager backward formula
(backward). Measured on an MI355X, max |err| against fp64 of the fp32 eager
forward: 7.3e-8 to 1.5e-7 with per-batch masks or none, 8.2e-6 to 1.7e-4
with the fully hidden batch (scores - 9984 loses the low bits in fp32, in
the kernel and in eager alike); the kernel was between 0.73 and 1.14 times
that, and at most 2.2 times the eager backward's error.
"""

from __future__ import annotations

import pytest
import torch

from . import kernel_checks as kc
from .test_attn_bwd_dbias_gpu import make_mask

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import eager, hiplib
    from skycomputing_amd.ops.functions import MaskedSoftmaxFn


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


B, H, SQ = 3, 2, 5
SKS = [8, 48, 136, 264, 512, 100, 520]


def _inputs(Sk, dtype, mask_kind):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(Sk * 7 + len(mask_kind))
    scores = (torch.randn(B, H, SQ, Sk, device="cuda", generator=gen) * 40.0).to(dtype)
    dp = torch.randn(B, H, SQ, Sk, device="cuda", generator=gen).to(dtype)
    if mask_kind == "none":
        mask = None
    else:
        for _ in range(100):  # at Sk = 8 two batches can draw the same mask
            mask = make_mask(B, Sk, gen)
            if mask_kind == "one_batch_all_hidden":
                mask[1] = -10000.0  # softmax of the scores alone
            if len({tuple(m.flatten().tolist()) for m in mask}) == B:
                break
        else:
            raise AssertionError("no batch-distinct mask drawn")
        mask = mask.to(dtype)
    return scores.requires_grad_(True), mask, dp


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mask_kind", ["per_batch", "one_batch_all_hidden", "none"])
@pytest.mark.parametrize("Sk", SKS)
def test_masked_softmax_fwd_bwd(Sk, mask_kind, dtype):
    scale = 1.0
    scores, mask, dp = _inputs(Sk, dtype, mask_kind)
    probs = MaskedSoftmaxFn.apply(scores, mask, scale)
    probs.backward(dp)
    p = probs.detach()
    ref = kc.softmax_ref64(scores.detach(), mask, scale)
    if mask_kind == "one_batch_all_hidden":
        alone = kc.softmax_ref64(scores.detach()[1], None, scale)
        assert torch.allclose(ref[1], alone, rtol=1e-9, atol=0.0)

    kc.assert_output(
        p, ref, lambda: eager.masked_softmax(scores.detach().float() * scale,
                                             None if mask is None else mask.float()),
        "probs")
    kc.assert_bounded(p.double().sum(-1), torch.ones(B, H, SQ, dtype=torch.float64,
                                                     device="cuda"),
                      torch.full((B, H, SQ), Sk * 2.0 ** -9, dtype=torch.float64,
                                 device="cuda"), "row sums")

    # backward from the probabilities the kernel saved (its own input)
    ds_ref = kc.softmax_bwd_ref64(dp, p, scale)

    def eager_ds():
        pf, df = p.float(), dp.float()
        return scale * pf * (df - (df * pf).sum(-1, keepdim=True))

    kc.assert_output(scores.grad, ds_ref, eager_ds, "ds")
