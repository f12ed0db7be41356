"""Flash forward (FlashAttentionFn): the two-query-blocks-per-workgroup
instantiation, which a launch only picks at B*h*ceil(nqb/2) >= 512, and the
dropout mask shared between the forward kernel and the decomposed backward.
"""

from __future__ import annotations

import pytest
import torch

from . import kernel_checks as kc
from .test_attn_bwd_dbias_gpu import make_mask

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.ops.hiplib import check, ptr


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


D = 64


def _split(qkv):
    return tuple(qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))


@pytest.mark.parametrize("B,h,S", [(8, 64, 130), (4, 64, 300)], ids=["S130", "S300"])
def test_flash_forward_two_query_blocks_per_workgroup(B, h, S):
    """S = 130: two query blocks, the second with two rows. S = 300: three,
    so the last workgroup of a head has an empty second block. Masked, no
    dropout; out at the suite's 6e-2 bound, the saved row max and row sum
    within 8 x the error of the same quantities computed in fp32 by torch."""
    nqb = (S + 127) // 128
    assert nqb >= 2 and B * h * ((nqb + 1) // 2) >= 512  # the launch's own rule
    gen = torch.Generator(device="cuda")
    gen.manual_seed(S)
    qkv = torch.randn(B, S, 3, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    mask = make_mask(B, S, gen)
    scale = 1.0 / D ** 0.5
    out = torch.full((B, S, h, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    m = torch.full((B, h, S), float("nan"), dtype=torch.float32, device="cuda")
    lsum = torch.full_like(m, float("nan"))
    check(
        hiplib.require().sky_attn_flash_fwd(
            torch.cuda.current_stream().cuda_stream, ptr(qkv), ptr(mask), ptr(out),
            ptr(m), ptr(lsum), B, S, h, D, scale, 1.0, 0, F.rng_state().data_ptr()),
        "sky_attn_flash_fwd",
    )

    def stats(dtype):
        q, k, v = (t.to(dtype) for t in _split(qkv))
        z = torch.matmul(q, k.transpose(-1, -2)) * scale + mask.to(dtype)
        zm = z.max(-1).values
        e = torch.exp(z - zm.unsqueeze(-1))
        ls = e.sum(-1)
        o = torch.matmul(e / ls.unsqueeze(-1), v).permute(0, 2, 1, 3)
        return zm, ls, o

    m64, l64, o64 = stats(torch.float64)
    m32, l32, _ = stats(torch.float32)
    err = (out.double() - o64).abs().max().item()
    print(f"S={S} out max|err| {err:.4f}")
    assert torch.allclose(out.double(), o64, atol=6e-2, rtol=6e-2), err
    kc.assert_within_eager(m, m32, m64, "row max")
    kc.assert_within_eager(lsum, l32, l64, "row sum")


def test_flash_dropout_mask_is_the_backwards_mask():
    """The forward kernel draws its keep mask inline; the backward
    regenerates it with sky_dropout_*. The mask recovered from
    sky_dropout_fwd on ones with the node's salt feeds an fp64 reference;
    out and qkv.grad must match it at the bounds of
    test_fused_attention_dropout_mask_shared_by_all_backwards (6e-2, 8e-2).
    A forward that drew another mask misses on most elements."""
    B, h, S, p = 2, 2, 192, 0.5
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    qkv = torch.randn(B, S, 3, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    qkv.requires_grad_(True)
    mask = make_mask(B, S, gen)
    scale = 1.0 / D ** 0.5
    F.set_dropout_seed(5)
    out = F.FlashAttentionFn.apply(qkv, mask, scale, p, True)
    dout = torch.randn(B, S, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    out.backward(dout)
    fn = out.grad_fn
    assert fn.keep == 1.0 - p and fn.salt != 0

    ones = torch.ones(B, h, S, S, dtype=torch.bfloat16, device="cuda")
    kept = torch.empty_like(ones)
    check(
        hiplib.require().sky_dropout_fwd(
            torch.cuda.current_stream().cuda_stream, ptr(ones), ptr(kept),
            ones.numel(), fn.keep, fn.salt, F.rng_state().data_ptr(), F._dt(ones)),
        "sky_dropout_fwd",
    )
    keepmask = (kept != 0).double()
    n = keepmask.numel()
    assert abs(keepmask.mean().item() - fn.keep) < 5 * (0.25 / n) ** 0.5 + 2.0 ** -16

    q64 = qkv.detach().double().requires_grad_(True)
    q, k, v = _split(q64)
    z = torch.matmul(q, k.transpose(-1, -2)) * scale + mask.double()
    probs = torch.softmax(z, dim=-1) * keepmask / fn.keep
    ref = torch.matmul(probs, v).permute(0, 2, 1, 3)
    ref.backward(dout.double())
    err = (out.double() - ref).abs().max().item()
    gerr = (qkv.grad.double() - q64.grad).abs().max().item()
    print(f"out max|err| {err:.4f}, qkv.grad max|err| {gerr:.4f}")
    assert torch.allclose(out.detach().double(), ref.detach(), atol=6e-2, rtol=6e-2), err
    assert torch.allclose(qkv.grad.double(), q64.grad, atol=8e-2, rtol=8e-2), gerr
