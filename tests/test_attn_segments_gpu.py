"""Segment mode of the long attention kernels (packed sequences), held to
tests/test_attn_long_gpu.py's rule: fp64 _math on the dense additive mask (-inf
off segment), _math rounded to bf16 as comparator, keep mask through the forward."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd import ops
    from skycomputing_amd.ops import eager, hiplib
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops.hiplib import check, ptr

from tests import test_attn_long_gpu as L
from tests.test_attn_long_gpu import D, _math
from tests.test_attn_segments_cpu import ROWS_300, ids_from_runs

# (B, S, h), per-row run boundaries: a one-key segment and a run across the
# chunk edge; two different rows; a lane whose first visited chunk holds no key
# of its run (query 150), a block past chunk 0, a pad run; five chunks, NC = 9.
LAYOUTS = [
    ((1, 129, 1), [([0, 1], False)]),
    ((2, 192, 2), [([0, 70], False), ([0], False)]),
    ((2, 300, 1), ROWS_300),
    ((1, 520, 1), [([0, 130, 131, 390], False)]),
]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _fwd(c, qkv=None):  # (out, m, l), NaN-filled before the launch
    B, S, h = c["B"], c["S"], c["h"]
    out = c["qkv"].new_full((B, S, h, D), float("nan"))
    m, lsum = (torch.full((B, h, S), float("nan"), device="cuda") for _ in range(2))
    check(hiplib.require().sky_attn_long_seg_fwd(
        L._stream(), ptr(c["qkv"] if qkv is None else qkv), ptr(c["ids"]), ptr(c["bounds"]),
        ptr(out), ptr(m), ptr(lsum), B, S, h, D, c["scale"], c["keep"], c["salt"],
        c["state"]), "sky_attn_long_seg_fwd")
    return out, m, lsum


def _bwd(c):
    dqkv, dot = torch.full_like(c["qkv"], float("nan")), torch.full_like(c["m"], float("nan"))
    args = F._attn_long_bwd_args(c["qkv"], c["dout"], c["out"], None, c["m"], c["l"], dot,
                                 dqkv, c["scale"], c["keep"], c["salt"])
    check(hiplib.require().sky_attn_long_seg_bwd(
        *args[:4], ptr(c["ids"]), ptr(c["bounds"]), *args[5:]), "sky_attn_long_seg_bwd")
    return dqkv


def _inputs(B, S, h, rows, p):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * S + 10 * h + B)
    c = dict(B=B, S=S, h=h, scale=1.0 / math.sqrt(D), keep=1.0 - p,
             salt=L.SALT if p > 0 else 0, state=F.rng_state().data_ptr())
    c["qkv"] = torch.randn(B, S, 3, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["dout"] = torch.randn(B, S, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    ids = ids_from_runs(S, rows)
    c["ids"] = ids.to("cuda", torch.int32)
    c["bounds"] = F.attn_seg_bounds(c["ids"])
    assert torch.equal(c["bounds"].cpu(), eager.seg_bounds(ids))
    return c


@functools.lru_cache(maxsize=None)
def _case(i, p):
    (B, S, h), rows = LAYOUTS[i]
    c = _inputs(B, S, h, rows, p)
    c["out"], c["m"], c["l"] = _fwd(c)
    c["dqkv"] = _bwd(c)
    same = eager.segment_mask(c["ids"], check=False)
    c["mask"] = torch.zeros(same.shape, device="cuda").masked_fill_(~same, float("-inf"))
    Pd = torch.ones(B, h, S, 64 * ((S + 63) // 64), device="cuda")
    for cb in range((S + 63) // 64 if p > 0 else 0):  # out = Pd[..., 64 cb + j]
        qkv, n = c["qkv"].clone(), min(64, S - 64 * cb)
        qkv[:, :, 2] = 0
        qkv[:, 64 * cb:64 * cb + n, 2] = torch.eye(64, device="cuda", dtype=qkv.dtype)[:n, None]
        Pd[..., 64 * cb:64 * cb + 64] = _fwd(c, qkv)[0].permute(0, 2, 1, 3).float()
    keepmask = (Pd[..., :S] != 0).float()
    c["ref"], _ = _math(c, keepmask, lambda x: x)
    c["model"], _ = _math(c, keepmask, lambda x: x.to(torch.bfloat16).double())
    return c


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("i", range(len(LAYOUTS)))
def test_accuracy_against_fp64(i, p):
    c = _case(i, p)
    got = [c["out"]] + [c["dqkv"][:, :, j] for j in range(3)]
    for name, new, ref, model in zip(("out", "dQ", "dK", "dV"), got, c["ref"], c["model"]):
        e_new, e_cmp = ((x - ref).abs().max().item() for x in (new.double(), model))
        bound = 1.5 * e_cmp + 2.0 ** -9 * ref.abs().max().item()
        print(f"{LAYOUTS[i][0]} p={p} {name}: err {e_new:.4e} model {e_cmp:.4e} bound {bound:.4e}")
        assert torch.isfinite(new.float()).all() and e_new <= bound, name


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_one_segment_equals_no_mask(p):
    """Every row one run: the bits of sky_attn_long_fwd / _bwd with mask = None."""
    c = _inputs(2, 300, 1, [([0], False), ([0], False)], p)
    c["mask"] = None
    c["out"], c["m"], c["l"] = dense = L._fwd(c)
    assert all(torch.equal(a, b) for a, b in zip(_fwd(c), dense))
    assert torch.equal(_bwd(c), L._bwd(c)[0])


def test_skipped_chunks_are_not_read():
    """Three chunk-aligned runs through ops.attention: NaN inputs in the middle
    run change no bit of the other two, as a visited chunk (0 * NaN) would."""
    c = _inputs(1, 384, 1, [([0, 128, 256], False)], 0.0)
    res = []
    for poison in (False, True):
        qkv, dout = c["qkv"].clone(), c["dout"].reshape(1, 384, D).clone()
        if poison:
            qkv[:, 128:256], dout[:, 128:256] = float("nan"), float("nan")
        qkv.requires_grad_(True)
        out = ops.attention(qkv, None, 0.0, True, segment_ids=c["ids"])
        assert type(out.grad_fn.next_functions[0][0]).__name__ == "FusedAttentionFnBackward"
        out.backward(dout)
        res.append((out.detach(), qkv.grad))
    for clean, poisoned in zip(*res):
        for rows in (slice(0, 128), slice(256, 384)):
            assert torch.isfinite(clean[:, rows].float()).all()
            assert torch.equal(clean[:, rows], poisoned[:, rows])
