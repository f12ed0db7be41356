"""The head-dim-128 attention kernels (ops/hip/attention_d128.hip,
1 <= S <= 4096): forward with per-lane online softmax over 64-key chunks, dQ
with dot = dO . O, dK/dV with the accumulators in registers; additive key
mask or causal.

Reference: the same mathematics in fp64 (_math with no rounding), keep mask
recovered through the kernel's own forward (V = one-hot 128-column blocks, so
out = Pd). Comparator for the accuracy bound: _math with Pd, dS and the
outputs rounded to bf16 where the kernels round them, dot = (dP * P).sum;
bound 1.5 * e_cmp + 2^-9 * max|ref| (tests/test_attn_long_gpu.py's rule). The
head mask (keys 1..139 at -10000) is used at S = 192 and 300 only: up to
S = 140 it leaves one visible key and the bound degenerates to 0 (see there).
"""

from __future__ import annotations

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd import ops
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.ops.hiplib import check, ptr

from tests.test_attn_bwd_dbias_gpu import make_mask

D = 128
SALT = 0x5EED1234
# (B, S, h): a partial tile inside one chunk; one token past 64 (the chunk
# length) and past 128; three chunks; a partial 16-tile in the fifth chunk
SHAPES = [(1, 40, 1), (1, 65, 2), (1, 129, 1), (2, 192, 2), (2, 300, 1)]
CASES = [(B, S, h, mk, p) for (B, S, h) in SHAPES
         for mk in ("none", "random", "head", "causal") for p in (0.0, 0.1)
         if mk != "head" or S in (192, 300)]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fwd(c, qkv=None, salt=None):
    B, S, h = c["B"], c["S"], c["h"]
    out = torch.full((B, S, h, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    m = torch.full((B, h, S), float("nan"), dtype=torch.float32, device="cuda")
    lsum = torch.full_like(m, float("nan"))
    name = "sky_attn_d128_causal_fwd" if c["causal"] else "sky_attn_d128_fwd"
    masks = () if c["causal"] else (ptr(c["mask"]),)
    check(getattr(hiplib.require(), name)(
        _stream(), ptr(c["qkv"] if qkv is None else qkv), *masks, ptr(out), ptr(m),
        ptr(lsum), B, S, h, D, c["scale"], c["keep"],
        c["salt"] if salt is None else salt, c["state"]), name)
    return out, m, lsum


def _bwd(c):
    B, S, h = c["B"], c["S"], c["h"]
    dqkv = torch.full_like(c["qkv"], float("nan"))
    dot = torch.full((B * h * S,), float("nan"), dtype=torch.float32, device="cuda")
    name = "sky_attn_d128_causal_bwd" if c["causal"] else "sky_attn_d128_bwd"
    masks = () if c["causal"] else (ptr(c["mask"]),)
    check(getattr(hiplib.require(), name)(
        _stream(), ptr(c["qkv"]), ptr(c["dout"]), ptr(c["out"]), *masks, ptr(c["m"]),
        ptr(c["l"]), ptr(dot), ptr(dqkv), B, S, h, D, c["scale"], c["keep"], c["salt"],
        c["state"]), name)
    return dqkv


def _scores(c, dtype):
    """scale * Q K^T + the additive mask (causal: the lower triangle, so every
    row holds its diagonal) in dtype, [B,h,S,S]."""
    q, k = (c["qkv"][:, :, i].permute(0, 2, 1, 3).to(dtype) for i in range(2))
    s = torch.matmul(q, k.transpose(-1, -2)) * c["scale"]
    if c["causal"]:
        tri = torch.ones(c["S"], c["S"], dtype=torch.bool, device="cuda").tril()
        s = s.masked_fill(~tri, float("-inf"))
    elif c["mask"] is not None:
        s = s + c["mask"].to(dtype)
    return s


def _math(c, keepmask, rnd):
    """out, dQ, dK, dV ([B,S,h,d]) and the row logsumexp in fp64; rnd is
    applied where the kernels round to bf16 (Pd, dS, the outputs)."""
    q, k, v = (c["qkv"][:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    dO = c["dout"].permute(0, 2, 1, 3).double()
    s = _scores(c, torch.float64)
    P = torch.softmax(s, dim=-1)
    drop = keepmask.double() / c["keep"]
    Pd = rnd(P * drop)
    dP = torch.matmul(dO, v.transpose(-1, -2)) * drop
    dS = rnd(c["scale"] * P * (dP - (dP * P).sum(-1, keepdim=True)))
    res = (torch.matmul(Pd, v), torch.matmul(dS, k),
           torch.matmul(dS.transpose(-1, -2), q), torch.matmul(Pd.transpose(-1, -2), dO))
    return [rnd(x.permute(0, 2, 1, 3)) for x in res], torch.logsumexp(s, dim=-1)


def _keepmask(c):
    """The forward's keep mask, through the forward itself: with V the
    one-hot block V[k, j] = (k == 128c + j), out[q, j] = Pd[q, 128c + j]."""
    B, S, h = c["B"], c["S"], c["h"]
    nb = (S + D - 1) // D
    Pd = torch.zeros(B, h, S, D * nb, device="cuda")
    qkv = c["qkv"].clone()
    for cb in range(nb):
        qkv[:, :, 2] = 0
        n = min(D, S - D * cb)
        qkv[:, D * cb:D * cb + n, 2] = torch.eye(D, device="cuda", dtype=qkv.dtype)[:n, None]
        Pd[..., D * cb:D * cb + D] = _fwd(c, qkv)[0].permute(0, 2, 1, 3).float()
    return (Pd[..., :S] != 0).float()


@functools.lru_cache(maxsize=None)
def _case(B, S, h, mk, p):
    """Inputs, kernel results, fp64 reference and bf16 model of one case:
    computed once, shared by the tests below, never modified."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * S + 10 * h + B)
    c = dict(B=B, S=S, h=h, scale=1.0 / math.sqrt(D), keep=1.0 - p, causal=mk == "causal",
             salt=SALT if p > 0 else 0, state=F.rng_state().data_ptr())
    c["qkv"] = torch.randn(B, S, 3, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["dout"] = torch.randn(B, S, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["mask"] = make_mask(B, S, gen) if mk in ("random", "head") else None
    if mk == "head":  # m jumps by 1e4 between chunks: alpha = 0
        c["mask"][:] = 0
        c["mask"][..., 1:140] = -10000.0
    c["out"], c["m"], c["l"] = _fwd(c)
    c["dqkv"] = _bwd(c)
    keepmask = _keepmask(c) if p > 0 else torch.ones(B, h, S, S, device="cuda")
    if c["causal"]:  # Pd is zero above the diagonal whatever the draw
        keepmask = keepmask.tril()
    c["keepmask"] = keepmask
    c["ref"], c["lse"] = _math(c, keepmask, lambda x: x)
    c["model"], _ = _math(c, keepmask, lambda x: x.to(torch.bfloat16).double())
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("B,S,h,mk,p", CASES)
def test_accuracy_against_fp64(B, S, h, mk, p):
    c = _case(B, S, h, mk, p)
    got = [c["out"]] + [c["dqkv"][:, :, i] for i in range(3)]
    bad = []
    for name, new, ref, model in zip(("out", "dQ", "dK", "dV"), got, c["ref"], c["model"]):
        assert torch.isfinite(new.float()).all(), name
        e_new = (new.double() - ref).abs().max().item()
        e_cmp = (model - ref).abs().max().item()
        bound = 1.5 * e_cmp + 2.0 ** -9 * ref.abs().max().item()
        print(f"[{B},{S},{h}] mask={mk} p={p} {name}: err {e_new:.4e} model {e_cmp:.4e} "
              f"ratio {e_new / e_cmp:.3f}")
        if not e_new <= bound:
            bad.append((name, e_new, e_cmp, bound))
    assert not bad, bad


@pytest.mark.parametrize("B,S,h,mk,p", [c for c in CASES if c[4] == 0.0])
def test_row_statistics(B, S, h, mk, p):
    """m + log(l) against the fp64 logsumexp: at most 8x the error of fp32
    torch on the same bf16 inputs, plus 2^-22 |lse|. m and l do not depend on
    dropout, so p = 0 only."""
    c = _case(B, S, h, mk, p)
    e_t = (torch.logsumexp(_scores(c, torch.float32), dim=-1).double()
           - c["lse"]).abs().max().item()
    err = (c["m"].double() + c["l"].double().log() - c["lse"]).abs()
    bound = 8 * e_t + 2.0 ** -22 * c["lse"].abs()
    print(f"[{B},{S},{h}] mask={mk} lse err {err.max().item():.3e} torch fp32 {e_t:.3e} "
          f"max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


def test_rng_contract_and_shape_limits():
    """The keep mask is the d = 64 long kernels' bit for bit; same (salt,
    state): equal bits; after rng_tick() another mask; p = 0 does not read the
    salt. d = 64, S = 0, S = 4097 and causal S = 1 are rejected."""
    from tests.test_attn_long_gpu import _keepmask as keepmask_d64

    c = _case(2, 192, 2, "none", 0.1)
    c64 = dict(c, mask=None, scale=0.125)
    c64["qkv"] = c["qkv"][..., :64].contiguous()
    assert torch.equal(c["keepmask"], keepmask_d64(c64))
    assert 0.85 < c["keepmask"].mean().item() < 0.95
    assert torch.equal(_fwd(c)[0], c["out"])
    assert torch.equal(_bwd(c), c["dqkv"])
    saved = F.rng_state().clone()
    F.rng_tick()
    ticked = _fwd(c)[0]
    F.rng_state().copy_(saved)
    assert not torch.equal(ticked, c["out"])
    c0 = _case(2, 192, 2, "none", 0.0)
    assert torch.equal(_fwd(c0, salt=SALT)[0], c0["out"])
    lib = hiplib.require()
    tail = (0.125, 1.0, 0, 0)
    for S, d in ((192, 64), (0, 128), (4097, 128)):
        assert lib.sky_attn_d128_fwd(0, 1, 0, 1, 1, 1, 1, S, 1, d, *tail) != 0
        assert lib.sky_attn_d128_bwd(0, 1, 1, 1, 0, 1, 1, 1, 1, 1, S, 1, d, *tail) != 0
    for S, d in ((192, 64), (0, 128), (4097, 128), (1, 128)):
        assert lib.sky_attn_d128_causal_fwd(0, 1, 1, 1, 1, 1, S, 1, d, *tail) != 0
        assert lib.sky_attn_d128_causal_bwd(0, 1, 1, 1, 1, 1, 1, 1, 1, S, 1, d, *tail) != 0


@pytest.mark.parametrize("mk", ["none", "causal"])
def test_ops_attention_d128(monkeypatch, mk):
    """ops.attention at d = 128 under SKY_ATTN_D128=1 is FusedAttentionFn on
    the d = 128 entry points, bit for bit; under SKY_ATTN_D128=0 it is not."""
    base = _case(2, 192, 2, mk, 0.0)
    B, S, h = 2, 192, 2
    mask = None
    if mk == "none":  # a tail padding mask
        mask = torch.zeros(B, 1, 1, S, dtype=torch.bfloat16, device="cuda")
        mask[..., S - S // 5:] = -10000.0
    c = dict(base, mask=mask)
    c["out"], c["m"], c["l"] = _fwd(c)
    dqkv = _bwd(c)
    for env in ("1", "0"):
        monkeypatch.setenv("SKY_ATTN_D128", env)
        qkv = c["qkv"].clone().requires_grad_(True)
        out = ops.attention(qkv, mask, 0.0, True, causal=mk == "causal")
        node = type(out.grad_fn.next_functions[0][0]).__name__
        if env == "0":
            assert node != "FusedAttentionFnBackward"
            continue
        assert node == "FusedAttentionFnBackward"
        out.backward(c["dout"].reshape(B, S, h * D))
        assert torch.equal(out.detach(), c["out"].reshape(B, S, h * D))
        assert torch.equal(qkv.grad, dqkv)
