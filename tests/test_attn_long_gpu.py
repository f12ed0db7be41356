"""The long-sequence attention kernels (ops/hip/attention_long.hip,
128 < S <= 4096): forward with per-lane online softmax over 128-key chunks,
dQ with dot = dO . O, dK/dV with the accumulators in registers.

Reference: the same mathematics in fp64 (_math with no rounding), keep mask
recovered through the kernel's own forward (V = one-hot 64-column blocks, so
out = Pd). Comparator for the accuracy bound: _math with Pd, dS and the
outputs rounded to bf16 where the kernels round them; bound
1.5 * e_cmp + 2^-9 * max|ref| (tests/test_attn_krows_gpu.py's rule).

One parameter set is degenerate, (1, 129, 1) with the head mask: key 0 is the
only visible key, P is one-hot, dS and the fp64 dQ and dK are exactly 0, and
so are the model's: the bound is 0. At p = 0 the kernels meet it to the bit.
At p = 0.1 they cannot: dot is specified as dO . O over the stored bf16 O,
here bf16(v0 / keep), so dP - dot is that rounding times |dO . O| ~ 10
(max|dK| 5.6e-02 to 8.1e-02 measured, by the mask drawn) where sum dP * P
cancels exactly. For this
parameter set alone the model takes dot as the kernels do, dO . bf16(O), and
then shows the same figure (ratio 1.000); every other case is held to the model above.
"""

from __future__ import annotations

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

from tests.test_attn_bwd_dbias_gpu import make_mask

D = 64
SALT = 0x5EED1234
# (B, S, h): one key / one query past the first chunk and block; a half
# chunk, three query blocks; two full chunks; a partial 16-tile in the third
# chunk, five blocks; three chunks; five chunks with NC = 9.
SHAPES = [(1, 129, 1), (2, 192, 2), (1, 256, 2), (2, 300, 1), (1, 384, 1), (1, 520, 1)]
CASES = [(B, S, h, mk, p) for (B, S, h) in SHAPES
         for mk in ("none", "random", "tail", "head") for p in (0.0, 0.1)]


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
    check(hiplib.require().sky_attn_long_fwd(
        _stream(), ptr(c["qkv"] if qkv is None else qkv), ptr(c["mask"]), ptr(out),
        ptr(m), ptr(lsum), B, S, h, D, c["scale"], c["keep"],
        c["salt"] if salt is None else salt, c["state"]), "sky_attn_long_fwd")
    return out, m, lsum


def _bwd(c, entry="sky_attn_long_bwd"):
    """One of the three backward entry points on NaN-filled buffers:
    (dqkv, slabs, dbias), the last two None for the plain entry."""
    B, S, h = c["B"], c["S"], c["h"]
    lib = hiplib.require()
    dqkv = torch.full_like(c["qkv"], float("nan"))
    dot = torch.full((B * h * S,), float("nan"), dtype=torch.float32, device="cuda")
    args = list(F._attn_long_bwd_args(c["qkv"], c["dout"], c["out"], c["mask"], c["m"],
                                      c["l"], dot, dqkv, c["scale"], c["keep"], c["salt"]))
    if entry == "sky_attn_long_bwd":
        check(lib.sky_attn_long_bwd(*args), entry)
        return dqkv, None, None
    slabs = torch.full((B * ((S + 63) // 64) * 3 * h * D,), float("nan"),
                       dtype=torch.float32, device="cuda")
    dbias = torch.full((3 * h * D,), float("nan"), dtype=torch.bfloat16, device="cuda")
    args += [ptr(slabs), ptr(dbias), F._dt(dbias)]
    if entry == "sky_attn_long_bwd_dbias":
        check(lib.sky_attn_long_bwd_dbias(*args), entry)
    else:
        pending = F.PendingFinish()
        check(lib.sky_attn_long_bwd_dbias_parts(*args, pending.slot()), entry)
        assert pending.took(slabs)
        pending.run()
    return dqkv, slabs, dbias


def _math(c, keepmask, rnd, dot_from_out=False):
    """out, dQ, dK, dV ([B,S,h,d]) and the row logsumexp in fp64; rnd is
    applied where the kernels round to bf16 (Pd, dS, the outputs)."""
    q, k, v = (c["qkv"][:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    dO = c["dout"].permute(0, 2, 1, 3).double()
    s = torch.matmul(q, k.transpose(-1, -2)) * c["scale"]
    if c["mask"] is not None:
        s = s + c["mask"].double()
    P = torch.softmax(s, dim=-1)
    drop = keepmask.double() / c["keep"]
    Pd = rnd(P * drop)
    dP = torch.matmul(dO, v.transpose(-1, -2)) * drop
    out = torch.matmul(Pd, v)
    dot = (dO * rnd(out)).sum(-1, keepdim=True) if dot_from_out else (dP * P).sum(-1, keepdim=True)
    dS = rnd(c["scale"] * P * (dP - dot))
    res = (out, torch.matmul(dS, k),
           torch.matmul(dS.transpose(-1, -2), q), torch.matmul(Pd.transpose(-1, -2), dO))
    return [rnd(x.permute(0, 2, 1, 3)) for x in res], torch.logsumexp(s, dim=-1)


def _keepmask(c):
    """The forward's keep mask, through the forward itself: with V the
    one-hot block V[k, j] = (k == 64c + j), out[q, j] = Pd[q, 64c + j]."""
    B, S, h = c["B"], c["S"], c["h"]
    Pd = torch.zeros(B, h, S, 64 * ((S + 63) // 64), device="cuda")
    qkv = c["qkv"].clone()
    for cb in range((S + 63) // 64):
        qkv[:, :, 2] = 0
        n = min(64, S - 64 * cb)
        qkv[:, 64 * cb:64 * cb + n, 2] = torch.eye(64, device="cuda", dtype=qkv.dtype)[:n, None]
        Pd[..., 64 * cb:64 * cb + 64] = _fwd(c, qkv)[0].permute(0, 2, 1, 3).float()
    return (Pd[..., :S] != 0).float()


@functools.lru_cache(maxsize=None)
def _case(B, S, h, mk, p):
    """Inputs, kernel results, fp64 reference and bf16 model of one case:
    computed once, shared by the tests below, never modified."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * S + 10 * h + B)
    c = dict(B=B, S=S, h=h, scale=1.0 / math.sqrt(D), keep=1.0 - p,
             salt=SALT if p > 0 else 0, state=F.rng_state().data_ptr())
    c["qkv"] = torch.randn(B, S, 3, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["dout"] = torch.randn(B, S, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["mask"] = make_mask(B, S, gen) if mk != "none" else None
    if mk == "tail":    # padding: the last 140 keys, a whole chunk masked (S = 129: all)
        c["mask"][:] = 0
        c["mask"][..., max(0, S - 140):] = -10000.0
    elif mk == "head":  # m jumps by 1e4 between chunks: alpha = 0
        c["mask"][:] = 0
        c["mask"][..., 1:140] = -10000.0
    c["out"], c["m"], c["l"] = _fwd(c)
    c["dqkv"], _, _ = _bwd(c)
    keepmask = _keepmask(c) if p > 0 else torch.ones(B, h, S, S, device="cuda")
    c["ref"], c["lse"] = _math(c, keepmask, lambda x: x)
    one_key = mk == "head" and S <= 140  # the degenerate set of the module docstring
    c["model"], _ = _math(c, keepmask, lambda x: x.to(torch.bfloat16).double(), one_key)
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
        ratio = e_new / e_cmp if e_cmp > 0 else float(e_new > 0)  # one visible key: exact
        print(f"[{B},{S},{h}] mask={mk} p={p} {name}: err {e_new:.4e} model {e_cmp:.4e} "
              f"ratio {ratio:.3f}")
        if not e_new <= bound:
            bad.append((name, e_new, e_cmp, bound))
    assert not bad, bad


@pytest.mark.parametrize("B,S,h,mk,p", [c for c in CASES if c[4] == 0.0])
def test_row_statistics(B, S, h, mk, p):
    """m + log(l) against the fp64 logsumexp: at most 8x the error of fp32
    torch on the same bf16 inputs, plus 2^-22 |lse|. m and l do not depend on
    dropout, so p = 0 only."""
    c = _case(B, S, h, mk, p)
    q, k = (c["qkv"][:, :, i].permute(0, 2, 1, 3).float() for i in range(2))
    s32 = torch.matmul(q, k.transpose(-1, -2)) * c["scale"]
    if c["mask"] is not None:
        s32 = s32 + c["mask"].float()
    e_t = (torch.logsumexp(s32, dim=-1).double() - c["lse"]).abs().max().item()
    err = (c["m"].double() + c["l"].double().log() - c["lse"]).abs()
    bound = 8 * e_t + 2.0 ** -22 * c["lse"].abs()
    print(f"[{B},{S},{h}] mask={mk} p={p} lse err {err.max().item():.3e} torch fp32 "
          f"{e_t:.3e} max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("B,S,h,mk,p", CASES)
def test_entry_points_and_dbias(B, S, h, mk, p):
    """The three backward entries give one dqkv; NaN-filled slabs and dbias
    end finite; dbias is the column sum of dqkv as stored."""
    c = _case(B, S, h, mk, p)
    rows = c["dqkv"].float().view(B * S, 3 * h * D)
    ref = rows.sum(0)
    bound = 2.0 ** -7 * ref.abs() + 1e-4 * rows.abs().sum(0)
    for entry in ("sky_attn_long_bwd_dbias", "sky_attn_long_bwd_dbias_parts"):
        dqkv, slabs, dbias = _bwd(c, entry)
        torch.cuda.synchronize()
        assert torch.isfinite(slabs).all(), f"{entry}: slab element left unwritten"
        assert torch.equal(dqkv, c["dqkv"]), f"{entry}: dqkv differs from sky_attn_long_bwd"
        err = (dbias.float() - ref).abs()
        print(f"[{B},{S},{h}] mask={mk} p={p} {entry}: max err/bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all(), (entry, (err / bound).max().item())


def test_rng_contract_and_shape_limits():
    """Same (salt, state): equal bits; after rng_tick() another mask; p = 0
    does not read the salt. S <= 128, S > 4096 and d != 64 are rejected."""
    c = _case(2, 192, 2, "random", 0.1)
    assert torch.equal(_fwd(c)[0], c["out"])
    assert torch.equal(_bwd(c)[0], c["dqkv"])
    saved = F.rng_state().clone()
    F.rng_tick()
    ticked = _fwd(c)[0]
    F.rng_state().copy_(saved)
    assert not torch.equal(ticked, c["out"])
    c0 = _case(2, 192, 2, "random", 0.0)
    assert torch.equal(_fwd(c0, salt=SALT)[0], c0["out"])
    lib = hiplib.require()
    for S, d in ((128, 64), (4097, 64), (192, 32)):
        assert lib.sky_attn_long_fwd(0, 1, 0, 1, 1, 1, 1, S, 1, d, 0.125, 1.0, 0, 0) != 0
        assert lib.sky_attn_long_bwd(0, 1, 1, 1, 0, 1, 1, 1, 1, 1, S, 1, d, 0.125, 1.0, 0, 0) != 0


def test_block_node_long(monkeypatch):
    """ops.attention_block at S = 192 under SKY_ATTN_LONG=1: one node, y
    bit-identical to the three-node composition with the same seed, every
    gradient inside tests/test_attention_block_gpu.py's atol = rtol = 2e-2."""
    from tests.test_attention_block_gpu import NAMES, _inputs, _run

    base, mask, dy = _inputs(2, 192, 2, True, seed=50 + 192)
    monkeypatch.setenv("SKY_ATTN_LONG", "1")
    y_n, g_n, node_n = _run(base, mask, dy, 2, 0.1)
    monkeypatch.setenv("SKY_NO_ATTN_BLOCK", "1")
    y_c, g_c, node_c = _run(base, mask, dy, 2, 0.1)
    assert node_n == "AttentionBlockFnBackward"
    assert node_c == "LinearResidualLayerNormFnBackward"
    assert torch.equal(y_n, y_c)
    for name, a, b in zip(NAMES, g_n, g_c):
        err = (a.float() - b.float()).abs().max().item()
        print(f"{name}: max abs diff {err:.3e}")
        assert torch.allclose(a.float(), b.float(), atol=2e-2, rtol=2e-2), (name, err)


def test_ops_attention_long(monkeypatch):
    """ops.attention at S = 192 under SKY_ATTN_LONG=1 runs FusedAttentionFn;
    tolerances of test_attention_sdpa_dispatch_long_seq."""
    torch.manual_seed(22)
    B, S, h = 2, 192, 4
    qkv = torch.randn(B, S, 3, h, D, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    mask = torch.zeros(B, 1, 1, S, dtype=torch.bfloat16, device="cuda")
    mask[..., S - S // 5:] = -10000.0
    monkeypatch.setenv("SKY_ATTN_LONG", "1")
    out = ops.attention(qkv, mask, 0.0, True)
    assert type(out.grad_fn.next_functions[0][0]).__name__ == "FusedAttentionFnBackward"
    dout = torch.randn_like(out)
    out.backward(dout)
    qf = qkv.detach().float().requires_grad_(True)
    q, k, v = F._split_heads(qf)
    ref = eager.attention_context(q, k, v, mask.float()).permute(0, 2, 1, 3).reshape(B, S, h * D)
    ref.backward(dout.float())
    assert torch.allclose(out.float(), ref, atol=6e-2, rtol=6e-2)
    assert torch.allclose(qkv.grad.float(), qf.grad, atol=8e-2, rtol=8e-2)
