"""Grouped-query attention at head dim 128 (sky_attn_d128_gqa_*): out, m, l and dQ bit for bit
against the multi-head entries on eager.expand_kv's tensor with the same (salt, state), so that
case's keep mask is the grouped kernels' too; dK and dV against fp64 summed over each group, model
with Pd, dS rounded to bf16 per head, dK and dV once after the sum; test_attn_d128_gpu's bound."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd import ops
    from skycomputing_amd.ops import functions as F, hiplib
    from skycomputing_amd.ops.eager import expand_kv
    from skycomputing_amd.ops.hiplib import check, ptr

from tests.test_attn_d128_gpu import (  # noqa: F401 (the fixture is autouse here as well)
    SALT, D, _bwd, _fwd, _keepmask, _require_gpu_and_lib, _scores, _stream, make_mask,
)

# (B, S, h, h_kv): MQA, a partial tile; chunk + 1, two K/V heads; G = 3; three chunks, two groups
SHAPES = [(1, 40, 2, 1), (1, 65, 4, 2), (2, 129, 3, 1), (2, 192, 4, 2)]
CASES = [(B, S, h, kv, mk, p) for (B, S, h, kv) in SHAPES
         for mk in ("none", "random", "head", "causal") for p in (0.0, 0.1)
         if mk != "head" or S == 192]


def _gqa(c):
    B, S, h = c["B"], c["S"], c["h"]
    out = torch.full((B, S, h, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    m = torch.full((B, h, S), float("nan"), dtype=torch.float32, device="cuda")
    lsum, dot = torch.full_like(m, float("nan")), torch.full_like(m, float("nan"))
    dqkv = torch.full_like(c["qkv4"], float("nan"))
    mid = "causal_" if c["causal"] else ""
    masks = () if c["causal"] else (ptr(c["mask"]),)
    tail = (B, S, h, c["h_kv"], D, c["scale"], c["keep"], c["salt"], c["state"])
    lib = hiplib.require()
    check(getattr(lib, f"sky_attn_d128_gqa_{mid}fwd")(
        _stream(), ptr(c["qkv4"]), *masks, ptr(out), ptr(m), ptr(lsum), *tail), "gqa fwd")
    check(getattr(lib, f"sky_attn_d128_gqa_{mid}bwd")(
        _stream(), ptr(c["qkv4"]), ptr(c["dout"]), ptr(out), *masks, ptr(m), ptr(lsum),
        ptr(dot), ptr(dqkv), *tail), "gqa bwd")
    return out, m, lsum, dqkv


def _math(c, rnd):
    """out, dQ and the group sums of dK, dV in fp64; rnd where the kernels round to bf16."""
    q, k, v = (c["qkv"][:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    dO = c["dout"].permute(0, 2, 1, 3).double()
    P = torch.softmax(_scores(c, torch.float64), dim=-1)
    drop = c["keepmask"].double() / c["keep"]
    Pd = rnd(P * drop)
    dP = torch.matmul(dO, v.transpose(-1, -2)) * drop
    dS = rnd(c["scale"] * P * (dP - (dP * P).sum(-1, keepdim=True)))
    dK, dV = (x.view(c["B"], c["h_kv"], -1, c["S"], D).sum(2) for x in (
        torch.matmul(dS.transpose(-1, -2), q), torch.matmul(Pd.transpose(-1, -2), dO)))
    return [rnd(x.permute(0, 2, 1, 3)) for x in (torch.matmul(Pd, v), torch.matmul(dS, k), dK, dV)]


@functools.lru_cache(maxsize=None)
def _case(B, S, h, kv, mk, p):
    """Inputs, both kernels' results, reference and model: computed once, never modified."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * S + 10 * h + kv)
    c = dict(B=B, S=S, h=h, h_kv=kv, scale=1.0 / math.sqrt(D), keep=1.0 - p, causal=mk == "causal")
    c.update(salt=SALT if p > 0 else 0, state=F.rng_state().data_ptr())
    c["qkv4"] = torch.randn(B, S, h + 2 * kv, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["dout"] = torch.randn(B, S, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["mask"] = make_mask(B, S, gen) if mk in ("random", "head") else None
    if mk == "head":
        c["mask"][:] = 0
        c["mask"][..., 1:140] = -10000.0
    c["gqa"] = _gqa(c)
    c["qkv"] = expand_kv(c["qkv4"], kv).contiguous()
    c["out"], c["m"], c["l"] = _fwd(c)
    c["dqkv"] = _bwd(c)
    keepmask = _keepmask(c) if p > 0 else torch.ones(B, h, S, S, device="cuda")
    c["keepmask"] = keepmask.tril() if c["causal"] else keepmask
    c["ref"] = _math(c, lambda x: x)
    c["model"] = _math(c, lambda x: x.to(torch.bfloat16).double())
    c["e_cmp"] = [(mo - r).abs().max().item() for mo, r in zip(c["model"], c["ref"])]
    c["bound"] = [1.5 * e + 2.0 ** -9 * r.abs().max().item() for e, r in zip(c["e_cmp"], c["ref"])]
    return c


@pytest.mark.parametrize("B,S,h,kv,mk,p", CASES)
def test_bit_equal_to_mha_and_dk_dv_against_fp64(B, S, h, kv, mk, p):
    c = _case(B, S, h, kv, mk, p)
    out, m, lsum, dqkv = c["gqa"]
    assert torch.equal(out, c["out"]) and torch.equal(m, c["m"]) and torch.equal(lsum, c["l"])
    assert torch.equal(dqkv[:, :, :h], c["dqkv"][:, :, 0])
    bad = []
    for i, name, new in ((2, "dK", dqkv[:, :, h:h + kv]), (3, "dV", dqkv[:, :, h + kv:])):
        assert torch.isfinite(new.float()).all(), name
        e_new = (new.double() - c["ref"][i]).abs().max().item()
        print(f"[{B},{S},{h},{kv}] mask={mk} p={p} {name}: err {e_new:.4e} model "
              f"{c['e_cmp'][i]:.4e} ratio {e_new / c['e_cmp'][i]:.3f}")
        if not e_new <= c["bound"][i]:
            bad.append((name, e_new, c["e_cmp"][i], c["bound"][i]))
    assert not bad, bad


@pytest.mark.parametrize("mk", ["random", "causal"])
def test_equal_heads_is_mha(mk):
    c = dict(_case(2, 192, 4, 2, mk, 0.1), h=2, h_kv=2)
    c["qkv"] = c["qkv4"][:, :, :6].reshape(2, 192, 3, 2, D).contiguous()
    c["qkv4"] = c["qkv"].view(2, 192, 6, D)
    c["dout"] = c["dout"][:, :, :2].contiguous()
    out, m, lsum, dqkv = _gqa(c)
    c["out"], c["m"], c["l"] = _fwd(c)
    assert torch.equal(out, c["out"]) and torch.equal(m, c["m"]) and torch.equal(lsum, c["l"])
    assert torch.equal(dqkv, _bwd(c).view(2, 192, 6, D))


def test_rejections():
    """Non-zero before any launch (the pointers are dummies)."""
    lib, tail = hiplib.require(), (0.125, 1.0, 0, 0)
    bad = [(192, 2, 0, 128), (192, 3, 2, 128), (192, 2, 1, 64), (0, 2, 1, 128), (4097, 2, 1, 128)]
    for S, h, kv, d in bad:
        assert lib.sky_attn_d128_gqa_fwd(0, 1, 0, 1, 1, 1, 1, S, h, kv, d, *tail) != 0
        assert lib.sky_attn_d128_gqa_bwd(0, 1, 1, 1, 0, 1, 1, 1, 1, 1, S, h, kv, d, *tail) != 0
    for S, h, kv, d in bad + [(1, 2, 1, 128)]:
        assert lib.sky_attn_d128_gqa_causal_fwd(0, 1, 1, 1, 1, 1, S, h, kv, d, *tail) != 0
        assert lib.sky_attn_d128_gqa_causal_bwd(0, 1, 1, 1, 1, 1, 1, 1, 1, S, h, kv, d, *tail) != 0


@pytest.mark.parametrize("mk", ["random", "causal"])
def test_ops_attention_gqa(monkeypatch, mk):
    """SKY_ATTN_GQA=1: FusedGqaAttentionFn, the entry points' bits; =0: another node, in bound."""
    B, S, h, kv = 2, 192, 4, 2
    c = _case(B, S, h, kv, mk, 0.0)
    want = (c["gqa"][0].reshape(B, S, h * D), c["gqa"][3])
    for env in ("1", "0"):
        monkeypatch.setenv("SKY_ATTN_GQA", env)
        qkv = c["qkv4"].clone().requires_grad_(True)
        out = ops.attention(qkv, c["mask"], 0.0, True, causal=mk == "causal", num_kv_heads=kv)
        node = type(out.grad_fn.next_functions[0][0]).__name__
        out.backward(c["dout"].reshape(B, S, h * D))
        assert (node == "FusedGqaAttentionFnBackward") == (env == "1")
        if env == "1":
            assert torch.equal(out.detach(), want[0]) and torch.equal(qkv.grad, want[1])
            continue
        diffs = [(out.detach().double() - want[0].double()).abs().max().item()] + [
            (qkv.grad[:, :, lo:hi].double() - want[1][:, :, lo:hi].double()).abs().max().item()
            for lo, hi in ((0, h), (h, h + kv), (h + kv, h + 2 * kv))]
        print(f"mask={mk} =0 against =1 (out, dQ, dK, dV): {diffs} bounds {c['bound']}")
        assert all(d <= b for d, b in zip(diffs, c["bound"]))
