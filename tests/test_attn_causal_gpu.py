"""Causal (triangle) mode of the keys-on-rows attention kernels, 2 <= S <= 4096, with and
without segment ids, held to tests/test_attn_long_gpu.py's rule: fp64 _math on the dense
additive mask (-inf above the diagonal and off segment), _math rounded to bf16 as
comparator, keep mask through the forward."""

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

from tests.test_attention_block_gpu import NAMES
from tests.test_attention_block_gpu import _inputs as block_inputs
from tests.test_attn_long_gpu import D, SALT, _math, _stream
from tests.test_attn_segments_cpu import ids_from_runs

# (B, S, h), per-row run boundaries or None for "no ids": the smallest S; one query in a
# second tile whose diagonal tile holds one key; segment cuts off the tile grid inside the
# triangle; two query blocks and a partial tile; full size; one query past the first
# chunk; an odd query block, entering its diagonal chunk at the half; a run across a chunk
# edge; five chunks.
LAYOUTS = [
    ((1, 2, 1), None),
    ((2, 17, 1), None),
    ((2, 64, 2), [([0, 15, 16, 40], False), ([0, 33], False)]),
    ((1, 100, 1), None),
    ((2, 128, 2), [([0, 1, 65, 127], False), ([0, 32, 64, 96], False)]),
    ((1, 129, 1), None),
    ((2, 192, 2), None),
    ((2, 300, 1), [([0, 130, 260], False), ([0], False)]),
    ((1, 520, 1), None),
]
WITH_IDS = (2, 7)  # one short and one long layout with ids


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _ids(c):  # the ids (and bounds) pointers of the causal entry points
    return (ptr(c["ids"]), ptr(c["bounds"]))[:2 if c["S"] > 128 else 1]


def _fwd(c, qkv=None):
    """(out, m, l) of sky_attn[_long]_causal_fwd; NaN-filled before the launch."""
    B, S, h = c["B"], c["S"], c["h"]
    name = "sky_attn_long_causal_fwd" if S > 128 else "sky_attn_causal_fwd"
    out = c["qkv"].new_full((B, S, h, D), float("nan"))
    m, lsum = (torch.full((B, h, S), float("nan"), device="cuda") for _ in range(2))
    check(getattr(hiplib.require(), name)(
        _stream(), ptr(c["qkv"] if qkv is None else qkv), *_ids(c), ptr(out), ptr(m),
        ptr(lsum), B, S, h, D, c["scale"], c["keep"], c["salt"], c["state"]), name)
    return out, m, lsum


def _bwd(c, entry="bwd", **over):
    """(dqkv, slabs, dbias) of sky_attn[_long]_causal_<entry>, NaN-filled; over replaces
    S, d or the ids pointers for the rejection test (returns the error code then)."""
    B, S, h = c["B"], c["S"], c["h"]
    name = ("sky_attn_long_causal_" if S > 128 else "sky_attn_causal_") + entry
    dqkv = torch.full_like(c["qkv"], float("nan"))
    dot = torch.full((B * h * S,), float("nan"), device="cuda")
    slabs = torch.full((B * ((S + 63) // 64) * 3 * h * D,), float("nan"), device="cuda")
    dbias = torch.full((3 * h * D,), float("nan"), dtype=torch.bfloat16, device="cuda")
    ids, tail = over.get("ids", _ids(c)), [B, over.get("S", S), h, over.get("d", D), c["scale"],
                                           c["keep"], c["salt"], c["state"]]
    if S > 128:
        args = [_stream(), ptr(c["qkv"]), ptr(c["dout"]), ptr(c["out"]), *ids, ptr(c["m"]),
                ptr(c["l"]), ptr(dot), ptr(dqkv)] + tail
    else:
        args = [_stream(), ptr(c["qkv"]), ptr(c["dout"]), *ids, ptr(c["m"]), ptr(c["l"]),
                ptr(dot), 0, ptr(dqkv)] + tail
    if entry != "bwd":
        args += [ptr(slabs), ptr(dbias), F._dt(dbias)]
    pending = F.PendingFinish() if entry.endswith("_parts") else None
    rc = getattr(hiplib.require(), name)(*args, *([pending.slot()] if pending else []))
    if over:
        return rc
    check(rc, name)
    if pending:
        assert pending.took(slabs)
        pending.run()
    return dqkv, slabs, dbias


@functools.lru_cache(maxsize=None)
def _case(i, p):
    (B, S, h), rows = LAYOUTS[i]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * S + 10 * h + B)
    c = dict(B=B, S=S, h=h, scale=1.0 / math.sqrt(D), keep=1.0 - p,
             salt=SALT if p > 0 else 0, state=F.rng_state().data_ptr(), ids=None, bounds=None)
    c["qkv"] = torch.randn(B, S, 3, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["dout"] = torch.randn(B, S, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    vis = eager.causal_mask(S, "cuda")
    if rows is not None:
        c["ids"] = ids_from_runs(S, rows).to("cuda", torch.int32)
        c["bounds"] = F.attn_seg_bounds(c["ids"]) if S > 128 else None
        vis = vis & eager.segment_mask(c["ids"], check=False)
    c["out"], c["m"], c["l"] = _fwd(c)
    c["dqkv"] = _bwd(c)[0]
    c["mask"] = torch.zeros(vis.shape, device="cuda").masked_fill_(~vis, float("-inf"))
    Pd = torch.ones(B, h, S, 64 * ((S + 63) // 64), device="cuda")
    for cb in range((S + 63) // 64 if p > 0 else 0):  # out = Pd[..., 64 cb + j]
        qkv, n = c["qkv"].clone(), min(64, S - 64 * cb)
        qkv[:, :, 2] = 0
        qkv[:, 64 * cb:64 * cb + n, 2] = torch.eye(64, device="cuda", dtype=qkv.dtype)[:n, None]
        Pd[..., 64 * cb:64 * cb + 64] = _fwd(c, qkv)[0].permute(0, 2, 1, 3).float()
    keepmask = (Pd[..., :S] != 0).float()
    c["ref"], c["lse"] = _math(c, keepmask, lambda x: x)
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


@pytest.mark.parametrize("i", range(len(LAYOUTS)))
def test_row_statistics(i):
    """m + log(l) against the fp64 logsumexp by tests/test_attn_long_gpu.py's rule: at most
    8x the error of fp32 torch on the same inputs, plus 2^-22 |lse|."""
    c = _case(i, 0.0)
    q, k = (c["qkv"][:, :, j].permute(0, 2, 1, 3).float() for j in range(2))
    s32 = torch.matmul(q, k.transpose(-1, -2)) * c["scale"] + c["mask"]
    e_t = (torch.logsumexp(s32, dim=-1).double() - c["lse"]).abs().max().item()
    err = (c["m"].double() + c["l"].double().log() - c["lse"]).abs()
    bound = 8 * e_t + 2.0 ** -22 * c["lse"].abs()
    print(f"{LAYOUTS[i][0]} lse err {err.max().item():.3e} torch fp32 {e_t:.3e} "
          f"max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("S,cut", [(96, 64), (384, 256)])
def test_skipped_tiles_and_chunks_are_not_read(monkeypatch, S, cut):
    """NaN in K and V of the tokens from cut on changes no bit of out and dQ of the rows
    before it, as a visited tile or chunk (0 * NaN) would."""
    monkeypatch.setenv("SKY_ATTN_CAUSAL", "1")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(S)
    base = torch.randn(1, S, 3, 1, D, device="cuda", generator=gen).to(torch.bfloat16)
    dout = torch.randn(1, S, D, device="cuda", generator=gen).to(torch.bfloat16)
    res = []
    for poison in (False, True):
        qkv = base.clone()
        if poison:
            qkv[:, cut:, 1:] = float("nan")
        qkv.requires_grad_(True)
        out = ops.attention(qkv, None, 0.0, True, causal=True)
        assert type(out.grad_fn.next_functions[0][0]).__name__ == "FusedAttentionFnBackward"
        out.backward(dout)
        res.append((out.detach()[:, :cut], qkv.grad[:, :cut, 0]))
    for clean, poisoned in zip(*res):
        assert torch.isfinite(clean.float()).all() and torch.equal(clean, poisoned)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("i", WITH_IDS)
def test_entry_points(i, p):
    """The three backward entries give one dqkv; NaN-filled slabs and dbias end finite;
    _parts gives the bits of the plain dbias entry; bad shapes and pointers are rejected."""
    c = _case(i, p)
    plain, parts = _bwd(c, "bwd_dbias"), _bwd(c, "bwd_dbias_parts")
    assert torch.equal(plain[0], c["dqkv"])
    assert all(torch.isfinite(t.float()).all() for t in plain)
    assert all(torch.equal(a, b) for a, b in zip(plain, parts))
    bad = [dict(d=32), dict(S=129 if c["S"] <= 128 else 128), dict(S=1 if c["S"] <= 128 else 4097)]
    if c["S"] > 128:
        bad += [dict(ids=(ptr(c["ids"]), 0)), dict(ids=(0, ptr(c["bounds"])))]
    for over in bad:
        for entry in ("bwd", "bwd_dbias", "bwd_dbias_parts"):
            assert _bwd(c, entry, **over) != 0, (entry, over)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S,rows", [(64, LAYOUTS[2][1]), (192, None)])
def test_block_is_one_node(monkeypatch, S, rows, p):
    """ops.attention_block(causal=True): AttentionBlockFn, y bit-identical to the three-node
    composition with the same seed, every gradient inside test_node_vs_composition's
    atol = rtol = 2e-2; the merged and the plain finish give the same bits."""
    monkeypatch.setenv("SKY_ATTN_CAUSAL", "1")
    base, _, dy = block_inputs(2, S, 2, False, seed=60 + S)
    ids = ids_from_runs(S, rows).cuda() if rows else None

    def run():
        F.set_dropout_seed(4321)
        leaves = [t.clone().requires_grad_(True) for t in base]
        hidden, wqkv, bqkv, wo, bo, ln_w, ln_b = leaves
        y = ops.attention_block(hidden, None, wqkv, bqkv, 2, p, wo, bo, ln_w, ln_b,
                                1e-12, p, True, segment_ids=ids, causal=True)
        y.backward(dy)
        return y.detach(), [t.grad for t in leaves], type(y.grad_fn).__name__

    y_n, g_n, node_n = run()
    monkeypatch.setenv("SKY_NO_MERGED_FINISH", "1")
    _, g_plain, _ = run()
    monkeypatch.setenv("SKY_NO_ATTN_BLOCK", "1")
    y_c, g_c, node_c = run()
    assert node_n == "AttentionBlockFnBackward"
    assert node_c == "LinearResidualLayerNormFnBackward"
    assert torch.equal(y_n, y_c)
    for name, a, plain, b in zip(NAMES, g_n, g_plain, g_c):
        print(f"S={S} p={p} {name}: max abs diff {(a.float() - b.float()).abs().max().item():.3e}")
        assert torch.equal(a, plain), name
        assert torch.allclose(a.float(), b.float(), atol=2e-2, rtol=2e-2), name
