"""Segment mode of the one-chunk attention kernels (packed sequences, 2 <= S <= 128),
held to tests/test_attn_long_gpu.py's rule: fp64 _math on the dense additive mask
(-inf off segment), _math rounded to bf16 as comparator, keep mask through the forward."""

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

# (B, S, h), per-row run boundaries: the smallest S with a one-token run; a run of
# one key in a second tile, rows that differ; cuts off the tile grid in one block;
# two query blocks, a run across the block edge, a partial tile, a pad run; full size.
LAYOUTS = [
    ((1, 3, 1), [([0, 1], False)]),
    ((2, 17, 1), [([0, 16], False), ([0], False)]),
    ((2, 64, 2), [([0, 15, 16, 40], False), ([0, 33], False)]),
    ((1, 100, 1), [([0, 33, 70], True)]),
    ((2, 128, 2), [([0, 1, 65, 127], False), ([0, 32, 64, 96], False)]),
]


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _fwd(c, ids, qkv=None):
    """(out, m, l) of sky_attn_seg_fwd on ids, of sky_attn_fwd with mask = None for
    ids = None; NaN-filled before the launch."""
    B, S, h = c["B"], c["S"], c["h"]
    name = "sky_attn_fwd" if ids is None else "sky_attn_seg_fwd"
    out = c["qkv"].new_full((B, S, h, D), float("nan"))
    m, lsum = (torch.full((B, h, S), float("nan"), device="cuda") for _ in range(2))
    check(getattr(hiplib.require(), name)(
        _stream(), ptr(c["qkv"] if qkv is None else qkv), ptr(ids), ptr(out), ptr(m),
        ptr(lsum), B, S, h, D, c["scale"], c["keep"], c["salt"], c["state"]), name)
    return out, m, lsum


def _bwd(c, ids, entry="bwd"):
    """(dqkv, slabs, dbias) of sky_attn_seg_<entry> on ids, of sky_attn_<entry> with
    mask = None for ids = None; NaN-filled, the fp32 row dots in pdT's place."""
    B, S, h = c["B"], c["S"], c["h"]
    name = ("sky_attn_" if ids is None else "sky_attn_seg_") + entry
    dqkv = torch.full_like(c["qkv"], float("nan"))
    dot = torch.full((B * h * S,), float("nan"), device="cuda")
    slabs = torch.full((B * ((S + 63) // 64) * 3 * h * D,), float("nan"), device="cuda")
    dbias = torch.full((3 * h * D,), float("nan"), dtype=torch.bfloat16, device="cuda")
    args = [_stream(), ptr(c["qkv"]), ptr(c["dout"]), ptr(ids), ptr(c["m"]), ptr(c["l"]),
            ptr(dot), 0, ptr(dqkv), B, S, h, D, c["scale"], c["keep"], c["salt"], c["state"]]
    if entry != "bwd":
        args += [ptr(slabs), ptr(dbias), F._dt(dbias)]
    pending = F.PendingFinish() if entry.endswith("_parts") else None
    check(getattr(hiplib.require(), name)(*args, *([pending.slot()] if pending else [])), name)
    if pending:
        assert pending.took(slabs)
        pending.run()
    return dqkv, slabs, dbias


def _inputs(B, S, h, rows, p):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * S + 10 * h + B)
    c = dict(B=B, S=S, h=h, scale=1.0 / math.sqrt(D), keep=1.0 - p,
             salt=SALT if p > 0 else 0, state=F.rng_state().data_ptr())
    c["qkv"] = torch.randn(B, S, 3, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["dout"] = torch.randn(B, S, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["ids"] = ids_from_runs(S, rows).to("cuda", torch.int32)
    return c


@functools.lru_cache(maxsize=None)
def _case(i, p):
    (B, S, h), rows = LAYOUTS[i]
    c = _inputs(B, S, h, rows, p)
    c["out"], c["m"], c["l"] = _fwd(c, c["ids"])
    c["dqkv"] = _bwd(c, c["ids"])[0]
    same = eager.segment_mask(c["ids"], check=False)
    c["mask"] = torch.zeros(same.shape, device="cuda").masked_fill_(~same, float("-inf"))
    Pd = torch.ones(B, h, S, 64 * ((S + 63) // 64), device="cuda")
    for cb in range((S + 63) // 64 if p > 0 else 0):  # out = Pd[..., 64 cb + j]
        qkv, n = c["qkv"].clone(), min(64, S - 64 * cb)
        qkv[:, :, 2] = 0
        qkv[:, 64 * cb:64 * cb + n, 2] = torch.eye(64, device="cuda", dtype=qkv.dtype)[:n, None]
        Pd[..., 64 * cb:64 * cb + 64] = _fwd(c, c["ids"], qkv)[0].permute(0, 2, 1, 3).float()
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
    """Every row one run: the bits of sky_attn_fwd / _bwd / _bwd_dbias with mask = None."""
    c = _inputs(2, 100, 1, [([0], False), ([0], False)], p)
    c["out"], c["m"], c["l"] = dense = _fwd(c, None)
    assert all(torch.equal(a, b) for a, b in zip(_fwd(c, c["ids"]), dense))
    assert torch.equal(_bwd(c, c["ids"])[0], _bwd(c, None)[0])
    want = _bwd(c, None, "bwd_dbias")
    for entry in ("bwd_dbias", "bwd_dbias_parts"):
        assert all(torch.equal(a, b) for a, b in zip(_bwd(c, c["ids"], entry), want)), entry


def test_skipped_tiles_are_not_read(monkeypatch):
    """Three 32-aligned runs through ops.attention: NaN inputs in the middle run
    change no bit of the other two, as a visited tile (0 * NaN) would."""
    monkeypatch.setenv("SKY_ATTN_SEG_SHORT", "1")
    c = _inputs(1, 96, 1, [([0, 32, 64], False)], 0.0)
    res = []
    for poison in (False, True):
        qkv, dout = c["qkv"].clone(), c["dout"].reshape(1, 96, D).clone()
        if poison:
            qkv[:, 32:64], dout[:, 32:64] = float("nan"), float("nan")
        qkv.requires_grad_(True)
        out = ops.attention(qkv, None, 0.0, True, segment_ids=c["ids"])
        assert type(out.grad_fn.next_functions[0][0]).__name__ == "FusedAttentionFnBackward"
        out.backward(dout)
        res.append((out.detach(), qkv.grad))
    for clean, poisoned in zip(*res):
        for rows in (slice(0, 32), slice(64, 96)):
            assert torch.isfinite(clean[:, rows].float()).all()
            assert torch.equal(clean[:, rows], poisoned[:, rows])


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S,rows", [(64, LAYOUTS[2][1]), (192, [([0, 70], False), ([0], False)])])
def test_block_is_one_node(monkeypatch, S, rows, p):
    """ops.attention_block on ids: AttentionBlockFn, y bit-identical to the three-node
    composition with the same seed, every gradient inside test_node_vs_composition's
    atol = rtol = 2e-2; the _parts entries give the bits of the plain dbias entries."""
    monkeypatch.setenv("SKY_ATTN_SEG_SHORT", "1")
    base, _, dy = block_inputs(2, S, 2, False, seed=50 + S)
    ids = ids_from_runs(S, rows).cuda()

    def run():
        F.set_dropout_seed(4321)
        leaves = [t.clone().requires_grad_(True) for t in base]
        hidden, wqkv, bqkv, wo, bo, ln_w, ln_b = leaves
        y = ops.attention_block(hidden, None, wqkv, bqkv, 2, p, wo, bo, ln_w, ln_b,
                                1e-12, p, True, segment_ids=ids)
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
