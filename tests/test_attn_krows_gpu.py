"""The keys-on-rows attention kernels (attn_fwd_krows_kernel,
attn_bwd_dq_krows_kernel, attn_bwd_dkv_krows_kernel): P and dS stay in the
registers one MFMA left them in and feed the next MFMA as its B operand.

Reference: an fp64 eager composition with the keep mask recovered from
sky_attn_probs (Pd != 0). Comparator: the kernels they replace by default,
on the same inputs and salt (SKY_ATTN_KROWS=0). Both round P, dS and every
output to bf16 at the same points, so their errors against fp64 should be
equal in distribution: the new kernels' max |err| may be at most 1.5x the
comparator's (the maximum of a few thousand samples moving between two
summation orders) plus 2^-9 * max|ref| (half a bf16 ulp of the largest
value). A kernel that drew a different dropout mask misses on most elements.
"""

from __future__ import annotations

import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.ops.hiplib import check, ptr

from tests.test_attn_bwd_dbias_gpu import make_mask

D = 64
SALT = 0x5EED1234


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


# (B, S, h): full tiles; a single 64 block (QB = 1); a second block with one
# row; partial 16-tiles (100 with two blocks, 48 with one, 17 with one row in
# its second tile); one tile; the smallest S the dot hand-off through the
# pdT scratch serves; the S = 1 fallback to the old pair.
SHAPES = [(2, 128, 2), (2, 64, 2), (2, 65, 1), (3, 100, 2), (1, 48, 1),
          (1, 17, 1), (1, 16, 1), (1, 2, 1), (1, 1, 1)]

CASES = [(B, S, h, masked, p) for (B, S, h) in SHAPES
         for masked in (False, True) for p in (0.0, 0.1)]


class _Env:
    """SKY_ATTN_KROWS for the calls inside; the kernels read it at launch."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("SKY_ATTN_KROWS")
        if self.value is None:
            os.environ.pop("SKY_ATTN_KROWS", None)
        else:
            os.environ["SKY_ATTN_KROWS"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("SKY_ATTN_KROWS", None)
        else:
            os.environ["SKY_ATTN_KROWS"] = self.old


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fwd(c):
    B, S, h = c["B"], c["S"], c["h"]
    out = torch.full((B, S, h, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    m = torch.full((B, h, S), float("nan"), dtype=torch.float32, device="cuda")
    lsum = torch.full_like(m, float("nan"))
    check(hiplib.require().sky_attn_fwd(
        _stream(), ptr(c["qkv"]), ptr(c["mask"]), ptr(out), ptr(m), ptr(lsum),
        B, S, h, D, c["scale"], c["keep"], c["salt"], c["state"]), "sky_attn_fwd")
    return out, m, lsum


def _nan_scratch(c):
    """pdT, dsT with their B*h*S*S elements NaN; the zero tail that bwd2's
    last fragment load runs into (F._attn_bwd_scratch) stays zero."""
    pdT, dsT = F._attn_bwd_scratch(c["qkv"])
    n = c["B"] * c["h"] * c["S"] ** 2
    pdT[:n] = float("nan")
    dsT[:n] = float("nan")
    return pdT, dsT


def _bwd_args(c, m, lsum, pdT, dsT, dqkv):
    return [_stream(), ptr(c["qkv"]), ptr(c["dout"]), ptr(c["mask"]), ptr(m),
            ptr(lsum), ptr(pdT), ptr(dsT), ptr(dqkv), c["B"], c["S"], c["h"], D,
            c["scale"], c["keep"], c["salt"], c["state"]]


def _bwd(c, m, lsum, nan_scratch=False):
    pdT, dsT = _nan_scratch(c) if nan_scratch else F._attn_bwd_scratch(c["qkv"])
    dqkv = torch.full_like(c["qkv"], float("nan"))
    check(hiplib.require().sky_attn_bwd(*_bwd_args(c, m, lsum, pdT, dsT, dqkv)),
          "sky_attn_bwd")
    return dqkv, pdT, dsT


def _reference(c, keepmask):
    x = c["qkv"].double().requires_grad_(True)
    q = x[:, :, 0].permute(0, 2, 1, 3)
    k = x[:, :, 1].permute(0, 2, 1, 3)
    v = x[:, :, 2].permute(0, 2, 1, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) * c["scale"]
    if c["mask"] is not None:
        s = s + c["mask"].double()
    pd = torch.softmax(s, dim=-1) * keepmask.double() / c["keep"]
    out = torch.matmul(pd, v).permute(0, 2, 1, 3)
    out.backward(c["dout"].double())
    return out.detach(), x.grad


_cache: dict = {}


def _case(B, S, h, masked, p):
    """Inputs, the fp64 reference and both kernel generations' results for one
    case: computed once, shared by the tests below, never modified."""
    key = (B, S, h, masked, p)
    if key in _cache:
        return _cache[key]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * S + 10 * h + B)
    c = dict(B=B, S=S, h=h, scale=1.0 / math.sqrt(D), keep=1.0 - p,
             salt=SALT if p > 0 else 0, state=F.rng_state().data_ptr())
    c["qkv"] = torch.randn(B, S, 3, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["dout"] = torch.randn(B, S, h, D, device="cuda", generator=gen).to(torch.bfloat16)
    c["mask"] = make_mask(B, S, gen) if masked else None
    with _Env("0"):
        c["old_out"], c["old_m"], c["old_l"] = _fwd(c)
        c["old_dqkv"], _, _ = _bwd(c, c["old_m"], c["old_l"])
        keepmask = torch.ones(B, h, S, S, device="cuda")
        if p > 0:
            P = torch.empty(B, h, S, S, dtype=torch.bfloat16, device="cuda")
            Pd = torch.empty_like(P)
            check(hiplib.require().sky_attn_probs(
                _stream(), ptr(c["qkv"]), ptr(c["mask"]), ptr(c["old_m"]),
                ptr(c["old_l"]), ptr(P), ptr(Pd), B, S, h, D, c["scale"],
                c["keep"], c["salt"], c["state"]), "sky_attn_probs")
            keepmask = (Pd != 0).float()
    with _Env(None):
        c["new_out"], c["new_m"], c["new_l"] = _fwd(c)
        c["new_dqkv"], _, _ = _bwd(c, c["new_m"], c["new_l"])
    with _Env("2"):  # the forward with one block per (b, h, 128 queries)
        c["wide_out"], c["wide_m"], c["wide_l"] = _fwd(c)
    c["ref_out"], c["ref_dqkv"] = _reference(c, keepmask)
    torch.cuda.synchronize()
    _cache[key] = c
    return c


def test_mfma_chain():
    """Two stacked D tiles of one MFMA, packed by att_pack_dpair, are the B
    operand of the next, with the A operand read by abf_tr_rows64_2.
    Small-integer data: D (|.| <= 128) is exact in bf16 and every sum is exact
    in fp32, so the chain must give A2 @ (A @ B) to the bit; the matrices are
    random, hence asymmetric, and a wrong slot order misses almost everywhere."""
    g = torch.Generator().manual_seed(7)
    A = torch.randint(-2, 3, (32, 32), generator=g).float()
    Bm = torch.randint(-2, 3, (32, 16), generator=g).float()
    A2 = torch.randint(-3, 4, (16, 32), generator=g).float()
    D2 = torch.full((16, 16), float("nan"), dtype=torch.float32, device="cuda")
    dev = [t.to(torch.bfloat16).cuda().contiguous() for t in (A, Bm, A2)]
    check(hiplib.require().sky_mfma_chain_probe(
        _stream(), ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), D2.data_ptr()), "chain")
    torch.cuda.synchronize()
    ref = A2 @ (A @ Bm)
    assert (A @ Bm).abs().max() <= 256
    assert torch.equal(D2.cpu(), ref), (D2.cpu() - ref).abs().max()


@pytest.mark.parametrize("B,S,h,masked,p", CASES)
def test_accuracy_against_fp64(B, S, h, masked, p):
    c = _case(B, S, h, masked, p)
    parts = [("out", c["new_out"], c["old_out"], c["ref_out"]),
             ("out(128q)", c["wide_out"], c["old_out"], c["ref_out"])]
    for i, name in enumerate(("dQ", "dK", "dV")):
        parts.append((name, c["new_dqkv"][:, :, i], c["old_dqkv"][:, :, i],
                      c["ref_dqkv"][:, :, i]))
    bad = []
    for name, new, old, ref in parts:
        assert torch.isfinite(new.float()).all(), name
        e_new = (new.double() - ref).abs().max().item()
        e_old = (old.double() - ref).abs().max().item()
        bound = 1.5 * e_old + 2.0 ** -9 * ref.abs().max().item()
        ratio = e_new / e_old if e_old > 0 else float(e_new > 0)
        print(f"[{B},{S},{h}] mask={masked} p={p} {name}: new {e_new:.4e} "
              f"old {e_old:.4e} ratio {ratio:.3f} bound {bound:.4e}")
        if not e_new <= bound:
            bad.append((name, e_new, e_old, bound))
    assert not bad, bad


@pytest.mark.parametrize("B,S,h,masked,p", CASES)
def test_row_statistics(B, S, h, masked, p):
    """m: a maximum has no order, so the bits are the old forward's. l: the
    sum order over S positive terms differs, 8 * 2^-24 * sqrt(S) relative."""
    c = _case(B, S, h, masked, p)
    bound = 8 * 2.0 ** -24 * math.sqrt(S)
    for tag in ("new", "wide"):  # wide: SKY_ATTN_KROWS=2, 128 queries per block
        assert torch.equal(c[tag + "_m"].view(torch.int32), c["old_m"].view(torch.int32)), tag
        rel = ((c[tag + "_l"] - c["old_l"]).abs() / c["old_l"]).max().item()
        print(f"[{B},{S},{h}] mask={masked} p={p} {tag} l rel diff {rel:.3e} bound {bound:.3e}")
        assert rel <= bound, tag


@pytest.mark.parametrize("B,S,h,masked,p", CASES)
def test_entry_points_and_dbias(B, S, h, masked, p):
    """sky_attn_bwd, sky_attn_bwd_dbias and sky_attn_bwd_dbias_parts +
    sky_colsum_finish give one dqkv; slabs and dbias start NaN-filled and every
    element is written; dbias is the column sum of dqkv as stored."""
    lib = hiplib.require()
    c = _case(B, S, h, masked, p)
    want = c["new_dqkv"]
    QB = (S + 63) // 64
    rows = want.float().view(B * S, 3 * h * D)
    ref = rows.sum(0)
    bound = 2.0 ** -7 * ref.abs() + 1e-4 * rows.abs().sum(0)
    for entry in ("dbias", "parts"):
        pdT, dsT = F._attn_bwd_scratch(c["qkv"])
        dqkv = torch.full_like(c["qkv"], float("nan"))
        slabs = torch.full((B * QB * 3 * h * D,), float("nan"), dtype=torch.float32,
                           device="cuda")
        dbias = torch.full((3 * h * D,), float("nan"), dtype=torch.bfloat16, device="cuda")
        args = _bwd_args(c, c["new_m"], c["new_l"], pdT, dsT, dqkv) + [
            ptr(slabs), ptr(dbias), F._dt(dbias)]
        if entry == "dbias":
            check(lib.sky_attn_bwd_dbias(*args), "sky_attn_bwd_dbias")
        else:
            pending = F.PendingFinish()
            check(lib.sky_attn_bwd_dbias_parts(*args, pending.slot()),
                  "sky_attn_bwd_dbias_parts")
            assert pending.took(slabs)
            pending.run()
        torch.cuda.synchronize()
        assert torch.isfinite(slabs).all(), f"{entry}: slab element left unwritten"
        assert torch.equal(dqkv, want), f"{entry}: dqkv differs from sky_attn_bwd"
        err = (dbias.float() - ref).abs()
        print(f"[{B},{S},{h}] mask={masked} p={p} {entry}: max |dbias - ref| "
              f"{err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all(), (entry, (err / bound).max().item())


@pytest.mark.parametrize("B,S,h", [(2, 128, 2), (2, 65, 1), (1, 2, 1)])
def test_switch_and_scratch(B, S, h):
    """SKY_ATTN_KROWS=0 runs the old pair: the NaN-filled pdT and dsT end
    finite, and a second run has the same bits. By default nothing but the
    dot values (fp32 [B*h*S] at the head of pdT) is written.

    This shows which kernels ran and that they are deterministic. That the
    switch gives the PARENT's bits (forward and backward) cannot be shown
    from inside one build: it is the bench.py --dump-outputs comparison
    against the parent build recorded in profiles/r11_notes.md."""
    c = _case(B, S, h, True, 0.1)
    n = B * h * S * S
    with _Env("0"):
        dqkv, pdT, dsT = _bwd(c, c["old_m"], c["old_l"], nan_scratch=True)
        torch.cuda.synchronize()
        assert torch.isfinite(pdT[:n].float()).all() and torch.isfinite(dsT[:n].float()).all()
        assert torch.equal(dqkv, c["old_dqkv"])
    with _Env(None):
        dqkv, pdT, dsT = _bwd(c, c["new_m"], c["new_l"], nan_scratch=True)
        torch.cuda.synchronize()
        assert torch.equal(dqkv, c["new_dqkv"])
        ndot = B * h * S  # fp32 values = 2 * ndot bf16 slots
        assert torch.isfinite(pdT[:2 * ndot].view(torch.float32)).all()
        assert torch.isnan(pdT[2 * ndot:n].float()).all()
        assert torch.isnan(dsT[:n].float()).all()


def test_s1_runs_the_old_pair():
    """S = 1: the scratch cannot hold dot, the entry points run bwd1s + bwd2,
    which write pdT and dsT."""
    c = _case(1, 1, 1, False, 0.0)
    with _Env(None):
        dqkv, pdT, dsT = _bwd(c, c["new_m"], c["new_l"], nan_scratch=True)
        torch.cuda.synchronize()
    assert torch.isfinite(pdT[:1].float()).all() and torch.isfinite(dsT[:1].float()).all()
    assert torch.equal(dqkv, c["old_dqkv"])
