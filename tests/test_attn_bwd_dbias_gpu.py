"""sky_attn_bwd_dbias: the two-kernel attention backward that also returns
the column sums of dqkv (the qkv linear's bias gradient) from the kernels'
registers. Checked against sky_attn_bwd on the same inputs and salt: dqkv
must not change by a bit, and dbias must be the column sum of dqkv as
stored.
"""

from __future__ import annotations

import math

import pytest
import torch

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


# (B, S, h): full tiles; one q block; a second q block that holds one row
# (three of its waves inactive); partial 32-q blocks in bwd2 (S = 100 with
# two q blocks, S = 48 with one); a single 16-row tile.
SHAPES = [(2, 128, 2), (2, 64, 2), (2, 65, 1), (3, 100, 2), (1, 48, 1), (1, 16, 1)]


def make_mask(B, S, gen):
    """Additive [B, 1, 1, S] bf16 mask, about a quarter of the keys masked,
    key 0 always visible."""
    drop = torch.rand(B, S, device="cuda", generator=gen) < 0.25
    drop[:, 0] = False
    return (drop.float() * -10000.0).to(torch.bfloat16).view(B, 1, 1, S)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,S,h", SHAPES)
def test_dbias_matches_plain_backward(B, S, h, masked, p):
    lib = hiplib.require()
    d = 64
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 * S + 10 * h + B)
    qkv = torch.randn(B, S, 3, h, d, device="cuda", generator=gen).to(torch.bfloat16)
    dout = torch.randn(B, S, h, d, device="cuda", generator=gen).to(torch.bfloat16)
    mask = make_mask(B, S, gen) if masked else None
    scale = 1.0 / math.sqrt(d)
    keep = 1.0 - p
    F.set_dropout_seed(77)
    _, m, lsum, salt = F._attn_fwd(qkv, mask, scale, keep)
    assert (salt != 0) == (p > 0)
    stream = torch.cuda.current_stream().cuda_stream
    state = F.rng_state().data_ptr()

    def run(with_dbias):
        pdT, dsT = F._attn_bwd_scratch(qkv)
        dqkv = torch.full_like(qkv, float("nan"))
        args = [stream, ptr(qkv), ptr(dout), ptr(mask), ptr(m), ptr(lsum),
                ptr(pdT), ptr(dsT), ptr(dqkv), B, S, h, d, scale, keep, salt, state]
        if not with_dbias:
            check(lib.sky_attn_bwd(*args), "sky_attn_bwd")
            return dqkv, None
        # NaN-filled scratch and output: every element must be written
        QB = (S + 63) // 64
        slabs = torch.full((B * QB, 3 * h * d), float("nan"), dtype=torch.float32,
                           device="cuda")
        dbias = torch.full((3 * h * d,), float("nan"), dtype=torch.bfloat16, device="cuda")
        check(lib.sky_attn_bwd_dbias(*args, ptr(slabs), ptr(dbias), F._dt(dbias)),
              "sky_attn_bwd_dbias")
        assert torch.isfinite(slabs).all(), "scratch element left unwritten"
        return dqkv, dbias

    want, _ = run(False)
    got, dbias = run(True)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), "dqkv changed"

    rows = got.float().view(B * S, 3 * h * d)
    ref = rows.sum(0)
    a = rows.abs().sum(0)
    err = (dbias.float() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 1e-4 * a
    print(f"max |dbias - ref| {err.max().item():.3e}, "
          f"max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), (err / bound).max().item()


def test_rejects_missing_buffers():
    """No scratch or no dbias buffer is an error, not a silent skip."""
    lib = hiplib.require()
    qkv = torch.zeros(1, 16, 3, 1, 64, device="cuda", dtype=torch.bfloat16)
    rc = lib.sky_attn_bwd_dbias(0, ptr(qkv), ptr(qkv), 0, ptr(qkv), ptr(qkv),
                                ptr(qkv), ptr(qkv), ptr(qkv), 1, 16, 1, 64,
                                0.125, 1.0, 0, 0, 0, 0, 1)
    assert rc != 0
