"""The counter-based dropout RNG through the raw sky_dropout_fwd / _bwd entry
points with fixed salts: index-absolute masks (scalar and vector kernels
agree), backward mask == forward mask, keep fraction and independence of
neighbouring keep bits (the four 16-bit lanes of one hash), sensitivity to
the salt and to the device step counter, and keep = 1.
"""

from __future__ import annotations

import pytest
import torch

from . import kernel_checks as kc

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


DTYPES = [torch.bfloat16, torch.float32]
SALT = 0x1234_5678_9ABC


def _drop(x, keep, salt, state=0, bwd=False):
    """Raw kernel into a NaN-filled output; state is a device pointer or 0."""
    lib = hiplib.require()
    y = torch.full_like(x, float("nan"))
    fn = lib.sky_dropout_bwd if bwd else lib.sky_dropout_fwd
    check(fn(torch.cuda.current_stream().cuda_stream, ptr(x), ptr(y), x.numel(),
             keep, salt, state, F._dt(x)), "sky_dropout")
    assert not torch.isnan(y).any(), "output element left unwritten"
    return y


def _mask(n, keep, salt, dtype=torch.float32, state=0):
    return _drop(torch.ones(n, dtype=dtype, device="cuda"), keep, salt, state) != 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_scalar_and_vector_kernels_draw_the_same_mask(dtype):
    vec = _mask(4096, 0.5, SALT, dtype)       # n % 8 == 0: dropout_vec_kernel
    sca = _mask(4099, 0.5, SALT, dtype)       # n % 8 != 0: dropout_kernel
    assert 0.4 < vec.double().mean().item() < 0.6
    assert torch.equal(vec, sca[:4096])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [4096, 4099], ids=["vec", "scalar"])
def test_backward_mask_is_forward_mask(n, dtype):
    keep = 0.7
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n)
    x = (torch.rand(n, device="cuda", generator=gen) + 0.5).to(dtype)
    dy = (torch.rand(n, device="cuda", generator=gen) + 0.5).to(dtype)
    y = _drop(x, keep, SALT)
    dx = _drop(dy, keep, SALT, bwd=True)
    mask = y != 0
    assert torch.equal(dx != 0, mask)
    for got, src, name in ((y, x, "y"), (dx, dy, "dx")):
        ref = src.double() * mask.double() / keep
        # one output rounding: bf16 2^-8, fp32 2^-24 plus the fp32 1/keep
        rel = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -22
        kc.assert_bounded(got, ref, rel * ref.abs(), name)


@pytest.mark.parametrize("keep", [0.1, 0.5, 0.9])
def test_keep_fraction_and_neighbour_independence(keep):
    n = 1 << 20
    m = _mask(n, keep, SALT + int(keep * 10)).double()
    frac = m.mean().item()
    tol = 5 * (keep * (1 - keep) / n) ** 0.5 + 2.0 ** -16
    print(f"keep {keep}: fraction {frac:.6f}, |diff| {abs(frac - keep):.2e}, tol {tol:.2e}")
    assert abs(frac - keep) <= tol
    c = m - frac
    var = (c * c).mean().item()
    for lag in (1, 2, 3):
        corr = (c[:-lag] * c[lag:]).mean().item() / var
        print(f"keep {keep}: lag-{lag} correlation {corr:+.2e}, tol {5 / n ** 0.5:.2e}")
        assert abs(corr) <= 5 / n ** 0.5, (lag, corr)


def test_salt_and_step_counter_sensitivity():
    keep, n = 0.7, 1 << 20
    a = _mask(n, keep, SALT)
    b = _mask(n, keep, SALT + 1)
    agree = (a == b).double().mean().item()
    want = keep * keep + (1 - keep) * (1 - keep)
    print(f"two salts agree on {agree:.5f}, independent masks would on {want:.5f}")
    assert abs(agree - want) <= 5 * (want * (1 - want) / n) ** 0.5

    # a null state pointer is counter 0
    state = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert torch.equal(_mask(n, keep, SALT, state=state.data_ptr()), a)

    # the op's own counter: the mask changes with a tick ...
    st = F.rng_state()
    before = int(st.item())
    m0 = _mask(n, keep, SALT, state=st.data_ptr())
    F.rng_tick()
    assert int(st.item()) == before + 1
    m1 = _mask(n, keep, SALT, state=st.data_ptr())
    agree = (m0 == m1).double().mean().item()
    assert abs(agree - want) <= 5 * (want * (1 - want) / n) ** 0.5, agree
    # ... and is a function of the counter's value alone: a fresh zeroed
    # counter ticked (through sky_rng_tick) to the same value reproduces it
    fresh = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if before + 1 <= 64:
        for _ in range(before + 1):
            check(hiplib.require().sky_rng_tick(stream, fresh.data_ptr()), "sky_rng_tick")
    else:
        fresh.fill_(before)
        check(hiplib.require().sky_rng_tick(stream, fresh.data_ptr()), "sky_rng_tick")
    assert int(fresh.item()) == before + 1
    assert torch.equal(_mask(n, keep, SALT, state=fresh.data_ptr()), m1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [4096, 4099], ids=["vec", "scalar"])
def test_keep_one_is_identity(n, dtype):
    x = torch.randn(n, device="cuda").to(dtype)
    assert torch.equal(_drop(x, 1.0, SALT), x)
