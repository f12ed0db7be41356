"""The LayerNorm backward's merge of its four waves' column partials.

ln_bwd_dx_cs_kernel merges in one barrier where the per-wave LDS regions fit
(up to 1024 columns, the dropout kernels): each thread sums its columns over
waves 0, 1, 2, 3 from 0.f, the order of the serial merge it replaces. So with
SKY_LN_MERGE_SERIAL=1 (the serial merge) and without, every output and every
slab must have the same bits. The switch is read at every launch, so both
settings run in this process. 2048 columns (and the kernels without dropout)
keep the serial merge under either setting and must come out the same too.

db is also checked against the column sum of dy, independently of either
merge: fp32 sums rounded once to the output dtype, the bound of
tests/test_finish_reductions_gpu.py's off-path case.
"""

from __future__ import annotations

import pytest
import torch

from tests.test_finish_reductions_gpu import BF16, FP32, LnBwd, _bits

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.ops.hiplib import check, ptr


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _run(case):
    """The existing entry point (dx kernel + its own final) on NaN-filled
    buffers; returns the outputs and the slabs the dx kernel wrote."""
    lib = hiplib.require()
    out, scratch, args = case._buffers()
    if case.ns == 3:
        check(lib.sky_layernorm_bwd_xsum(*args, ptr(out["dxsum"])), "xsum")
    else:
        check(lib.sky_layernorm_bwd(*args), "ln_bwd")
    torch.cuda.synchronize()
    nslabs = min((case.rows + 3) // 4, 512)
    out["slabs"] = scratch[: nslabs * case.ns * case.cols].clone()
    return out


def _check_both_merges(monkeypatch, rows, cols, ns, dtype, keep):
    dt = BF16 if dtype == "bf16" else FP32
    case = LnBwd(rows, cols, dt, True, keep, ns)
    monkeypatch.delenv("SKY_LN_MERGE_SERIAL", raising=False)
    new = _run(case)
    monkeypatch.setenv("SKY_LN_MERGE_SERIAL", "1")
    old = _run(case)
    assert new.keys() == old.keys()
    for key in old:
        assert torch.isfinite(old[key]).all(), (key, "serial")
        assert torch.isfinite(new[key]).all(), key
        assert torch.equal(_bits(new[key]), _bits(old[key])), key
    dy = case.dy.double()
    want, a = dy.sum(0), dy.abs().sum(0)
    err = (new["db"].double() - want).abs()
    bound = 2.0 ** -7 * want.abs() + 1e-4 * a
    print(f"bit-identical: {', '.join(old)}; db max err/bound "
          f"{(err / bound).max().item():.3f}")
    assert (err <= bound).all()


# rows 1, 3: waves with no row at all (their partials are the zeros the sum
# starts from); 5: a second block with one row; 2049: the grid cap of 512
# blocks, one wave with a second row. cols 512 / 1024: one and two chunks.
@pytest.mark.parametrize("keep", [0.9, 1.0])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("ns", [2, 3])
@pytest.mark.parametrize("cols", [512, 1024])
@pytest.mark.parametrize("rows", [1, 3, 5, 2049])
def test_one_barrier_merge_has_the_serial_merge_bits(monkeypatch, rows, cols,
                                                     ns, dtype, keep):
    _check_both_merges(monkeypatch, rows, cols, ns, dtype, keep)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("ns", [2, 3])
@pytest.mark.parametrize("rows", [5, 2049])
def test_four_chunks_keep_the_serial_merge(monkeypatch, rows, ns, dtype):
    _check_both_merges(monkeypatch, rows, 2048, ns, dtype, 0.9)
