"""The fused LayerNorm kernels draw exactly the generic dropout kernel's mask.

Both use the LINEAR index scheme (docs/ARCHITECTURE.md section 4): element
e of the flattened [rows, cols] tensor keeps iff 16-bit slice e & 3 of
rng_hash(seed, e >> 2) is below the threshold. The reference mask is
sky_dropout_fwd on ones with the same salt; every vectorized LayerNorm
kernel (forward, the backward dx kernel with 0, 2 and 3 column sums, the
split chain's wb_part) is called through the raw entry points with that
salt and a null step counter, and must agree with it on every element.

Shapes: cols 520 is 65 vec8 per row, a partly filled second chunk and row
bases that are not wave-aligned; 2048 is CH=4; 4096 is CH=8, which the
three-sum kernel is not built for. Rows 9 and 5 leave the last block with one
wave active; SKY_LN_CS_GRID=2 makes the blocks loop over rows.

Bounds
  dx against dres / keep, where kept: dx and dres are each one rounding of
      the same fp32 value (times the fp32 1/keep for dx) to the output dtype.
      bf16: 2^-8 relative for dx's rounding plus 2^-8 for that of dres, which
      stands in for the exact value on the reference side. fp32: dres is the
      fp32 value itself, so only dx's 2^-22 (one product rounding plus the
      rounding of 1/keep, as in test_dropout_rng_gen1_gpu.py).
  Without a residual the mask is read off dx != 0, which needs every kept
      element's gradient to be non-zero: the inputs' seeds are fixed and the
      smallest fp64 |gradient| over kept elements is printed and held above
      1e-5, two decades over the fp32 cancellation error of the kernel's
      dxhat - s1 - xhat * s2 (about 1e-7 at these unit-scale inputs).
  y: fp32 within 8 x the error of the eager composition (generic dropout
      kernel, then the fp32 eager LayerNorm); bf16 to one rounding + 1e-6.

Measured on an MI355X, worst case over all 56 cases: bf16 dx against
dres / keep at 0.80 of its bound (1.6 x 2^-8, so one rounding alone would
not cover the two stored values), fp32 at 0.33; smallest kept |gradient|
1.47e-5 (rows 5, cols 4096, fp32); fp32 y at 1.37 x the eager error; bf16 y
at 0.996 of its bound.
"""

from __future__ import annotations

import functools

import pytest
import torch

from . import kernel_checks as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import eager, hiplib
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops.hiplib import check, ptr


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


KEEP = 0.7
EPS = 1e-12
SALT = 0x5A17_0DD5_EED5
NAN = float("nan")
SHAPES = [(9, 520), (9, 2048), (5, 4096)]
DTYPES = [torch.bfloat16, torch.float32]
MIN_GRAD = 1e-5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(rows, cols, dtype):
    """Inputs, the reference mask and the forward kernels' outputs for one
    shape and dtype, computed once and left unchanged. The inputs come from
    a CPU generator, so they are the same on every machine."""
    lib = hiplib.require()
    g = torch.Generator()
    g.manual_seed(7300 + 10 * cols + rows + (1 if dtype == torch.float32 else 0))

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(dtype).cuda()

    c = dict(x=rn(rows, cols), res=rn(rows, cols), dy=rn(rows, cols), b=rn(cols),
             w=(torch.rand(cols, generator=g) + 0.5).to(dtype).cuda())
    ones = torch.ones(rows * cols, dtype=dtype, device="cuda")
    dropped = _nan(rows * cols, dtype=dtype)
    check(lib.sky_dropout_fwd(_stream(), ptr(ones), ptr(dropped), rows * cols, KEEP,
                              SALT, 0, F._dt(ones)), "sky_dropout_fwd")
    assert not torch.isnan(dropped).any()
    c["mask"] = (dropped != 0).view(rows, cols)
    frac = c["mask"].double().mean().item()
    assert abs(frac - KEEP) < 0.05, frac
    # x through the generic dropout kernel, for the eager composition
    c["xdrop"] = _nan(rows, cols, dtype=dtype)
    check(lib.sky_dropout_fwd(_stream(), ptr(c["x"]), ptr(c["xdrop"]), rows * cols,
                              KEEP, SALT, 0, F._dt(ones)), "sky_dropout_fwd")
    for has_res in (False, True):
        y = _nan(rows, cols, dtype=dtype)
        mean = _nan(rows, dtype=torch.float32)
        rstd = _nan(rows, dtype=torch.float32)
        check(lib.sky_layernorm_fwd(
            _stream(), ptr(c["x"]), ptr(c["res"]) if has_res else 0, ptr(c["w"]),
            ptr(c["b"]), ptr(y), ptr(mean), ptr(rstd), rows, cols, EPS,
            F._dt(y), KEEP, SALT, 0), "sky_layernorm_fwd")
        c["fwd", has_res] = (y, mean, rstd)
    return c


def _xs64(c, has_res):
    xs = c["x"].double() * c["mask"].double() / KEEP
    return xs + c["res"].double() if has_res else xs


def _ids(v):
    if isinstance(v, torch.dtype):
        return "bf16" if v == torch.bfloat16 else "fp32"
    if isinstance(v, bool):
        return "res" if v else "nores"
    return None


@pytest.mark.parametrize("has_res", [True, False], ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_forward_uses_the_dropout_kernels_mask(rows, cols, dtype, has_res):
    c = _case(rows, cols, dtype)
    y, mean, rstd = c["fwd", has_res]
    assert not torch.isnan(y).any() and not torch.isnan(mean).any() and not torch.isnan(rstd).any()
    y64, _, _, _ = kc.layernorm_ref64(_xs64(c, has_res), c["w"], c["b"], EPS)
    if dtype == torch.float32:
        ey = eager.layer_norm(c["xdrop"], c["w"], c["b"], EPS, c["res"] if has_res else None)
        kc.assert_within_eager(y, ey, y64, "y")
    else:
        kc.assert_bf16_close(y, y64, 1e-6, "y")


# the three-sum kernel stops at CH=4 (sky_layernorm_bwd_xsum_ok)
BWD_CASES = [(r, c, p) for r, c in SHAPES
             for p in ("default", "split_wb", "cs_grid2", "xsum")
             if not (p == "xsum" and c > 2048)]


@pytest.mark.parametrize("has_res", [True, False], ids=_ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("rows,cols,path", BWD_CASES)
def test_backward_regenerates_the_dropout_kernels_mask(rows, cols, path, dtype, has_res,
                                                       monkeypatch):
    lib = hiplib.require()
    monkeypatch.delenv("SKY_LN_SPLIT_WB", raising=False)
    monkeypatch.delenv("SKY_LN_CS_GRID", raising=False)
    if path == "split_wb":
        monkeypatch.setenv("SKY_LN_SPLIT_WB", "1")
    if path == "cs_grid2":
        monkeypatch.setenv("SKY_LN_CS_GRID", "2")
    c = _case(rows, cols, dtype)
    mask = c["mask"]
    _, mean, rstd = c["fwd", has_res]
    dx = _nan(rows, cols, dtype=dtype)
    dres = _nan(rows, cols, dtype=dtype) if has_res else None
    dw, db, dxsum = (_nan(cols, dtype=dtype) for _ in range(3))
    scratch = _nan(F._CS_SLABS * 3 * cols, dtype=torch.float32)
    args = (_stream(), ptr(c["dy"]), ptr(c["x"]), ptr(c["res"]) if has_res else 0,
            ptr(c["w"]), ptr(mean), ptr(rstd), ptr(dx), ptr(dw), ptr(db), ptr(scratch),
            rows, cols, F._dt(dx), KEEP, SALT, 0, ptr(dres))
    if path == "xsum":
        check(lib.sky_layernorm_bwd_xsum(*args, ptr(dxsum)), "sky_layernorm_bwd_xsum")
    else:
        check(lib.sky_layernorm_bwd(*args), "sky_layernorm_bwd")
    outs = [("dx", dx), ("dw", dw), ("db", db)]
    outs += [("dres", dres)] if has_res else []
    outs += [("dxsum", dxsum)] if path == "xsum" else []
    for name, t in outs:
        assert not torch.isnan(t).any(), f"{name}: element left unwritten"

    if has_res:
        assert torch.equal(dx != 0, mask & (dres != 0))
        ref = dres.double() / KEEP
        rel = 2 * 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -22
        kc.assert_bounded(dx[mask], ref[mask], rel * ref[mask].abs(), "dx vs dres/keep")
    else:
        dxs64, _, _ = kc.layernorm_bwd_ref64(c["dy"], _xs64(c, False), c["w"], EPS)
        smallest = dxs64[mask].abs().min().item()
        print(f"min |dxs| over kept elements {smallest:.3e} (must exceed {MIN_GRAD:g})")
        assert smallest > MIN_GRAD, "choose another seed: a kept gradient is too close to 0"
        assert torch.equal(dx != 0, mask)
