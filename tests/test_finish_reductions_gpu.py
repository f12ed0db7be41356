"""One finishing launch for several column-sum jobs (sky_colsum_finish).

Each producer of slab partials (LayerNorm backward with 2 or 3 sums, the
streaming bias-gelu backward, the attention backward with dbias) has a
*_parts entry point that leaves its final reduction pending as a job. Run as
"parts + merged finish", every output must have the bits the producer's
existing entry point (with its own final launch) writes on the same inputs.
Outputs and scratch are NaN-filled before every call and must be finite
afterwards; every output tensor is compared whole.
"""

from __future__ import annotations

import math

import pytest
import torch

from tests.test_attn_bwd_dbias_gpu import make_mask

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import functions as F
    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.ops.hiplib import check, ptr

NAN = float("nan")
BF16, FP32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), NAN,
                      dtype=dtype, device="cuda")


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _rn(gen, *shape, dtype=BF16, scale=1.0):
    return (torch.randn(*shape, device="cuda", generator=gen) * scale).to(dtype)


class LnBwd:
    """LayerNorm backward on rows x cols, ns = 2 (dw, db) or 3 (+ dxsum)."""

    def __init__(self, rows, cols, dtype, has_res, keep, ns, seed=0):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + rows * 7 + cols)
        self.rows, self.cols, self.dtype, self.keep, self.ns = rows, cols, dtype, keep, ns
        self.x = _rn(g, rows, cols, dtype=dtype)
        self.res = _rn(g, rows, cols, dtype=dtype) if has_res else None
        self.w = (torch.rand(cols, device="cuda", generator=g) + 0.5).to(dtype)
        b = _rn(g, cols, dtype=dtype)
        self.dy = _rn(g, rows, cols, dtype=dtype)
        F.set_dropout_seed(99)
        _, self.mean, self.rstd, self.salt = F._ln_fwd(
            self.x, self.res, self.w, b, 1e-12, keep)
        self.state = F.rng_state().data_ptr() if keep < 1.0 else 0
        self.name = f"ln{ns}[{rows}x{cols}]"

    def _buffers(self):
        out = dict(dx=_nan((self.rows, self.cols), self.dtype),
                   dw=_nan(self.cols, self.dtype), db=_nan(self.cols, self.dtype))
        if self.keep < 1.0 and self.res is not None:
            out["dres"] = _nan((self.rows, self.cols), self.dtype)
        if self.ns == 3:
            out["dxsum"] = _nan(self.cols, self.dtype)
        scratch = _nan(F._CS_SLABS * self.ns * self.cols, FP32)
        args = (_stream(), ptr(self.dy), ptr(self.x), ptr(self.res), ptr(self.w),
                ptr(self.mean), ptr(self.rstd), ptr(out["dx"]), ptr(out["dw"]),
                ptr(out["db"]), ptr(scratch), self.rows, self.cols,
                F._dt(self.x), self.keep, self.salt, self.state,
                ptr(out.get("dres")))
        return out, scratch, args

    def reference(self):
        lib = hiplib.require()
        out, scratch, args = self._buffers()
        if self.ns == 3:
            check(lib.sky_layernorm_bwd_xsum(*args, ptr(out["dxsum"])), "xsum")
        else:
            check(lib.sky_layernorm_bwd(*args), "ln_bwd")
        return out

    def parts(self, pending):
        out, scratch, args = self._buffers()
        check(hiplib.require().sky_layernorm_bwd_parts(
            *args, ptr(out.get("dxsum")), pending.slot()), "ln_parts")
        return out, scratch


class GeluBwd:
    """Bias-gelu backward on rows x cols; has_b False = x is the saved
    pre-activation, as LinearGeluFn calls it."""

    def __init__(self, rows, cols, dtype, has_b, seed=0):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + rows * 5 + cols)
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.x = _rn(g, rows, cols, dtype=dtype)
        self.b = _rn(g, cols, dtype=dtype) if has_b else None
        self.dy = _rn(g, rows, cols, dtype=dtype)
        self.name = f"gelu[{rows}x{cols}]"

    def _buffers(self):
        out = dict(dx=_nan((self.rows, self.cols), self.dtype),
                   db=_nan(self.cols, self.dtype))
        scratch = _nan(F._CS_SLABS * self.cols, FP32)
        args = (_stream(), ptr(self.dy), ptr(self.x), ptr(self.b), ptr(out["dx"]),
                ptr(out["db"]), ptr(scratch), self.rows, self.cols, F._dt(self.x))
        return out, scratch, args

    def reference(self):
        out, scratch, args = self._buffers()
        check(hiplib.require().sky_bias_gelu_bwd(*args), "gelu_bwd")
        return out

    def parts(self, pending):
        out, scratch, args = self._buffers()
        check(hiplib.require().sky_bias_gelu_bwd_parts(*args, pending.slot()),
              "gelu_parts")
        return out, scratch


class AttnBwd:
    """Two-kernel attention backward with dbias, d = 64."""

    def __init__(self, B, S, h, masked, p, dbias_dtype=BF16, seed=0):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + 1000 * S + 10 * h + B)
        self.B, self.S, self.h = B, S, h
        self.qkv = _rn(g, B, S, 3, h, 64)
        self.dout = _rn(g, B, S, h, 64)
        self.mask = make_mask(B, S, g) if masked else None
        self.scale, self.keep = 1.0 / math.sqrt(64), 1.0 - p
        self.dbias_dtype = dbias_dtype
        F.set_dropout_seed(77)
        _, self.m, self.lsum, self.salt = F._attn_fwd(
            self.qkv, self.mask, self.scale, self.keep)
        self.name = f"attn[{B},{S},{h}]"

    def _buffers(self):
        B, S, h = self.B, self.S, self.h
        self.pdT, self.dsT = F._attn_bwd_scratch(self.qkv)
        out = dict(dqkv=torch.full_like(self.qkv, NAN),
                   dbias=_nan(3 * h * 64, self.dbias_dtype))
        scratch = _nan(B * ((S + 63) // 64) * 3 * h * 64, FP32)
        args = (_stream(), ptr(self.qkv), ptr(self.dout), ptr(self.mask),
                ptr(self.m), ptr(self.lsum), ptr(self.pdT), ptr(self.dsT),
                ptr(out["dqkv"]), B, S, h, 64, self.scale, self.keep, self.salt,
                F.rng_state().data_ptr(), ptr(scratch), ptr(out["dbias"]),
                F._dt(out["dbias"]))
        return out, scratch, args

    def reference(self):
        out, scratch, args = self._buffers()
        check(hiplib.require().sky_attn_bwd_dbias(*args), "attn_dbias")
        return out

    def parts(self, pending):
        out, scratch, args = self._buffers()
        check(hiplib.require().sky_attn_bwd_dbias_parts(*args, pending.slot()),
              "attn_parts")
        return out, scratch


def _check_parts_plus_finish(producers, expect_pending=None):
    """Runs every producer's existing entry point, then all their *_parts in
    order and ONE sky_colsum_finish; compares every output tensor's bits.
    Returns the merged run's outputs per producer."""
    want = [p.reference() for p in producers]
    pending = F.PendingFinish()
    got, used = [], []
    for k, p in enumerate(producers):
        out, scratch = p.parts(pending)
        n0 = pending.n
        took = pending.took(scratch)
        if expect_pending is not None:
            assert took == expect_pending[k], p.name
        if took:
            job = pending._jobs[n0]
            used.append((p.name, scratch, job.nslabs * job.nv * job.cols))
        got.append(out)
    assert pending.n == len(used)
    pending.run()
    torch.cuda.synchronize()
    for name, scratch, n in used:
        assert 0 < n <= scratch.numel(), name
        assert torch.isfinite(scratch[:n]).all(), f"{name}: scratch left unwritten"
    compared = []
    for p, g, w in zip(producers, got, want):
        assert g.keys() == w.keys()
        for key in w:
            assert torch.isfinite(w[key]).all(), (p.name, key, "reference")
            assert torch.isfinite(g[key]).all(), (p.name, key)
            assert g[key].dtype == w[key].dtype
            assert torch.equal(_bits(g[key]), _bits(w[key])), (p.name, key)
            compared.append(f"{p.name}.{key}")
    print("bit-identical:", ", ".join(compared))
    return got


# 5 x 520: fewer slabs than the final's 64 groups, last 16-column block half
# full. 2100 x 1024: the producer's grid cap (512 slabs), rows no multiple of
# it. 300 x 2048: widest three-sum width, 75 slabs (not a multiple of 64).
LN_SHAPES = [(5, 520), (2100, 1024), (300, 2048)]


@pytest.mark.parametrize("keep", [1.0, 0.7])
@pytest.mark.parametrize("has_res", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("ns", [3, 2])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_ln_bwd_parts_plus_finish(rows, cols, ns, dtype, has_res, keep):
    dt = BF16 if dtype == "bf16" else FP32
    _check_parts_plus_finish([LnBwd(rows, cols, dt, has_res, keep, ns)], [True])


@pytest.mark.parametrize("has_b", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("rows,cols", [(256, 2048), (700, 4096)])
def test_gelu_bwd_parts_plus_finish(rows, cols, dtype, has_b):
    dt = BF16 if dtype == "bf16" else FP32
    _check_parts_plus_finish([GeluBwd(rows, cols, dt, has_b)], [True])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_gelu_bwd_off_the_slab_path_reports_nothing_pending(dtype):
    """64 x 1000 is not a width of the streaming kernel: the parts entry
    point finishes db itself, leaves no job, and the (empty) finish launches
    nothing. db is also the column sum of dx as stored: fp32 slab sums
    (error ~ rows * 2^-24 * sum|dx|, far inside 1e-4 * sum|dx|) rounded once
    to the output dtype (2^-8 relative for bf16, bound 2^-7)."""
    dt = BF16 if dtype == "bf16" else FP32
    (got,) = _check_parts_plus_finish([GeluBwd(64, 1000, dt, True)], [False])
    dx = got["dx"].double()
    ref, a = dx.sum(0), dx.abs().sum(0)
    err = (got["db"].double() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 1e-4 * a
    print(f"max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,S,h", [(1, 48, 2), (2, 128, 4), (3, 100, 16)])
def test_attn_bwd_dbias_parts_plus_finish(B, S, h, masked, p):
    _check_parts_plus_finish([AttnBwd(B, S, h, masked, p)], [True])


def test_ffn_node_pair_ln3_then_gelu():
    """The two jobs FfnBlockFn.backward issues, in its order."""
    _check_parts_plus_finish(
        [LnBwd(512, 1024, BF16, True, 0.9, 3), GeluBwd(512, 4096, BF16, False)],
        [True, True])


def test_attention_node_pair_ln3_then_attn():
    """The two jobs AttentionBlockFn.backward issues, in its order."""
    _check_parts_plus_finish(
        [LnBwd(256, 1024, BF16, True, 0.9, 3), AttnBwd(2, 128, 16, True, 0.1)],
        [True, True])


def test_max_jobs_mixed_nv_and_output_dtype():
    """Four jobs in one launch: NV 3, 1, 2, 1; bf16 and fp32 outputs; 520
    (half-full last block), 2048, 1024 and 384 columns, so every job's first
    block sits at a different offset in the grid."""
    assert hiplib.FINISH_MAX_JOBS == 4
    _check_parts_plus_finish(
        [LnBwd(5, 520, BF16, True, 0.7, 3),
         GeluBwd(256, 2048, FP32, True),
         LnBwd(300, 1024, FP32, False, 1.0, 2),
         AttnBwd(1, 48, 2, True, 0.1, dbias_dtype=FP32)],
        [True, True, True, True])


def test_off_path_producer_between_pending_ones():
    """A producer that leaves nothing pending takes no job slot."""
    _check_parts_plus_finish(
        [GeluBwd(256, 2048, BF16, False), GeluBwd(64, 1000, BF16, True),
         LnBwd(300, 2048, BF16, True, 1.0, 3)],
        [True, False, True])


@pytest.mark.parametrize("njobs", [1, 2, 4])
def test_finish_on_exact_integer_slabs(njobs):
    """Independent of the separate finals: scratch of small integers, whose
    fp32 sums are exact in any order, so out[v][c] must EQUAL the sum over
    slabs of scratch[slab][v][c] for every job, vector and column."""
    lib = hiplib.require()
    g = torch.Generator(device="cuda")
    g.manual_seed(njobs)
    spec = [(3, 5, 520, FP32), (1, 525, 1000, BF16), (2, 64, 16, FP32),
            (1, 1000, 24, FP32)][:njobs]  # (nv, nslabs, cols, out dtype)
    jobs = (hiplib.FinishJob * hiplib.FINISH_MAX_JOBS)()
    keep = []
    for k, (nv, nslabs, cols, dt) in enumerate(spec):
        # bf16 outputs: |sum| <= 256 is exact in bf16's 8 significant bits
        hi = 3 if dt == FP32 else 1
        scratch = torch.randint(-hi, hi + 1, (nslabs, nv, cols), device="cuda",
                                generator=g).float()
        if dt == BF16:
            scratch[256:] = 0.0
        outs = [_nan(cols, dt) for _ in range(nv)]
        jobs[k].scratch = ptr(scratch)
        for v in range(nv):
            jobs[k].out[v] = ptr(outs[v])
        jobs[k].nslabs, jobs[k].cols, jobs[k].nv = nslabs, cols, nv
        jobs[k].dtout = F._dt(outs[0])
        keep.append((scratch, outs))
    import ctypes
    check(lib.sky_colsum_finish(_stream(), ctypes.addressof(jobs), njobs), "finish")
    torch.cuda.synchronize()
    for k, (scratch, outs) in enumerate(keep):
        for v, o in enumerate(outs):
            assert torch.equal(o.float(), scratch[:, v, :].sum(0)), (k, v)


def test_finish_rejects_bad_job_lists():
    lib = hiplib.require()
    import ctypes
    jobs = (hiplib.FinishJob * (hiplib.FINISH_MAX_JOBS + 1))()
    addr = ctypes.addressof(jobs)
    assert lib.sky_colsum_finish(_stream(), addr, 0) == 0  # nothing to do
    assert lib.sky_colsum_finish(_stream(), addr, hiplib.FINISH_MAX_JOBS + 1) != 0
    assert lib.sky_colsum_finish(_stream(), 0, 1) != 0
    assert lib.sky_colsum_finish(_stream(), addr, 1) != 0  # nv = 0, no buffers
    pending = F.PendingFinish()
    for _ in range(hiplib.FINISH_MAX_JOBS):
        pending._jobs[pending.n].nv = 1
        assert pending.took()
    with pytest.raises(RuntimeError):
        pending.slot()
