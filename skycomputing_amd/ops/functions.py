"""torch.autograd.Function wrappers over the HIP kernel library.

Each Function's forward/backward launches hand-written gfx950 kernels on the
current HIP stream via the C ABI in hiplib. Numerics contract: bf16 (or fp32)
I/O, fp32 accumulation inside the kernels; tested against ops/eager.py in
fp32 (tests/test_ops_gpu.py).
"""

from __future__ import annotations

import ctypes
import math
import os

import torch

from . import hiplib
from .hiplib import check, ptr

_DT = {torch.float32: 0, torch.bfloat16: 1}

_seed_gen = torch.Generator()
_seed_gen.manual_seed(0x5EED)


def set_dropout_seed(seed: int):
    _seed_gen.manual_seed(seed)


def _next_seed() -> int:
    return int(torch.randint(0, 2**62, (1,), generator=_seed_gen).item())


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


_CS_SLABS = 1024  # MAX_SLABS in ops/hip/common.h


def _red_scratch(cols: int, pairs: int, device) -> torch.Tensor:
    """fp32 scratch for the two-stage column reductions:
    [_CS_SLABS slabs][pairs*cols]."""
    return torch.empty(_CS_SLABS * pairs * cols, dtype=torch.float32, device=device)


def merged_finish_enabled() -> bool:
    """SKY_NO_MERGED_FINISH=1 keeps every producer's own final reduction
    launch in the block nodes (A/B)."""
    return os.environ.get("SKY_NO_MERGED_FINISH") != "1"


class PendingFinish:
    """The slab reductions a backward has left pending: producers run
    through their sky_*_parts entry points with slot() as the job argument,
    then ONE sky_colsum_finish launch writes all their outputs, in the
    order the producers ran. The jobs live in host memory and travel to the
    kernel by value, so nothing is allocated or copied under graph capture.
    Holds the producers' scratch tensors until the finish is enqueued."""

    def __init__(self):
        self._jobs = (hiplib.FinishJob * hiplib.FINISH_MAX_JOBS)()
        self.n = 0
        self._keep = []

    def slot(self) -> int:
        """Address of the next free job, to hand to a *_parts entry point."""
        if self.n >= hiplib.FINISH_MAX_JOBS:
            raise RuntimeError("too many pending finish jobs")
        self._jobs[self.n].nv = 0
        return ctypes.addressof(self._jobs[self.n])

    def took(self, *scratch) -> bool:
        """After a *_parts call: keep the job if the producer left one.
        False means the producer finished its outputs itself."""
        if self._jobs[self.n].nv == 0:
            return False
        self._keep.extend(scratch)
        self.n += 1
        return True

    def run(self):
        if self.n:
            check(
                hiplib.require().sky_colsum_finish(
                    _stream(), ctypes.addressof(self._jobs), self.n),
                "sky_colsum_finish",
            )
        self.n = 0
        self._keep.clear()


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype} (fp32/bf16 only)") from None


class LayerNormFn(torch.autograd.Function):
    """Fused (dropout + residual-add +) LayerNorm, fwd+bwd in single-pass
    HIP kernels (replaces the reference's optional apex FusedLayerNorm +
    preceding nn.Dropout, reference: scaelum/model/bert_layers.py:128-168,
    283-288). With dropout_p > 0 the op computes
    LN(dropout(x) + residual); the mask regenerates from (salt, device
    step counter) in backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, residual, dropout_p=0.0):
        x = x.contiguous()
        residual = residual.contiguous() if residual is not None else None
        keep = 1.0 - dropout_p
        y, mean, rstd, salt = _ln_fwd(x, residual, weight, bias, eps, keep)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.residual = residual
        ctx.has_residual = residual is not None
        ctx.keep, ctx.salt = keep, salt
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        cols = x.shape[-1]
        if cols % 8 == 0:
            dx, dw, db, _, dgrad_res = _ln_bwd(
                dy, x, ctx.residual, weight, mean, rstd, ctx.keep, ctx.salt,
                xsum=False)
            return dx, dw, db, None, dgrad_res, None
        # odd widths: scalar kernels, dw/db through fp32 atomics; the kernels
        # refuse dropout there, so the residual's gradient is dx itself
        dx = torch.empty_like(x)
        dw = torch.zeros(cols, dtype=torch.float32, device=x.device)
        db = torch.zeros(cols, dtype=torch.float32, device=x.device)
        check(
            hiplib.require().sky_layernorm_bwd(
                _stream(), ptr(dy), ptr(x), ptr(ctx.residual), ptr(weight),
                ptr(mean), ptr(rstd), ptr(dx), ptr(dw), ptr(db), 0,
                x.numel() // cols, cols, _dt(x), ctx.keep, ctx.salt,
                rng_state().data_ptr() if ctx.keep < 1.0 else 0, 0,
            ),
            "sky_layernorm_bwd",
        )
        return (dx, dw.to(weight.dtype), db.to(weight.dtype), None,
                dx if ctx.has_residual else None, None)


class BiasGeluFn(torch.autograd.Function):
    """Fused bias + erf-GELU (reference: scaelum/model/bert_layers.py:21-44)."""

    @staticmethod
    def forward(ctx, x, bias):
        lib = hiplib.require()
        x = x.contiguous()
        cols = x.shape[-1]
        rows = x.numel() // cols
        y = torch.empty_like(x)
        check(
            lib.sky_bias_gelu_fwd(_stream(), ptr(x), ptr(bias), ptr(y), rows, cols, _dt(x)),
            "sky_bias_gelu_fwd",
        )
        ctx.save_for_backward(x, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = hiplib.require()
        x, bias = ctx.saved_tensors
        dy = dy.contiguous()
        cols = x.shape[-1]
        rows = x.numel() // cols
        dx = torch.empty_like(x)
        fast = cols % 8 == 0
        db = (torch.empty(cols, dtype=bias.dtype, device=x.device) if fast
              else torch.zeros(cols, dtype=torch.float32, device=x.device))
        scratch = _red_scratch(cols, 1, x.device) if fast else None
        check(
            lib.sky_bias_gelu_bwd(
                _stream(), ptr(dy), ptr(x), ptr(bias), ptr(dx), ptr(db),
                ptr(scratch), rows, cols, _dt(x)
            ),
            "sky_bias_gelu_bwd",
        )
        return dx, (db if fast else db.to(bias.dtype))


class MaskedSoftmaxFn(torch.autograd.Function):
    """Fused scale + additive-mask + row softmax over attention scores
    [B, h, Sq, Sk]; mask [B, 1, 1, Sk] additive, broadcast over (h, Sq).
    Replaces the reference's eager mask-add + softmax
    (reference: scaelum/model/bert_layers.py:259-269)."""

    @staticmethod
    def forward(ctx, scores, mask, scale):
        lib = hiplib.require()
        scores = scores.contiguous()
        B, h, Sq, Sk = scores.shape
        probs = torch.empty_like(scores)
        mask = mask.contiguous() if mask is not None else None
        check(
            lib.sky_masked_softmax_fwd(
                _stream(), ptr(scores), ptr(mask), ptr(probs),
                B, h, Sq, Sk, scale, 1.0, 0, _dt(scores),
            ),
            "sky_masked_softmax_fwd",
        )
        ctx.save_for_backward(probs)
        ctx.scale = scale
        return probs

    @staticmethod
    def backward(ctx, dp):
        lib = hiplib.require()
        (probs,) = ctx.saved_tensors
        dp = dp.contiguous()
        B, h, Sq, Sk = probs.shape
        ds = torch.empty_like(probs)
        check(
            lib.sky_masked_softmax_bwd(
                _stream(), ptr(dp), ptr(probs), ptr(ds),
                B, h, Sq, Sk, ctx.scale, 1.0, 0, _dt(probs),
            ),
            "sky_masked_softmax_bwd",
        )
        return ds, None, None


_RNG_STATE: torch.Tensor | None = None


def rng_state() -> torch.Tensor:
    """Device-side step counter mixed into every dropout seed. Bump it with
    rng_tick() at iteration start — as a captured hipGraph node this keeps
    dropout masks varying under graph replay (launch args are frozen)."""
    global _RNG_STATE
    if _RNG_STATE is None:
        _RNG_STATE = torch.zeros(1, dtype=torch.int64, device="cuda")
    return _RNG_STATE


def rng_tick():
    lib = hiplib.require()
    check(lib.sky_rng_tick(_stream(), rng_state().data_ptr()), "sky_rng_tick")


class DropoutFn(torch.autograd.Function):
    """Dropout with counter-based RNG: the keep mask is regenerated from
    (salt, device step counter) in backward, so no mask tensor is stored
    and the op is hipGraph-capture safe."""

    @staticmethod
    def forward(ctx, x, p):
        lib = hiplib.require()
        x = x.contiguous()
        y = torch.empty_like(x)
        salt = _next_seed()
        keep = 1.0 - p
        state = rng_state()
        check(
            lib.sky_dropout_fwd(
                _stream(), ptr(x), ptr(y), x.numel(), keep, salt,
                state.data_ptr(), _dt(x),
            ),
            "sky_dropout_fwd",
        )
        ctx.salt = salt
        ctx.keep = keep
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = hiplib.require()
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(
            lib.sky_dropout_bwd(
                _stream(), ptr(dy), ptr(dx), dy.numel(), ctx.keep, ctx.salt,
                rng_state().data_ptr(), _dt(dy),
            ),
            "sky_dropout_bwd",
        )
        return dx, None


def _split_heads(qkv):
    """q, k, v views [B, h, S, d] of a packed qkv [B, S, 3, h, d]."""
    return tuple(qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def _attn_bwd_decomposed(qkv, P, Pd, dout, scale, dP_of):
    """Five-GEMM attention backward from materialized probabilities P and
    their dropped-out copy Pd (both [B, h, S, S]); dP_of maps dPd to dP
    with the caller's own way of regenerating the dropout mask. Returns
    dqkv packed like qkv."""
    lib = hiplib.require()
    B, S, _, h, d = qkv.shape
    q, k, v = _split_heads(qkv)
    dO = dout.permute(0, 2, 1, 3).contiguous()  # one copy, used twice
    dV = torch.matmul(Pd.transpose(-1, -2), dO)
    dPd = torch.matmul(dO, v.transpose(-1, -2)).contiguous()
    dP = dP_of(dPd)
    dS = torch.empty_like(dP)
    check(
        lib.sky_masked_softmax_bwd(
            _stream(), ptr(dP), ptr(P), ptr(dS), B, h, S, S, scale,
            1.0, 0, _dt(P),
        ),
        "sky_masked_softmax_bwd",
    )
    dQ = torch.matmul(dS, k)                      # [B,h,S,d]
    dK = torch.matmul(dS.transpose(-1, -2), q)    # [B,h,S,d]
    dqkv = torch.empty_like(qkv)
    check(
        lib.sky_pack3(
            _stream(), ptr(dQ.contiguous()), ptr(dK.contiguous()),
            ptr(dV.contiguous()), ptr(dqkv), B, S, h, d, _dt(qkv),
        ),
        "sky_pack3",
    )
    return dqkv


def _attn_fwd(qkv, mask, scale, keep):
    """sky_attn_fwd on a contiguous packed qkv [B, S, 3, h, 64]; draws the
    dropout salt when keep < 1. Returns (out [B, S, h, d], m, lsum, salt)."""
    lib = hiplib.require()
    B, S, _, h, d = qkv.shape
    out = torch.empty(B, S, h, d, dtype=qkv.dtype, device=qkv.device)
    m = torch.empty(B, h, S, dtype=torch.float32, device=qkv.device)
    lsum = torch.empty_like(m)
    salt = _next_seed() if keep < 1.0 else 0
    state = rng_state()
    check(
        lib.sky_attn_fwd(
            _stream(), ptr(qkv), ptr(mask), ptr(out), ptr(m), ptr(lsum),
            B, S, h, d, scale, keep, salt, state.data_ptr(),
        ),
        "sky_attn_fwd",
    )
    return out, m, lsum, salt


def _attn_bwd_scratch(qkv):
    """The two-kernel backward's transposed scratch (pdT, dsT), [B,h,S,S]
    each. bwd2 loads whole 32-q fragments, so for S % 32 != 0 the last
    row's load runs past the tensor; zero B rows null it only if those
    bytes are finite -> zeroed tail.
    The default keys-on-rows pair keeps P and dS in registers and uses only
    the head of pdT, for the fp32 row dots [B*h*S] its dQ kernel hands to its
    dK/dV kernel; SKY_ATTN_KROWS=0 (and S = 1) runs bwd1s + bwd2, which fill
    both tensors."""
    B, S, _, h, _ = qkv.shape
    alloc = torch.empty if S == 128 else torch.zeros
    n = B * h * S * S + (32 if S % 32 else 0)
    return (alloc(n, dtype=qkv.dtype, device=qkv.device),
            alloc(n, dtype=qkv.dtype, device=qkv.device))


class FusedAttentionFn(torch.autograd.Function):
    """Fused attention: out = dropout(softmax(scale*QK^T + mask)) V in ONE
    MFMA kernel (ops/hip/attention.hip); S x S probabilities are never
    materialized in forward (row max/sum saved, flash-style).

    Backward default: TWO fused MFMA kernels (sky_attn_bwd,
    ops/hip/attention_bwd.hip) — recompute + dS + dQ, then dK/dV from a
    second recompute (SKY_ATTN_KROWS=0: over transposed scratch) — no torch
    ops at all.
    SKY_NO_FUSED_ATTN_BWD=1 selects the decomposed fallback (sky_attn_probs
    recompute + hipBLASLt batched GEMMs + HIP softmax-backward).

    qkv: [B, S, 3, h, d] (d = 64), mask: [B, 1, 1, S] additive or None.
    Returns [B, S, h, d].
    """

    @staticmethod
    def forward(ctx, qkv, mask, scale, dropout_p, training):
        B, S, three, h, d = qkv.shape
        assert three == 3 and d == 64 and S <= 128
        qkv = qkv.contiguous()
        mask = mask.contiguous() if mask is not None else None
        keep = 1.0 - dropout_p if (dropout_p > 0 and training) else 1.0
        out, m, lsum, salt = _attn_fwd(qkv, mask, scale, keep)
        ctx.save_for_backward(qkv, mask, m, lsum)
        ctx.scale, ctx.keep, ctx.salt = scale, keep, salt
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = hiplib.require()
        qkv, mask, m, lsum = ctx.saved_tensors
        B, S, _, h, d = qkv.shape
        dev = qkv.device
        if os.environ.get("SKY_NO_FUSED_ATTN_BWD") != "1":
            dout = dout.contiguous()
            dqkv = torch.empty_like(qkv)
            if os.environ.get("SKY_ATTN_FUSED_BWD") == "1":
                # single-kernel path: dQ/dK/dV in one launch, P and dS
                # never leave LDS (no pdT/dsT scratch tensors). Measured
                # in-app TIE vs the split pair (111.97 vs 111.73 ms step)
                # with lower memory churn; opt-in until it wins.
                check(
                    lib.sky_attn_bwd_fused(
                        _stream(), ptr(qkv), ptr(dout), ptr(mask), ptr(m),
                        ptr(lsum), ptr(dqkv), B, S, h, d, ctx.scale,
                        ctx.keep, ctx.salt, rng_state().data_ptr(),
                    ),
                    "sky_attn_bwd_fused",
                )
                return dqkv, None, None, None, None
            # two-kernel path (bwd1s + bwd2 over transposed scratch)
            pdT, dsT = _attn_bwd_scratch(qkv)
            check(
                lib.sky_attn_bwd(
                    _stream(), ptr(qkv), ptr(dout), ptr(mask), ptr(m),
                    ptr(lsum), ptr(pdT), ptr(dsT), ptr(dqkv),
                    B, S, h, d, ctx.scale, ctx.keep, ctx.salt,
                    rng_state().data_ptr(),
                ),
                "sky_attn_bwd",
            )
            return dqkv, None, None, None, None
        P = torch.empty(B, h, S, S, dtype=qkv.dtype, device=dev)
        Pd = torch.empty_like(P) if ctx.keep < 1.0 else P
        check(
            lib.sky_attn_probs(
                _stream(), ptr(qkv), ptr(mask), ptr(m), ptr(lsum), ptr(P),
                ptr(Pd), B, S, h, d, ctx.scale, ctx.keep, ctx.salt,
                rng_state().data_ptr(),
            ),
            "sky_attn_probs",
        )

        def dP_of(dPd):
            if ctx.keep < 1.0:
                # regenerate the dropout mask from Pd (zero where dropped; a
                # P-underflow zero also zeroes dS, so no false positives matter)
                return torch.where(
                    Pd != 0, dPd * (1.0 / ctx.keep), torch.zeros((), dtype=dPd.dtype, device=dPd.device)
                )
            return dPd

        dqkv = _attn_bwd_decomposed(qkv, P, Pd, dout, ctx.scale, dP_of)
        return dqkv, None, None, None, None


class FlashAttentionFn(torch.autograd.Function):
    """Flash-style attention for arbitrary S (d = 64, bf16): the forward is
    one online-softmax MFMA kernel (ops/hip/attention_flash.hip) per
    (batch, head, 128-query block); the
    S x S matrix never exists in forward. Backward recomputes probabilities
    (hipBLASLt scores GEMM + HIP masked-softmax) and regenerates the
    dropout mask from the saved salt (linear element indices match the
    generic dropout kernels), then runs the standard five-GEMM backward."""

    @staticmethod
    def forward(ctx, qkv, mask, scale, dropout_p, training):
        lib = hiplib.require()
        B, S, three, h, d = qkv.shape
        assert three == 3 and d == 64
        qkv = qkv.contiguous()
        mask = mask.contiguous() if mask is not None else None
        out = torch.empty(B, S, h, d, dtype=qkv.dtype, device=qkv.device)
        m = torch.empty(B, h, S, dtype=torch.float32, device=qkv.device)
        lsum = torch.empty_like(m)
        keep = 1.0 - dropout_p if (dropout_p > 0 and training) else 1.0
        salt = _next_seed() if keep < 1.0 else 0
        check(
            lib.sky_attn_flash_fwd(
                _stream(), ptr(qkv), ptr(mask), ptr(out), ptr(m), ptr(lsum),
                B, S, h, d, scale, keep, salt, rng_state().data_ptr(),
            ),
            "sky_attn_flash_fwd",
        )
        ctx.save_for_backward(qkv, mask)
        ctx.scale, ctx.keep, ctx.salt = scale, keep, salt
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = hiplib.require()
        qkv, mask = ctx.saved_tensors
        B, S, _, h, d = qkv.shape
        q, k, _ = _split_heads(qkv)
        scores = torch.matmul(q, k.transpose(-1, -2)).contiguous()
        P = torch.empty_like(scores)
        check(
            lib.sky_masked_softmax_fwd(
                _stream(), ptr(scores), ptr(mask), ptr(P), B, h, S, S,
                ctx.scale, 1.0, 0, _dt(scores),
            ),
            "sky_masked_softmax_fwd",
        )
        if ctx.keep < 1.0:
            Pd = torch.empty_like(P)
            check(
                lib.sky_dropout_fwd(
                    _stream(), ptr(P), ptr(Pd), P.numel(), ctx.keep, ctx.salt,
                    rng_state().data_ptr(), _dt(P),
                ),
                "sky_dropout_fwd",
            )
        else:
            Pd = P

        def dP_of(dPd):
            if ctx.keep < 1.0:
                dP = torch.empty_like(dPd)
                check(
                    lib.sky_dropout_bwd(
                        _stream(), ptr(dPd), ptr(dP), dPd.numel(), ctx.keep,
                        ctx.salt, rng_state().data_ptr(), _dt(dPd),
                    ),
                    "sky_dropout_bwd",
                )
                return dP
            return dPd

        dqkv = _attn_bwd_decomposed(qkv, P, Pd, dout, ctx.scale, dP_of)
        return dqkv, None, None, None, None


def colsum(src: torch.Tensor, out_dtype=None) -> torch.Tensor:
    """Column sum over a 2D [rows, cols] tensor via the HIP column-parallel
    reduction (fp32 accumulation)."""
    lib = hiplib.require()
    src = src.contiguous()
    rows, cols = src.shape
    fast = cols % 8 == 0
    want = out_dtype if (out_dtype is not None and fast) else torch.float32
    out = (torch.empty if fast else torch.zeros)(cols, dtype=want, device=src.device)
    scratch = _red_scratch(cols, 1, src.device) if fast else None
    check(
        lib.sky_colsum(_stream(), ptr(src), ptr(out), ptr(scratch), rows, cols,
                       _dt(src), _dt(out)),
        "sky_colsum",
    )
    if out_dtype is not None and out.dtype != out_dtype:
        out = out.to(out_dtype)
    return out


def _use_hblt() -> bool:
    return os.environ.get("SKY_NO_HBLT") != "1"


# ---- v2 hand GEMM dispatch (ops/hip/gemm2.hip) ----
# SKY_GEMM2 unset -> per-site measured defaults (the ffn-up trio, which
# ties hipBLASLt in-app: gpurun_out/ab_*.json r02 matrix); "0" = off;
# "1" = all sites; or a comma list of {fwd,dgrad,wgrad}. Only perfect-fit
# shapes (M,N %256; K %64) route here; everything else stays on hipBLASLt.

_G2_SITES: set | None = None
_G2_SITES_SET = False
_G2_WK: dict = {}

# in-app A/B (160L bench, r02): the fused ffn-up forward (one v2 GEMM with
# bias+gelu+Z epilogue) ties the library chain (112.26 vs 112.3 ms);
# v2 dgrad/wgrad regress ~25-35 us/layer against hipBLASLt and stay off
# by default (they only dispatch at all when the fused fwd owns the op).
_G2_DEFAULT = {
    "fwd": {(4096, 4096, 1024)},     # ffn-up fwd, bias+gelu+Z fused
    "dgrad": set(),
    "wgrad": set(),
}


def _g2_sites() -> set | None:
    """None means: use the measured per-site default allowlist."""
    global _G2_SITES, _G2_SITES_SET
    if not _G2_SITES_SET:
        v = os.environ.get("SKY_GEMM2", "").strip()
        if v == "":
            _G2_SITES = None
        elif v == "0":
            _G2_SITES = set()
        elif v == "1":
            _G2_SITES = {"fwd", "dgrad", "wgrad"}
        else:
            _G2_SITES = {s.strip() for s in v.split(",") if s.strip()}
        _G2_SITES_SET = True
    return _G2_SITES


def _g2_enabled(site: str, M: int, N: int, K: int) -> bool:
    sites = _g2_sites()
    if sites is None:
        return (M, N, K) in _G2_DEFAULT[site]
    return site in sites and _g2_shape_ok(M, N, K)


_G2_SHAPES: set | None = None


def _g2_shape_ok(M: int, N: int, K: int) -> bool:
    """Optional per-shape allowlist: SKY_GEMM2_SHAPES="MxNxK,MxNxK"."""
    global _G2_SHAPES
    if _G2_SHAPES is None:
        v = os.environ.get("SKY_GEMM2_SHAPES", "").strip()
        _G2_SHAPES = ({tuple(int(d) for d in s.split("x")) for s in v.split(",") if s}
                      if v else set())
    return not _G2_SHAPES or (M, N, K) in _G2_SHAPES


def _g2_fit(M: int, N: int, K: int) -> bool:
    return (M % 256 == 0 and N % 256 == 0 and K % 64 == 0
            and _g2_shape_ok(M, N, K))


def _g2_gsu(M: int, N: int, K: int) -> int:
    # split-K only where the tile grid badly underfills 256 CUs AND K is
    # deep enough to amortize the fp32 partial round-trip (measured:
    # K=1024 shapes run best at gsu=1 despite 64-WG grids)
    ntiles = (M // 256) * (N // 256)
    if ntiles < 128 and K >= 2048 and K % 256 == 0:
        return 4
    return 1


def _g2_workspace(M: int, N: int, gsu: int, device) -> torch.Tensor | None:
    if gsu <= 1:
        return None
    key = (M, N, gsu, device)
    wk = _G2_WK.get(key)
    if wk is None:
        wk = torch.empty(gsu * M * N, dtype=torch.float32, device=device)
        _G2_WK[key] = wk
    return wk


def _g2_call(a, b, c, bias, z, M, N, K, lda, ldb, ldc, tA, tB, epi, gsu):
    lib = hiplib.require()
    wk = _g2_workspace(M, N, gsu, a.device)
    check(
        lib.sky_gemm2(
            _stream(), ptr(a), ptr(b), ptr(c), ptr(bias), ptr(z),
            ptr(wk) if wk is not None else 0, M, N, K, lda, ldb, ldc,
            tA, tB, epi, gsu,
        ),
        "sky_gemm2",
    )
    return c


def gemm2_fwd(x2, weight, bias=None, gelu=False, want_z=False):
    """NT forward y = x2 @ weight.T (+bias)(+gelu). Returns (y, z|None) or
    None when the shape doesn't fit or the site is disabled."""
    if x2.dtype != torch.bfloat16:
        return None
    M, K = x2.shape
    N = weight.shape[0]
    if not (_g2_enabled("fwd", M, N, K) and _g2_fit(M, N, K)):
        return None
    epi = 2 if gelu else (1 if bias is not None else 0)
    gsu = _g2_gsu(M, N, K)
    y = torch.empty(M, N, dtype=x2.dtype, device=x2.device)
    z = torch.empty_like(y) if (gelu and want_z) else None
    _g2_call(x2, weight, y, bias, z, M, N, K, x2.stride(0), weight.stride(0),
             y.stride(0), 0, 0, epi, gsu)
    return y, z


def gemm2_dgrad(dy2, weight):
    """NN dgrad dx = dy2 @ weight (weight stored [N,K] = kmajor operand)."""
    if dy2.dtype != torch.bfloat16:
        return None
    M, Kred = dy2.shape
    N = weight.shape[1]
    if not (_g2_enabled("dgrad", M, N, Kred) and _g2_fit(M, N, Kred)):
        return None
    dx = torch.empty(M, N, dtype=dy2.dtype, device=dy2.device)
    _g2_call(dy2, weight, dx, None, None, M, N, Kred, dy2.stride(0),
             weight.stride(0), dx.stride(0), 0, 1, 0, _g2_gsu(M, N, Kred))
    return dx


def gemm2_wgrad(dy2, x2):
    """TN wgrad dw = dy2.T @ x2 (both stored [Mtok, out] = kmajor)."""
    if dy2.dtype != torch.bfloat16:
        return None
    Kred, M = dy2.shape
    N = x2.shape[1]
    if not (_g2_enabled("wgrad", M, N, Kred) and _g2_fit(M, N, Kred)):
        return None
    dw = torch.empty(M, N, dtype=dy2.dtype, device=dy2.device)
    _g2_call(dy2, x2, dw, None, None, M, N, Kred, dy2.stride(0),
             x2.stride(0), dw.stride(0), 1, 1, 0, _g2_gsu(M, N, Kred))
    return dw


def _linear_fwd(x2, weight, bias):
    """y = x2 @ weight.T + bias on 2D x2: the v2 hand GEMM where the site is
    enabled for the shape, torch (hipBLASLt) otherwise."""
    g2 = gemm2_fwd(x2 if x2.is_contiguous() else x2.contiguous(), weight, bias)
    if g2 is not None:
        return g2[0]
    return torch.nn.functional.linear(x2, weight, bias)


def _wgrad_plain(dy2, x2, weight):
    """dW = dy2.T @ x2 for a linear whose dbias comes from elsewhere: the
    v2 hand GEMM if enabled, else a plain hipBLASLt GEMM with measured
    algorithm selection (sky_hblt_wgrad), else torch (SKY_NO_HBLT=1)."""
    xc = x2 if x2.is_contiguous() else x2.contiguous()
    dw = gemm2_wgrad(dy2, xc)
    if dw is None and _use_hblt():
        M, K = xc.shape
        dw = torch.empty_like(weight)
        check(
            hiplib.require().sky_hblt_wgrad(
                _stream(), ptr(xc), ptr(dy2), ptr(dw), M, weight.shape[0], K,
                _dt(xc)
            ),
            "sky_hblt_wgrad",
        )
    elif dw is None:
        dw = dy2.t().mm(x2)
    return dw


def _dgrad(dy2, weight):
    """dx = dy2 @ weight (2D)."""
    dx = gemm2_dgrad(dy2, weight)
    return dx if dx is not None else dy2.mm(weight)


class LinearBiasFn(torch.autograd.Function):
    """Linear + bias with a custom backward: dgrad stays a hipBLASLt GEMM;
    wgrad is a direct hipBLASLt call whose BGRADB epilogue produces dbias
    inside the GEMM (ops/hip/hblt.hip), removing the separate column
    reduction per linear (a measured hot spot — profiles/r01_notes.md).
    SKY_NO_HBLT=1 falls back to torch wgrad + HIP colsum."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1])
        y = _linear_fwd(x2, weight, bias)
        ctx.save_for_backward(x2, weight)
        ctx.xshape = xs
        ctx.has_bias = bias is not None
        return y.view(*xs[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, weight.shape[0])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx = _dgrad(dy2, weight).view(ctx.xshape)
        dw2 = gemm2_wgrad(dy2, x2 if x2.is_contiguous() else x2.contiguous())
        if dw2 is not None:
            db = colsum(dy2, weight.dtype) if ctx.has_bias else None
            return dx, dw2, db
        if ctx.has_bias and _use_hblt():
            lib = hiplib.require()
            M, K = x2.shape
            N = weight.shape[0]
            dw = torch.empty_like(weight)
            db = torch.empty(N, dtype=weight.dtype, device=weight.device)
            check(
                lib.sky_hblt_wgrad_bgrad(
                    _stream(), ptr(x2), ptr(dy2), ptr(dw), ptr(db), M, N, K, _dt(x2)
                ),
                "sky_hblt_wgrad_bgrad",
            )
            return dx, dw, db
        dw = dy2.t().mm(x2)
        db = colsum(dy2, weight.dtype) if ctx.has_bias else None
        return dx, dw, db


def ln_dbias_enabled() -> bool:
    """SKY_NO_LN_DBIAS=1 keeps linear -> LayerNorm as two Functions (A/B)."""
    return os.environ.get("SKY_NO_LN_DBIAS") != "1"


def ln_xsum_width_ok(cols: int) -> bool:
    """Row widths the three-sum LayerNorm backward is built for."""
    return bool(hiplib.require().sky_layernorm_bwd_xsum_ok(cols))


def _ln_fwd(h, residual, ln_w, ln_b, eps, keep):
    """sky_layernorm_fwd: LN(dropout(h) + residual) on contiguous inputs;
    draws the dropout salt when keep < 1. Returns (y, mean, rstd, salt)."""
    cols = h.shape[-1]
    rows = h.numel() // cols
    y = torch.empty_like(h)
    mean = torch.empty(rows, dtype=torch.float32, device=h.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=h.device)
    salt = _next_seed() if keep < 1.0 else 0
    state_ptr = rng_state().data_ptr() if keep < 1.0 else 0
    check(
        hiplib.require().sky_layernorm_fwd(
            _stream(), ptr(h), ptr(residual), ptr(ln_w), ptr(ln_b),
            ptr(y), ptr(mean), ptr(rstd), rows, cols, eps, _dt(h),
            keep, salt, state_ptr,
        ),
        "sky_layernorm_fwd",
    )
    return y, mean, rstd, salt


def _ln_bwd(dy, h, residual, ln_w, mean, rstd, keep, salt, xsum,
            pending=None):
    """sky_layernorm_bwd (or, with xsum, sky_layernorm_bwd_xsum) for
    cols % 8 == 0, where the final reduction stage writes the param dtype
    directly. Returns (dh, d_ln_w, d_ln_b, dxsum, dres) with dxsum the
    column sum of dh as stored (None without xsum) and dres the residual's
    gradient (dh itself without dropout, None without a residual). With a
    PendingFinish the final reduction is left to pending.run(): d_ln_w,
    d_ln_b and dxsum hold nothing until then."""
    lib = hiplib.require()
    cols = h.shape[-1]
    rows = h.numel() // cols
    dh = torch.empty_like(h)
    d_ln_w = torch.empty(cols, dtype=ln_w.dtype, device=h.device)
    d_ln_b = torch.empty_like(d_ln_w)
    dxsum = torch.empty_like(d_ln_w) if xsum else None
    scratch = _red_scratch(cols, 3 if xsum else 2, h.device)
    drop = keep < 1.0
    dres = torch.empty_like(h) if (drop and residual is not None) else None
    state_ptr = rng_state().data_ptr() if drop else 0
    args = (_stream(), ptr(dy), ptr(h), ptr(residual), ptr(ln_w), ptr(mean),
            ptr(rstd), ptr(dh), ptr(d_ln_w), ptr(d_ln_b), ptr(scratch), rows,
            cols, _dt(h), keep, salt, state_ptr, ptr(dres))
    if pending is not None:
        check(lib.sky_layernorm_bwd_parts(*args, ptr(dxsum), pending.slot()),
              "sky_layernorm_bwd_parts")
        pending.took(scratch)
    elif xsum:
        check(lib.sky_layernorm_bwd_xsum(*args, ptr(dxsum)),
              "sky_layernorm_bwd_xsum")
    else:
        check(lib.sky_layernorm_bwd(*args), "sky_layernorm_bwd")
    if residual is not None and not drop:
        dres = dh
    return dh, d_ln_w, d_ln_b, dxsum, dres


class LinearResidualLayerNormFn(torch.autograd.Function):
    """LN(dropout(x @ W^T + b) + residual) as ONE autograd node, so the
    backward can take the linear's dbias from the LayerNorm backward pass:
    d(linear out) is exactly the dx that ln_bwd_dx_cs_kernel holds in
    registers, and its column sum comes out of the same slab reduction as
    LN's dw/db (sky_layernorm_bwd_xsum). The weight gradient is then a
    plain GEMM (sky_hblt_wgrad) instead of the BGRADB-epilogue one plus its
    post-reduction kernel. Forward kernels, saved tensors and the dropout
    salt draw are those of LinearBiasFn followed by LayerNormFn."""

    @staticmethod
    def forward(ctx, x, weight, bias, ln_w, ln_b, eps, residual, dropout_p=0.0):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1])
        cols = weight.shape[0]
        h = _linear_fwd(x2, weight, bias).view(*xs[:-1], cols).contiguous()
        residual = residual.contiguous() if residual is not None else None
        keep = 1.0 - dropout_p
        y, mean, rstd, salt = _ln_fwd(h, residual, ln_w, ln_b, eps, keep)
        ctx.save_for_backward(x2, weight, h, ln_w, mean, rstd)
        ctx.residual = residual
        ctx.has_residual = residual is not None
        ctx.keep, ctx.salt = keep, salt
        ctx.xshape = xs
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, weight, h, ln_w, mean, rstd = ctx.saved_tensors
        dh, d_ln_w, d_ln_b, dbias, dgrad_res = _ln_bwd(
            dy.contiguous(), h, ctx.residual, ln_w, mean, rstd, ctx.keep,
            ctx.salt, xsum=True)
        if dbias.dtype != weight.dtype:
            dbias = dbias.to(weight.dtype)
        dh2 = dh.view(-1, h.shape[-1])
        dx = _dgrad(dh2, weight).view(ctx.xshape)
        dw = _wgrad_plain(dh2, x2, weight)
        return dx, dw, dbias, d_ln_w, d_ln_b, None, dgrad_res, None


def attn_block_enabled() -> bool:
    """SKY_NO_ATTN_BLOCK=1 keeps the attention third of an encoder block as
    its three autograd nodes (A/B)."""
    return os.environ.get("SKY_NO_ATTN_BLOCK") != "1"


class AttentionBlockFn(torch.autograd.Function):
    """The attention third of an encoder block as ONE autograd node:

        LN(dropout(attention(hidden @ Wqkv^T + bqkv) @ Wo^T + bo) + hidden)

    Forward kernels, saved tensors and the order of the two dropout-salt
    draws are those of LinearBiasFn, FusedAttentionFn and
    LinearResidualLayerNormFn in sequence, so y is bit-identical to that
    composition. One node lets the backward
      * take the qkv linear's dbias from the attention backward kernels,
        which hold dQ / dK / dV in registers (sky_attn_bwd_dbias), so the
        qkv weight gradient is a plain GEMM instead of the BGRADB-epilogue
        one plus its post-reduction kernel, and
      * fold autograd's add of hidden's two gradients (residual branch and
        qkv linear) into the qkv dgrad GEMM (beta = 1 on dres).
    bf16, d = 64, S <= 128 only (the fused attention kernels' domain);
    mask [B, 1, 1, S] additive or None."""

    @staticmethod
    def forward(ctx, hidden, wqkv, bqkv, mask, num_heads, attn_p, wo, bo,
                ln_w, ln_b, eps, hidden_p):
        B, S, H = hidden.shape
        d = H // num_heads
        assert d == 64 and S <= 128 and hidden.dtype == torch.bfloat16
        hidden = hidden.contiguous()
        x2 = hidden.view(-1, H)
        qkv = _linear_fwd(x2, wqkv, bqkv).view(B, S, 3, num_heads, d)
        mask = mask.contiguous() if mask is not None else None
        scale = 1.0 / math.sqrt(d)
        akeep = 1.0 - attn_p
        ctxl, m, lsum, asalt = _attn_fwd(qkv, mask, scale, akeep)
        c2 = ctxl.view(-1, H)
        h = _linear_fwd(c2, wo, bo).view(B, S, H)
        keep = 1.0 - hidden_p
        y, mean, rstd, salt = _ln_fwd(h, hidden, ln_w, ln_b, eps, keep)
        ctx.save_for_backward(x2, wqkv, qkv, mask, m, lsum, c2, wo, h, ln_w,
                              mean, rstd)
        ctx.scale, ctx.akeep, ctx.asalt = scale, akeep, asalt
        ctx.keep, ctx.salt = keep, salt
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = hiplib.require()
        (x2, wqkv, qkv, mask, m, lsum, c2, wo, h, ln_w, mean,
         rstd) = ctx.saved_tensors
        B, S, _, nh, d = qkv.shape
        H = nh * d
        # the LN and dbqkv slab reductions finish in one launch, after the
        # attention backward (SKY_NO_MERGED_FINISH=1: one launch each)
        pending = PendingFinish() if merged_finish_enabled() else None
        dh, d_ln_w, d_ln_b, dbo, dres = _ln_bwd(
            dy.contiguous(), h, x2, ln_w, mean, rstd, ctx.keep, ctx.salt,
            xsum=True, pending=pending)
        dh2 = dh.view(-1, H)
        dctx = _dgrad(dh2, wo)
        dwo = _wgrad_plain(dh2, c2, wo)
        dqkv = torch.empty_like(qkv)
        dbqkv = torch.empty(3 * H, dtype=wqkv.dtype, device=qkv.device)
        pdT, dsT = _attn_bwd_scratch(qkv)
        # column partials of dqkv, one slab per (batch, 64-query block);
        # the kernels write every element, so no memset
        slabs = torch.empty(B * ((S + 63) // 64) * 3 * H, dtype=torch.float32,
                            device=qkv.device)
        args = (_stream(), ptr(qkv), ptr(dctx), ptr(mask), ptr(m), ptr(lsum),
                ptr(pdT), ptr(dsT), ptr(dqkv), B, S, nh, d, ctx.scale,
                ctx.akeep, ctx.asalt, rng_state().data_ptr(), ptr(slabs),
                ptr(dbqkv), _dt(dbqkv))
        if pending is not None:
            check(lib.sky_attn_bwd_dbias_parts(*args, pending.slot()),
                  "sky_attn_bwd_dbias_parts")
            pending.took(slabs)
            pending.run()
        else:
            check(lib.sky_attn_bwd_dbias(*args), "sky_attn_bwd_dbias")
        dqkv2 = dqkv.view(-1, 3 * H)
        dwqkv = _wgrad_plain(dqkv2, x2, wqkv)
        # d hidden = dres + dqkv @ Wqkv, accumulated by the GEMM. Without
        # dropout dres IS dh; its readers above are already enqueued on
        # this stream, so updating it in place is safe.
        dres2 = dres.view(-1, H)
        g2 = gemm2_dgrad(dqkv2, wqkv)
        if g2 is not None:
            dres2.add_(g2)
        else:
            dres2.addmm_(dqkv2, wqkv)
        if dbo.dtype != wo.dtype:
            dbo = dbo.to(wo.dtype)
        return (dres.view(B, S, H), dwqkv, dbqkv, None, None, None, dwo, dbo,
                d_ln_w, d_ln_b, None, None)


def _linear_gelu_fwd(x2, weight, bias):
    """gelu(x2 @ weight.T + bias) on contiguous 2D x2 in ONE GEMM that also
    stores the pre-activation: the v2 hand GEMM where its fwd site is
    enabled for the shape, else the hipBLASLt GELU_AUX_BIAS epilogue.
    Returns (y, aux)."""
    M, K = x2.shape
    N = weight.shape[0]
    g2 = gemm2_fwd(x2, weight, bias, gelu=True, want_z=True)
    if g2 is not None:
        return g2
    y = torch.empty(M, N, dtype=x2.dtype, device=x2.device)
    aux = torch.empty(M, N, dtype=x2.dtype, device=x2.device)
    check(
        hiplib.require().sky_hblt_linear_gelu_aux(
            _stream(), ptr(x2), ptr(weight), ptr(bias), ptr(y), ptr(aux),
            M, N, K, _dt(x2), _dt(aux)
        ),
        "sky_hblt_linear_gelu_aux",
    )
    return y, aux


def _gelu_bwd(dy2, aux, weight, pending=None):
    """sky_bias_gelu_bwd with aux as the pre-activation: returns
    (dpre, dbias). With a PendingFinish, dbias's slab reduction is left to
    pending.run() where the kernel's streaming path applies."""
    lib = hiplib.require()
    rows, N = dy2.shape
    dpre = torch.empty_like(dy2)
    db = torch.empty(N, dtype=weight.dtype, device=weight.device)
    scratch = _red_scratch(N, 1, dy2.device)
    args = (_stream(), ptr(dy2), ptr(aux), 0, ptr(dpre), ptr(db),
            ptr(scratch), rows, N, _dt(dy2))
    if pending is not None:
        check(lib.sky_bias_gelu_bwd_parts(*args, pending.slot()),
              "sky_bias_gelu_bwd_parts")
        pending.took(scratch)
    else:
        check(lib.sky_bias_gelu_bwd(*args), "sky_bias_gelu_bwd")
    return dpre, db


class LinearGeluFn(torch.autograd.Function):
    """Fused linear + bias + GELU via the hipBLASLt GELU_AUX_BIAS epilogue
    (the reference's LinearActivation, scaelum/model/bert_layers.py:60-108):
    the forward is ONE GEMM that also writes the pre-activation `aux`; the
    backward reuses the bias_gelu kernel with aux as the pre-activation
    (dpre + fused dbias), then plain dgrad/wgrad GEMMs. hipBLASLt's GELU is
    the tanh approximation; the erf-derivative backward differs by less
    than bf16 rounding (tests/test_ops_gpu.py)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xs = x.shape
        x2 = x.reshape(-1, xs[-1]).contiguous()
        y, aux = _linear_gelu_fwd(x2, weight, bias)
        ctx.save_for_backward(x2, weight, aux)
        ctx.xshape = xs
        return y.view(*xs[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight, aux = ctx.saved_tensors
        dy2 = dy.reshape(-1, weight.shape[0])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dpre, db = _gelu_bwd(dy2, aux, weight)
        dx = _dgrad(dpre, weight).view(ctx.xshape)
        dw = gemm2_wgrad(dpre, x2)
        if dw is None:
            dw = dpre.t().mm(x2)
        return dx, dw, db


def ffn_block_enabled() -> bool:
    """SKY_NO_FFN_BLOCK=1 keeps the FFN two-thirds of an encoder block as
    its two autograd nodes (A/B)."""
    return os.environ.get("SKY_NO_FFN_BLOCK") != "1"


class FfnBlockFn(torch.autograd.Function):
    """The FFN two-thirds of an encoder block as ONE autograd node:

        LN(dropout(gelu(x @ Wup^T + bup) @ Wdown^T + bdown) + x)

    Forward kernels, saved tensors and the single dropout-salt draw are
    those of LinearGeluFn followed by LinearResidualLayerNormFn, so y is
    bit-identical to that composition. One node lets the backward
      * fold autograd's add of x's two gradients (residual branch and
        ffn-up linear) into the ffn-up dgrad GEMM (beta = 1 on dres), and
      * finish its four column sums (d_ln_w, d_ln_b, dbdown from the LN
        backward, dbup from the gelu backward) in one launch.
    Domain: where ops.linear_act takes LinearGeluFn and
    ops.linear_residual_layer_norm takes its node (ops.ffn_block)."""

    @staticmethod
    def forward(ctx, x, wup, bup, wdown, bdown, ln_w, ln_b, eps, dropout_p):
        xs = x.shape
        H = xs[-1]
        x2 = x.reshape(-1, H).contiguous()
        inter, aux = _linear_gelu_fwd(x2, wup, bup)
        h = _linear_fwd(inter, wdown, bdown)
        keep = 1.0 - dropout_p
        y, mean, rstd, salt = _ln_fwd(h, x2, ln_w, ln_b, eps, keep)
        ctx.save_for_backward(x2, wup, aux, inter, wdown, h, ln_w, mean, rstd)
        ctx.keep, ctx.salt = keep, salt
        ctx.xshape = xs
        return y.view(xs)

    @staticmethod
    def backward(ctx, dy):
        (x2, wup, aux, inter, wdown, h, ln_w, mean,
         rstd) = ctx.saved_tensors
        H = x2.shape[-1]
        pending = PendingFinish() if merged_finish_enabled() else None
        dh, d_ln_w, d_ln_b, dbdown, dres = _ln_bwd(
            dy.contiguous().view(-1, H), h, x2, ln_w, mean, rstd, ctx.keep,
            ctx.salt, xsum=True, pending=pending)
        d_inter = _dgrad(dh, wdown)
        dwdown = _wgrad_plain(dh, inter, wdown)
        dpre, dbup = _gelu_bwd(d_inter, aux, wup, pending)
        if pending is not None:
            pending.run()
        dwup = gemm2_wgrad(dpre, x2)
        if dwup is None:
            dwup = dpre.t().mm(x2)
        # d x = dres + dpre @ Wup, accumulated by the GEMM. Without dropout
        # dres IS dh; its readers above are already enqueued on this
        # stream, so updating it in place is safe.
        g2 = gemm2_dgrad(dpre, wup)
        if g2 is not None:
            dres.add_(g2)
        else:
            dres.addmm_(dpre, wup)
        if dbdown.dtype != wdown.dtype:
            dbdown = dbdown.to(wdown.dtype)
        return (dres.view(ctx.xshape), dwup, dbup, dwdown, dbdown, d_ln_w,
                d_ln_b, None, None)


class EmbeddingFusedFn(torch.autograd.Function):
    """Fused word+position+type gather, 3-way add and LayerNorm
    (reference eager sequence: scaelum/model/bert_layers.py:191-212)."""

    @staticmethod
    def forward(ctx, input_ids, token_type_ids, position_ids,
                word_emb, pos_emb, type_emb, ln_w, ln_b, eps):
        lib = hiplib.require()
        ids = input_ids.contiguous().view(-1).to(torch.int64)
        tids = token_type_ids.contiguous().view(-1).to(torch.int64)
        pids = position_ids.contiguous().view(-1).to(torch.int64)
        rows = ids.numel()
        cols = word_emb.shape[1]
        y = torch.empty(
            (*input_ids.shape, cols), dtype=word_emb.dtype, device=word_emb.device
        )
        mean = torch.empty(rows, dtype=torch.float32, device=y.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=y.device)
        check(
            lib.sky_embedding_fwd(
                _stream(), ptr(ids), ptr(tids), ptr(pids),
                ptr(word_emb), ptr(type_emb), ptr(pos_emb),
                ptr(ln_w), ptr(ln_b), ptr(y), ptr(mean), ptr(rstd),
                rows, cols, word_emb.shape[0], eps, _dt(y),
            ),
            "sky_embedding_fwd",
        )
        ctx.save_for_backward(ids, tids, pids, word_emb, pos_emb, type_emb, ln_w, mean, rstd)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = hiplib.require()
        ids, tids, pids, word_emb, pos_emb, type_emb, ln_w, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        cols = word_emb.shape[1]
        rows = ids.numel()
        dev = dy.device
        dwe = torch.zeros(word_emb.shape, dtype=torch.float32, device=dev)
        dte = torch.zeros(type_emb.shape, dtype=torch.float32, device=dev)
        dpe = torch.zeros(pos_emb.shape, dtype=torch.float32, device=dev)
        dlnw = torch.zeros(cols, dtype=torch.float32, device=dev)
        dlnb = torch.zeros(cols, dtype=torch.float32, device=dev)
        check(
            lib.sky_embedding_bwd(
                _stream(), ptr(dy), ptr(ids), ptr(tids), ptr(pids),
                ptr(word_emb), ptr(type_emb), ptr(pos_emb), ptr(ln_w),
                ptr(mean), ptr(rstd), ptr(dwe), ptr(dte), ptr(dpe),
                ptr(dlnw), ptr(dlnb),
                rows, cols, _dt(dy),
            ),
            "sky_embedding_bwd",
        )
        return (
            None, None, None,
            dwe.to(word_emb.dtype), dpe.to(pos_emb.dtype), dte.to(type_emb.dtype),
            dlnw.to(ln_w.dtype), dlnb.to(ln_w.dtype), None,
        )


def xent_forward(logits2, labels1, num_classes: int, ignore_index: int):
    """The forward launches of softmax cross-entropy (ops/hip/xent.hip) on
    logits2 [N, ld] (contiguous, fp32/bf16) and labels1 [N] (int64):
    sky_xent_fwd, then sky_xent_finish. Returns fp32
    (rowmax [N], logsum [N], rowloss [N], block [2]) with
    block = {mean loss over valid rows, 1 / valid count}, both 0 when no row
    is valid. Nothing here synchronises or depends on the labels' values."""
    lib = hiplib.require()
    N, ld = logits2.shape
    dev = logits2.device
    stats = torch.empty(3, N, dtype=torch.float32, device=dev)
    block = torch.empty(2, dtype=torch.float32, device=dev)
    rowmax, logsum, rowloss = stats[0], stats[1], stats[2]
    check(
        lib.sky_xent_fwd(
            _stream(), ptr(logits2), ptr(labels1), ptr(rowmax), ptr(logsum),
            ptr(rowloss), N, num_classes, ld, ignore_index, _dt(logits2)),
        "sky_xent_fwd",
    )
    check(
        lib.sky_xent_finish(
            _stream(), ptr(rowloss), ptr(labels1), ptr(block), N, num_classes,
            ignore_index),
        "sky_xent_finish",
    )
    return rowmax, logsum, rowloss, block


class SoftmaxCrossEntropyFn(torch.autograd.Function):
    """Mean softmax cross-entropy over the valid rows of logits [..., ld]
    (classes 0..num_classes-1, the rest padding) in two row kernels and a
    one-block finish (ops/hip/xent.hip). The valid count and its reciprocal
    stay on the device, and backward reads the incoming gradient from
    device memory too, so the node makes no synchronisation and replays
    correctly in a hipGraph when the labels change.

    With inplace_backward the gradient is written over the saved logits and
    returned as an alias of them: right only when nothing else reads the
    logits after this loss (see ops.softmax_cross_entropy)."""

    @staticmethod
    def forward(ctx, logits, labels, num_classes, ignore_index, inplace_backward):
        ld = logits.shape[-1]
        if not 1 <= num_classes <= ld:
            raise ValueError(f"num_classes {num_classes} outside 1..{ld}")
        if labels.shape != logits.shape[:-1]:
            raise ValueError(
                f"labels {tuple(labels.shape)} do not match logits "
                f"{tuple(logits.shape)}")
        logits2 = logits.reshape(-1, ld)
        if not logits2.is_contiguous():
            if inplace_backward:
                raise ValueError("inplace_backward needs contiguous logits")
            logits2 = logits2.contiguous()
        labels1 = labels.reshape(-1).to(torch.int64).contiguous()
        rowmax, logsum, _, block = xent_forward(
            logits2, labels1, num_classes, ignore_index)
        ctx.save_for_backward(logits2, labels1, rowmax, logsum, block)
        ctx.args = (num_classes, ignore_index, inplace_backward)
        ctx.shape = logits.shape
        return block[0].clone()

    @staticmethod
    def backward(ctx, gout):
        lib = hiplib.require()
        logits2, labels1, rowmax, logsum, block = ctx.saved_tensors
        num_classes, ignore_index, inplace = ctx.args
        N, ld = logits2.shape
        gout = gout.to(torch.float32).contiguous()
        if inplace:
            dlogits = logits2.detach()
        else:
            # the kernel splits rows into head/body/tail once for loads and
            # stores: give the output the logits' offset from a 16-byte line
            es = logits2.element_size()
            off = (logits2.data_ptr() % 16) // es
            flat = torch.empty(N * ld + off, dtype=logits2.dtype,
                               device=logits2.device)
            dlogits = flat[off:].view(N, ld)
        check(
            lib.sky_xent_bwd(
                _stream(), ptr(logits2), ptr(labels1), ptr(rowmax),
                ptr(logsum), ptr(block), ptr(gout), ptr(dlogits), N,
                num_classes, ld, ignore_index, _dt(logits2)),
            "sky_xent_bwd",
        )
        return dlogits.view(ctx.shape), None, None, None, None
