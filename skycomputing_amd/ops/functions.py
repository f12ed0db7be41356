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


# S above which attention runs the chunked kernels of ops/hip/attention_long.hip
ATTN_SMAX = 128
ATTN_LONG_SMAX = 4096
# SKY_ATTN_LONG unset: the (lo, hi] range of S that takes the long kernels by
# default: 256 <= S <= 512, the two lengths at which the in-application A/B
# against sdpa met the bar of ARCHITECTURE section 7 (profiles/r12_notes.md).
# Outside it nothing was measured in the application and sdpa stays.
_ATTN_LONG_DEFAULT = (255, 512)


def attn_long_enabled(S: int) -> bool:
    """Whether ops.attention / ops.attention_block run the long-sequence
    kernels at this S: SKY_ATTN_LONG=1 everywhere in 128 < S <= 4096,
    SKY_ATTN_LONG=0 nowhere (torch sdpa, as before), unset by measurement."""
    if not ATTN_SMAX < S <= ATTN_LONG_SMAX:
        return False
    e = os.environ.get("SKY_ATTN_LONG")
    if e in ("0", "1"):
        return e == "1"
    return (_ATTN_LONG_DEFAULT is not None
            and _ATTN_LONG_DEFAULT[0] < S <= _ATTN_LONG_DEFAULT[1])


# SKY_ATTN_SEG_SHORT unset: whether packed attention at 2 <= S <= 128 runs the
# segment mode of the one-chunk kernels. On: at B = 32, S = 128, h = 16 its
# forward + backward median beat sdpa with the dense boolean mask with
# non-overlapping ranges, 127 against 198 us (profiles/r15_notes.md).
_ATTN_SEG_SHORT_DEFAULT = True


def attn_seg_enabled(S: int) -> bool:
    """Whether ops.attention / ops.attention_block run the hand kernels on
    segment ids at this S. 2 <= S <= 128: SKY_ATTN_SEG_SHORT=1 / 0, unset by
    measurement, and never under an env switch that selects another S <= 128
    attention path; 128 < S <= 4096: unless SKY_ATTN_LONG=0. S = 1: never."""
    if S > ATTN_SMAX:
        return S <= ATTN_LONG_SMAX and os.environ.get("SKY_ATTN_LONG") != "0"
    if S < 2 or any(os.environ.get(v) == "1" for v in (
            "SKY_NO_FUSED_ATTN", "SKY_NO_FUSED_ATTN_BWD", "SKY_ATTN_FUSED_BWD")):
        return False
    e = os.environ.get("SKY_ATTN_SEG_SHORT")
    return e == "1" if e in ("0", "1") else _ATTN_SEG_SHORT_DEFAULT


# SKY_ATTN_CAUSAL unset: the (lo, hi] range of S at which causal attention
# runs the triangle mode of the hand kernels by default: 2 <= S <= 2048. At
# S = 128, 512 and 2048 (h = 16, 4096 tokens, bf16, p = 0.1) its forward +
# backward median was below sdpa(is_causal=True)'s with non-overlapping
# ranges in both runs: 129 / 65 against 202 / 198, 148 against 271 and 474
# against 614 us (profiles/r16_notes.md). Above 2048 nothing was measured and
# sdpa stays; SKY_ATTN_CAUSAL=1 opts in.
_ATTN_CAUSAL_DEFAULT = (1, 2048)


def attn_causal_enabled(S: int) -> bool:
    """Whether ops.attention / ops.attention_block run the hand kernels'
    causal (triangle) mode at this S, 2 <= S <= 4096: SKY_ATTN_CAUSAL=1 / 0
    forces it, unset by measurement. Never under an env switch that selects
    another S <= 128 attention path, nor above 128 under SKY_ATTN_LONG=0.
    S = 1: never (the dense path; causal is the identity there)."""
    if not 2 <= S <= ATTN_LONG_SMAX or any(os.environ.get(v) == "1" for v in (
            "SKY_NO_FUSED_ATTN", "SKY_NO_FUSED_ATTN_BWD", "SKY_ATTN_FUSED_BWD")):
        return False
    if S > ATTN_SMAX and os.environ.get("SKY_ATTN_LONG") == "0":
        return False
    e = os.environ.get("SKY_ATTN_CAUSAL")
    if e in ("0", "1"):
        return e == "1"
    return (_ATTN_CAUSAL_DEFAULT is not None
            and _ATTN_CAUSAL_DEFAULT[0] < S <= _ATTN_CAUSAL_DEFAULT[1])


# Head dim 128 (ops/hip/attention_d128.hip). SKY_ATTN_D128 unset: the (lo, hi]
# range of S at which ops.attention runs the d = 128 hand kernels by default:
# 128 <= S <= 2048. At S = 128, 512 and 2048 (h = 8, 4096 tokens, bf16,
# p = 0.1) their forward + backward median was below sdpa's with
# non-overlapping ranges in both runs, with the additive mask (128 / 63
# against 176 / 173, 127 against 281, 396 / 391 against 738 us) and causal
# (128 / 64 against 195 / 193, 133 against 251, 428 / 427 against 617 us;
# profiles/r17_notes.md). Below 128 and above 2048 nothing was measured and
# the call goes where it went before; SKY_ATTN_D128=1 opts in.
ATTN_D128 = 128
_ATTN_D128_DEFAULT = (127, 2048)


def attn_d128_enabled(S: int) -> bool:
    """Whether ops.attention runs the head-dim-128 hand kernels at this S,
    1 <= S <= 4096 (causal: 2 <= S, the caller's condition): SKY_ATTN_D128=1
    / 0 forces it, unset by measurement. Never under SKY_NO_FUSED_ATTN=1,
    SKY_NO_FUSED_ATTN_BWD=1 or SKY_ATTN_FUSED_BWD=1."""
    if not 1 <= S <= ATTN_LONG_SMAX or any(os.environ.get(v) == "1" for v in (
            "SKY_NO_FUSED_ATTN", "SKY_NO_FUSED_ATTN_BWD", "SKY_ATTN_FUSED_BWD")):
        return False
    e = os.environ.get("SKY_ATTN_D128")
    if e in ("0", "1"):
        return e == "1"
    return (_ATTN_D128_DEFAULT is not None
            and _ATTN_D128_DEFAULT[0] < S <= _ATTN_D128_DEFAULT[1])


# Grouped-query attention at head dim 128 (FusedGqaAttentionFn). SKY_ATTN_GQA
# unset: the (lo, hi] range of S at which ops.attention(num_kv_heads=) runs
# the sky_attn_d128_gqa_* kernels by default; None: nowhere, which is what
# the measurement gave (profiles/r18_notes.md; MI355X, 4096 tokens, h = 8,
# h_kv = 2 and 1, bf16, p = 0.1, forward + backward, against expand_kv + the
# multi-head d = 128 kernels and against sdpa(enable_gqa=True), mask and
# causal, two runs). S = 128: 73 / 103 us (h_kv = 2 / 1) against 145 / 143 us
# expanded, but one of the eight comparisons (h_kv = 1, causal, run 1) had
# overlapping ranges, 108.6 to 143.8 against 143.0 to 159.8, so the length
# does not meet the rule. S = 512: level at h_kv = 2 (206 against 206 us),
# slower at h_kv = 1 (332 against 236 / 208). S = 2048: slower, 738 / 1239
# against 470 / 482 us: the dK/dV grid is B * h_kv * ceil(S/64) blocks of G
# times the work, 128 or 64 blocks on 256 CUs there. SKY_ATTN_GQA=1 opts in.
_ATTN_GQA_DEFAULT = None


def attn_gqa_enabled(S: int) -> bool:
    """Whether ops.attention(num_kv_heads=) runs the grouped-query hand
    kernels at this S, 1 <= S <= 4096 (causal: 2 <= S, the caller's
    condition): SKY_ATTN_GQA=1 / 0 forces it, unset by measurement. Never
    under SKY_NO_FUSED_ATTN=1, SKY_NO_FUSED_ATTN_BWD=1 or
    SKY_ATTN_FUSED_BWD=1."""
    if not 1 <= S <= ATTN_LONG_SMAX or any(os.environ.get(v) == "1" for v in (
            "SKY_NO_FUSED_ATTN", "SKY_NO_FUSED_ATTN_BWD", "SKY_ATTN_FUSED_BWD")):
        return False
    e = os.environ.get("SKY_ATTN_GQA")
    if e in ("0", "1"):
        return e == "1"
    return (_ATTN_GQA_DEFAULT is not None
            and _ATTN_GQA_DEFAULT[0] < S <= _ATTN_GQA_DEFAULT[1])


def _attn_seg(segment_ids):
    """Segment ids as the kernels take them: (int32 ids,) for S <= 128, where
    the kernels find their ranges from the ids, (ids, bounds) above."""
    ids = segment_ids.to(torch.int32).contiguous()
    return (ids, attn_seg_bounds(ids)) if ids.shape[1] > ATTN_SMAX else (ids,)


def attn_seg_bounds(ids):
    """sky_attn_seg_bounds on int32 segment ids [B, S], 128 < S <= 4096: per
    64-token block the run start of its first token and the run end of its
    last one, int32 [B, ceil(S/64), 2] (eager.seg_bounds)."""
    B, S = ids.shape
    bounds = torch.empty(B, (S + 63) // 64, 2, dtype=torch.int32, device=ids.device)
    check(hiplib.require().sky_attn_seg_bounds(_stream(), ptr(ids), ptr(bounds), B, S),
          "sky_attn_seg_bounds")
    return bounds


def _attn_ids(seg, n):
    """The n pointers (ids, or ids and bounds) a causal entry point takes in
    the segment form's place: 0s without ids."""
    return tuple(ptr(t) for t in seg) if seg else (0,) * n


def _attn_fwd(qkv, mask, scale, keep, seg=None, causal=False):
    """sky_attn_fwd (S <= 128) or sky_attn_long_fwd on a contiguous packed
    qkv [B, S, 3, h, 64]; draws the dropout salt when keep < 1. Returns
    (out [B, S, h, d], m, lsum, salt). seg (_attn_seg): the segment form,
    sky_attn_long_seg_fwd on (ids, bounds) or sky_attn_seg_fwd on (ids,).
    causal: sky_attn_long_causal_fwd / sky_attn_causal_fwd, with or without
    seg. d = 128 (no seg): sky_attn_d128_fwd / sky_attn_d128_causal_fwd at
    every S; the causal entry takes no mask pointer at all."""
    lib = hiplib.require()
    B, S, _, h, d = qkv.shape
    out = torch.empty(B, S, h, d, dtype=qkv.dtype, device=qkv.device)
    m = torch.empty(B, h, S, dtype=torch.float32, device=qkv.device)
    lsum = torch.empty_like(m)
    salt = _next_seed() if keep < 1.0 else 0
    state = rng_state()
    if d == ATTN_D128:
        name = "sky_attn_d128_causal_fwd" if causal else "sky_attn_d128_fwd"
        masks = () if causal else (ptr(mask),)
    elif causal:
        long_ = S > ATTN_SMAX
        name = "sky_attn_long_causal_fwd" if long_ else "sky_attn_causal_fwd"
        masks = _attn_ids(seg, 2 if long_ else 1)
    elif seg is not None:
        name = "sky_attn_long_seg_fwd" if S > ATTN_SMAX else "sky_attn_seg_fwd"
        masks = tuple(ptr(t) for t in seg)
    else:
        name = "sky_attn_long_fwd" if S > ATTN_SMAX else "sky_attn_fwd"
        masks = (ptr(mask),)
    check(
        getattr(lib, name)(
            _stream(), ptr(qkv), *masks, ptr(out), ptr(m), ptr(lsum),
            B, S, h, d, scale, keep, salt, state.data_ptr(),
        ),
        name,
    )
    return out, m, lsum, salt


def _attn_long_bwd_args(qkv, dout, out, mask, m, lsum, dot, dqkv, scale,
                        keep, salt):
    """The arguments the three sky_attn_long_bwd* entry points share. out is
    the forward's output (the dQ kernel takes the row dot from dO * O); dot,
    fp32 [B*h*S] from the caller, is the only scratch: the dQ kernel hands
    it to the dK/dV kernel."""
    B, S, _, h, d = qkv.shape
    return (_stream(), ptr(qkv), ptr(dout), ptr(out), ptr(mask), ptr(m),
            ptr(lsum), ptr(dot), ptr(dqkv), B, S, h, d, scale, keep, salt,
            rng_state().data_ptr())


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

    qkv: [B, S, 3, h, d] (d = 64 or 128), mask: [B, 1, 1, S] additive or
    None. d = 128 (1 <= S <= 4096, mask or causal, no segment_ids): the
    chunked kernels of ops/hip/attention_d128.hip at every S; out is saved
    for the backward, whose dQ kernel takes the row dots from dO * O, and the
    fp32 row dots [B*h*S] are the only scratch.
    segment_ids (packed sequences, 2 <= S <= 4096, no mask): integer
    [B, S], q attends k iff their ids are equal; equal ids must form one
    contiguous run per row, which is NOT checked here (a check would
    synchronise). The ids are converted to int32 once and saved; above
    S = 128 the block bounds are computed once and saved with them, up to
    S = 128 each wave finds its range from the ids (the segment mode of the
    keys-on-rows kernels; the env switches of the backward do not apply).
    causal (2 <= S <= 4096, no mask, with or without segment_ids): q attends
    k iff k <= q, and the ids equal where given: the triangle mode of the
    same kernels, which skip the tiles and chunks past the diagonal. Nothing
    beyond the segment mode's tensors is saved, and nothing at all for the
    triangle itself.
    Returns [B, S, h, d].
    """

    @staticmethod
    def forward(ctx, qkv, mask, scale, dropout_p, training, segment_ids=None,
                causal=False):
        B, S, three, h, d = qkv.shape
        assert three == 3 and d in (64, ATTN_D128) and S <= ATTN_LONG_SMAX
        assert d == 64 or segment_ids is None
        qkv = qkv.contiguous()
        mask = mask.contiguous() if mask is not None else None
        keep = 1.0 - dropout_p if (dropout_p > 0 and training) else 1.0
        assert not causal or (mask is None and S >= 2)
        seg = ()
        if segment_ids is not None:
            assert mask is None and S >= 2 and segment_ids.shape == (B, S)
            seg = _attn_seg(segment_ids)
        out, m, lsum, salt = _attn_fwd(qkv, mask, scale, keep, seg or None, causal)
        # the long backward takes its row dots from dO * O
        extra = (out,) if S > ATTN_SMAX or d == ATTN_D128 else ()
        ctx.save_for_backward(qkv, mask, m, lsum, *extra, *seg)
        ctx.scale, ctx.keep, ctx.salt, ctx.causal = scale, keep, salt, causal
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = hiplib.require()
        qkv, mask, m, lsum, *extra = ctx.saved_tensors
        B, S, _, h, d = qkv.shape
        dev = qkv.device
        if d == ATTN_D128:
            # dQ + dot, then dK/dV (ops/hip/attention_d128.hip), every S
            dout = dout.contiguous()
            dqkv = torch.empty_like(qkv)
            dot = torch.empty(B * h * S, dtype=torch.float32, device=dev)
            args = _attn_long_bwd_args(
                qkv, dout, extra[0], mask, m, lsum, dot, dqkv, ctx.scale,
                ctx.keep, ctx.salt)
            if ctx.causal:  # no mask pointer
                check(lib.sky_attn_d128_causal_bwd(*args[:4], *args[5:]),
                      "sky_attn_d128_causal_bwd")
            else:
                check(lib.sky_attn_d128_bwd(*args), "sky_attn_d128_bwd")
            return dqkv, None, None, None, None, None, None
        if S > ATTN_SMAX:
            # dQ + dot, then dK/dV (ops/hip/attention_long.hip); the env
            # switches below select among the S <= 128 kernels only
            dout = dout.contiguous()
            dqkv = torch.empty_like(qkv)
            dot = torch.empty(B * h * S, dtype=torch.float32, device=dev)
            args = _attn_long_bwd_args(
                qkv, dout, extra[0], mask, m, lsum, dot, dqkv, ctx.scale,
                ctx.keep, ctx.salt)
            if ctx.causal:  # (out,) or (out, ids, bounds)
                args = args[:4] + _attn_ids(extra[1:], 2) + args[5:]
                check(lib.sky_attn_long_causal_bwd(*args), "sky_attn_long_causal_bwd")
            elif len(extra) == 3:  # (out, ids, bounds): the segment form
                args = args[:4] + (ptr(extra[1]), ptr(extra[2])) + args[5:]
                check(lib.sky_attn_long_seg_bwd(*args), "sky_attn_long_seg_bwd")
            else:
                check(lib.sky_attn_long_bwd(*args), "sky_attn_long_bwd")
            return dqkv, None, None, None, None, None, None
        if extra or ctx.causal:
            # (ids,): the segment mode of the keys-on-rows pair (causal: its
            # triangle mode, with or without ids); its only scratch is the
            # fp32 row dots, passed in pdT's place
            dout = dout.contiguous()
            dqkv = torch.empty_like(qkv)
            dot = torch.empty(B * h * S, dtype=torch.float32, device=dev)
            entry = "sky_attn_causal_bwd" if ctx.causal else "sky_attn_seg_bwd"
            check(
                getattr(lib, entry)(
                    _stream(), ptr(qkv), ptr(dout), *_attn_ids(extra, 1), ptr(m),
                    ptr(lsum), ptr(dot), 0, ptr(dqkv), B, S, h, d, ctx.scale,
                    ctx.keep, ctx.salt, rng_state().data_ptr(),
                ),
                entry,
            )
            return dqkv, None, None, None, None, None, None
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
                return dqkv, None, None, None, None, None, None
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
            return dqkv, None, None, None, None, None, None
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
        return dqkv, None, None, None, None, None, None


class FusedGqaAttentionFn(torch.autograd.Function):
    """Grouped-query attention at head dim 128 (bf16, 1 <= S <= 4096, causal:
    2 <= S): h query heads on h_kv shared key / value heads, the
    sky_attn_d128_gqa_* entry points of ops/hip/attention_d128.hip.

    qkv: [B, S, h + 2*h_kv, 128], query heads, then key heads, then value
    heads; query head hh attends K/V head hh // (h // h_kv). mask:
    [B, 1, 1, S] additive or None; causal takes no mask. Forward and dQ run
    one block per query head on the shared K/V columns; the dK/dV kernel
    runs one block per K/V head and sums the group's heads in its registers,
    so dqkv holds each shared head's gradient rounded once. Saves qkv, mask,
    m, l and out; the fp32 row dots [B*h*S] are the only scratch. Dropout
    draws by the query head, so for equal (salt, state, B, S, h) the keep
    mask is FusedAttentionFn's on the expanded heads. Returns [B, S, h, 128].
    """

    @staticmethod
    def forward(ctx, qkv, mask, num_kv_heads, scale, dropout_p, training,
                causal=False):
        lib = hiplib.require()
        B, S, heads, d = qkv.shape
        h = heads - 2 * num_kv_heads
        assert d == ATTN_D128 and 1 <= num_kv_heads <= h and h % num_kv_heads == 0
        assert S <= ATTN_LONG_SMAX and (not causal or (mask is None and S >= 2))
        qkv = qkv.contiguous()
        mask = mask.contiguous() if mask is not None else None
        keep = 1.0 - dropout_p if (dropout_p > 0 and training) else 1.0
        out = torch.empty(B, S, h, d, dtype=qkv.dtype, device=qkv.device)
        m = torch.empty(B, h, S, dtype=torch.float32, device=qkv.device)
        lsum = torch.empty_like(m)
        salt = _next_seed() if keep < 1.0 else 0
        name = "sky_attn_d128_gqa_causal_fwd" if causal else "sky_attn_d128_gqa_fwd"
        masks = () if causal else (ptr(mask),)  # the causal entry takes no mask
        check(
            getattr(lib, name)(
                _stream(), ptr(qkv), *masks, ptr(out), ptr(m), ptr(lsum), B, S,
                h, num_kv_heads, d, scale, keep, salt, rng_state().data_ptr(),
            ),
            name,
        )
        ctx.save_for_backward(qkv, mask, m, lsum, out)
        ctx.h_kv, ctx.scale, ctx.keep = num_kv_heads, scale, keep
        ctx.salt, ctx.causal = salt, causal
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = hiplib.require()
        qkv, mask, m, lsum, out = ctx.saved_tensors
        B, S, h, d = out.shape
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dot = torch.empty(B * h * S, dtype=torch.float32, device=qkv.device)
        name = "sky_attn_d128_gqa_causal_bwd" if ctx.causal else "sky_attn_d128_gqa_bwd"
        masks = () if ctx.causal else (ptr(mask),)
        check(
            getattr(lib, name)(
                _stream(), ptr(qkv), ptr(dout), ptr(out), *masks, ptr(m),
                ptr(lsum), ptr(dot), ptr(dqkv), B, S, h, ctx.h_kv, d, ctx.scale,
                ctx.keep, ctx.salt, rng_state().data_ptr(),
            ),
            name,
        )
        return dqkv, None, None, None, None, None, None


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
    bf16, d = 64, S <= 4096 only (the fused attention kernels' domain; the
    long kernels above S = 128); mask [B, 1, 1, S] additive or None.
    segment_ids (packed sequences, S >= 2) in place of mask: integer [B, S]
    as in FusedAttentionFn, whose segment forward this runs; the backward
    takes the segment forms of the dbias entry points (the bounds table of
    S > 128 is computed once in forward and saved). causal (S >= 2, no mask,
    with or without segment_ids): the triangle mode, as FusedAttentionFn."""

    @staticmethod
    def forward(ctx, hidden, wqkv, bqkv, mask, num_heads, attn_p, wo, bo,
                ln_w, ln_b, eps, hidden_p, segment_ids=None, causal=False):
        B, S, H = hidden.shape
        d = H // num_heads
        assert d == 64 and S <= ATTN_LONG_SMAX and hidden.dtype == torch.bfloat16
        hidden = hidden.contiguous()
        x2 = hidden.view(-1, H)
        qkv = _linear_fwd(x2, wqkv, bqkv).view(B, S, 3, num_heads, d)
        mask = mask.contiguous() if mask is not None else None
        scale = 1.0 / math.sqrt(d)
        akeep = 1.0 - attn_p
        assert not causal or (mask is None and S >= 2)
        seg = ()
        if segment_ids is not None:
            assert mask is None and S >= 2 and segment_ids.shape == (B, S)
            seg = _attn_seg(segment_ids)
        ctxl, m, lsum, asalt = _attn_fwd(qkv, mask, scale, akeep, seg or None,
                                         causal)
        c2 = ctxl.view(-1, H)
        h = _linear_fwd(c2, wo, bo).view(B, S, H)
        keep = 1.0 - hidden_p
        y, mean, rstd, salt = _ln_fwd(h, hidden, ln_w, ln_b, eps, keep)
        ctx.save_for_backward(x2, wqkv, qkv, mask, m, lsum, c2, wo, h, ln_w,
                              mean, rstd, *seg)
        ctx.scale, ctx.akeep, ctx.asalt = scale, akeep, asalt
        ctx.keep, ctx.salt, ctx.causal = keep, salt, causal
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = hiplib.require()
        (x2, wqkv, qkv, mask, m, lsum, c2, wo, h, ln_w, mean,
         rstd, *seg) = ctx.saved_tensors
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
        # the S <= 128 scratch first, then the slabs: the allocation order
        # this node has always had
        if S > ATTN_SMAX or seg or ctx.causal:
            scratch = (torch.empty(B * nh * S, dtype=torch.float32, device=qkv.device),)
        else:
            scratch = _attn_bwd_scratch(qkv)
        # column partials of dqkv, one slab per (batch, 64-query block);
        # the kernels write every element, so no memset
        slabs = torch.empty(B * ((S + 63) // 64) * 3 * H, dtype=torch.float32,
                            device=qkv.device)
        if S > ATTN_SMAX:
            # c2 is the attention output the forward saved for dWo;
            # scratch is dot, fp32 [B*h*S]
            entry = "sky_attn_long_bwd_dbias"
            args = _attn_long_bwd_args(qkv, dctx, c2, mask, m, lsum, scratch[0],
                                       dqkv, ctx.scale, ctx.akeep, ctx.asalt)
            if ctx.causal:  # (ids, bounds) or (0, 0) in the mask's place
                entry = "sky_attn_long_causal_bwd_dbias"
                args = args[:4] + _attn_ids(seg, 2) + args[5:]
            elif seg:  # (ids, bounds) in the mask's place
                entry = "sky_attn_long_seg_bwd_dbias"
                args = args[:4] + (ptr(seg[0]), ptr(seg[1])) + args[5:]
        elif seg or ctx.causal:
            # (ids,) in the mask's place (causal: ids or 0); the row dots are
            # the only scratch
            entry = "sky_attn_causal_bwd_dbias" if ctx.causal else "sky_attn_seg_bwd_dbias"
            args = (_stream(), ptr(qkv), ptr(dctx), *_attn_ids(seg, 1), ptr(m),
                    ptr(lsum), ptr(scratch[0]), 0, ptr(dqkv), B, S, nh, d,
                    ctx.scale, ctx.akeep, ctx.asalt, rng_state().data_ptr())
        else:
            entry = "sky_attn_bwd_dbias"
            pdT, dsT = scratch
            args = (_stream(), ptr(qkv), ptr(dctx), ptr(mask), ptr(m),
                    ptr(lsum), ptr(pdT), ptr(dsT), ptr(dqkv), B, S, nh, d,
                    ctx.scale, ctx.akeep, ctx.asalt, rng_state().data_ptr())
        args += (ptr(slabs), ptr(dbqkv), _dt(dbqkv))
        if pending is not None:
            check(getattr(lib, entry + "_parts")(*args, pending.slot()),
                  entry + "_parts")
            pending.took(slabs)
            pending.run()
        else:
            check(getattr(lib, entry)(*args), entry)
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
                d_ln_w, d_ln_b, None, None, None, None)


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
