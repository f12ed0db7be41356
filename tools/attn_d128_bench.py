#!/usr/bin/env python3
"""Attention at head dim 128, bf16, p = 0.1, forward + backward of
  hand / sdpa:               the additive key mask (a padded tail) on both,
  hand_causal / sdpa_causal: causal=True against is_causal=True,
hand being FusedAttentionFn on ops/hip/attention_d128.hip and sdpa torch's
scaled_dot_product_attention on the same packed qkv.
Shapes of profiles/r17_notes.md (4096 tokens, h = 8): --batch 32 --seq 128,
--batch 8 --seq 512, --batch 2 --seq 2048. Device events around ITERS steps,
ROUNDS alternating rounds after warm-up, one process; prints one JSON line (us
per step, median and range over the rounds).

--kv-heads N (grouped-query attention, profiles/r18_notes.md): the packed qkv
is [B, S, h + 2*N, 128] and the variants, each with the mask and causal, are
  gqa:    FusedGqaAttentionFn, the grouped-query kernels,
  expand: eager.expand_kv + FusedAttentionFn, the multi-head kernels on K and
          V repeated per group, the expansion and its backward included,
  sdpa:   torch's, enable_gqa=True on the h_kv-head K and V."""

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from skycomputing_amd.ops.eager import expand_kv  # noqa: E402
from skycomputing_amd.ops.functions import (  # noqa: E402
    FusedAttentionFn, FusedGqaAttentionFn, _split_heads,
)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--seq", type=int, default=512)
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--kv-heads", type=int, default=None)
args = ap.parse_args()
B, S, h, kv, d, P = args.batch, args.seq, args.heads, args.kv_heads, 128, 0.1
ROUNDS, ITERS = 5, 20

torch.manual_seed(0)
shape = (B, S, 3, h, d) if kv is None else (B, S, h + 2 * kv, d)
qkv = torch.randn(shape, dtype=torch.bfloat16, device="cuda", requires_grad=True)
dout = torch.randn(B, S, h, d, dtype=torch.bfloat16, device="cuda")
mask = torch.zeros(B, 1, 1, S, dtype=torch.bfloat16, device="cuda")
mask[..., S - S // 8:] = -10000.0
scale = 1.0 / math.sqrt(d)


def sdpa(causal):
    if kv is None:
        q, k, v = _split_heads(qkv)
        gqa = {}
    else:
        q, k, v = (t.permute(0, 2, 1, 3) for t in qkv.split((h, kv, kv), dim=2))
        gqa = dict(enable_gqa=True)
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, attn_mask=None if causal else mask, is_causal=causal,
        dropout_p=P, **gqa).permute(0, 2, 1, 3)


if kv is None:
    variants = {
        "hand": lambda: FusedAttentionFn.apply(qkv, mask, scale, P, True),
        "sdpa": lambda: sdpa(False),
        "hand_causal": lambda: FusedAttentionFn.apply(qkv, None, scale, P, True, None, True),
        "sdpa_causal": lambda: sdpa(True),
    }
else:
    variants = {
        "gqa": lambda: FusedGqaAttentionFn.apply(qkv, mask, kv, scale, P, True),
        "expand": lambda: FusedAttentionFn.apply(expand_kv(qkv, kv), mask, scale, P, True),
        "sdpa": lambda: sdpa(False),
        "gqa_causal": lambda: FusedGqaAttentionFn.apply(qkv, None, kv, scale, P, True, True),
        "expand_causal": lambda: FusedAttentionFn.apply(
            expand_kv(qkv, kv), None, scale, P, True, None, True),
        "sdpa_causal": lambda: sdpa(True),
    }


def steps(fn, n):
    for _ in range(n):
        qkv.grad = None
        fn().backward(dout)


times = {name: [] for name in variants}
for name, fn in variants.items():
    steps(fn, 10)
torch.cuda.synchronize()
for _ in range(ROUNDS):
    for name, fn in variants.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        steps(fn, ITERS)
        t1.record()
        t1.synchronize()
        times[name].append(t0.elapsed_time(t1) * 1e3 / ITERS)
print(json.dumps({
    "shape": [B, S, h, d], "kv_heads": kv, "p": P,
    "us_per_step": {k: dict(median=sorted(v)[len(v) // 2], min=min(v), max=max(v))
                    for k, v in times.items()}}))
