#!/usr/bin/env python3
"""Attention at head dim 128, bf16, p = 0.1, forward + backward of
  hand / sdpa:               the additive key mask (a padded tail) on both,
  hand_causal / sdpa_causal: causal=True against is_causal=True,
hand being FusedAttentionFn on ops/hip/attention_d128.hip and sdpa torch's
scaled_dot_product_attention on the same packed qkv.
Shapes of profiles/r17_notes.md (4096 tokens, h = 8): --batch 32 --seq 128,
--batch 8 --seq 512, --batch 2 --seq 2048. Device events around ITERS steps,
ROUNDS alternating rounds after warm-up, one process; prints one JSON line (us
per step, median and range over the rounds)."""

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from skycomputing_amd.ops.functions import FusedAttentionFn, _split_heads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--seq", type=int, default=512)
ap.add_argument("--heads", type=int, default=8)
args = ap.parse_args()
B, S, h, d, P = args.batch, args.seq, args.heads, 128, 0.1
ROUNDS, ITERS = 5, 20

torch.manual_seed(0)
qkv = torch.randn(B, S, 3, h, d, dtype=torch.bfloat16, device="cuda", requires_grad=True)
dout = torch.randn(B, S, h, d, dtype=torch.bfloat16, device="cuda")
mask = torch.zeros(B, 1, 1, S, dtype=torch.bfloat16, device="cuda")
mask[..., S - S // 8:] = -10000.0
scale = 1.0 / math.sqrt(d)


def sdpa(causal):
    q, k, v = _split_heads(qkv)
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, attn_mask=None if causal else mask, is_causal=causal,
        dropout_p=P).permute(0, 2, 1, 3)


variants = {
    "hand": lambda: FusedAttentionFn.apply(qkv, mask, scale, P, True),
    "sdpa": lambda: sdpa(False),
    "hand_causal": lambda: FusedAttentionFn.apply(qkv, None, scale, P, True, None, True),
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
    "shape": [B, S, h, d], "p": P,
    "us_per_step": {k: dict(median=sorted(v)[len(v) // 2], min=min(v), max=max(v))
                    for k, v in times.items()}}))
