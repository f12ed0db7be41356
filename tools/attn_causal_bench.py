#!/usr/bin/env python3
"""Causal attention, bf16, p = 0.1, no ids, forward + backward of
  causal: the triangle mode of the hand kernels (FusedAttentionFn, causal=True),
  dense:  the same kernels with mask = None and no triangle (twice the visible pairs),
  sdpa:   torch scaled_dot_product_attention(is_causal=True).
Shapes of profiles/r16_notes.md: --batch 32 --seq 128, --batch 8 --seq 512,
--batch 2 --seq 2048, h = 16. Device events around ITERS steps, ROUNDS alternating
rounds after warm-up, one process; prints one JSON line (us per step, median and
range over the rounds).
--trace: a few steps of causal and dense only, for a kernel trace."""

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
ap.add_argument("--heads", type=int, default=16)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
B, S, h, d, P = args.batch, args.seq, args.heads, 64, 0.1
ROUNDS, ITERS = 5, 20

torch.manual_seed(0)
qkv = torch.randn(B, S, 3, h, d, dtype=torch.bfloat16, device="cuda", requires_grad=True)
dout = torch.randn(B, S, h, d, dtype=torch.bfloat16, device="cuda")
scale = 1.0 / math.sqrt(d)


def sdpa():
    q, k, v = _split_heads(qkv)
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, is_causal=True, dropout_p=P).permute(0, 2, 1, 3)


variants = {
    "causal": lambda: FusedAttentionFn.apply(qkv, None, scale, P, True, None, True),
    "dense": lambda: FusedAttentionFn.apply(qkv, None, scale, P, True),
    "sdpa": sdpa,
}


def steps(fn, n):
    for _ in range(n):
        qkv.grad = None
        fn().backward(dout)


if args.trace:
    for name in ("causal", "dense"):
        steps(variants[name], 10)
    torch.cuda.synchronize()
    sys.exit(0)

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
# chunk visits of a 64-query block under the triangle against all chunks (S > 128)
QB, NCH = (S + 63) // 64, (S + 127) // 128
walked = sum(min(NCH, (qb * 64 + 63) // 128 + 1) for qb in range(QB)) / (QB * NCH)
print(json.dumps({
    "shape": [B, S, h, d], "p": P, "chunk_visits_share": walked,
    "us_per_step": {k: dict(median=sorted(v)[len(v) // 2], min=min(v), max=max(v))
                    for k, v in times.items()}}))
