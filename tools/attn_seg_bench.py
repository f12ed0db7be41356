#!/usr/bin/env python3
"""Packed-sequence attention, bf16, p = 0.1, forward + backward of
  seg:   the segment kernels, --runs runs of random lengths per row (seed 0),
  dense: the same kernels with mask = None (the dense upper bound),
  sdpa:  torch sdpa with the dense boolean [B, 1, S, S] mask.
Default shape B = 32, h = 12, S = 512 (the long kernels); --seq 128 --heads 16
is the benchmark's attention shape (the one-chunk kernels' segment mode).
Device events around ITERS steps, ROUNDS alternating rounds after warm-up;
prints one JSON line (us per step, median and range over the rounds).
--trace: a few steps of seg and dense only, for a kernel trace."""

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from skycomputing_amd.ops import eager  # noqa: E402
from skycomputing_amd.ops.functions import FusedAttentionFn, _split_heads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--seq", type=int, default=512)
ap.add_argument("--heads", type=int, default=12)
ap.add_argument("--runs", type=int, default=4, help="runs per row; 1 = one run")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
B, S, h, d, P = args.batch, args.seq, args.heads, 64, 0.1
ROUNDS, ITERS = 5, 20

gen = torch.Generator().manual_seed(0)
ids = torch.zeros(B, S, dtype=torch.int32)
for b in range(B):
    cuts = (torch.randperm(S - 1, generator=gen)[:args.runs - 1] + 1).sort().values.tolist()
    for j, c in enumerate(cuts):
        ids[b, c:] = j + 1
ids = ids.cuda()
same = eager.segment_mask(ids, check=False)
torch.manual_seed(0)
qkv = torch.randn(B, S, 3, h, d, dtype=torch.bfloat16, device="cuda", requires_grad=True)
dout = torch.randn(B, S, h, d, dtype=torch.bfloat16, device="cuda")
scale = 1.0 / math.sqrt(d)


def sdpa():
    q, k, v = _split_heads(qkv)
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, attn_mask=same, dropout_p=P).permute(0, 2, 1, 3)


variants = {
    "seg": lambda: FusedAttentionFn.apply(qkv, None, scale, P, True, ids),
    "dense": lambda: FusedAttentionFn.apply(qkv, None, scale, P, True),
    "sdpa": sdpa,
}


def steps(fn, n):
    for _ in range(n):
        qkv.grad = None
        fn().backward(dout)


if args.trace:
    for name in ("seg", "dense"):
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
runs = (ids[:, 1:] != ids[:, :-1]).sum(1) + 1
res = {"shape": [B, S, h, d], "p": P, "runs_per_row": int(runs.max()),
       "sum_len2_over_S2": float((same.sum((-1, -2)).float() / (S * S)).mean())}
if S > 128:
    bd = eager.seg_bounds(ids)
    res["chunks_walked_per_block"] = float(
        ((bd[..., 1] + 127) // 128 - bd[..., 0] // 128).float().mean())
else:
    # a wave's 16 tokens: 16-token tiles and 32-token pairs between the run
    # start of its first token and the run end of its last one
    start, end = eager.seg_runs(ids)
    first = torch.arange(0, S, 16, device=ids.device)
    lo, hi = start[:, first], end[:, (first + 15).clamp(max=S - 1)]
    res["tiles_visited_share"] = float(
        (((hi + 15) // 16 - lo // 16).float() / ((S + 15) // 16)).mean())
    res["pairs_visited_share"] = float(
        (((hi + 31) // 32 - lo // 32).float() / ((S + 31) // 32)).mean())
res["us_per_step"] = {k: dict(median=sorted(v)[len(v) // 2], min=min(v), max=max(v))
                      for k, v in times.items()}
print(json.dumps(res))
