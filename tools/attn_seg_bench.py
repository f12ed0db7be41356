#!/usr/bin/env python3
"""Packed-sequence attention at B = 32, h = 12, S = 512, bf16, p = 0.1,
forward + backward of
  seg:   the segment kernels, four runs of random lengths per row,
  dense: the long kernels with mask = None (the dense upper bound),
  sdpa:  torch sdpa with the dense boolean [B, 1, S, S] mask.
Device events around ITERS steps, ROUNDS alternating rounds after warm-up;
prints one JSON line (us per step, median and range over the rounds).
--trace: a few steps of seg and dense only, for a kernel trace."""

import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from skycomputing_amd.ops import eager  # noqa: E402
from skycomputing_amd.ops.functions import FusedAttentionFn, _split_heads  # noqa: E402

B, S, h, d, P = 32, 512, 12, 64, 0.1
ROUNDS, ITERS = 5, 20

gen = torch.Generator().manual_seed(0)
ids = torch.zeros(B, S, dtype=torch.int32)
for b in range(B):
    cuts = (torch.randperm(S - 1, generator=gen)[:3] + 1).sort().values.tolist()
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


if "--trace" in sys.argv:
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
bd = eager.seg_bounds(ids)
print(json.dumps({
    "shape": [B, S, h, d], "p": P, "runs_per_row": int(runs.max()),
    "chunks_walked_per_block": float(((bd[..., 1] + 127) // 128 - bd[..., 0] // 128).float().mean()),
    "sum_len2_over_S2": float((same.sum((-1, -2)).float() / (S * S)).mean()),
    "us_per_step": {k: dict(median=sorted(v)[len(v) // 2], min=min(v), max=max(v))
                    for k, v in times.items()}}))
