#!/usr/bin/env python3
"""Time the optimizer steps against each other on ~1B bf16 parameters.

In ONE process, warmed, in alternating rounds, each window ending in a
device synchronise:
  adamw         FusedAdamW (fp32 masters), no clipping       28 B/element
  adamw+clip    FusedAdamW(max_grad_norm=1.0)                30 B/element
  sgd-mom       FusedSGD(momentum=0.9) (fp32 masters)        20 B/element
  torch-fused   torch.optim.AdamW(fused=True) on fp32 masters with fp32
                gradients already in place, then _foreach_copy_ into the
                bf16 parameters                              34 B/element
Bytes per element are counts of what each step has to move (reads and
writes of g, p, master, m, v), not measurements; TB/s = count / time.

    python tools/adamw_bench.py [--tensors 8] [--numel 134217728]
                                [--steps 80] [--rounds 3]
Prints one line per variant and round, then one JSON line with the median
ms and the min-max spread over rounds. Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tensors", type=int, default=8)
    ap.add_argument("--numel", type=int, default=128 << 20)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adamw_bench needs a GPU")

    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.optim import FusedAdamW, FusedSGD

    hiplib.require()
    torch.manual_seed(0)

    def make_params():
        ps = [torch.randn(args.numel, dtype=torch.bfloat16, device="cuda", requires_grad=True)
              for _ in range(args.tensors)]
        for p in ps:
            p.grad = (0.01 * torch.randn(args.numel, device="cuda")).to(torch.bfloat16)
        return ps

    # each optimizer owns its parameters, so every launch plan is built once
    variants = {}
    p_adam, p_clip, p_sgd, p_torch = (make_params() for _ in range(4))
    adam = FusedAdamW(p_adam, lr=1e-3)
    clip = FusedAdamW(p_clip, lr=1e-3, max_grad_norm=1.0)
    sgd = FusedSGD(p_sgd, lr=1e-3, momentum=0.9)
    variants["adamw"] = (adam.step, 28)
    variants["adamw+clip"] = (clip.step, 30)
    variants["sgd-mom"] = (sgd.step, 20)

    masters = [torch.nn.Parameter(p.detach().float()) for p in p_torch]
    for m, p in zip(masters, p_torch):
        m.grad = p.grad.float()
    topt = torch.optim.AdamW(masters, lr=1e-3, weight_decay=0.01, fused=True)
    p_torch_data = [p.detach() for p in p_torch]
    m_torch_data = [m.detach() for m in masters]

    def torch_step():
        topt.step()
        torch._foreach_copy_(p_torch_data, m_torch_data)

    variants["torch-fused"] = (torch_step, 34)

    n = args.tensors * args.numel
    for step, _ in variants.values():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()

    times = {k: [] for k in variants}
    for r in range(args.rounds):
        for name, (step, nbytes) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            times[name].append(dt)
            print(f"round {r} {name:12s} {dt * 1e3:8.3f} ms/step  "
                  f"{n * nbytes / dt / 1e12:6.2f} TB/s ({nbytes} B/element)", flush=True)

    result = {"params": n, "steps_per_window": args.steps, "rounds": args.rounds}
    for name, (_, nbytes) in variants.items():
        ts = times[name]
        med = statistics.median(ts)
        result[name] = {
            "ms_median": round(med * 1e3, 4),
            "ms_min": round(min(ts) * 1e3, 4),
            "ms_max": round(max(ts) * 1e3, 4),
            "bytes_per_element": nbytes,
            "tbps_median": round(n * nbytes / med / 1e12, 3),
        }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
