#!/usr/bin/env python3
"""Time one FusedLAMB step on the 24-layer pretraining model's parameters.

The parameter set of the masked-LM model (embeddings, 24 encoder layers,
BertLMHead; H=1024) in bf16 with fp32 masters, clipping on, gradients in
place. In ONE process, warmed, in alternating rounds, each window timed by
device events:
  lamb        FusedLAMB(max_grad_norm=1.0, no_decay="1d")     42 B/element
  adamw       FusedAdamW(max_grad_norm=1.0, no_decay="1d")    30 B/element
  sgd-mom     FusedSGD(momentum=0.9)                          20 B/element
  eager-lamb  ops.eager.lamb_step on the same kind of GPU tensors
Bytes per element are counts of what each step has to move (the update
kernels' 40 / 28 / 20 plus 2 for the gradient norm's read of g), not
measurements; TB/s = count / time.

    python tools/lamb_bench.py [--layers 24] [--steps 100] [--rounds 3]
                               [--only lamb]
Prints one line per variant and round, then one JSON line with the median
ms and the min-max spread over rounds. Needs a GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--eager-steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="time this variant alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lamb_bench needs a GPU")

    from skycomputing_amd import ops
    from skycomputing_amd.builder import build_module_from_cfg
    from skycomputing_amd.models import bert_pretraining_pipeline_config
    from skycomputing_amd.ops import hiplib
    from skycomputing_amd.optim import FusedAdamW, FusedLAMB, FusedSGD

    hiplib.require()
    torch.manual_seed(0)
    cfgs = bert_pretraining_pipeline_config(
        args.layers, dict(vocab_size=30522, hidden_size=1024, num_attention_heads=16,
                          intermediate_size=4096, max_position_embeddings=512))
    model = build_module_from_cfg(cfgs, device="cuda:0", dtype=torch.bfloat16,
                                  record_forward_time=False)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    n = sum(torch.Size(s).numel() for s in shapes)
    print(f"{len(shapes)} tensors, {n} parameters", flush=True)

    def make_params():
        # each optimizer owns its parameters, so every launch plan is built once
        ps = [(0.02 * torch.randn(s, device="cuda")).to(torch.bfloat16).requires_grad_(True)
              for s in shapes]
        for p in ps:
            p.grad = (0.01 * torch.randn(p.shape, device="cuda")).to(torch.bfloat16)
        return ps

    def eager_variant():
        ps = make_params()
        opt = FusedLAMB(ps, lr=1e-3, max_grad_norm=1.0, no_decay="1d")
        t = [0]

        def step():
            t[0] += 1
            ops.eager.lamb_step(
                opt.params, [p.grad for p in ps], opt.exp_avgs, opt.exp_avg_sqs, t[0],
                opt.lr, *opt.betas, opt.eps, opt.weight_decay, opt.masters,
                opt.max_grad_norm, opt.no_decay, opt.adapt)
        return step

    makers = {
        "lamb": lambda: (FusedLAMB(make_params(), lr=1e-3, max_grad_norm=1.0,
                                   no_decay="1d").step, 42, args.steps),
        "adamw": lambda: (FusedAdamW(make_params(), lr=1e-3, max_grad_norm=1.0,
                                     no_decay="1d").step, 30, args.steps),
        "sgd-mom": lambda: (FusedSGD(make_params(), lr=1e-3, momentum=0.9).step, 20,
                            args.steps),
        "eager-lamb": lambda: (eager_variant(), None, args.eager_steps),
    }
    if args.only is not None:
        makers = {args.only: makers[args.only]}
    variants = {name: make() for name, make in makers.items()}

    for step, _, _ in variants.values():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()

    times = {k: [] for k in variants}
    for r in range(args.rounds):
        for name, (step, nbytes, steps) in variants.items():
            start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            torch.cuda.synchronize()
            start.record()
            for _ in range(steps):
                step()
            end.record()
            torch.cuda.synchronize()
            ms = start.elapsed_time(end) / steps
            times[name].append(ms)
            rate = f"{n * nbytes / ms / 1e9:6.2f} TB/s ({nbytes} B/element)" if nbytes else ""
            print(f"round {r} {name:11s} {ms:8.3f} ms/step  {rate}", flush=True)

    result = {"tensors": len(shapes), "params": n, "rounds": args.rounds}
    for name, (_, nbytes, steps) in variants.items():
        ts = times[name]
        med = statistics.median(ts)
        result[name] = {"ms_median": round(med, 4), "ms_min": round(min(ts), 4),
                        "ms_max": round(max(ts), 4), "steps_per_window": steps}
        if nbytes:
            result[name]["bytes_per_element"] = nbytes
            result[name]["tbps_median"] = round(n * nbytes / med / 1e9, 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
