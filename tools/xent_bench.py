#!/usr/bin/env python3
"""Time ops.softmax_cross_entropy against the torch composition at the
masked-LM shape: logits [4096, 30528] bf16 with 30522 classes.

In ONE process, warmed, in alternating rounds, for (a) all rows valid and
(b) 15 % of the rows valid:
  fused          ops.softmax_cross_entropy(logits, labels, num_classes=V)
  fused-inplace  the same with inplace_backward=True (its logits are
                 overwritten each step, so after the first step it runs on
                 other values than the two above; times are comparable, losses
                 are not)
  torch          cross_entropy(logits[:, :V].float(), labels)
Forward and backward are timed apart with device events (recorded around
each phase of every step, read after a synchronise that ends the window);
fwd+bwd is their sum. The logits are the output of a stand-in producer node,
like a linear's output, so no variant keeps a .grad on them.

Peak memory is torch.cuda.max_memory_allocated over one forward + backward,
above what is allocated with the logits and labels in place.

Bytes are counts from the shapes (what the algorithm must move), not
measurements: forward reads the valid rows' V logits; backward reads them
again and writes every row's ld gradients. With --profile the run is only
12 fused steps of case (a), then 12 of case (b), and is meant to go under
`rocprofv3 --kernel-trace --stats` (no counters); --trace-db reads that
run's rocpd database, takes the median time of each case's xent_fwd and
xent_bwd dispatches and prints the achieved bytes/s (--kernel-times does
the same from four times in microseconds given by hand).

    python tools/xent_bench.py [--rows 4096] [--vocab 30522] [--steps 30]
                               [--rounds 3] [--profile]
    python tools/xent_bench.py --trace-db results.db
    python tools/xent_bench.py --kernel-times FWD_A BWD_A FWD_B BWD_B
Prints one line per variant, case and round, then one JSON line. Needs a
GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def algorithm_bytes(rows, valid_rows, V, ld, es=2):
    """(forward, backward) bytes the fused kernels have to move."""
    fwd = valid_rows * V * es
    bwd = valid_rows * V * es + rows * ld * es
    return fwd, bwd


PROFILE_STEPS = 12


def trace_kernel_times(db_path):
    """Median microseconds of xent_fwd / xent_bwd per case from the rocpd
    database of a --profile run: the dispatches in start order, the first
    PROFILE_STEPS of each kernel being case (a), the rest case (b)."""
    import sqlite3

    cur = sqlite3.connect(db_path).cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    disp = next(t for t in tabs if t.startswith("rocpd_kernel_dispatch"))
    sym = next(t for t in tabs if t.startswith("rocpd_info_kernel_symbol"))
    names = {r[0]: r[1] for r in cur.execute(f"select id, display_name from {sym}")}
    runs = {"xent_fwd_kernel": [], "xent_bwd_kernel": []}
    for kid, start, end in cur.execute(f"select kernel_id, start, end from {disp} order by start"):
        for key in runs:
            if key in names.get(kid, ""):
                runs[key].append((end - start) / 1e3)
    out = []
    for case in (0, 1):
        for key in ("xent_fwd_kernel", "xent_bwd_kernel"):
            ts = runs[key]
            if len(ts) != 2 * PROFILE_STEPS:
                sys.exit(f"{key}: {len(ts)} dispatches, expected {2 * PROFILE_STEPS}")
            out.append(statistics.median(ts[case * PROFILE_STEPS:(case + 1) * PROFILE_STEPS]))
    return out


class _Producer(torch.autograd.Function):
    """Hands out a preallocated logits buffer as a non-leaf, and drops the
    gradient that comes back: what a linear's output looks like to the loss,
    without the linear."""

    @staticmethod
    def forward(ctx, anchor, buf):
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, g):
        return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", action="store_true",
                    help="short run of the fused variant only, for a kernel trace")
    ap.add_argument("--kernel-times", type=float, nargs=4, default=None,
                    metavar=("FWD_A", "BWD_A", "FWD_B", "BWD_B"),
                    help="mean kernel us from a trace -> achieved bytes/s (no GPU needed)")
    ap.add_argument("--trace-db", default=None,
                    help="rocpd database of a --profile run -> achieved bytes/s (no GPU needed)")
    args = ap.parse_args()
    if args.trace_db is not None:
        args.kernel_times = trace_kernel_times(args.trace_db)

    N, V = args.rows, args.vocab
    ld = (V + 63) // 64 * 64
    n_valid_b = int(round(0.15 * N))

    if args.kernel_times is not None:
        out = {}
        for tag, nv, (tf, tb) in (("a", N, args.kernel_times[:2]),
                                  ("b", n_valid_b, args.kernel_times[2:])):
            fb, bb = algorithm_bytes(N, nv, V, ld)
            out[tag] = {"fwd_us": round(tf, 2), "bwd_us": round(tb, 2),
                        "fwd_bytes": fb, "bwd_bytes": bb,
                        "fwd_tbps": round(fb / (tf * 1e-6) / 1e12, 3),
                        "bwd_tbps": round(bb / (tb * 1e-6) / 1e12, 3)}
        print(json.dumps(out))
        return

    if not torch.cuda.is_available():
        sys.exit("xent_bench needs a GPU")
    from skycomputing_amd import ops
    from skycomputing_amd.ops import hiplib

    hiplib.require()
    torch.manual_seed(0)
    dev = "cuda"
    master = (3.0 * torch.randn(N, ld, device=dev)).to(torch.bfloat16)
    anchor = torch.zeros(1, device=dev, requires_grad=True)
    labels_a = torch.randint(0, V, (N,), device=dev)
    labels_b = torch.full((N,), -100, device=dev)
    pick = torch.randperm(N, device=dev)[:n_valid_b]
    labels_b[pick] = labels_a[pick]
    cases = {"a": labels_a, "b": labels_b}

    def fused(lg, lab):
        return ops.softmax_cross_entropy(lg, lab, num_classes=V)

    def fused_inplace(lg, lab):
        return ops.softmax_cross_entropy(lg, lab, num_classes=V, inplace_backward=True)

    def torch_comp(lg, lab):
        return torch.nn.functional.cross_entropy(lg[:, :V].float(), lab)

    variants = {"fused": fused, "fused-inplace": fused_inplace, "torch": torch_comp}
    if args.profile:
        variants = {"fused": fused}

    # every variant owns its logits buffer (the in-place one destroys its own)
    bufs = {name: master.clone() for name in variants}

    def step(name, lab, events=None):
        lg = _Producer.apply(anchor, bufs[name])
        if events:
            events[0].record()
        loss = variants[name](lg, lab)
        if events:
            events[1].record()
        loss.backward()
        if events:
            events[2].record()
        return loss

    if args.profile:
        for lab in cases.values():
            for _ in range(PROFILE_STEPS):
                step("fused", lab)
        torch.cuda.synchronize()
        return

    # peak memory of one forward + backward above the resident tensors
    memory = {}
    for name in variants:
        for tag, lab in cases.items():
            step(name, lab)  # warm: code objects, allocator pools
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            loss = step(name, lab)
            torch.cuda.synchronize()
            memory[f"{name}/{tag}"] = torch.cuda.max_memory_allocated() - base
            del loss
    for name in variants:
        bufs[name].copy_(master)
        for lab in cases.values():
            for _ in range(args.warmup):
                step(name, lab)
    torch.cuda.synchronize()

    times = {f"{n}/{t}": {"fwd": [], "bwd": []} for n in variants for t in cases}
    for r in range(args.rounds):
        for tag, lab in cases.items():
            for name in variants:
                evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)]
                       for _ in range(args.steps)]
                torch.cuda.synchronize()
                for e in evs:
                    step(name, lab, e)
                torch.cuda.synchronize()
                fwd = sum(e[0].elapsed_time(e[1]) for e in evs) / args.steps
                bwd = sum(e[1].elapsed_time(e[2]) for e in evs) / args.steps
                times[f"{name}/{tag}"]["fwd"].append(fwd)
                times[f"{name}/{tag}"]["bwd"].append(bwd)
                print(f"round {r} case {tag} {name:14s} fwd {fwd * 1e3:8.1f} us  "
                      f"bwd {bwd * 1e3:8.1f} us  sum {(fwd + bwd) * 1e3:8.1f} us", flush=True)

    result = {"rows": N, "vocab": V, "ld": ld, "valid_rows": {"a": N, "b": n_valid_b},
              "steps_per_window": args.steps, "rounds": args.rounds,
              "logits_bytes": N * ld * 2}
    for key, t in times.items():
        f, b = statistics.median(t["fwd"]), statistics.median(t["bwd"])
        result[key] = {
            "fwd_us": round(f * 1e3, 1), "bwd_us": round(b * 1e3, 1),
            "sum_us": round((f + b) * 1e3, 1),
            "sum_us_min": round(min(x + y for x, y in zip(t["fwd"], t["bwd"])) * 1e3, 1),
            "sum_us_max": round(max(x + y for x, y in zip(t["fwd"], t["bwd"])) * 1e3, 1),
            "peak_bytes_above_logits": memory[key],
        }
    if "torch" in variants:
        for tag in cases:
            result[f"speedup/{tag}"] = round(
                result[f"torch/{tag}"]["sum_us"] / result[f"fused/{tag}"]["sum_us"], 2)
        result["fused_b_over_a"] = round(
            result["fused/b"]["sum_us"] / result["fused/a"]["sum_us"], 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
