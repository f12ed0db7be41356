#!/usr/bin/env python3
"""Flagship benchmark: 160-layer BERT (H=1024, A=16) training step,
MNLI-shaped synthetic data, bsz=32 seq=128, bf16, pipeline-parallel over
N MI355X GPUs (BASELINE.json metric: sec/iter).

Run directly (N=1) or under torch.distributed.run with --nproc-per-node N
(one rank per GPU over RCCL). Emits ONE JSON line from rank 0.

Extra knobs beyond the driver contract:
  --layers L            encoder layers (default 160)
  --allocate MODE       even | dynamic | optimal (default even)
  --microbatches M      pipeline microbatches (default: 1 if N==1 else N/2)
  --slowdowns CSV       per-rank injected compute slowdown factors
  --stimulate           seeded synthetic heterogeneity for the allocator
  --dump-outputs DIR    after the timed steps, write what the last timed step
                        returned/updated as DIR/<name>.npy (float32)
  --full                also run the benchmark's secondary measurements; a
                        plain run does only setup, warmup, the timed steps
                        and the result line (there are none today: the flag
                        is accepted so callers can rely on it)
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", 1)))
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--layers", type=int, default=160)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--seq", type=int, default=128)
    p.add_argument("--allocate", default="even", choices=["even", "dynamic", "optimal"])
    p.add_argument("--microbatches", type=int, default=0)
    p.add_argument("--schedule", default="gpipe", choices=["gpipe", "sequential", "1f1b"])
    p.add_argument("--virtual-stages", type=int, default=1,
                   help="interleaved chunks per rank (N>1; eager, no graphs)")
    p.add_argument("--slowdowns", default="")
    p.add_argument("--stimulate", action="store_true")
    p.add_argument("--dropout", type=float, default=0.1)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"],
                   help="compute dtype on GPU (CPU runs are always fp32)")
    p.add_argument("--no-graph", action="store_true",
                   help="disable hipGraph step capture (1-GPU path)")
    p.add_argument("--json-out", default="")
    p.add_argument("--dump-outputs", default="", metavar="DIR",
                   help="write the last timed step's outputs as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run secondary measurements (none today)")
    return p.parse_args()


_DUMP_PER_PARAM = 256  # sampled elements per parameter tensor


def dump_outputs(dirname, loss, params):
    """Write the arrays a caller of the timed step receives: the step's
    returned loss and the parameters it updated in place. The parameters
    are a fixed seeded sample (the full 160-layer model is ~8 GB in fp32):
    _DUMP_PER_PARAM flat indices per tensor, drawn from a private generator
    so the sample is identical from run to run and build to build."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    if loss is not None:
        val = float(loss.detach().float().cpu()) if torch.is_tensor(loss) else float(loss)
        np.save(os.path.join(dirname, "loss.npy"), np.asarray([val], dtype=np.float32))
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0xD0)
    chunks = []
    for prm in params:
        flat = prm.detach().reshape(-1)
        idx = torch.randint(0, flat.numel(), (_DUMP_PER_PARAM,), generator=gen)
        chunks.append(flat[idx.to(flat.device)].float().cpu())
    if chunks:
        np.save(os.path.join(dirname, "params_sample.npy"),
                torch.cat(chunks).numpy().astype(np.float32))


def main():
    args = parse_args()
    from skycomputing_amd.dataset import SyntheticGlueDataset
    from skycomputing_amd.dynamics import (
        Allocator, DeviceBenchmarker, ModelBenchmarker, WorkerManager,
    )
    from skycomputing_amd.models import bert_pipeline_config
    from skycomputing_amd.optim import FusedSGD
    from skycomputing_amd.parallel import PartitionPlan, PipelineEngine, init_distributed
    from skycomputing_amd.stimulator import Stimulator

    use_cuda = torch.cuda.is_available()
    comm = init_distributed()
    world = comm.world_size
    rank = comm.rank
    dtype = (
        torch.bfloat16 if (use_cuda and args.dtype == "bf16") else torch.float32
    )
    torch.manual_seed(1234 + rank)

    # Default microbatch count: measured at N=1, total work W(M) grows
    # steeply as microbatches shrink the GEMM/attention shapes (bsz 32:
    # W(1,2,4,8) = 110/166/253/439 ms) — the bubble model
    # step = (W(M)/N) * (M+N-1)/M then favors M ~= N/2 over the naive
    # M=N (predicted N=8: 87 ms at M=4 vs 103 at M=8).
    M = args.microbatches or (1 if world == 1 else max(1, world // 2))
    assert args.batch % M == 0

    bert_cfg = dict(
        hidden_size=1024, num_attention_heads=16, intermediate_size=4096,
        vocab_size=30522, max_position_embeddings=512,
        hidden_dropout_prob=args.dropout, attention_probs_dropout_prob=args.dropout,
    )
    layer_cfgs = bert_pipeline_config(args.layers, bert_cfg)
    L = len(layer_cfgs)

    slowdowns = [float(s) for s in args.slowdowns.split(",") if s] or [0.0] * world
    wm = WorkerManager.from_world(world, [dict(slowdown=s) for s in slowdowns])

    # ---- allocation ----
    if args.allocate == "even" and not args.stimulate:
        base, rem = divmod(L, world)
        bounds = [0]
        for i in range(world):
            bounds.append(bounds[-1] + base + (1 if i < rem else 0))
        plan = PartitionPlan(
            stage_ranks=list(range(world)),
            ranges=[(bounds[i], bounds[i + 1]) for i in range(world)],
        )
    else:
        stim = Stimulator(world) if args.stimulate else None
        db = DeviceBenchmarker(comm, batch_size=args.batch, seq_len=args.seq,
                               iterations=5, stimulator=stim)
        dev_results = db.benchmark(wm)
        mb = ModelBenchmarker(layer_cfgs, batch_size=args.batch // M, seq_len=args.seq)
        model_results = mb.benchmark() if rank == 0 else None
        if rank == 0:
            workers = [dict(rank=r, **dev_results[r]) for r in range(world)]
            alloc = Allocator(model_results["flops"], model_results["mem"], workers)
            v = args.virtual_stages if world > 1 else 1
            if v > 1:
                plan = alloc.interleaved_allocate(v)
            else:
                plan = alloc.allocate(args.allocate)
            plan_d = plan.to_dict()
        else:
            plan_d = None
        plan = PartitionPlan.from_dict(comm.broadcast_object(plan_d, src=0))

    sd = slowdowns[rank] if rank < len(slowdowns) else 0.0
    virtual = args.virtual_stages if world > 1 else 1
    if virtual > 1:
        from skycomputing_amd.parallel.interleaved import (
            InterleavedPipelineEngine, build_interleaved_plan,
        )

        if args.allocate == "even" and not args.stimulate:
            plan = build_interleaved_plan(L, world, virtual)
        # else: the benchmark-driven interleaved_allocate plan from above
        engine = InterleavedPipelineEngine(
            comm, layer_cfgs, plan,
            loss_fn=lambda logits, labels: torch.nn.functional.cross_entropy(
                logits.float(), labels
            ),
            dtype=dtype,
            stage_kwargs=dict(record_forward_time=bool(sd > 0), slowdown=sd),
        )
    else:
        engine = PipelineEngine(
            comm, layer_cfgs, plan,
            loss_fn=lambda logits, labels: torch.nn.functional.cross_entropy(
                logits.float(), labels
            ),
            dtype=dtype,
            stage_kwargs=dict(record_forward_time=bool(sd > 0), slowdown=sd),
        )
    opt = FusedSGD(engine.parameters(), lr=1e-3)

    ds = SyntheticGlueDataset(size=args.batch * 4, max_seq_length=args.seq, seed=7)
    loader = torch.utils.data.DataLoader(ds, batch_size=args.batch, shuffle=False, drop_last=True)
    batches = list(loader)

    graphed = None
    if use_cuda and sd == 0 and not args.no_graph and virtual > 1:
        from skycomputing_amd.parallel.interleaved_graph import GraphedInterleavedStep

        data0, labels0 = batches[0]
        try:
            graphed = GraphedInterleavedStep(engine, opt, M, list(data0), labels0)
        except Exception as e:  # pragma: no cover - eager fallback
            print(f"[bench] rank {rank}: interleaved graph capture failed "
                  f"({e!r}); falling back to eager", flush=True)
            graphed = None
    if (use_cuda and sd == 0 and not args.no_graph
            and args.schedule == "gpipe" and virtual == 1):
        data0, labels0 = batches[0]
        if world == 1 and M == 1:
            from skycomputing_amd.parallel.graph import GraphedTrainStep

            graphed = GraphedTrainStep(
                engine.stage, opt,
                lambda logits, labels: torch.nn.functional.cross_entropy(logits.float(), labels),
                list(data0), labels0,
            )
        elif engine.stage_idx is not None:
            from skycomputing_amd.parallel.static_exec import GraphedPipelineStep

            try:
                graphed = GraphedPipelineStep(engine, opt, M, list(data0), labels0)
            except Exception as e:  # pragma: no cover - safety net for the
                # unattended multi-GPU run: the eager schedule is comm-
                # compatible with graphed peers, so a per-rank fallback is
                # safe.
                print(f"[bench] rank {rank}: stage-graph capture failed "
                      f"({e!r}); falling back to eager", flush=True)
                graphed = None

    def step(i):
        data, labels = batches[i % len(batches)]
        if graphed is not None:
            return graphed.step(data, labels)
        opt.zero_grad(set_to_none=True)
        if virtual > 1:
            loss = engine.run_iteration(data, labels, num_microbatches=M)
        else:
            loss = engine.run_iteration(data, labels, num_microbatches=M,
                                        schedule=args.schedule)
        opt.step()
        return loss

    def barrier():
        # a one-rank world has nobody to wait for, and the first device
        # barrier would spend seconds creating an RCCL communicator that
        # the single-GPU step never uses
        if world > 1:
            comm.barrier()

    for i in range(args.warmup):
        step(i)
    barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last_loss = None
    for i in range(args.steps):
        last_loss = step(i)
    barrier()
    if use_cuda:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    elapsed = max(comm.all_gather_object(elapsed))
    sec_per_iter = elapsed / args.steps

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_loss, list(engine.parameters()))

    if rank == 0:
        result = {
            "metric": "sec_per_iter_bert160_mnli_bsz32",
            "value": sec_per_iter,
            "unit": "sec/iter",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": sec_per_iter * 1e3,
            "higher_is_better": False,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "bf16" if dtype == torch.bfloat16 else "fp32",
            "data": "synthetic",
            "config": {
                "model": f"bert-{args.layers}L-H1024-A16",
                "global_batch": args.batch,
                "seq_len": args.seq,
                "parallelism": (f"pp{world}x{virtual}" if virtual > 1
                                 else f"pp{world}"),
                "microbatches": M,
                "schedule": args.schedule,
                "allocate": args.allocate,
                "dropout": args.dropout,
                "num_pipeline_layers": L,
                "hipgraph": bool(graphed is not None),
            },
        }
        line = json.dumps(result)
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
