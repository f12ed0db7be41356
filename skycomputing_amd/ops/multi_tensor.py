"""Multi-tensor optimizer launch planning (SGD and AdamW).

Packs per-parameter {param, grad, master, state...} pointers into a device
descriptor array (one entry per <=1M-element slab) so the whole stage
updates in ONE kernel launch (ops/hip/sgd.hip, ops/hip/adamw.hip). SGD rows
are {p, g, master, momentum, n, 0}; AdamW rows are {p, g, master, m, v, n,
flags} with flags bit 0 = "no weight decay". The plan is rebuilt only
when one of those pointers changes (autograd reuses .grad buffers and the
optimizer owns the rest, so in steady state this is built once).
"""

from __future__ import annotations

import os

import torch

from . import hiplib
from .hiplib import check

_SLAB = int(os.environ.get("SKY_SGD_SLAB", 1 << 18))  # elements per descriptor (256k default: 1M-elem slabs win standalone (5.5 vs 4.7 TB/s) but LOSE in-app (+0.6 ms/step) - tools/sgd_bench.py + c7 profile)

_PLAN_CACHE: dict = {}  # id(params) -> SGD plan, ("adamw", id(params)) -> AdamW plan


def _build_plan(params, grads, masters, *states, flags=None):
    """One int64 row per slab: [p, g, master, *state pointers, count, flag].
    ``states`` are fp32 per-parameter buffers (None for an absent one);
    ``flags`` is one int per parameter (0 when not given)."""
    rows = []
    for i, (p, g) in enumerate(zip(params, grads)):
        n = p.numel()
        pa, ga = p.data_ptr(), g.data_ptr()
        ma = masters[i].data_ptr() if masters is not None else 0
        sa = [s[i].data_ptr() if s is not None else 0 for s in states]
        esz_p = p.element_size()
        esz_g = g.element_size()
        flag = flags[i] if flags is not None else 0
        off = 0
        while off < n:
            cnt = min(_SLAB, n - off)
            rows.append([
                pa + off * esz_p, ga + off * esz_g,
                (ma + off * 4) if ma else 0,
                *[(a + off * 4) if a else 0 for a in sa],
                cnt, flag,
            ])
            off += cnt
    # pinned staging so the H2D copy is legal inside hipGraph capture
    cpu = torch.tensor(rows, dtype=torch.int64)
    try:
        cpu = cpu.pin_memory()
    except RuntimeError:
        pass
    return cpu.to(params[0].device, non_blocking=True), len(rows)


def _plan_signature(params, grads, masters, *states) -> tuple:
    """Every pointer (and count) a descriptor is built from. A parameter
    that gets new storage (``p.data = ...``, a checkpoint restore) keeps
    its ``.grad`` buffer, so grad pointers alone would leave the cached
    descriptors writing the old storage."""
    sig = [_SLAB]
    for group in (params, grads, masters, *states):
        if group is None:
            sig.append(None)
        else:
            sig.extend(t.data_ptr() for t in group)
    sig.extend(p.numel() for p in params)
    return tuple(sig)


def _cached_plan(key, sig, build):
    """The plan stored under ``key`` if it was built from ``sig``, else a
    fresh ``build()`` stored in its place. A plan is a tuple; the cache
    keeps ``(sig, *plan)``."""
    cached = _PLAN_CACHE.get(key)
    if cached is None or cached[0] != sig:
        cached = (sig, *build())
        _PLAN_CACHE[key] = cached
    return cached[1:]


def multi_tensor_sgd(params, grads, masters, moms, lr, momentum, wd):
    sig = _plan_signature(params, grads, masters, moms)
    desc, n = _cached_plan(
        id(params), sig, lambda: _build_plan(params, grads, masters, moms))
    lib = hiplib.require()
    dt = 1 if params[0].dtype == torch.bfloat16 else 0
    flags = (1 if masters is not None else 0) | (2 if moms is not None else 0)
    stream = torch.cuda.current_stream().cuda_stream
    check(
        lib.sky_sgd_step(stream, desc.data_ptr(), n, lr, momentum, wd, dt, flags),
        "sky_sgd_step",
    )


def _build_adamw_plan(params, grads, masters, exp_avgs, exp_avg_sqs, no_decay):
    # the kernels' 8-wide vector body assumes 16-byte aligned slab bases
    assert _SLAB % 8 == 0, _SLAB
    for group in (params, grads, masters, exp_avgs, exp_avg_sqs):
        for t in group or ():
            assert t.data_ptr() % 16 == 0, (
                f"tensor of shape {tuple(t.shape)} is not 16-byte aligned")
    desc, n = _build_plan(params, grads, masters, exp_avgs, exp_avg_sqs,
                          flags=[1 if nd else 0 for nd in no_decay])
    # per-slab sums of squares for the gradient norm (ops/hip/adamw.hip)
    partials = torch.zeros(n, dtype=torch.float32, device=params[0].device)
    return desc, n, partials


def multi_tensor_adamw(params, grads, masters, exp_avgs, exp_avg_sqs, hyper,
                       beta1, beta2, eps, wd, no_decay, max_grad_norm=None):
    """One AdamW step over all tensors: the gradient norm and clip factor
    (when ``max_grad_norm`` is set), the device step counter's tick, and the
    update. ``hyper`` is the optimizer's device hyper block (layout in
    ops/hip/adamw.hip): lr, the clip factor and the bias corrections are
    read from it by the kernels, so nothing here changes between the
    replays of a captured step. ``no_decay``: one bool per parameter."""
    sig = _plan_signature(params, grads, masters, exp_avgs, exp_avg_sqs)
    sig += tuple(bool(nd) for nd in no_decay)
    desc, n, partials = _cached_plan(
        ("adamw", id(params)), sig,
        lambda: _build_adamw_plan(params, grads, masters, exp_avgs,
                                  exp_avg_sqs, no_decay))
    lib = hiplib.require()
    dt = 1 if params[0].dtype == torch.bfloat16 else 0
    flags = 1 if masters is not None else 0
    stream = torch.cuda.current_stream().cuda_stream
    if max_grad_norm is not None:
        check(lib.sky_gradnorm_partials(stream, desc.data_ptr(), n,
                                        partials.data_ptr(), dt),
              "sky_gradnorm_partials")
        check(lib.sky_gradnorm_finish(stream, partials.data_ptr(), n,
                                      hyper.data_ptr(), max_grad_norm),
              "sky_gradnorm_finish")
    check(lib.sky_adamw_tick(stream, hyper.data_ptr(), beta1, beta2),
          "sky_adamw_tick")
    check(
        lib.sky_adamw_step(stream, desc.data_ptr(), n, hyper.data_ptr(),
                           beta1, beta2, eps, wd, dt, flags),
        "sky_adamw_step",
    )
