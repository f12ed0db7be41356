"""FusedLAMB / the kernels of ops/hip/lamb.hip against the fp64 loop of
tests/lamb_checks.py, by its bounds; a bf16 parameter is its master rounded
or, without a master, within one bf16 rounding of the fp64 update of the
parameter the kernel read. Slabs are 1024 elements (lamb_checks.SIZES).
Gradients are fresh every step and copied into the same .grad tensors.
"""

import pytest
import torch

from . import kernel_checks as kc
from . import lamb_checks as lc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import hiplib, multi_tensor
    from skycomputing_amd.optim import FusedLAMB


@pytest.fixture(autouse=True)
def _gpu_lib_and_small_slab(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"
    monkeypatch.setattr(multi_tensor, "_SLAB", lc.SLAB)


KINDS = [(torch.float32, False), (torch.bfloat16, True), (torch.bfloat16, False)]
KIND_IDS = ["fp32-nomaster", "bf16-master", "bf16-nomaster"]


def _run(dtype, master, wd, max_norm, always_adapt=False, seed=17):
    start, history = lc.make_case(seed, "cuda", dtype)
    params = [p.clone().requires_grad_(True) for p in start]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = FusedLAMB(params, lr=lc.LR, weight_decay=wd, master_weights=master,
                    max_grad_norm=max_norm, no_decay=lc.NO_DECAY, always_adapt=always_adapt)
    ref = lc.LambRef64(start, wd, max_norm, lc.NO_DECAY, always_adapt)
    nomaster_bf16 = dtype == torch.bfloat16 and not master
    for grads in history:
        for p, g in zip(params, grads):
            p.grad.copy_(g)  # same .grad tensors: the plan is built once
        before = [p.detach().clone() for p in params]
        opt.step()
        ref.step(grads, lc.LR, params_read=before if nomaster_bf16 else None)
        if nomaster_bf16:
            for k, p in enumerate(params):
                kc.assert_bf16_close(p.detach(), ref.p[k], 0.0, f"param[{lc.SIZES[k]}]")
    return params, opt, ref


@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("dtype,master", KINDS, ids=KIND_IDS)
def test_fused_lamb_matches_fp64_loop(dtype, master, wd, max_norm):
    params, opt, ref = _run(dtype, master, wd, max_norm)
    assert (opt.masters is not None) == master
    assert ("lamb", id(opt.params)) in multi_tensor._PLAN_CACHE
    assert opt.step_count == lc.STEPS
    assert max_norm is None or ref.clip < 0.5  # the clip was active
    lc.assert_state(opt, params, ref)
    lc.assert_norms(opt, ref)
    ratios = opt.trust_ratios.tolist()
    assert ratios[1] == 1.0 and ratios[3] == 1.0  # exempt: plain Adam
    # the zero-gradient tensor: no moments, no NaN, u = wd*p
    z = lc.ZERO_G
    assert not opt.exp_avgs[z].any() and not opt.exp_avg_sqs[z].any()
    assert torch.isfinite(params[z]).all()
    assert ratios[z] == (1.0 if wd == 0.0 else pytest.approx(1.0 / wd, rel=1e-6))

    # no atomics, fixed summation order: the same case gives the same bits
    params2, opt2, _ = _run(dtype, master, wd, max_norm)
    assert torch.equal(opt.trust_ratios, opt2.trust_ratios)
    for k in range(len(params)):
        assert torch.equal(params[k].detach(), params2[k].detach()), k
        assert torch.equal(opt.exp_avgs[k], opt2.exp_avgs[k]), k
        assert torch.equal(opt.exp_avg_sqs[k], opt2.exp_avg_sqs[k]), k
        if master:
            assert torch.equal(opt.masters[k], opt2.masters[k]), k


@pytest.mark.parametrize("dtype,master", KINDS[:2], ids=KIND_IDS[:2])
def test_always_adapt_gives_exempt_tensors_their_ratio(dtype, master):
    params, opt, ref = _run(dtype, master, 0.01, 1.0, always_adapt=True)
    lc.assert_state(opt, params, ref)
    lc.assert_norms(opt, ref)
    assert (opt.trust_ratios[[1, 3]] < 0.5).all()


@pytest.mark.parametrize("dtype,master", KINDS[:2], ids=KIND_IDS[:2])
def test_captured_step_follows_ratio_clip_lr_and_count(dtype, master):
    """One eager step, then opt.step() captured once and replayed three
    times, each with new gradients of another scale and a new opt.lr: a
    ratio, clip factor, lr or step number frozen at capture would miss."""
    start, history = lc.make_case(41, "cuda", dtype, steps=4)
    history = [[g * (1.0 + 0.5 * i) for g in gs] for i, gs in enumerate(history)]
    lrs = [1e-3, 2e-3, 5e-4, 1.5e-3]
    params = [p.clone().requires_grad_(True) for p in start]
    for p, g in zip(params, history[0]):
        p.grad = g.clone()
    opt = FusedLAMB(params, lr=lrs[0], weight_decay=0.01, master_weights=master,
                    max_grad_norm=1.0, no_decay=lc.NO_DECAY)
    opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    # capture records, it does not run: state is as after the eager step
    with torch.cuda.graph(graph):
        opt.step()
    for grads, lr in zip(history[1:], lrs[1:]):
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        opt.lr = lr
        graph.replay()
    torch.cuda.synchronize()
    assert opt.step_count == 4
    ref = lc.LambRef64(start, 0.01, 1.0, lc.NO_DECAY)
    for grads, lr in zip(history, lrs):
        ref.step(grads, lr)
    lc.assert_state(opt, params, ref)
    lc.assert_norms(opt, ref)
