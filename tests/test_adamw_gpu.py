"""FusedAdamW / the multi-tensor AdamW kernels (ops/hip/adamw.hip) against
an fp64 loop, by the rule of tests/adamw_checks.py: every fp32 quantity
(master or fp32 parameter, m, v) within 8x the error of fp32
torch.optim.AdamW(foreach=False) on the same inputs, torch clipping with
clip_grad_norm_ first where the optimizer clips. A bf16 parameter is its
master rounded, or, without a master, within one bf16 rounding of the fp64
update of the parameter the kernel read. The gradient norm is held to the
column-sum bound on the sum of squares.

Slabs are 1024 elements, so the sizes end before, on and past a slab and
take the vector body, the scalar tail and both. Gradients are 0.1 * randn,
fresh every step and copied into the same .grad tensors; one tensor's
gradient is zero throughout.
"""

from __future__ import annotations

import pytest
import torch

from . import adamw_checks as ac
from . import kernel_checks as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import hiplib, multi_tensor
    from skycomputing_amd.optim import FusedAdamW


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


SLAB = 1024
SIZES = (1, 7, 8, 77, SLAB - 8, SLAB, SLAB + 5, 3 * SLAB + 1)
ZERO_G = 5  # SIZES[5]'s gradient is all zeros
BIG = 300 * SLAB + 3  # 301 partials: more than the finish kernel's 256 threads
LR = 1e-3
STEPS = 3

# (dtype, master)
KINDS = [(torch.float32, False), (torch.bfloat16, True), (torch.bfloat16, False)]
KIND_IDS = ["fp32-nomaster", "bf16-master", "bf16-nomaster"]


@pytest.fixture(autouse=True)
def _small_slab(monkeypatch):
    monkeypatch.setattr(multi_tensor, "_SLAB", SLAB)


def _gen(seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return gen


def _make(dtype, gen, sizes=SIZES):
    params = [torch.randn(n, device="cuda", generator=gen).to(dtype).requires_grad_(True)
              for n in sizes]
    for p in params:
        p.grad = torch.zeros_like(p)
    return params


def _fresh_grads(params, gen, zero=None):
    grads = [(0.1 * torch.randn(p.numel(), device="cuda", generator=gen)).to(p.dtype)
             for p in params]
    if zero is not None:
        grads[zero].zero_()
    return grads


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad.copy_(g)  # same .grad tensors: the plan is built once


def _check_final(params, opt, start, history, lrs, wd, max_norm, no_decay=None, tag=""):
    """The rule for m and v, and for the master or fp32 parameter; a bf16
    parameter with a master is the master rounded. Returns the fp64 ref."""
    ref = ac.adamw_ref64(start, history, lrs, wd, max_norm, no_decay)
    eager = ac.torch_adamw32(start, history, lrs, wd, max_norm, no_decay)
    ac.assert_rule(f"{tag}m", opt.exp_avgs, eager[1], ref.m)
    ac.assert_rule(f"{tag}v", opt.exp_avg_sqs, eager[2], ref.v)
    if opt.masters is not None:
        ac.assert_rule(f"{tag}master", opt.masters, eager[0], ref.p)
        for p, m in zip(params, opt.masters):
            if p.dtype == torch.bfloat16:
                assert torch.equal(p.detach(), m.to(torch.bfloat16)), (
                    f"param[{p.numel()}] is not its master rounded to bf16")
    elif params[0].dtype == torch.float32:
        ac.assert_rule(f"{tag}param", [p.detach() for p in params], eager[0], ref.p)
    if max_norm is not None:
        ac.assert_sumsq(opt.grad_norm, ref.sumsq, f"{tag}grad norm^2")
    return ref


@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("dtype,master", KINDS, ids=KIND_IDS)
def test_fused_adamw_matches_fp64_loop(dtype, master, wd, max_norm):
    gen = _gen(17)
    params = _make(dtype, gen)
    start = [p.detach().clone() for p in params]
    opt = FusedAdamW(params, lr=LR, weight_decay=wd, master_weights=master,
                     max_grad_norm=max_norm)
    assert (opt.masters is not None) == master
    stepwise = ac.AdamWRef64(start, wd=wd, max_norm=max_norm)
    history = []
    for _ in range(STEPS):
        grads = _fresh_grads(params, gen, zero=ZERO_G)
        _set_grads(params, grads)
        history.append(grads)
        before = [p.detach().clone() for p in params]
        opt.step()
        if dtype == torch.bfloat16 and not master:
            # no fp32 copy to compare: each step from the parameter the
            # kernel read, to one bf16 rounding
            stepwise.step(grads, LR, params_read=before)
            for k, p in enumerate(params):
                kc.assert_bf16_close(p.detach(), stepwise.p[k], 0.0, f"param[{SIZES[k]}]")
    assert ("adamw", id(opt.params)) in multi_tensor._PLAN_CACHE
    assert opt.step_count == STEPS

    ref = _check_final(params, opt, start, history, LR, wd, max_norm)
    if max_norm is not None:
        assert ref.clip < 0.5  # the clip was active

    # the zero-gradient tensor: moments stay 0, no NaN, decay only
    assert not opt.exp_avgs[ZERO_G].any() and not opt.exp_avg_sqs[ZERO_G].any()
    if master or dtype == torch.float32:
        got = opt.masters[ZERO_G] if master else params[ZERO_G].detach()
        want = start[ZERO_G].double() * (1.0 - LR * wd) ** STEPS
        if wd == 0.0:
            assert torch.equal(got.double(), want)
        else:
            # per step one rounding of the product (2^-24 relative) and the
            # factor 1 - lr*wd itself rounded to fp32 (2^-25, it lies below
            # 1): 3 * 1.5 * 2^-24, rounded up to 5 * 2^-24
            kc.assert_bounded(got, want, 5 * 2.0 ** -24 * want.abs(), "decay-only param")


@pytest.mark.parametrize("dtype,master", KINDS[:2], ids=KIND_IDS[:2])
def test_gradnorm_finish_loops_over_partials(dtype, master):
    """301 slabs in one tensor: the single-block finish kernel adds more
    partials than it has threads. The norm and the clipped update follow."""
    gen = _gen(29)
    sizes = (77, BIG, SLAB + 5)
    params = _make(dtype, gen, sizes)
    start = [p.detach().clone() for p in params]
    opt = FusedAdamW(params, lr=LR, weight_decay=0.01, master_weights=master,
                     max_grad_norm=1.0)
    history = []
    for _ in range(2):
        grads = _fresh_grads(params, gen)
        _set_grads(params, grads)
        history.append(grads)
        opt.step()
    n_desc = multi_tensor._PLAN_CACHE[("adamw", id(opt.params))][2]
    assert n_desc == 1 + 301 + 2
    ref = _check_final(params, opt, start, history, LR, 0.01, 1.0)
    assert ref.clip < 0.05


@pytest.mark.parametrize("dtype,master", KINDS, ids=KIND_IDS)
def test_huge_max_norm_is_bitwise_no_clipping(dtype, master):
    """max_grad_norm=1e30 makes the clip factor exactly 1: the update that
    multiplies it in gives the bits of the run that never computed it."""
    results = []
    for max_norm in (None, 1e30):
        gen = _gen(31)
        params = _make(dtype, gen, SIZES + (BIG,))
        opt = FusedAdamW(params, lr=LR, weight_decay=0.01, master_weights=master,
                         max_grad_norm=max_norm)
        for _ in range(2):
            _set_grads(params, _fresh_grads(params, gen, zero=ZERO_G))
            opt.step()
        results.append((params, opt))
    (p0, o0), (p1, o1) = results
    assert o1._hyper[1].item() == 1.0 and o1.grad_norm.item() > 1.0
    assert o0.grad_norm.item() == 0.0  # never computed
    for k in range(len(p0)):
        assert torch.equal(p0[k].detach(), p1[k].detach()), k
        assert torch.equal(o0.exp_avgs[k], o1.exp_avgs[k]), k
        assert torch.equal(o0.exp_avg_sqs[k], o1.exp_avg_sqs[k]), k
        if master:
            assert torch.equal(o0.masters[k], o1.masters[k]), k


@pytest.mark.parametrize("dtype,master", KINDS[:2], ids=KIND_IDS[:2])
def test_no_decay_flag_travels_per_descriptor(dtype, master):
    """Two equal tensors with equal gradients, the second exempt: it follows
    the wd=0 reference, the first the wd reference. wd is large enough
    (0.1) that the two references are far apart."""
    gen = _gen(37)
    wd = 0.1
    n = 2 * SLAB + 5
    one = torch.randn(n, device="cuda", generator=gen).to(dtype)
    params = [one.clone().requires_grad_(True) for _ in range(2)]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = FusedAdamW(params, lr=LR, weight_decay=wd, master_weights=master,
                     no_decay=[False, True])
    history = []
    for _ in range(STEPS):
        g = _fresh_grads(params[:1], gen)[0]
        _set_grads(params, [g, g])
        history.append([g])
        opt.step()
    got = opt.masters if master else [p.detach() for p in params]
    refs = [ac.adamw_ref64([one], history, LR, w) for w in (wd, 0.0)]
    eagers = [ac.torch_adamw32([one], history, LR, w) for w in (wd, 0.0)]
    for k, ref_wd in enumerate((wd, 0.0)):
        ac.assert_rule(f"wd={ref_wd} p", [got[k]], eagers[k][0], refs[k].p)
    assert not torch.equal(got[0], got[1])
    assert torch.equal(opt.exp_avgs[0], opt.exp_avgs[1])
    # and the rule tells the two apart: the exempt tensor against the
    # decayed reference fails
    with pytest.raises(AssertionError):
        ac.assert_rule("crossed", [got[1]], eagers[0][0], refs[0].p)


@pytest.mark.parametrize("dtype,master", KINDS[:2], ids=KIND_IDS[:2])
def test_captured_step_counts_clips_and_follows_lr(dtype, master):
    """One eager step, then opt.step() captured once and replayed three
    times with new gradients in the static .grad buffers and a new opt.lr
    before each replay. A step number, clip factor or lr frozen at capture
    would miss the four-step fp64 loop with that lr sequence."""
    gen = _gen(41)
    params = _make(dtype, gen)
    start = [p.detach().clone() for p in params]
    lrs = [1e-3, 2e-3, 5e-4, 1.5e-3]
    opt = FusedAdamW(params, lr=lrs[0], weight_decay=0.01, master_weights=master,
                     max_grad_norm=1.0)
    history = [_fresh_grads(params, gen, zero=ZERO_G)]
    _set_grads(params, history[0])
    opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    # capture records, it does not run: state is as after the eager step
    with torch.cuda.graph(graph):
        opt.step()
    for i, lr in enumerate(lrs[1:]):
        # gradient norms differ by step, so a frozen clip factor would show
        grads = [g * (1.0 + i) for g in _fresh_grads(params, gen, zero=ZERO_G)]
        history.append(grads)
        _set_grads(params, grads)
        opt.lr = lr
        graph.replay()
    torch.cuda.synchronize()
    assert opt.step_count == 4
    _check_final(params, opt, start, history, lrs, 0.01, 1.0)


def test_whole_step_executor_with_adamw_follows_lr():
    """GraphedTrainStep captures FusedAdamW.step() where it captures
    FusedSGD's: a 2-layer bf16 stage trains (finite, decreasing loss on a
    repeated batch), the device step count follows the replays, and opt.lr
    reaches the captured step: at lr 0 (and no decay) replays leave every
    master and parameter bit-identical."""
    from skycomputing_amd.builder import build_module_from_cfg
    from skycomputing_amd.models import bert_pipeline_config
    from skycomputing_amd.parallel.graph import GraphedTrainStep

    torch.manual_seed(2)
    cfgs = bert_pipeline_config(
        2, dict(hidden_size=256, num_attention_heads=4, intermediate_size=1024,
                vocab_size=2000, hidden_dropout_prob=0.1,
                attention_probs_dropout_prob=0.1)
    )
    stage = build_module_from_cfg(cfgs, device="cuda:0", dtype=torch.bfloat16,
                                  record_forward_time=False)
    opt = FusedAdamW(stage.parameters(), lr=1e-3, weight_decay=0.0,
                     max_grad_norm=1.0, no_decay="1d")
    assert any(opt.no_decay) and not all(opt.no_decay)
    ids = torch.randint(0, 2000, (8, 32), device="cuda")
    inputs = [ids, torch.zeros_like(ids), torch.ones_like(ids)]
    labels = torch.randint(0, 3, (8,), device="cuda")
    g = GraphedTrainStep(
        stage, opt,
        lambda lg, lb: torch.nn.functional.cross_entropy(lg.float(), lb),
        inputs, labels,
    )
    built = opt.step_count  # the executor's warm-up and plan-building steps
    losses = []
    for _ in range(10):
        g.step(inputs, labels)
        losses.append(g.loss_value())
    print("losses", losses, "grad norm", opt.grad_norm.item())
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0], losses
    assert opt.step_count == built + 10
    assert opt.grad_norm.item() > 0
    assert all(torch.isfinite(m).all() for m in opt.masters)
    opt.lr = 0.0
    frozen = [m.clone() for m in opt.masters]
    params = [p.detach().clone() for p in opt.params]
    for _ in range(2):
        g.step(inputs, labels)
    torch.cuda.synchronize()
    assert opt.step_count == built + 12
    for k in range(len(frozen)):
        assert torch.equal(opt.masters[k], frozen[k]), k
        assert torch.equal(opt.params[k].detach(), params[k]), k


@pytest.mark.parametrize("dtype,master", KINDS[:2], ids=KIND_IDS[:2])
def test_plan_cache_follows_new_parameter_storage(dtype, master):
    """A parameter that gets new storage keeps its .grad tensor. The next
    step must update the new storage and leave the old one alone."""
    gen = _gen(23)
    params = _make(dtype, gen, sizes=(77, SLAB + 5, 8))
    grads = _fresh_grads(params, gen)
    _set_grads(params, grads)
    start = [q.detach().clone() for q in params]
    opt = FusedAdamW(params, lr=LR, master_weights=master, max_grad_norm=1.0)
    opt.step()
    p = params[1]
    grad_before = p.grad
    old = p.data
    p.data = p.data.clone()
    assert p.data.data_ptr() != old.data_ptr() and p.grad is grad_before
    old_copy, new_copy = old.clone(), p.data.clone()
    opt.step()
    assert torch.equal(old, old_copy), "the step wrote the parameter's old storage"
    assert not torch.equal(p.data, new_copy), "the new storage did not get the update"
    # and the update is the right one: two steps of the same gradients from
    # the start (the clone kept the values)
    _check_final(params, opt, start, [grads] * 2, LR, 0.01, 1.0)
