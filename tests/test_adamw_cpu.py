"""FusedAdamW without a GPU: the acceptance rule of tests/adamw_checks.py
rejects four subtly wrong AdamW variants, the eager step passes it,
build_optimizer, sync_masters, the state_dict round trip, and an AdamW run
through the launch CLI.

Inputs: parameters randn, gradients 0.1 * randn and fresh every step, except
one tensor whose gradients are 1e-4 * randn (where sqrt(v) is small enough
for the place of eps to matter) and one whose gradients are all zero.
"""

from __future__ import annotations

import os
import re
import subprocess
import sys

import pytest
import torch

from skycomputing_amd import FusedAdamW, FusedSGD, build_optimizer
from skycomputing_amd.ops import adamw_step

from . import adamw_checks as ac
from .test_launch_e2e import REPO, TINY_CONFIG

SIZES = (1, 7, 8, 77, 1016, 1024, 1029, 3073)
TINY_G, ZERO_G = 3, 5  # indices into SIZES
LR = 1e-3
STEPS = 3


def _case(seed, dtype=torch.float32, steps=STEPS):
    g = torch.Generator()
    g.manual_seed(seed)
    params = [torch.randn(n, generator=g).to(dtype) for n in SIZES]
    grads = []
    for _ in range(steps):
        gs = [(0.1 * torch.randn(n, generator=g)) for n in SIZES]
        gs[TINY_G] = gs[TINY_G] * 1e-3
        gs[ZERO_G] = torch.zeros_like(gs[ZERO_G])
        grads.append([x.to(dtype) for x in gs])
    return params, grads


@pytest.mark.parametrize("steps", [3, 10])
def test_rule_accepts_faithful_and_rejects_wrong_variants(steps):
    params, grads = _case(1, steps=steps)
    wd, max_norm = 0.01, 1.0
    ref = ac.adamw_ref64(params, grads, LR, wd, max_norm)
    eager = ac.torch_adamw32(params, grads, LR, wd, max_norm)
    assert ref.clip < 0.5  # the clip is active
    ac.assert_rule_pmv(*ac.adamw_fp32_loop(params, grads, LR, wd, max_norm), eager, ref,
                       "faithful ")
    for wrong in ac.WRONG:
        with pytest.raises(AssertionError):
            ac.assert_rule_pmv(
                *ac.adamw_fp32_loop(params, grads, LR, wd, max_norm, wrong=wrong),
                eager, ref, f"{wrong} ")


def test_sumsq_bound_rejects_a_left_out_slab():
    g = torch.Generator()
    g.manual_seed(2)
    grad = 0.1 * torch.randn(3073, generator=g)
    ref = (grad.double() ** 2).sum()
    ac.assert_sumsq(grad.square().sum().sqrt(), ref)
    with pytest.raises(AssertionError):
        ac.assert_sumsq(grad[:3072].square().sum().sqrt() * 0.99, ref)
    with pytest.raises(AssertionError):
        ac.assert_sumsq(torch.tensor(float("nan")), ref)


def _run_opt(params, grads, **kw):
    ps = [p.clone().requires_grad_(True) for p in params]
    opt = FusedAdamW(ps, lr=LR, **kw)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
    return ps, opt


@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("dtype,master", [(torch.float32, False), (torch.bfloat16, True)],
                         ids=["fp32", "bf16-master"])
def test_eager_adamw_passes_the_rule(dtype, master, wd, max_norm):
    params, grads = _case(3, dtype)
    no_decay = [n in (7, 1029) for n in SIZES]
    ps, opt = _run_opt(params, grads, weight_decay=wd, max_grad_norm=max_norm,
                       master_weights=master, no_decay=no_decay)
    assert (opt.masters is not None) == master
    ref = ac.adamw_ref64(params, grads, LR, wd, max_norm, no_decay)
    eager = ac.torch_adamw32(params, grads, LR, wd, max_norm, no_decay)
    got_p = opt.masters if master else [p.detach() for p in ps]
    ac.assert_rule_pmv(got_p, opt.exp_avgs, opt.exp_avg_sqs, eager, ref)
    if master:
        for p, m in zip(ps, opt.masters):
            assert torch.equal(p.detach(), m.to(torch.bfloat16))
    assert opt.step_count == STEPS
    if max_norm is not None:
        ac.assert_sumsq(opt.grad_norm, ref.sumsq)
    # the zero-gradient tensor: no moments, no NaN, decay only
    assert not opt.exp_avgs[ZERO_G].any() and not opt.exp_avg_sqs[ZERO_G].any()
    want = params[ZERO_G].double() * (1.0 - LR * wd) ** STEPS
    assert torch.allclose(got_p[ZERO_G].double(), want, rtol=1e-6, atol=0)
    # no_decay was honoured: the same run with decay everywhere differs
    # exactly on the flagged tensors when wd is on
    if wd:
        _, opt2 = _run_opt(params, grads, weight_decay=wd, max_grad_norm=max_norm,
                           master_weights=master)
        got2 = opt2.masters if master else opt2.params
        for k, nd in enumerate(no_decay):
            assert torch.equal(got_p[k], got2[k].detach()) == (not nd), SIZES[k]


def test_eager_adamw_step_skips_missing_grads():
    params, grads = _case(4)
    ps = [p.clone() for p in params]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    gs = list(grads[0])
    gs[1] = None
    norm, clip = adamw_step(ps, gs, ms, vs, 1, LR, max_grad_norm=1.0)
    assert torch.equal(ps[1], params[1]) and not ms[1].any()
    assert not torch.equal(ps[2], params[2])
    want = sum((g.double() ** 2).sum() for g in gs if g is not None)
    ac.assert_sumsq(norm, want)
    assert 0 < clip.item() < 1


def test_no_decay_forms():
    ps = [torch.zeros(4, 4, requires_grad=True), torch.zeros(4, requires_grad=True),
          torch.zeros(3, requires_grad=False), torch.zeros((), requires_grad=True)]
    assert FusedAdamW(ps).no_decay == [False, False, False]
    assert FusedAdamW(ps, no_decay="1d").no_decay == [False, True, True]
    assert FusedAdamW(ps, no_decay=lambda p: p.ndim == 2).no_decay == [True, False, False]
    assert FusedAdamW(ps, no_decay=[True, False, True, False]).no_decay == [True, False, False]
    with pytest.raises(ValueError):
        FusedAdamW(ps, no_decay=[True])


def test_descriptor_rows_sgd_unchanged_and_adamw_layout(monkeypatch):
    """The shared slab splitter: SGD rows stay {p, g, master, momentum, n,
    0}; AdamW rows are {p, g, master, m, v, n, flags}; the plan signature
    covers m and v; a misaligned tensor is refused."""
    from skycomputing_amd.ops import multi_tensor as mt

    monkeypatch.setattr(mt, "_SLAB", 1024)
    ps = [torch.zeros(1029, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.bfloat16)]
    gs = [torch.zeros_like(p) for p in ps]
    ma, m, v = ([torch.zeros(p.shape) for p in ps] for _ in range(3))
    a = lambda t: t.data_ptr()

    desc, n = mt._build_plan(ps, gs, ma, m)
    assert n == 3 and desc.dtype == torch.int64
    assert desc.tolist() == [
        [a(ps[0]), a(gs[0]), a(ma[0]), a(m[0]), 1024, 0],
        [a(ps[0]) + 2048, a(gs[0]) + 2048, a(ma[0]) + 4096, a(m[0]) + 4096, 5, 0],
        [a(ps[1]), a(gs[1]), a(ma[1]), a(m[1]), 8, 0],
    ]
    desc, n = mt._build_plan(ps, gs, None, None)
    assert desc.tolist()[1] == [a(ps[0]) + 2048, a(gs[0]) + 2048, 0, 0, 5, 0]

    desc, n, partials = mt._build_adamw_plan(ps, gs, ma, m, v, [False, True])
    assert partials.shape == (3,) and partials.dtype == torch.float32
    assert desc.tolist() == [
        [a(ps[0]), a(gs[0]), a(ma[0]), a(m[0]), a(v[0]), 1024, 0],
        [a(ps[0]) + 2048, a(gs[0]) + 2048, a(ma[0]) + 4096, a(m[0]) + 4096,
         a(v[0]) + 4096, 5, 0],
        [a(ps[1]), a(gs[1]), a(ma[1]), a(m[1]), a(v[1]), 8, 1],
    ]
    sig = mt._plan_signature(ps, gs, ma, m, v)
    v2 = [v[0], torch.zeros(8)]
    assert mt._plan_signature(ps, gs, ma, m, v2) != sig
    assert mt._plan_signature(ps, gs, ma, v2, v) != sig

    off = torch.zeros(12)[1:9]  # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 != 0
    with pytest.raises(AssertionError, match="16-byte"):
        mt._build_adamw_plan(ps, gs, ma, m, [v[0], off], [False, False])


def test_build_optimizer():
    ps = [torch.zeros(3, requires_grad=True)]
    sgd = build_optimizer({}, ps)
    assert type(sgd) is FusedSGD
    assert (sgd.lr, sgd.momentum, sgd.weight_decay) == (1e-3, 0.0, 0.0)
    sgd = build_optimizer(dict(lr=0.01, momentum=0.9, weight_decay=0.1), ps)
    assert type(sgd) is FusedSGD
    assert (sgd.lr, sgd.momentum, sgd.weight_decay) == (0.01, 0.9, 0.1)
    assert type(build_optimizer(dict(type="SGD", lr=0.5), ps)) is FusedSGD
    cfg = dict(type="AdamW", lr=2e-5, max_grad_norm=1.0, no_decay="1d")
    adam = build_optimizer(cfg, ps)
    assert type(adam) is FusedAdamW
    assert (adam.lr, adam.max_grad_norm, adam.no_decay) == (2e-5, 1.0, [True])
    assert cfg["type"] == "AdamW"  # the caller's dict is left alone
    with pytest.raises(ValueError, match="AdamW.*SGD"):
        build_optimizer(dict(type="Adagrad"), ps)


def test_lr_is_a_property_backed_by_the_hyper_block():
    p = torch.ones(5, requires_grad=True)
    opt = FusedAdamW([p], lr=1e-3)
    assert opt.lr == 1e-3 and opt._hyper[0].item() == pytest.approx(1e-3, rel=1e-6)
    opt.lr = 5e-4
    assert opt.lr == 5e-4 and opt._hyper[0].item() == pytest.approx(5e-4, rel=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sync_masters_restarts_the_optimizer(dtype):
    params, grads = _case(5, dtype)
    ps, opt = _run_opt(params, grads[:2], max_grad_norm=1.0)
    assert opt.step_count == 2 and opt.exp_avgs[0].any()
    # out-of-band restore of other weights
    restored, _ = _case(6, dtype)
    for p, r in zip(ps, restored):
        p.data.copy_(r)
    opt.sync_masters()
    assert opt.step_count == 0
    assert not any(b.any() for b in opt.exp_avgs + opt.exp_avg_sqs)
    for p, g in zip(ps, grads[2]):
        p.grad = g.clone()
    opt.step()
    fresh_ps, fresh = _run_opt(restored, grads[2:3], max_grad_norm=1.0)
    for k in range(len(ps)):
        assert torch.equal(ps[k].detach(), fresh_ps[k].detach()), SIZES[k]
        assert torch.equal(opt.exp_avgs[k], fresh.exp_avgs[k])
        assert torch.equal(opt.exp_avg_sqs[k], fresh.exp_avg_sqs[k])
        if opt.masters is not None:
            assert torch.equal(opt.masters[k], fresh.masters[k])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_state_dict_round_trip(dtype):
    params, grads = _case(7, dtype)
    no_decay = [n == 77 for n in SIZES]
    ps, opt = _run_opt(params, grads[:2], max_grad_norm=1.0, no_decay=no_decay,
                       betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05)
    sd = opt.state_dict()
    assert sd["step"] == 2
    ps2 = [p.detach().clone().requires_grad_(True) for p in ps]
    opt2 = FusedAdamW(ps2, lr=0.5)  # every hyper-parameter comes from sd
    opt2.load_state_dict(sd)
    assert (opt2.lr, opt2.betas, opt2.eps, opt2.weight_decay, opt2.max_grad_norm,
            opt2.no_decay, opt2.step_count) == (LR, (0.8, 0.99), 1e-6, 0.05, 1.0, no_decay, 2)
    for o, q in ((opt, ps), (opt2, ps2)):
        for p, g in zip(q, grads[2]):
            p.grad = g.clone()
        o.step()
    assert opt.step_count == opt2.step_count == 3
    for k in range(len(ps)):
        assert torch.equal(ps[k].detach(), ps2[k].detach()), SIZES[k]
        assert torch.equal(opt.exp_avgs[k], opt2.exp_avgs[k])
        assert torch.equal(opt.exp_avg_sqs[k], opt2.exp_avg_sqs[k])
        if opt.masters is not None:
            assert torch.equal(opt.masters[k], opt2.masters[k])


def test_launch_cli_adamw(tmp_path):
    """The driver with optimizer=dict(type="AdamW", ...): two ranks, clip in
    the optimizer, biases and LayerNorm parameters exempt from decay."""
    text = TINY_CONFIG.format(logdir=str(tmp_path / "logs"))
    old = "optimizer=dict(lr=0.01),"
    assert old in text
    text = text.replace(
        old, 'optimizer=dict(type="AdamW", lr=1e-3, max_grad_norm=1.0, no_decay="1d"),')
    cfg = tmp_path / "cfg.py"
    cfg.write_text(text)
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    r = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run", "--standalone",
            "--local-addr", "127.0.0.1", "--nproc-per-node", "2",
            os.path.join(REPO, "experiment", "launch.py"),
            "-c", str(cfg),
        ],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=400,
    )
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    logs = [(tmp_path / "logs" / f"rank{k}.log").read_text() for k in (0, 1)]
    assert all("done: 3 iterations" in log for log in logs)
    losses = re.findall(r"last loss ([^\s]+)", "\n".join(logs))
    finite = [float(x) for x in losses if x != "None"]
    assert finite and all(x == x and abs(x) != float("inf") for x in finite), losses
