"""FusedLAMB without a GPU: build_optimizer knows "LAMB", the eager step
(ops.lamb_step) follows the fp64 loop of tests/lamb_checks.py under the
bound the kernels are held to, and state_dict round-trips."""

import pytest
import torch

from skycomputing_amd import FusedLAMB, build_optimizer

from . import lamb_checks as lc


def _run(params, grads, **kw):
    ps = [p.clone().requires_grad_(True) for p in params]
    opt = build_optimizer(dict(type="LAMB", lr=lc.LR, **kw), ps)
    assert type(opt) is FusedLAMB
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
    return ps, opt


@pytest.mark.parametrize("always_adapt", [False, True], ids=["exempt", "always-adapt"])
@pytest.mark.parametrize("max_norm", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("dtype,master", [(torch.float32, False), (torch.bfloat16, True)],
                         ids=["fp32", "bf16-master"])
def test_eager_lamb_follows_fp64_loop(dtype, master, wd, max_norm, always_adapt):
    params, grads = lc.make_case(3, "cpu", dtype)
    ps, opt = _run(params, grads, weight_decay=wd, max_grad_norm=max_norm,
                   master_weights=master, no_decay=lc.NO_DECAY, always_adapt=always_adapt)
    assert (opt.eps, opt.betas, opt.step_count) == (lc.EPS, lc.BETAS, lc.STEPS)
    ref = lc.LambRef64(params, wd, max_norm, lc.NO_DECAY, always_adapt)
    for gs in grads:
        ref.step(gs, lc.LR)
    lc.assert_state(opt, ps, ref)
    lc.assert_norms(opt, ref)
    exempt = opt.trust_ratios[[1, 3]]
    assert (exempt != 1.0).all() if always_adapt else (exempt == 1.0).all()


def test_state_dict_round_trip_continues_bit_identically():
    params, grads = lc.make_case(7, "cpu")
    ps, opt = _run(params, grads[:2], max_grad_norm=1.0, no_decay=lc.NO_DECAY,
                   always_adapt=True, betas=(0.8, 0.99), eps=1e-5, weight_decay=0.05)
    sd = opt.state_dict()
    ps2 = [p.detach().clone().requires_grad_(True) for p in ps]
    opt2 = FusedLAMB(ps2, lr=0.5)  # every hyper-parameter comes from sd
    opt2.load_state_dict(sd)
    assert (opt2.lr, opt2.betas, opt2.eps, opt2.weight_decay, opt2.no_decay,
            opt2.always_adapt, opt2.step_count) == (
                lc.LR, (0.8, 0.99), 1e-5, 0.05, lc.NO_DECAY, True, 2)
    for o, q in ((opt, ps), (opt2, ps2)):
        for p, g in zip(q, grads[2]):
            p.grad = g.clone()
        o.step()
    assert torch.equal(opt.trust_ratios, opt2.trust_ratios)
    for k in range(len(ps)):
        assert torch.equal(ps[k].detach(), ps2[k].detach()), lc.SIZES[k]
        assert torch.equal(opt.exp_avgs[k], opt2.exp_avgs[k])
        assert torch.equal(opt.exp_avg_sqs[k], opt2.exp_avg_sqs[k])
