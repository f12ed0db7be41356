"""FusedSGD / the multi-tensor SGD kernel against an fp64 loop: weight decay,
momentum on and off, masters with and without momentum, tensor sizes that
end before, on and past a descriptor slab, the non-temporal and unrolled
variants, what fp32 master weights are for, and the launch-plan cache when a
parameter gets new storage.

Gradients are 0.1 * randn and change every step, parameters are randn. The
1e-6 relative + 1e-7 absolute bound then holds for a correct kernel: three
roundings of a parameter cost 3 * 2^-24 = 1.8e-7 relative, and a momentum
buffer that cancels to near zero carries 2^-24 * (|0.9 buf| + |g|) <= 2e-8.
"""

from __future__ import annotations

import pytest
import torch

from . import kernel_checks as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd.ops import hiplib, multi_tensor
    from skycomputing_amd.optim import FusedSGD


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


SLAB = 1024
SIZES = (1, 7, 8, 77, SLAB - 8, SLAB, SLAB + 5, 3 * SLAB + 1)
LR = 0.1
STEPS = 3

# (dtype, master, momentum, wd)
COMBOS = (
    [(torch.float32, False, m, wd) for m in (0.0, 0.9) for wd in (0.0, 0.01)]
    + [(torch.bfloat16, True, m, wd) for m in (0.0, 0.9) for wd in (0.0, 0.01)]
    + [(torch.bfloat16, False, 0.9, 0.0)]
)
COMBO_IDS = [f"{'bf16' if d == torch.bfloat16 else 'fp32'}-"
             f"{'master' if ma else 'nomaster'}-m{m}-wd{wd}" for d, ma, m, wd in COMBOS]

# kernel variants: (SKY_SGD_NONT, SKY_SGD_UNROLL)
VARIANTS = [(None, None), ("0", "2"), ("0", "4"), ("0", "8")]


@pytest.fixture(autouse=True)
def _small_slab(monkeypatch):
    monkeypatch.setattr(multi_tensor, "_SLAB", SLAB)
    monkeypatch.delenv("SKY_SGD_NONT", raising=False)
    monkeypatch.delenv("SKY_SGD_UNROLL", raising=False)


def _make(dtype, gen, sizes=SIZES):
    params = [torch.randn(n, device="cuda", generator=gen).to(dtype).requires_grad_(True)
              for n in sizes]
    for p in params:
        p.grad = torch.zeros_like(p)
    return params


@pytest.mark.parametrize("nont,unroll", VARIANTS, ids=["plain", "nt-u2", "nt-u4", "nt-u8"])
@pytest.mark.parametrize("dtype,master,momentum,wd", COMBOS, ids=COMBO_IDS)
def test_fused_sgd_matches_fp64_loop(dtype, master, momentum, wd, nont, unroll, monkeypatch):
    if nont is not None:
        monkeypatch.setenv("SKY_SGD_NONT", nont)
        monkeypatch.setenv("SKY_SGD_UNROLL", unroll)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    params = _make(dtype, gen)
    start = [p.detach().clone() for p in params]
    opt = FusedSGD(params, lr=LR, momentum=momentum, weight_decay=wd,
                   master_weights=master)
    assert (opt.masters is not None) == master
    assert (opt.momentum_bufs is not None) == (momentum != 0.0)
    history = []
    for _ in range(STEPS):
        grads = [(0.1 * torch.randn(p.numel(), device="cuda", generator=gen)).to(dtype)
                 for p in params]
        for p, g in zip(params, grads):
            p.grad.copy_(g)  # same .grad tensors: the plan is built once
        history.append(grads)
        before = [p.detach().clone() for p in params]
        opt.step()
        if dtype == torch.bfloat16 and not master:
            # no fp32 copy to compare: each step from the parameter the
            # kernel read, to one bf16 rounding
            _, bufs = kc.sgd_ref64(start, history, LR, momentum, wd)
            for k, p in enumerate(params):
                ref = before[k].double() - torch.tensor(LR, dtype=torch.float32).double() * bufs[k]
                kc.assert_bf16_close(p.detach(), ref, 0.0, f"param[{SIZES[k]}]")
    assert len(multi_tensor._PLAN_CACHE) >= 1

    ref_p, ref_buf = kc.sgd_ref64(start, history, LR, momentum, wd)
    for k, p in enumerate(params):
        n = SIZES[k]
        if momentum != 0.0:
            kc.assert_sgd_close(opt.momentum_bufs[k], ref_buf[k], f"momentum[{n}]")
        if master:
            kc.assert_sgd_close(opt.masters[k], ref_p[k], f"master[{n}]")
            assert torch.equal(p.detach(), opt.masters[k].to(torch.bfloat16)), (
                f"param[{n}] is not its master rounded to bf16")
        elif dtype == torch.float32:
            kc.assert_sgd_close(p.detach(), ref_p[k], f"param[{n}]")


def test_master_weights_keep_small_updates():
    """p = 1.0 in bf16, lr * g = 1e-4, 50 steps: half a bf16 ulp below 1.0
    is 2^-9 = 2e-3, so without a master every step rounds back to 1.0; the
    fp32 master reaches 0.995 and the parameter follows it to 0.9961."""
    n = SLAB + 5
    steps, lr, g = 50, 0.1, 1e-3

    def run(master):
        p = torch.ones(n, dtype=torch.bfloat16, device="cuda", requires_grad=True)
        p.grad = torch.full_like(p, g)
        opt = FusedSGD([p], lr=lr, master_weights=master)
        for _ in range(steps):
            opt.step()
        return p.detach(), opt

    start = [torch.ones(n, dtype=torch.bfloat16, device="cuda")]
    grads = [[torch.full((n,), g, dtype=torch.bfloat16, device="cuda")]] * steps
    (ref,), _ = kc.sgd_ref64(start, grads, lr, 0.0, 0.0)
    p, opt = run(True)
    kc.assert_sgd_close(opt.masters[0], ref, "master")
    want = torch.tensor(0.9961, dtype=torch.bfloat16, device="cuda")  # 255/256
    assert want.item() == 0.99609375
    assert torch.equal(p, want.expand(n)), p[:4]
    assert torch.equal(p, ref.to(torch.bfloat16))
    p, _ = run(False)
    assert torch.equal(p, torch.ones_like(p)), "bf16-only run was expected to stall"


@pytest.mark.parametrize("dtype,master,momentum", [
    (torch.float32, False, 0.0), (torch.bfloat16, True, 0.9)], ids=["fp32", "bf16-master-mom"])
def test_plan_cache_follows_new_parameter_storage(dtype, master, momentum):
    """A parameter that gets new storage keeps its .grad tensor. The next
    step must update the new storage and leave the old one alone."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    params = _make(dtype, gen, sizes=(77, SLAB + 5, 8))
    for p in params:
        p.grad.copy_((0.1 * torch.randn(p.numel(), device="cuda", generator=gen)).to(dtype))
    start = [q.detach().clone() for q in params]
    opt = FusedSGD(params, lr=LR, momentum=momentum, master_weights=master)
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
    ref_p, _ = kc.sgd_ref64(start, [[q.grad for q in params]] * 2, LR, momentum, 0.0)
    for k, q in enumerate(params):
        if master:
            kc.assert_sgd_close(opt.masters[k], ref_p[k], f"master[{k}]")
            assert torch.equal(q.data, opt.masters[k].to(torch.bfloat16))
        else:
            kc.assert_sgd_close(q.data, ref_p[k], f"param[{k}]")
