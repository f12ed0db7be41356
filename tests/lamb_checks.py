"""The fp64 reference shared by test_lamb_cpu.py and test_lamb_gpu.py, and
the shapes both run it on.

Every fp32 quantity (master or fp32 parameter, m, v) is held to this loop by
kernel_checks.assert_sgd_close, 1e-6*|ref| + 1e-7; the squared norms by the
column-sum bound (all terms positive); the trust ratio by that bound carried
through sqrt(P/U): with e = 1e-5 + 1e-4 on each sum, the quotient lies
within sqrt((1+e)/(1-e)) - 1 of the reference, relatively.
"""

import torch

from . import kernel_checks as kc

BETAS = (0.9, 0.999)
EPS = 1e-6
SLAB = 1024
# scalar tail only, vector body only, both, a slab edge, several slabs, and
# between smaller tensors one with more slabs (71) than a wave has lanes
SIZES = (1, 7, 8, 77, SLAB - 8, SLAB, SLAB + 5, 70 * SLAB + 3, 3 * SLAB + 1)
ZERO_G = 5  # SIZES[5]'s gradient is all zeros
NO_DECAY = [k in (1, 3) for k in range(len(SIZES))]
LR = 1e-3
STEPS = 3


def make_case(seed, device, dtype=torch.float32, steps=STEPS):
    """(params, grads per step): tensor k is 0.02*(k+1)*randn, gradients
    0.1*randn, fresh each step, zero for ZERO_G."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    params = [(0.02 * (k + 1) * torch.randn(n, device=device, generator=gen)).to(dtype)
              for k, n in enumerate(SIZES)]
    grads = []
    for _ in range(steps):
        gs = [(0.1 * torch.randn(n, device=device, generator=gen)).to(dtype) for n in SIZES]
        gs[ZERO_G].zero_()
        grads.append(gs)
    return params, grads


class LambRef64:
    """One LAMB step per call in fp64, the formula of FusedLAMB's docstring.
    psq, usq and ratio keep the last step's per-tensor sums and ratios."""

    def __init__(self, params, wd=0.01, max_norm=None, no_decay=None,
                 always_adapt=False, betas=BETAS, eps=EPS):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        (self.b1, self.b2), self.eps, self.wd, self.max_norm = betas, eps, wd, max_norm
        self.no_decay = no_decay or [False] * len(self.p)
        self.always_adapt = always_adapt
        self.t, self.clip = 0, 1.0

    def step(self, grads, lr, params_read=None):
        """params_read: update from these values (a bf16 run without
        masters continues from its own rounded parameters)."""
        self.t += 1
        gs = [g.detach().double() for g in grads]
        if self.max_norm is not None:
            self.sumsq = torch.stack([(g * g).sum() for g in gs]).sum()
            self.clip = min(1.0, self.max_norm / (self.sumsq.sqrt().item() + 1e-6))
        bc1 = 1.0 - self.b1 ** self.t
        bc2 = 1.0 - self.b2 ** self.t
        self.psq, self.usq, self.ratio = [], [], []
        for k, g in enumerate(gs):
            g = g * self.clip
            p = self.p[k] if params_read is None else params_read[k].detach().double()
            wd = 0.0 if self.no_decay[k] else self.wd
            self.m[k] = self.b1 * self.m[k] + (1.0 - self.b1) * g
            self.v[k] = self.b2 * self.v[k] + (1.0 - self.b2) * g * g
            u = (self.m[k] / bc1) / (self.v[k].sqrt() / bc2 ** 0.5 + self.eps) + wd * p
            psq, usq = (p * p).sum(), (u * u).sum()
            adapts = self.always_adapt or not self.no_decay[k]
            r = (psq / usq).sqrt().item() if adapts and psq > 0 and usq > 0 else 1.0
            self.p[k] = p - lr * r * u
            for kept, x in ((self.psq, psq), (self.usq, usq), (self.ratio, r)):
                kept.append(x)


def assert_state(opt, params, ref, tag=""):
    """m, v, the master or fp32 parameter; a bf16 parameter is its master rounded."""
    for k, n in enumerate(SIZES):
        kc.assert_sgd_close(opt.exp_avgs[k], ref.m[k], f"{tag}m[{n}]")
        kc.assert_sgd_close(opt.exp_avg_sqs[k], ref.v[k], f"{tag}v[{n}]")
        if opt.masters is not None:
            kc.assert_sgd_close(opt.masters[k], ref.p[k], f"{tag}master[{n}]")
            assert torch.equal(params[k].detach(), opt.masters[k].to(params[k].dtype)), n
        elif params[k].dtype == torch.float32:
            kc.assert_sgd_close(params[k].detach(), ref.p[k], f"{tag}param[{n}]")


def assert_norms(opt, ref, tag=""):
    """The last step's ||p||^2, ||u||^2 and trust ratios against the loop's."""
    psq = torch.stack(ref.psq).to(opt.param_norms.device)
    usq = torch.stack(ref.usq).to(psq.device)
    kc.assert_colsum_ref(opt.param_norms ** 2, psq, psq, f"{tag}|p|^2")
    kc.assert_colsum_ref(opt.update_norms ** 2, usq, usq, f"{tag}|u|^2")
    e = kc.COLSUM_REL[torch.float32] + kc.COLSUM_TERMS
    ratio = torch.tensor(ref.ratio, dtype=torch.float64, device=psq.device)
    kc.assert_bounded(opt.trust_ratios, ratio,
                      ratio * (((1 + e) / (1 - e)) ** 0.5 - 1), f"{tag}trust ratio")
