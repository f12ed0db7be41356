"""References and the acceptance rule shared by test_adamw_cpu.py and
test_adamw_gpu.py.

Three implementations of the same step, on whatever device the inputs live
on:
  AdamWRef64        the fp64 loop, the clip factor computed in fp64 too, with
                    the hyper-parameters as the Python doubles the user wrote
  torch_adamw32     fp32 torch.optim.AdamW(foreach=False), with
                    torch.nn.utils.clip_grad_norm_ before each step when
                    clipping: the comparator
  adamw_fp32_loop   a plain fp32 loop that can be told to get one thing
                    subtly wrong (the rule has to reject those)

The rule for every fp32 quantity (master or fp32 parameter, m, v), in
assert_rule: max|got - ref64| <= 8 x max|torch32 - ref64|
(kernel_checks.assert_within_eager). The maxima are taken over all tensors
of a case together. A maximum over a handful of elements is luck (one
element's rounding error lies anywhere in [0, ulp/2]), and a fault that
touches only one tensor, a tail or a slab edge shows as an error of the
size of an update or of a moment, hundreds of times the comparator's
rounding error, so pooling hides none.
"""

from __future__ import annotations

import torch

from . import kernel_checks as kc

BETAS = (0.9, 0.999)
EPS = 1e-8


def _per_step(lrs, steps):
    return [lrs] * steps if isinstance(lrs, float) else list(lrs)


class AdamWRef64:
    """torch.optim.AdamW's step in fp64, one call per step.

    p *= 1 - lr*wd; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
    p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps), g first multiplied
    by min(1, max_norm / (||g|| + 1e-6)) over all tensors when max_norm is
    set. sumsq and clip keep the last step's sum of squares and factor."""

    def __init__(self, params, betas=BETAS, eps=EPS, wd=0.01, max_norm=None,
                 no_decay=None):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.b1, self.b2 = betas
        self.eps, self.wd, self.max_norm = eps, wd, max_norm
        self.no_decay = no_decay or [False] * len(self.p)
        self.t = 0
        self.sumsq = None
        self.clip = 1.0

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
        for k, g in enumerate(gs):
            g = g * self.clip
            p = self.p[k] if params_read is None else params_read[k].detach().double()
            wd = 0.0 if self.no_decay[k] else self.wd
            self.m[k] = self.b1 * self.m[k] + (1.0 - self.b1) * g
            self.v[k] = self.b2 * self.v[k] + (1.0 - self.b2) * g * g
            denom = self.v[k].sqrt() / bc2 ** 0.5 + self.eps
            self.p[k] = p * (1.0 - lr * wd) - (lr / bc1) * self.m[k] / denom


def adamw_ref64(params, grads_per_step, lrs, wd, max_norm=None, no_decay=None,
                betas=BETAS, eps=EPS):
    ref = AdamWRef64(params, betas, eps, wd, max_norm, no_decay)
    for grads, lr in zip(grads_per_step, _per_step(lrs, len(grads_per_step))):
        ref.step(grads, lr)
    return ref


def torch_adamw32(params, grads_per_step, lrs, wd, max_norm=None, no_decay=None,
                  betas=BETAS, eps=EPS):
    """The comparator: fp32 copies of the parameters and gradients through
    torch.optim.AdamW(foreach=False). Returns (params, exp_avgs, exp_avg_sqs)."""
    ps = [torch.nn.Parameter(p.detach().float().clone()) for p in params]
    no_decay = no_decay or [False] * len(ps)
    groups = [
        dict(params=[p for p, nd in zip(ps, no_decay) if not nd], weight_decay=wd),
        dict(params=[p for p, nd in zip(ps, no_decay) if nd], weight_decay=0.0),
    ]
    opt = torch.optim.AdamW([g for g in groups if g["params"]], lr=1e-3,
                            betas=betas, eps=eps, foreach=False)
    for grads, lr in zip(grads_per_step, _per_step(lrs, len(grads_per_step))):
        for p, g in zip(ps, grads):
            p.grad = g.detach().float().clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        for group in opt.param_groups:
            group["lr"] = lr
        opt.step()
    return ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps],
            [opt.state[p]["exp_avg_sq"] for p in ps])


WRONG = ("no_bias_correction", "l2_decay", "eps_inside_sqrt", "unclipped")


def adamw_fp32_loop(params, grads_per_step, lrs, wd, max_norm=None, wrong=None,
                    betas=BETAS, eps=EPS):
    """AdamW in plain fp32 arithmetic, written the way a kernel would (the
    moments as multiply-adds, the sum of squares in chunks). wrong=None is
    faithful; each name in WRONG changes one thing. Returns (p, m, v)."""
    assert wrong is None or wrong in WRONG, wrong
    b1, b2 = betas
    ps = [p.detach().float().clone() for p in params]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    for t, (grads, lr) in enumerate(
            zip(grads_per_step, _per_step(lrs, len(grads_per_step))), start=1):
        gs = [g.detach().float() for g in grads]
        clip = 1.0
        if max_norm is not None and wrong != "unclipped":
            chunks = [c.square().sum() for g in gs for c in g.split(256)]
            clip = (max_norm / (torch.stack(chunks).sum().sqrt() + 1e-6)).clamp(max=1.0)
        bc1 = 1.0 if wrong == "no_bias_correction" else 1.0 - b1 ** t
        bc2 = 1.0 if wrong == "no_bias_correction" else 1.0 - b2 ** t
        for k, g in enumerate(gs):
            g = g * clip
            if wrong == "l2_decay":
                g = g + wd * ps[k]
            else:
                ps[k] = ps[k] * (1.0 - lr * wd)
            ms[k] = torch.addcmul(g * (1.0 - b1), ms[k], torch.tensor(b1, device=g.device))
            vs[k] = torch.addcmul(g * g * (1.0 - b2), vs[k], torch.tensor(b2, device=g.device))
            if wrong == "eps_inside_sqrt":
                denom = (vs[k] / bc2 + eps).sqrt()
            else:
                denom = vs[k].sqrt() * (1.0 / bc2 ** 0.5) + eps
            ps[k] = ps[k] - (lr / bc1) * ms[k] / denom
    return ps, ms, vs


def _cat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


def assert_rule(name, got, eager32, ref64):
    """The rule for one fp32 quantity: lists of tensors, pooled."""
    for t in got:
        assert t.dtype == torch.float32, (name, t.dtype)
    kc.assert_within_eager(_cat(got), _cat(eager32), _cat(ref64), name)


def assert_rule_pmv(got_p, got_m, got_v, eager, ref, tag=""):
    """assert_rule for parameters (or masters), m and v: eager is
    torch_adamw32's result, ref an AdamWRef64."""
    assert_rule(f"{tag}p", got_p, eager[0], ref.p)
    assert_rule(f"{tag}m", got_m, eager[1], ref.m)
    assert_rule(f"{tag}v", got_v, eager[2], ref.v)


def assert_sumsq(gnorm, ref_sumsq, name="grad norm^2"):
    """A computed gradient norm against the fp64 sum of squares, by the
    column-sum bound (every term is positive: sum|terms| == ref)."""
    got = gnorm.detach().float().reshape(()) ** 2
    kc.assert_colsum_ref(got, ref_sumsq.reshape(()), ref_sumsq.reshape(()), name)
