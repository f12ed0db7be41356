"""References, inputs and acceptance rules for softmax cross-entropy
(ops.softmax_cross_entropy, ops/hip/xent.hip), shared by test_xent_cpu.py
and test_xent_gpu.py. tests/kernel_checks.py supplies the bounds.

Everything is plain torch on the device of its inputs.

  xent_ref64       per-row loss, mean and gradient in fp64 from the kernel's
                   own inputs upcast
  torch_xent32     the comparator: torch fp32 cross_entropy on the upcast
                   inputs, reduction="none", and the autograd gradient of
                   its mean over the valid rows
  kernel_loop32    an fp32 loop written as the kernel computes: 256 threads
                   stride over a row in 8-element vectors, each folds its
                   vectors into a running (max, sum) pair, the pairs merge
                   across the wave (xor butterfly) and then across the four
                   waves; with wrong= it computes one of four subtly wrong
                   results, which the rules must reject. (The kernel takes
                   each row's final log and loss in double; the loop stays
                   fp32 throughout, the looser of the two.)

Rules (check_result):
  row losses (fp32, pooled over the case's rows) and fp32 gradients:
      max|err| <= 8 x the comparator's max|err|, both against fp64
  the mean: kernel_checks.assert_colsum_ref with the fp64 mean as the
      reference and as the sum of |terms|
  bf16 gradients: |got - ref64| <= 2^-8 |ref64| + 8 max|comparator - ref64|;
      the floor is the comparator's own fp32 error, because gradients here
      are about 1/(V count) and a constant floor would hide errors of
      that size
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import kernel_checks as kc

IGNORE = -100
THREADS = 256
WAVE = 64
FLT_MAX = torch.finfo(torch.float32).max

WRONG = ("unshifted_lse", "mean_over_all_rows", "no_onehot", "pad_in_softmax")

# (N, V, ld)
CASES = [
    (5, 30522, 30522),   # all four row alignments (bf16), the real width
    (5, 30522, 30528),   # pad columns
    (3, 7, 7),           # narrower than one vector
    (3, 3, 16),          # narrower than one vector, padded
    (4, 8, 8),           # exactly one aligned vector
    (2, 4099, 4099),     # the column loop loops, with a tail
    (9, 2051, 2056),     # the column loop loops, tail and pad
    (300, 37, 37),       # more rows than the finish block has threads
]


def case_id(case):
    return "N{}-V{}-ld{}".format(*case)


def make_case(case, dtype, device="cpu", seed=0):
    """logits [N, ld] = 3*randn in dtype (pad columns too), labels [N].
    Where V > 3, row 0 starts [80, -1e4, 79] with label 0: the cancellation
    the shifted loss exists for. labels[1] = -100 where N > 2; the last
    row's label is V - 1."""
    N, V, ld = case
    gen = torch.Generator().manual_seed(1000 * seed + N + V + ld)
    logits = (3.0 * torch.randn(N, ld, generator=gen)).to(dtype)
    labels = torch.randint(0, V, (N,), generator=gen)
    if V > 3:
        logits[0, :3] = torch.tensor([80.0, -1e4, 79.0]).to(dtype)
        labels[0] = 0
    if N > 2:
        labels[1] = IGNORE
    labels[N - 1] = V - 1
    return logits.to(device), labels.to(device)


def valid_rows(labels, V, ignore_index=IGNORE):
    return (labels >= 0) & (labels < V) & (labels != ignore_index)


def xent_ref64(logits, labels, V, ignore_index=IGNORE):
    """(rowloss [N], mean, grad [N, ld]) in fp64. Ignored rows have loss 0
    and gradient 0, pad columns gradient 0; no valid row gives mean 0."""
    N, ld = logits.shape
    z = logits[:, :V].double()
    valid = valid_rows(labels, V, ignore_index)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    lsm = torch.log_softmax(z, dim=-1)
    rowloss = torch.where(valid, -lsm.gather(1, lab[:, None]).squeeze(1),
                          torch.zeros(N, dtype=torch.float64, device=z.device))
    count = int(valid.sum())
    mean = rowloss.sum() / count if count else rowloss.sum() * 0.0
    g = torch.exp(lsm)
    g.scatter_add_(1, lab[:, None], -torch.ones(N, 1, dtype=torch.float64, device=z.device))
    g = g * (valid[:, None].double() / max(count, 1))
    grad = torch.zeros(N, ld, dtype=torch.float64, device=z.device)
    grad[:, :V] = g
    return rowloss, mean, grad


def torch_xent32(logits, labels, V, ignore_index=IGNORE):
    """The comparator: (rowloss [N], grad [N, ld]) of torch's fp32
    cross_entropy on the upcast inputs. Invalid labels are handed to torch
    as its ignore_index; with no valid row (where torch's mean is NaN) the
    gradient is taken as zero."""
    N, ld = logits.shape
    z = logits[:, :V].float().detach().clone().requires_grad_(True)
    valid = valid_rows(labels, V, ignore_index)
    lab = torch.where(valid, labels, torch.full_like(labels, -100))
    rowloss = F.cross_entropy(z, lab, ignore_index=-100, reduction="none")
    grad = torch.zeros(N, ld, dtype=torch.float32, device=z.device)
    if bool(valid.any()):
        F.cross_entropy(z, lab, ignore_index=-100, reduction="mean").backward()
        grad[:, :V] = z.grad
    return rowloss.detach(), grad


def _merge(m, s, mo, so):
    mn = torch.maximum(m, mo)
    return mn, s * torch.exp(m - mn) + so * torch.exp(mo - mn)


def kernel_loop32(logits, labels, V, ignore_index=IGNORE, wrong=None, gout=1.0):
    """(rowloss [N] fp32, mean fp32 0-dim, grad [N, ld] in the logits'
    dtype) by the kernels' arithmetic in fp32 torch ops. Rows are taken as
    16-byte aligned (no head peel): the grouping of elements into vectors
    moves with the alignment, the arithmetic does not."""
    assert wrong is None or wrong in WRONG, wrong
    N, ld = logits.shape
    dev = logits.device
    W = ld if wrong == "pad_in_softmax" else V
    z = logits[:, :W].float()
    valid = valid_rows(labels, V, ignore_index)
    lab = torch.where(valid, labels, torch.zeros_like(labels))

    # thread t folds vectors t, t + 256, ...; absent elements are -inf
    per_trip = THREADS * 8
    trips = (W + per_trip - 1) // per_trip
    zp = torch.full((N, trips * per_trip), float("-inf"), device=dev)
    zp[:, :W] = z
    zp = zp.view(N, trips, THREADS, 8)
    m = torch.full((N, THREADS), -FLT_MAX, device=dev)
    s = torch.zeros(N, THREADS, device=dev)
    for i in range(trips):
        x = zp[:, i]
        mn = torch.maximum(m, x.max(-1).values)
        e = torch.exp(x - mn[..., None])
        e = ((e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3])) + \
            ((e[..., 4] + e[..., 5]) + (e[..., 6] + e[..., 7]))
        s = s * torch.exp(m - mn) + e
        m = mn
    # the wave's xor butterfly, then wave 0 takes the others in order
    lane = torch.arange(THREADS, device=dev)
    off = WAVE // 2
    while off:
        m, s = _merge(m, s, m[:, lane ^ off], s[:, lane ^ off])
        off //= 2
    rm, rs = m[:, 0], s[:, 0]
    for w in range(1, THREADS // WAVE):
        rm, rs = _merge(rm, rs, m[:, w * WAVE], s[:, w * WAVE])
    lse = torch.log(rs)
    zl = z.gather(1, lab[:, None]).squeeze(1)
    if wrong == "unshifted_lse":
        rowloss = (rm + lse) - zl
    else:
        rowloss = lse - (zl - rm)
    rowloss = torch.where(valid, rowloss, torch.zeros_like(rowloss))

    # the finish block: thread-strided partial sums, then the block sum
    count = N if wrong == "mean_over_all_rows" else int(valid.sum())
    pad = (-N) % THREADS
    part = torch.cat([rowloss, torch.zeros(pad, device=dev)]).view(-1, THREADS).sum(0)
    total = part.view(-1, WAVE).sum(1).sum()
    cnt = torch.tensor(float(count), device=dev)
    zero = torch.zeros((), device=dev)
    mean = total / cnt if count else zero
    inv = 1.0 / cnt if count else zero

    scale = torch.tensor(gout, dtype=torch.float32, device=dev) * inv
    if wrong == "unshifted_lse":
        p = torch.exp(z - (rm + lse)[:, None])
    else:
        p = torch.exp((z - rm[:, None]) - lse[:, None])
    if wrong != "no_onehot":
        p = p.scatter_add(1, lab[:, None], -torch.ones(N, 1, device=dev))
    g = torch.where(valid[:, None], p * scale, torch.zeros_like(p))
    grad = torch.zeros(N, ld, device=dev)
    grad[:, :W] = g
    return rowloss, mean, grad.to(logits.dtype)


def check_rowloss(got_rowloss, logits, labels, V, name, ignore_index=IGNORE):
    ref_rows, _, _ = xent_ref64(logits, labels, V, ignore_index)
    eager_rows, _ = torch_xent32(logits, labels, V, ignore_index)
    assert got_rowloss.dtype == torch.float32, got_rowloss.dtype
    kc.assert_within_eager(got_rowloss, eager_rows, ref_rows, f"{name} row losses")


def check_mean(got_mean, logits, labels, V, name, ignore_index=IGNORE):
    _, ref_mean, _ = xent_ref64(logits, labels, V, ignore_index)
    assert got_mean.dtype == torch.float32 and got_mean.numel() == 1, got_mean
    kc.assert_colsum_ref(got_mean.reshape(1), ref_mean.reshape(1),
                         ref_mean.abs().reshape(1), f"{name} mean loss")


def check_grad(got_grad, logits, labels, V, name, ignore_index=IGNORE, gout=1.0):
    """got_grad is the gradient for an incoming gradient gout of the mean."""
    _, _, ref_grad = xent_ref64(logits, labels, V, ignore_index)
    _, eager_grad = torch_xent32(logits, labels, V, ignore_index)
    ref_grad = ref_grad * gout
    eager_grad = eager_grad * gout
    assert got_grad.dtype == logits.dtype, (got_grad.dtype, logits.dtype)
    if got_grad.dtype == torch.bfloat16:
        floor = kc.EAGER_FACTOR * (eager_grad.double() - ref_grad).abs().max().item()
        print(f"{name} gradient: bf16 floor 8 x comparator error = {floor:.3e}")
        kc.assert_bounded(got_grad, ref_grad, kc.BF16_REL * ref_grad.abs() + floor,
                          f"{name} gradient")
    else:
        kc.assert_within_eager(got_grad, eager_grad, ref_grad, f"{name} gradient")


def check_result(got_rowloss, got_mean, got_grad, logits, labels, V, name,
                 ignore_index=IGNORE):
    """All three rules; got_rowloss may be None (a caller that only sees
    the mean)."""
    if got_rowloss is not None:
        check_rowloss(got_rowloss, logits, labels, V, name, ignore_index)
    check_mean(got_mean, logits, labels, V, name, ignore_index)
    check_grad(got_grad, logits, labels, V, name, ignore_index)
