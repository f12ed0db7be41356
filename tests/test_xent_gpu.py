"""ops.softmax_cross_entropy on the GPU (ops/hip/xent.hip) against the fp64
reference by the rules of tests/xent_checks.py: per-row fp32 losses and
fp32 gradients within 8x the error of torch's fp32 cross_entropy on the
same inputs, the mean by the column-sum bound, bf16 gradients within one
bf16 rounding plus 8x the comparator's error.

The cases (xent_checks.CASES) take every path of the row loop: rows at all
four 16-byte alignments (ld = 30522 in bf16), pad columns, rows narrower
than one vector, exactly one vector, a looping body with a tail, and more
rows than the finish block has threads. Row 0 of every case with V > 3 is
the spike row [80, -1e4, 79, ...] that an unshifted log-sum-exp fails.
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from . import kernel_checks as kc
from . import xent_checks as xc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from skycomputing_amd import ops
    from skycomputing_amd.ops import functions as fn
    from skycomputing_amd.ops import hiplib


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert hiplib.available(), "libskyhip.so must be built (fail loudly, no eager fallback)"


DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["fp32", "bf16"]
PADDED = (5, 30522, 30528)


def _inv32(n):
    return (torch.tensor(1.0) / n).item()


def _run(logits, labels, V, **kw):
    """(loss, gradient) of the op on a fresh leaf copy of logits."""
    lg = logits.detach().clone().requires_grad_(True)
    loss = ops.softmax_cross_entropy(lg, labels, num_classes=V, **kw)
    assert isinstance(loss.grad_fn, fn.SoftmaxCrossEntropyFn._backward_cls)
    loss.backward()
    return loss.detach(), lg.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", xc.CASES, ids=xc.case_id)
def test_kernels_match_fp64(case, dtype):
    N, V, ld = case
    logits, labels = xc.make_case(case, dtype, "cuda")
    rowmax, logsum, rowloss, block = fn.xent_forward(logits, labels, V, xc.IGNORE)
    loss, grad = _run(logits, labels, V)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert torch.equal(loss, block[0])
    valid = xc.valid_rows(labels, V)
    assert block[1].item() == _inv32(int(valid.sum()))
    xc.check_result(rowloss, loss, grad, logits, labels, V, xc.case_id(case))
    assert not rowloss[~valid].any()
    assert not grad[~valid].any() and not grad[:, V:].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_incoming_gradient_is_read_from_the_device(dtype):
    """(loss / 4).backward(): the scale reaches the kernel."""
    case = (9, 2051, 2056)
    logits, labels = xc.make_case(case, dtype, "cuda")
    lg = logits.detach().clone().requires_grad_(True)
    (ops.softmax_cross_entropy(lg, labels, num_classes=2051) / 4).backward()
    xc.check_grad(lg.grad, logits, labels, 2051, "gout 1/4", gout=0.25)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", [(5, 30522, 30522), (9, 2051, 2056)], ids=xc.case_id)
def test_inplace_backward_is_bitwise_and_lands_in_the_logits(case, dtype):
    N, V, ld = case
    logits, labels = xc.make_case(case, dtype, "cuda")
    _, want = _run(logits, labels, V)

    leaf = logits.detach().clone().requires_grad_(True)
    lg = leaf * 1.0  # a non-leaf with storage of its own, like a linear's output
    seen = {}

    def note_grad(g):
        seen["ptr"] = g.data_ptr()

    lg.register_hook(note_grad)
    ops.softmax_cross_entropy(lg, labels, num_classes=V, inplace_backward=True).backward()
    assert seen["ptr"] == lg.data_ptr()
    assert torch.equal(lg.detach(), want)      # the logits now hold the gradient
    assert torch.equal(leaf.grad, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_ignored_rows_are_not_read(dtype):
    case = (9, 2051, 2056)
    N, V, ld = case
    logits, labels = xc.make_case(case, dtype, "cuda")
    labels[4] = V + 3  # out of range: ignored like the ignore index
    ignored = ~xc.valid_rows(labels, V)
    assert int(ignored.sum()) == 2
    loss, grad = _run(logits, labels, V)
    poisoned = logits.clone()
    poisoned[ignored] = float("nan")
    loss2, grad2 = _run(poisoned, labels, V)
    assert torch.isfinite(loss2) and torch.equal(loss, loss2)
    assert torch.equal(grad, grad2)
    assert not grad2[ignored].any()
    # in place too: the NaN rows are overwritten with zeros
    lg = poisoned.clone().requires_grad_(True) * 1.0
    ops.softmax_cross_entropy(lg, labels, num_classes=V, inplace_backward=True).backward()
    assert torch.equal(lg.detach(), grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_out_of_range_label_is_ignored(dtype):
    N, V, ld = PADDED
    logits, labels = xc.make_case(PADDED, dtype, "cuda")
    labels[0] = V  # a pad column's index
    loss, grad = _run(logits, labels, V)
    assert not grad[0].any()
    as_ignored = labels.clone()
    as_ignored[0] = xc.IGNORE
    loss2, grad2 = _run(logits, as_ignored, V)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    xc.check_result(None, loss, grad, logits, labels, V, "label = V")
    _, _, _, block = fn.xent_forward(logits, labels, V, xc.IGNORE)
    assert block[1].item() == _inv32(3)  # rows 2, 3, 4


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_all_rows_ignored(dtype):
    logits, labels = xc.make_case((9, 2051, 2056), dtype, "cuda")
    labels.fill_(xc.IGNORE)
    labels[3] = 2051
    loss, grad = _run(logits, labels, 2051)
    assert loss.item() == 0.0
    assert not grad.any()
    _, _, _, block = fn.xent_forward(logits, labels, 2051, xc.IGNORE)
    assert block.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_reproducible(dtype):
    N, V, ld = PADDED
    logits, labels = xc.make_case(PADDED, dtype, "cuda")
    a = _run(logits, labels, V)
    b = _run(logits, labels, V)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_pad_columns(dtype):
    N, V, ld = PADDED
    logits, labels = xc.make_case(PADDED, dtype, "cuda")
    loss, grad = _run(logits, labels, V)
    assert not grad[:, V:].any()
    loud = logits.clone()
    loud[:, V:] = 1e4
    loss2, grad2 = _run(loud, labels, V)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_batched_shapes_and_errors():
    logits, labels = xc.make_case((12, 37, 40), torch.bfloat16, "cuda")
    loss2, grad2 = _run(logits, labels, 37)
    loss3, grad3 = _run(logits.view(3, 4, 40), labels.view(3, 4), 37)
    assert torch.equal(loss2, loss3)
    assert grad3.shape == (3, 4, 40) and torch.equal(grad2, grad3.view(12, 40))
    with pytest.raises(ValueError):
        ops.softmax_cross_entropy(logits, labels, num_classes=41)
    with pytest.raises(ValueError):
        ops.softmax_cross_entropy(logits, labels[:5], num_classes=37)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_graph_capture_follows_new_labels(dtype):
    """Forward and backward captured once; replayed on labels with another
    valid count, loss and gradient are the bits of an eager call on those
    labels. A count or 1/count passed as a launch argument would be frozen
    at capture."""
    case = (9, 2051, 2056)
    N, V, ld = case
    logits, labels = xc.make_case(case, dtype, "cuda")
    static_logits = logits.clone().requires_grad_(True)
    static_labels = labels.clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.softmax_cross_entropy(static_logits, static_labels, num_classes=V).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    static_logits.grad = None

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = ops.softmax_cross_entropy(static_logits, static_labels, num_classes=V)
        static_loss.backward()
    static_grad = static_logits.grad

    new_labels = labels.clone()
    new_labels[2] = xc.IGNORE
    new_labels[5] = xc.IGNORE
    new_labels[7] = V  # out of range
    assert int(xc.valid_rows(new_labels, V).sum()) != int(xc.valid_rows(labels, V).sum())
    for lab in (new_labels, labels):
        static_labels.copy_(lab)
        graph.replay()
        torch.cuda.synchronize()
        want_loss, want_grad = _run(logits, lab, V)
        assert torch.equal(static_loss.detach(), want_loss)
        assert torch.equal(static_grad, want_grad)


# ----------------------------------------------------------------- end to end


def _note_input(seen):
    """A forward hook that keeps a copy of the module's input in seen["x"]
    (and returns None: a returned value would replace the output)."""
    def hook(mod, args, out):
        seen["x"] = args[0].detach().clone()

    return hook


def _dw_from_fp32_dlogits(x2, weight, bias, labels, V):
    """The decoder weight gradient of the torch composition when the logits
    gradient stays fp32: dlogits of cross_entropy on the upcast logits,
    times the decoder's input, in fp32."""
    logits = F.linear(x2, weight, bias)
    lg32 = logits.detach().float().requires_grad_(True)
    F.cross_entropy(lg32[..., :V].view(-1, V), labels.view(-1), ignore_index=-100).backward()
    return lg32.grad.t() @ x2.float()


def _head_comparator(x2, weight, bias, labels, V):
    """The torch composition on a decoder linear: (loss, dW from bf16
    logits gradients, floor), where floor is the largest difference between
    that dW and the one computed from fp32 logits gradients: what the
    comparator itself moves by when only the rounding of dlogits changes."""
    w = weight.detach().clone().requires_grad_(True)
    logits = F.linear(x2, w, bias)
    loss = F.cross_entropy(logits[..., :V].float().view(-1, V), labels.view(-1),
                           ignore_index=-100)
    loss.backward()
    dw32 = _dw_from_fp32_dlogits(x2, weight, bias, labels, V)
    floor = (w.grad.float() - dw32).abs().max().item()
    return loss.detach(), w.grad, floor


def test_pretraining_engine_matches_torch_loss():
    """A single-rank PipelineEngine on a 2-encoder-layer pretraining model,
    bf16, dropout 0, vocabulary 1003 (logits padded to 1024): the MaskedLM
    loss against the same model under torch's cross_entropy on the sliced,
    upcast logits."""
    from skycomputing_amd.dataset import SyntheticMlmDataset
    from skycomputing_amd.models import bert_pretraining_pipeline_config
    from skycomputing_amd.optim import build_loss
    from skycomputing_amd.parallel import PartitionPlan, PipelineEngine, init_distributed

    V = 1003
    comm = init_distributed()
    cfgs = bert_pretraining_pipeline_config(
        2, dict(hidden_size=256, num_attention_heads=4, intermediate_size=1024,
                vocab_size=V, hidden_dropout_prob=0.0,
                attention_probs_dropout_prob=0.0))
    plan = PartitionPlan(stage_ranks=[0], ranges=[(0, len(cfgs))])
    ds = SyntheticMlmDataset(size=16, max_seq_length=32, vocab_size=V, seed=3)
    inputs = (ds.input_ids, ds.token_type_ids, ds.attention_mask)
    labels = ds.labels

    def torch_loss(logits, lab):
        return F.cross_entropy(logits[..., :V].float().view(-1, V), lab.view(-1),
                               ignore_index=-100)

    results = {}
    for name, loss_fn in (("fused", build_loss(dict(type="MaskedLM", num_classes=V,
                                                     inplace_backward=True))),
                          ("torch", torch_loss)):
        torch.manual_seed(6)
        engine = PipelineEngine(comm, cfgs, plan, loss_fn=loss_fn, dtype=torch.bfloat16,
                                stage_kwargs=dict(record_forward_time=False))
        head = engine.stage.module[-1]
        assert head.padded_vocab == 1024
        seen = {}
        head.decoder.register_forward_hook(_note_input(seen))
        loss = engine.run_iteration(inputs, labels, num_microbatches=1,
                                    schedule="sequential")
        results[name] = (loss, head.decoder.weight.grad.clone(), seen["x"],
                         head.decoder.weight.detach(), head.decoder.bias.detach())

    got_loss, got_dw, x_f, w_f, _ = results["fused"]
    ref_loss, ref_dw, x_t, w_t, b_t = results["torch"]
    assert torch.equal(w_f, w_t) and torch.equal(x_f, x_t), "the two models differ"
    ref64 = torch.tensor([ref_loss], dtype=torch.float64)
    kc.assert_colsum_ref(torch.tensor([got_loss], dtype=torch.float32), ref64, ref64.abs(),
                         "engine loss")
    dw32 = _dw_from_fp32_dlogits(x_t.view(-1, x_t.shape[-1]), w_t, b_t, labels.cuda(), V)
    floor = (ref_dw.float() - dw32).abs().max().item()
    print(f"decoder dW floor (comparator, bf16 vs fp32 dlogits): {floor:.3e}")
    kc.assert_bf16_close(got_dw, ref_dw.double(), floor, "decoder weight gradient")
    assert not got_dw[V:].any()  # pad rows of the decoder get no gradient


def test_lm_head_at_the_real_vocabulary():
    """BertLMHead at vocab_size 30522 on an 8 x 128 hidden input, plus the
    loss: the decoder linear runs at N = 30528."""
    from skycomputing_amd.models import BertLMHead

    torch.manual_seed(8)
    V = 30522
    head = BertLMHead(dict(hidden_size=256, num_attention_heads=4,
                           intermediate_size=1024, vocab_size=V)).cuda().bfloat16()
    assert head.padded_vocab == 30528 and head.num_classes == V
    hidden = torch.randn(8, 128, 256, device="cuda").to(torch.bfloat16)
    labels = torch.randint(0, V, (8, 128), device="cuda")
    labels[torch.rand(8, 128, device="cuda") > 0.15] = -100
    seen = {}
    head.decoder.register_forward_hook(_note_input(seen))
    logits = head(hidden, None)
    assert logits.shape == (8, 128, 30528) and logits.dtype == torch.bfloat16
    loss = ops.softmax_cross_entropy(logits, labels, num_classes=head.num_classes,
                                     inplace_backward=True)
    loss.backward()
    got_dw = head.decoder.weight.grad
    x2 = seen["x"].view(-1, 256)
    ref_loss, ref_dw, floor = _head_comparator(
        x2, head.decoder.weight.detach(), head.decoder.bias.detach(), labels, V)
    ref64 = ref_loss.double().reshape(1)
    kc.assert_colsum_ref(loss.detach().reshape(1), ref64, ref64.abs(), "real-width loss")
    print(f"decoder dW floor (comparator, bf16 vs fp32 dlogits): {floor:.3e}")
    kc.assert_bf16_close(got_dw, ref_dw.double(), floor, "decoder weight gradient")
    assert not got_dw[V:].any()
    assert all(torch.isfinite(p.grad).all() for p in head.parameters())
