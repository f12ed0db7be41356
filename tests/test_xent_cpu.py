"""Masked-LM pretraining without a GPU: the eager softmax cross-entropy
against the fp64 reference by the rules of tests/xent_checks.py, the proof
that those rules pass the kernel's arithmetic and reject four subtly wrong
ones, the op's contracts against torch, SyntheticMlmDataset, BertLMHead,
build_loss, and a 2-rank gloo pretraining pipeline against one process.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import xent_checks as xc
from .helpers import run_multiprocess

from skycomputing_amd import ops

DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["fp32", "bf16"]


def _eager_run(logits, labels, V, **kw):
    lg = logits.detach().clone().requires_grad_(True)
    loss = ops.softmax_cross_entropy(lg, labels, num_classes=V, **kw)
    loss.backward()
    return loss.detach(), lg.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", xc.CASES, ids=xc.case_id)
def test_eager_op_matches_fp64(case, dtype):
    N, V, ld = case
    logits, labels = xc.make_case(case, dtype)
    loss, grad = _eager_run(logits, labels, V)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    xc.check_result(None, loss, grad, logits, labels, V, xc.case_id(case))
    assert not grad[:, V:].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", xc.CASES, ids=xc.case_id)
def test_kernel_arithmetic_passes_the_rules(case, dtype):
    """The fp32 loop written as the kernel computes (online max/sum over 256
    threads, shifted loss) is inside every rule."""
    N, V, ld = case
    logits, labels = xc.make_case(case, dtype)
    rowloss, mean, grad = xc.kernel_loop32(logits, labels, V)
    xc.check_result(rowloss, mean, grad, logits, labels, V, xc.case_id(case))


# (wrong variant, the rule that has to trip, cases). fp32, so that no bf16
# rounding of the gradient covers an fp32 mistake.
#   unshifted_lse: (rowmax + logsum) - z[label] carries an error of an ulp
#     of the spike, 80 (3.8e-6), where the loss itself is 0.31; the
#     gradient of the spike row inherits it through exp(z - (max + lse)).
#     Cases with the spike row (V > 3) and few enough rows that the
#     comparator's pooled error stays near an ulp of a loss.
#   mean_over_all_rows: cases with an ignored row (N > 2).
#   pad_in_softmax: cases with pad columns.
REJECTED = [
    ("unshifted_lse", xc.check_grad, [(3, 7, 7), (4, 8, 8), (2, 4099, 4099), (5, 30522, 30528)]),
    ("unshifted_lse", xc.check_rowloss, [(3, 7, 7), (4, 8, 8), (2, 4099, 4099)]),
    ("mean_over_all_rows", xc.check_mean, [c for c in xc.CASES if c[0] > 2]),
    ("mean_over_all_rows", xc.check_grad, [c for c in xc.CASES if c[0] > 2]),
    ("no_onehot", xc.check_grad, xc.CASES),
    ("pad_in_softmax", xc.check_rowloss, [c for c in xc.CASES if c[2] > c[1]]),
    ("pad_in_softmax", xc.check_grad, [c for c in xc.CASES if c[2] > c[1]]),
]


@pytest.mark.parametrize("wrong,rule,cases", REJECTED,
                         ids=[f"{w}-{r.__name__}" for w, r, _ in REJECTED])
def test_rules_reject_wrong_variant(wrong, rule, cases):
    for case in cases:
        N, V, ld = case
        logits, labels = xc.make_case(case, torch.float32)
        rowloss, mean, grad = xc.kernel_loop32(logits, labels, V, wrong=wrong)
        got = {xc.check_rowloss: rowloss, xc.check_mean: mean, xc.check_grad: grad}[rule]
        with pytest.raises(AssertionError):
            rule(got, logits, labels, V, f"{wrong} {xc.case_id(case)}")


# ------------------------------------------------------------------ contracts


def test_all_rows_ignored_gives_zero_loss_and_gradient():
    logits, _ = xc.make_case((4, 8, 8), torch.float32)
    labels = torch.full((4,), -100)
    loss, grad = _eager_run(logits, labels, 8)
    assert loss.item() == 0.0
    assert not grad.any()
    # torch, for the record, returns NaN there
    assert math.isnan(F.cross_entropy(logits, labels, ignore_index=-100).item())


def test_out_of_range_label_is_ignored():
    case = (9, 2051, 2056)
    N, V, ld = case
    logits, labels = xc.make_case(case, torch.float32)
    bad = labels.clone()
    bad[0] = V          # a pad column's index: would be in range of ld
    bad[3] = -7
    bad[4] = 10 ** 12
    loss, grad = _eager_run(logits, bad, V)
    as_ignored = labels.clone()
    as_ignored[[0, 3, 4]] = -100
    want = F.cross_entropy(logits[:, :V], as_ignored, ignore_index=-100)
    assert torch.allclose(loss, want, rtol=1e-6, atol=0)
    assert not grad[[0, 1, 3, 4]].any()
    assert grad[2].any()


def test_custom_ignore_index_inside_the_classes():
    logits, labels = xc.make_case((9, 2051, 2056), torch.float32)
    labels[2] = 5
    loss, grad = _eager_run(logits, labels, 2051, ignore_index=5)
    lab = labels.clone()
    lab[labels == -100] = 5  # torch knows one ignore index
    want = F.cross_entropy(logits[:, :2051], lab, ignore_index=5)
    assert torch.allclose(loss, want, rtol=1e-6, atol=0)
    assert not grad[2].any()


def test_pad_columns_are_excluded_and_get_zero_gradient():
    case = (9, 2051, 2056)
    N, V, ld = case
    logits, labels = xc.make_case(case, torch.float32)
    loss, grad = _eager_run(logits, labels, V)
    want = F.cross_entropy(logits[:, :V], labels, ignore_index=-100)
    assert torch.allclose(loss, want, rtol=1e-6, atol=0)
    assert not grad[:, V:].any()
    loud = logits.clone()
    loud[:, V:] = 1e4
    loss2, grad2 = _eager_run(loud, labels, V)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_batched_logits_and_labels():
    case = (12, 37, 40)
    logits, labels = xc.make_case(case, torch.float32)
    loss2, grad2 = _eager_run(logits, labels, 37)
    loss3, grad3 = _eager_run(logits.view(3, 4, 40), labels.view(3, 4), 37)
    assert torch.equal(loss2, loss3)
    assert grad3.shape == (3, 4, 40) and torch.equal(grad2, grad3.view(12, 40))
    with pytest.raises(ValueError):
        ops.softmax_cross_entropy(logits.view(3, 4, 40), labels, num_classes=37)
    with pytest.raises(ValueError):
        ops.softmax_cross_entropy(logits, labels, num_classes=41)


def test_nan_in_ignored_rows_stays_out():
    logits, labels = xc.make_case((9, 2051, 2056), torch.float32)
    loss, grad = _eager_run(logits, labels, 2051)
    poisoned = logits.clone()
    poisoned[1] = float("nan")
    loss2, grad2 = _eager_run(poisoned, labels, 2051)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


# -------------------------------------------------------------------- dataset


def _mlm(**kw):
    from skycomputing_amd.dataset import SyntheticMlmDataset

    return SyntheticMlmDataset(**kw)


def test_mlm_dataset_is_deterministic_per_seed():
    a = _mlm(size=32, max_seq_length=32, vocab_size=1003, seed=3)
    b = _mlm(size=32, max_seq_length=32, vocab_size=1003, seed=3)
    c = _mlm(size=32, max_seq_length=32, vocab_size=1003, seed=4)
    assert torch.equal(a.input_ids, b.input_ids) and torch.equal(a.labels, b.labels)
    assert not torch.equal(a.input_ids, c.input_ids)
    (ids, tids, mask), labels = a[5]
    assert ids.shape == tids.shape == mask.shape == labels.shape == (32,)
    assert labels.dtype == torch.int64


def test_mlm_dataset_is_registered():
    from skycomputing_amd.builder import build_dataloader_from_cfg

    loader = build_dataloader_from_cfg(
        4, dict(type="SyntheticMlmDataset", size=8, max_seq_length=16,
                vocab_size=500, seed=1))
    (ids, tids, mask), labels = next(iter(loader))
    assert ids.shape == (4, 16) and labels.shape == (4, 16)


@pytest.mark.parametrize("p", [0.15, 0.4])
def test_mlm_dataset_label_share_and_recipe(p):
    vocab = 30522
    ds = _mlm(size=512, max_seq_length=128, vocab_size=vocab, mlm_probability=p, seed=11)
    real = ds.attention_mask.bool()
    chosen = ds.labels != -100
    assert not (chosen & ~real).any(), "a padded position is labelled"
    assert (~real).any(), "the data has no padding to test with"
    n = int(real.sum())
    share = int(chosen.sum()) / n
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"labelled share {share:.4f} of {n} positions, p {p}, 4 sigma {4 * sigma:.4f}")
    assert abs(share - p) <= 4 * sigma
    # labelled positions hold the original id, the rest the ignore index
    assert torch.equal(ds.labels[chosen], ds.original_ids[chosen])
    assert (ds.labels[~chosen] == -100).all()
    # unchosen inputs are untouched; of the chosen 80 % are [MASK], about
    # 10 % keep their id, the rest is another id (each within 4 sigma)
    assert torch.equal(ds.input_ids[~chosen], ds.original_ids[~chosen])
    k = int(chosen.sum())
    masked = int((ds.input_ids[chosen] == 103).sum())
    kept = int((ds.input_ids[chosen] == ds.original_ids[chosen]).sum())
    for got, q in ((masked, 0.8 + 0.1 / vocab), (kept, 0.1 + 0.1 / vocab + 0.8 / vocab)):
        assert abs(got / k - q) <= 4 * math.sqrt(q * (1 - q) / k), (got, k, q)
    assert 0 <= int(ds.input_ids.min()) and int(ds.input_ids.max()) < vocab


# ----------------------------------------------------------------------- head


TINY = dict(hidden_size=64, num_attention_heads=4, intermediate_size=128,
            vocab_size=1003, max_position_embeddings=64,
            hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def test_lm_head_shapes_and_costs():
    from skycomputing_amd.models import BertLMHead

    head = BertLMHead(TINY)
    assert head.num_classes == 1003 and head.padded_vocab == 1024
    assert BertLMHead(dict(TINY, vocab_size=30522)).padded_vocab == 30528
    assert BertLMHead(dict(TINY, vocab_size=1024)).padded_vocab == 1024
    hidden = torch.randn(2, 5, 64)
    logits = head(hidden, torch.zeros(2, 1, 1, 5))
    assert logits.shape == (2, 5, 1024)
    B, S, H, Vp = 4, 16, 64, 1024
    assert head.layer_flops(B, S) == 2.0 * B * S * H * H + 2.0 * B * S * H * Vp
    assert head.activation_numel(B, S) == B * S * (2 * H + Vp)
    assert head.decoder.weight.shape == (1024, 64) and head.decoder.bias is not None


def test_pretraining_pipeline_config_builds():
    from skycomputing_amd.builder import build_module_from_cfg
    from skycomputing_amd.models import bert_pretraining_pipeline_config

    cfgs = bert_pretraining_pipeline_config(2, TINY)
    assert [c["layer_type"] for c in cfgs] == (
        ["BertEmbeddings"] + ["BertLayer_Head", "BertLayer_Body", "BertLayer_Tail"] * 2
        + ["BertLMHead"])
    stage = build_module_from_cfg(cfgs, record_forward_time=False)
    ids = torch.randint(0, 1003, (2, 8))
    logits = stage(ids, torch.zeros_like(ids), torch.ones_like(ids))
    assert logits.shape == (2, 8, 1024)
    # the embedding table and the decoder are separate parameters
    assert stage.module[0].word_embeddings.weight.data_ptr() != \
        stage.module[-1].decoder.weight.data_ptr()


def test_pretraining_configs_load():
    import os

    from skycomputing_amd.config import load_config

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "experiment", "configs", "pretraining")
    for name, layers in (("bert24_mlm_cpu.py", 24), ("bert160_mlm_8gpu.py", 160)):
        cfg = load_config(os.path.join(root, name))
        assert cfg.model_config["kind"] == "bert_mlm"
        assert cfg.model_config["num_encoder_layers"] == layers
        assert cfg.train_config["loss"]["type"] == "MaskedLM"
        assert cfg.train_config["loss"]["num_classes"] == \
            cfg.model_config["bert_config"]["vocab_size"]
        assert cfg.data_config["dataset"]["layer_type"] == "SyntheticMlmDataset"
        assert "logging_config" in cfg  # inherited from the base config


# ----------------------------------------------------------------- build_loss


def test_build_loss_default_is_the_classification_loss():
    from skycomputing_amd.optim import build_loss

    logits = torch.randn(6, 3)
    labels = torch.randint(0, 3, (6,))
    want = F.cross_entropy(logits.float(), labels)
    for cfg in (None, {}, dict(type="CrossEntropy")):
        assert torch.equal(build_loss(cfg)(logits, labels), want)


def test_build_loss_masked_lm_and_unknown():
    from skycomputing_amd.optim import build_loss

    logits, labels = xc.make_case((9, 2051, 2056), torch.float32)
    fn = build_loss(dict(type="MaskedLM", num_classes=2051, ignore_index=-100,
                         inplace_backward=False))
    want = ops.softmax_cross_entropy(logits, labels, num_classes=2051)
    assert torch.equal(fn(logits, labels), want)
    with pytest.raises(ValueError, match="unknown loss type"):
        build_loss(dict(type="Hinge"))


# ------------------------------------------------------------ 2-rank pipeline


def _mlm_batch(bsz=8, seq=16, vocab=1003, seed=5):
    from skycomputing_amd.dataset import SyntheticMlmDataset

    ds = SyntheticMlmDataset(size=bsz, max_seq_length=seq, vocab_size=vocab,
                             mlm_probability=0.3, seed=seed)
    return (ds.input_ids, ds.token_type_ids, ds.attention_mask), ds.labels


def _mlm_reference(layer_cfgs, batch, labels, lr, steps, M):
    from skycomputing_amd.builder import build_module_from_cfg
    from skycomputing_amd.optim import build_loss

    torch.manual_seed(1234)
    stage = build_module_from_cfg(layer_cfgs, record_forward_time=False)
    opt = torch.optim.SGD(stage.parameters(), lr=lr)
    loss_fn = build_loss(dict(type="MaskedLM", num_classes=TINY["vocab_size"]))
    mb_in = [torch.chunk(b, M) for b in batch]
    mb_lab = torch.chunk(labels, M)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        tot = 0.0
        for m in range(M):
            loss = loss_fn(stage(*(x[m] for x in mb_in)), mb_lab[m])
            (loss / M).backward()
            tot += float(loss.detach())
        losses.append(tot / M)  # the mean of per-microbatch valid-token means
        opt.step()
    return losses


def _mlm_pipeline_worker(rank, world_size, layer_cfgs, batch, labels, lr, steps, M, out_dir):
    torch.manual_seed(1234)
    from skycomputing_amd.builder import build_module_from_cfg
    from skycomputing_amd.optim import FusedSGD, build_loss
    from skycomputing_amd.parallel import (
        PartitionPlan, PipelineEngine, destroy, init_distributed,
    )

    comm = init_distributed(backend="gloo", timeout_s=60)
    full = build_module_from_cfg(layer_cfgs, record_forward_time=False)
    L = len(layer_cfgs)
    plan = PartitionPlan(stage_ranks=[0, 1], ranges=[(0, L // 2), (L // 2, L)])
    engine = PipelineEngine(
        comm, layer_cfgs, plan,
        loss_fn=build_loss(dict(type="MaskedLM", num_classes=TINY["vocab_size"])),
        stage_kwargs=dict(record_forward_time=False))
    start, end = plan.ranges[engine.stage_idx]
    engine.stage.load_layer_state_dicts(
        [{k: v.detach().clone() for k, v in full.module[i].state_dict().items()}
         for i in range(start, end)])
    opt = FusedSGD(engine.parameters(), lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        losses.append(engine.run_iteration(batch, labels, num_microbatches=M,
                                           schedule="gpipe"))
        opt.step()
    if rank == 0:
        np.save(f"{out_dir}/mlm_losses.npy", np.array(losses, dtype=np.float64))
    comm.barrier()
    destroy()


def test_two_rank_pretraining_pipeline_matches_one_process(tmp_path):
    from skycomputing_amd.models import bert_pretraining_pipeline_config

    layer_cfgs = bert_pretraining_pipeline_config(2, TINY)
    batch, labels = _mlm_batch()
    assert (labels != -100).any() and (labels == -100).any()
    lr, steps, M = 0.05, 3, 2
    ref = _mlm_reference(layer_cfgs, batch, labels, lr, steps, M)
    run_multiprocess(_mlm_pipeline_worker, 2, 29980, layer_cfgs, batch, labels,
                     lr, steps, M, str(tmp_path))
    got = np.load(f"{tmp_path}/mlm_losses.npy")
    assert np.allclose(got, np.array(ref), rtol=1e-4, atol=1e-5), (got, ref)
    assert got[-1] < got[0]
