"""Masked-LM pretraining, tiny: 24 narrow encoder layers + BertLMHead, even
allocation, 2-rank CPU plumbing check of the pretraining path (synthetic
MLM data, the MaskedLM loss through ops.softmax_cross_entropy's eager form).

Run: python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \
  --master-addr 127.0.0.1 experiment/launch.py \
  -c experiment/configs/pretraining/bert24_mlm_cpu.py
"""

base = "../../config.py"

VOCAB = 1003  # not a multiple of 64: the head pads its logits to 1024

BERT_CONFIG = dict(
    vocab_size=VOCAB,
    hidden_size=64,
    num_attention_heads=4,
    intermediate_size=128,
    max_position_embeddings=64,
    hidden_dropout_prob=0.1,
    attention_probs_dropout_prob=0.1,
)

model_config = dict(kind="bert_mlm", num_encoder_layers=24, bert_config=BERT_CONFIG)
data_config = dict(
    batch_size=8,
    dataset=dict(
        layer_type="SyntheticMlmDataset", size=64, max_seq_length=32,
        vocab_size=VOCAB, mlm_probability=0.15, seed=7,
    ),
)
allocator_config = dict(
    mode="even",
    benchmark=dict(batch_size=8, seq_len=32, hidden=64, iterations=2),
    stimulate=False,
)
train_config = dict(
    max_epoch=1,
    max_iter=4,
    optimizer=dict(type="AdamW", lr=1e-3, weight_decay=0.01, max_grad_norm=1.0,
                   no_decay="1d"),
    loss=dict(type="MaskedLM", num_classes=VOCAB, ignore_index=-100),
    num_microbatches=2,
    schedule="gpipe",
    log_interval=1,
    hooks=[dict(layer_type="TimerHook"), dict(layer_type="StopHook", root=".")],
)
