"""Masked-LM pretraining of the headline model: 160-layer BERT (H=1024,
A=16) + BertLMHead over the 30522-token vocabulary, dynamic allocation,
8xMI355X. The last stage carries the [B*S, 30528] logits; its loss is the
fused softmax cross-entropy (ops/hip/xent.hip), with the gradient written
over the logits (they are the decoder linear's output, which nothing else
reads).

Run: python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
  --master-addr 127.0.0.1 experiment/launch.py \
  -c experiment/configs/pretraining/bert160_mlm_8gpu.py
"""

base = "../../config.py"

BERT_CONFIG = dict(
    vocab_size=30522,
    hidden_size=1024,
    num_attention_heads=16,
    intermediate_size=4096,
    max_position_embeddings=512,
    hidden_dropout_prob=0.1,
    attention_probs_dropout_prob=0.1,
)

model_config = dict(kind="bert_mlm", num_encoder_layers=160, bert_config=BERT_CONFIG)
data_config = dict(
    batch_size=32,
    dataset=dict(
        layer_type="SyntheticMlmDataset", size=4096, max_seq_length=128,
        vocab_size=BERT_CONFIG["vocab_size"], mlm_probability=0.15, seed=7,
    ),
)
allocator_config = dict(
    mode="dynamic",
    benchmark=dict(batch_size=32, seq_len=128, iterations=5),
    stimulate=False,
)
train_config = dict(
    max_epoch=1,
    max_iter=30,
    optimizer=dict(type="AdamW", lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                   weight_decay=0.01, max_grad_norm=1.0, no_decay="1d"),
    loss=dict(type="MaskedLM", num_classes=BERT_CONFIG["vocab_size"],
              ignore_index=-100, inplace_backward=True),
    num_microbatches=0,  # auto
    schedule="gpipe",
    log_interval=1,
    hooks=[dict(layer_type="TimerHook"), dict(layer_type="StopHook", root=".")],
)
