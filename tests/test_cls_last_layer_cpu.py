"""CLS-only last encoder layer (``--cls-only-last-layer``) on CPU: the model
with the option on is the same function as with it off (fp64), the fallback
rule, the op's torch composition against a direct fp64 softmax, the flag
validation and the wiring down to the model's config."""

import copy
import math

import pytest
import torch

from pdnlp_amd import ops
from pdnlp_amd.config import Args, BertConfig
from pdnlp_amd.data import pack_batch
from pdnlp_amd.engine.trainer import (build_training,
                                      check_cls_only_last_layer)
from pdnlp_amd.models import (BertForSequenceClassification,
                              RobertaForSequenceClassification)
from pdnlp_amd.models.bert import cls_only_rows
from tests.test_token_budget_cpu import padded_batch

LENS = [5, 33, 1, 20, 64, 7]


def _kw(p):
    return dict(input_ids=p["input_ids"], token_type_ids=p["token_type_ids"],
                labels=p["label"], cu_seqlens=p["cu_seqlens"],
                max_seqlen=p["max_seqlen"], position_ids=p["position_ids"])


def _pair(cls=BertForSequenceClassification, cfg=None):
    torch.manual_seed(0)
    off = cls(cfg or BertConfig.tiny()).double().train()
    on = copy.deepcopy(off)
    on.cfg.cls_only_last_layer = True
    assert off.cfg.cls_only_last_layer is False
    return off, on


def _fwd_bwd(model, p):
    out = model(**_kw(p))
    out.loss.backward()
    return out


# -------------------------------------------------------------------- model
@pytest.mark.parametrize("ckpt", [False, True])
def test_model_is_the_same_function_in_fp64(ckpt):
    """In exact arithmetic option on and off are one function; in fp64 the
    rounding of a model this size is below 1e-12."""
    off, on = _pair()
    if ckpt:
        on.gradient_checkpointing_enable()
    p = pack_batch(padded_batch(LENS, 64), seq_multiple=8)
    T, B = p["input_ids"].numel(), p["cu_seqlens"].numel() - 1
    assert B == 8, "two empty sequences"
    assert cls_only_rows(on.cfg, T, B) == 64 < T
    a, b = _fwd_bwd(off, p), _fwd_bwd(on, p)
    assert b.logits.shape == a.logits.shape == (B, 6)
    assert (a.loss - b.loss).abs().item() <= 1e-9
    assert (a.logits[:6] - b.logits[:6]).abs().max().item() <= 1e-9
    for (n, x), (_, y) in zip(off.named_parameters(), on.named_parameters()):
        assert y.grad is not None and torch.isfinite(y.grad).all(), n
        assert (x.grad - y.grad).abs().max().item() <= 1e-9, n


def test_roberta_takes_cls_from_the_first_token_stream():
    cfg = BertConfig(vocab_size=512, hidden_size=64, num_hidden_layers=2,
                     num_attention_heads=4, intermediate_size=128,
                     max_position_embeddings=70, num_labels=6,
                     hidden_dropout_prob=0.0, pad_token_id=1,
                     type_vocab_size=1, attention_probs_dropout_prob=0.0,
                     model_type="roberta")
    off, on = _pair(RobertaForSequenceClassification, cfg)
    b = padded_batch(LENS, 64)
    b["token_type_ids"].zero_()
    p = pack_batch(b, seq_multiple=8, pad_token_id=1, roberta=True)
    a, c = _fwd_bwd(off, p), _fwd_bwd(on, p)
    assert (a.loss - c.loss).abs().item() <= 1e-9
    assert (a.logits[:6] - c.logits[:6]).abs().max().item() <= 1e-9
    for (n, x), (_, y) in zip(off.named_parameters(), on.named_parameters()):
        assert (x.grad - y.grad).abs().max().item() <= 1e-9, n


def test_hidden_states_come_back_as_the_first_token_stream():
    off, on = _pair()
    p = pack_batch(padded_batch(LENS, 64), seq_multiple=8)
    kw = {k: v for k, v in _kw(p).items() if k != "labels"}
    h_off, _ = off.bert(**kw)
    h_on, _ = on.bert(**kw)
    assert h_off.shape == (1, p["input_ids"].numel(), 64)
    assert h_on.shape == (1, 64, 64)
    first = p["cu_seqlens"][:6].long()
    assert (h_on[0, :6] - h_off[0, first]).abs().max().item() <= 1e-9


def test_fallback_rule_one_sequence_in_a_64_row_stream():
    """ceil64(B) >= T: nothing to save, the layer runs as with the option
    off, to the bit."""
    off, on = _pair()
    p = pack_batch(padded_batch([20], 64))
    assert p["input_ids"].numel() == 64
    assert cls_only_rows(on.cfg, 64, 1) is None
    a, b = _fwd_bwd(off, p), _fwd_bwd(on, p)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.logits, b.logits)
    for (n, x), (_, y) in zip(off.named_parameters(), on.named_parameters()):
        assert torch.equal(x.grad, y.grad), n


def test_rows_are_a_function_of_t_and_b():
    cfg = BertConfig(cls_only_last_layer=True)
    assert cls_only_rows(BertConfig(), 4096, 208) is None
    assert cls_only_rows(cfg, 4096, 208) == 256
    assert cls_only_rows(cfg, 320, 6) == 64
    assert cls_only_rows(cfg, 128, 64) == 64
    assert cls_only_rows(cfg, 128, 65) is None
    assert cls_only_rows(cfg, 64, 1) is None


# ----------------------------------------------------------------------- op
def test_op_fallback_against_a_direct_fp64_softmax():
    nh, hd = 2, 16
    H = nh * hd
    lens, T, rows = [4, 0, 9, 1], 16, 8
    cu = [0, 4, 4, 13, 14]
    torch.manual_seed(1)
    qkv = torch.randn(T, 3 * H, dtype=torch.float64, requires_grad=True)
    cu_t = torch.tensor(cu, dtype=torch.int32)
    o = ops.cls_attention(qkv, cu_t, rows, max(lens), nh)
    assert o.shape == (rows, H)
    ref = torch.zeros(rows, H, dtype=torch.float64)
    x = qkv.detach()
    for i, (s0, s1) in enumerate(zip(cu[:-1], cu[1:])):
        for h in range(nh):
            if s1 == s0:
                continue
            q = x[s0, h * hd:(h + 1) * hd]
            k = x[s0:s1, H + h * hd:H + (h + 1) * hd]
            v = x[s0:s1, 2 * H + h * hd:2 * H + (h + 1) * hd]
            pr = torch.softmax(k @ q / math.sqrt(hd), dim=0)
            ref[i, h * hd:(h + 1) * hd] = pr @ v
    assert (o - ref).abs().max().item() <= 1e-12
    assert (o[1] == 0).all() and (o[4:] == 0).all()
    # the same rows as the full packed attention, gathered
    full = ops.attention_varlen(qkv, cu_t, max(lens), nh)
    for i in (0, 2, 3):
        assert (o[i] - full[cu[i]]).abs().max().item() <= 1e-12
    o.sum().backward()
    g = qkv.grad
    assert (g[14:] == 0).all(), "rows outside the sequences"
    assert (g[1:4, :H] == 0).all() and (g[5:13, :H] == 0).all(), \
        "q columns of non-first rows"
    assert g[0, :H].abs().sum() > 0 and g[1:4, H:].abs().sum() > 0
    with pytest.raises(ValueError, match="rows_out"):
        ops.cls_attention(qkv, cu_t, 3, max(lens), nh)


# ------------------------------------------------------- checks and wiring
def _args(tmp_path, **kw):
    args = Args()
    args.strategy = "single"
    args.model = "tiny"
    args.epochs, args.do_dev, args.log_every = 1, False, 1000
    args.num_workers = 0
    args.output_dir = str(tmp_path)
    args.ckpt_path = str(tmp_path / "model.pt")
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def test_option_needs_unpad(tmp_path):
    msg = "--cls-only-last-layer needs --unpad"
    args = _args(tmp_path, cls_only_last_layer=True)
    with pytest.raises(ValueError, match=msg):
        check_cls_only_last_layer(args)
    with pytest.raises(ValueError, match=msg):
        build_training(args)
    from pdnlp_amd.cli import build_dataloaders
    with pytest.raises(ValueError, match=msg):
        build_dataloaders(args, 1, 0)
    args.unpad = True
    check_cls_only_last_layer(args)


def test_defaults_cli_and_training_arguments(tmp_path):
    assert Args().cls_only_last_layer is False
    assert BertConfig().cls_only_last_layer is False
    a = Args().apply_cli(["--unpad", "true", "--cls-only-last-layer", "true"])
    assert a.cls_only_last_layer is True and a.unpad is True
    from pdnlp_amd.engine.hf_trainer import TrainingArguments
    assert TrainingArguments(output_dir="x").cls_only_last_layer is False

    # the CLI flag reaches the model's config through the Trainer
    args = _args(tmp_path).apply_cli(
        ["--unpad", "true", "--cls-only-last-layer", "true"])
    model, _, _, _ = build_training(
        args, model=BertForSequenceClassification(BertConfig.tiny()))
    assert model.cfg.cls_only_last_layer is True
    # and stays off without it
    model, _, _, _ = build_training(
        _args(tmp_path, unpad=True),
        model=BertForSequenceClassification(BertConfig.tiny()))
    assert model.cfg.cls_only_last_layer is False


def test_training_arguments_reach_the_model(tmp_path):
    from pdnlp_amd.engine.hf_trainer import HFStyleTrainer, TrainingArguments
    hf = TrainingArguments(output_dir=str(tmp_path), unpad=True,
                           cls_only_last_layer=True)
    model = BertForSequenceClassification(BertConfig.tiny())
    tr = HFStyleTrainer(model, hf)
    assert tr.args.cls_only_last_layer is True
    assert model.cfg.cls_only_last_layer is True
    with pytest.raises(ValueError, match="needs --unpad"):
        HFStyleTrainer(
            BertForSequenceClassification(BertConfig.tiny()),
            TrainingArguments(output_dir=str(tmp_path),
                              cls_only_last_layer=True))


def test_engine_sets_the_flag_on_its_own_copy():
    from pdnlp_amd.engine import InferenceEngine
    torch.manual_seed(0)
    model = BertForSequenceClassification(BertConfig.tiny()).eval()
    g = torch.Generator().manual_seed(3)
    seqs = [(torch.randint(5, 512, (n,), generator=g).tolist(), [0] * n)
            for n in LENS]
    off = InferenceEngine(model, device="cpu", max_seq_len=64, packed=True)
    on = InferenceEngine(model, device="cpu", max_seq_len=64, packed=True,
                         cls_only_last_layer=True)
    assert model.config.cls_only_last_layer is False
    assert off.model.config.cls_only_last_layer is False
    assert on.model.config.cls_only_last_layer is True
    assert on.model.bert.cfg is on.model.config
    a, b = off.forward_sequences(seqs), on.forward_sequences(seqs)
    assert a.shape == b.shape == (len(LENS), 6)
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError, match="packed=True"):
        InferenceEngine(model, device="cpu", cls_only_last_layer=True)
