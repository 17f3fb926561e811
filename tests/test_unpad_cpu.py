"""Padding-free path (``--unpad``) on CPU: pack_batch, packed-vs-padded
model equivalence in fp32, the attention_varlen fallback, the Trainer wiring
and world-2 DDP, ZeRO and hooks. In fp32 ``exp(-10000)`` is exactly 0, so the
padded run and the packed run are the same arithmetic up to summation
order."""

import pytest
import torch
from torch.utils.data import DataLoader, Dataset

from pdnlp_amd import ops
from pdnlp_amd.config import Args, BertConfig
from pdnlp_amd.data import Collate, pack_batch
from pdnlp_amd.engine.trainer import Trainer, build_training
from pdnlp_amd.models import (BertForSequenceClassification,
                              RobertaForSequenceClassification)
from pdnlp_amd.ops.adamw import build_optimizer
from tests.utils_dist import run_distributed


def _padded_batch(lens, S, vocab=512, pad=0, seed=0, label_key="label"):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    ids = torch.randint(5, vocab, (B, S), generator=g)
    mask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = ids * mask + pad * (1 - mask)
    types = torch.randint(0, 2, (B, S), generator=g) * mask
    return {"input_ids": ids, "attention_mask": mask,
            "token_type_ids": types,
            label_key: torch.randint(0, 6, (B,), generator=g)}


# ------------------------------------------------------------------ pack_batch
def test_pack_batch_layout():
    lens = [1, 64, 65, 3]
    batch = _padded_batch(lens, 128)
    p = pack_batch(batch)
    assert p["input_ids"].shape == (192,)
    assert p["input_ids"].dtype == torch.int64
    assert p["cu_seqlens"].dtype == torch.int32
    assert p["cu_seqlens"].tolist() == [0, 1, 65, 130, 133]
    assert p["max_seqlen"] == 65 and isinstance(p["max_seqlen"], int)
    assert torch.equal(p["label"], batch["label"])
    cu = p["cu_seqlens"].tolist()
    for b, n in enumerate(lens):
        sl = slice(cu[b], cu[b + 1])
        # unpacking reproduces the input rows
        assert torch.equal(p["input_ids"][sl], batch["input_ids"][b, :n])
        assert torch.equal(p["token_type_ids"][sl],
                           batch["token_type_ids"][b, :n])
        # positions restart per sequence
        assert torch.equal(p["position_ids"][sl], torch.arange(n))
    # tail is pad / 0 / 0
    assert (p["input_ids"][133:] == 0).all()
    assert (p["token_type_ids"][133:] == 0).all()
    assert (p["position_ids"][133:] == 0).all()


def test_pack_batch_multiple_and_label_key():
    batch = _padded_batch([5, 7], 16, label_key="labels")
    p = pack_batch(batch, multiple=256, label_key="labels", pad_token_id=3)
    assert p["input_ids"].shape == (256,)
    assert (p["input_ids"][12:] == 3).all()
    assert torch.equal(p["labels"], batch["labels"])


def test_pack_batch_roberta_positions_match_padded(monkeypatch):
    cfg = BertConfig.tiny()
    cfg.model_type, cfg.pad_token_id = "roberta", 1
    cfg.type_vocab_size, cfg.max_position_embeddings = 1, 80
    lens = [1, 64, 33, 3]
    batch = _padded_batch(lens, 64, pad=1)
    batch["token_type_ids"].zero_()
    seen = {}
    real = ops.embedding_layernorm

    def spy(input_ids, token_type_ids, position_ids, *a, **k):
        seen["pos"] = position_ids
        return real(input_ids, token_type_ids, position_ids, *a, **k)

    monkeypatch.setattr(ops, "embedding_layernorm", spy)
    model = RobertaForSequenceClassification(cfg).eval()
    model(batch["input_ids"], batch["attention_mask"])
    padded_pos = seen["pos"]
    p = pack_batch(batch, pad_token_id=1, roberta=True)
    cu = p["cu_seqlens"].tolist()
    for b, n in enumerate(lens):
        assert torch.equal(p["position_ids"][cu[b]:cu[b + 1]],
                           padded_pos[b, :n])


def test_pack_batch_rejects_non_prefix_mask():
    batch = _padded_batch([4, 6], 8)
    batch["attention_mask"][0, 1] = 0   # a hole inside the ones
    with pytest.raises(ValueError, match="prefix"):
        pack_batch(batch)
    batch = _padded_batch([4, 6], 8)
    batch["attention_mask"][1, 7] = 1   # a stray one after the zeros
    with pytest.raises(ValueError, match="prefix"):
        pack_batch(batch)


def test_collate_unpad_packs():
    from pdnlp_amd.data import SyntheticClsDataset
    ds = SyntheticClsDataset(4, seq_len=16, vocab_size=512, var_len=True)
    samples = [ds[i] for i in range(4)]
    padded = Collate(None, 16)(samples)
    packed = Collate(None, 16, unpad=True)(samples)
    assert "attention_mask" not in packed
    ref = pack_batch(padded)
    for k in ("input_ids", "token_type_ids", "position_ids", "cu_seqlens",
              "label"):
        assert torch.equal(packed[k], ref[k])
    assert packed["max_seqlen"] == ref["max_seqlen"]


# ------------------------------------------------- model: packed vs padded
def _logits_and_grads(model, **inputs):
    model.zero_grad(set_to_none=True)
    out = model(**inputs)
    out.loss.backward()
    return out.logits.detach(), {n: p.grad.clone()
                                 for n, p in model.named_parameters()}


@pytest.mark.parametrize("kind", ["bert", "roberta", "bert-ckpt"])
def test_model_packed_matches_padded(kind):
    cfg = BertConfig.tiny()
    pad = 0
    if kind == "roberta":
        cfg.model_type, cfg.pad_token_id, pad = "roberta", 1, 1
        cfg.max_position_embeddings = 80
        model = RobertaForSequenceClassification(cfg)
    else:
        model = BertForSequenceClassification(cfg)
    model.train()   # tiny() has dropout 0: train mode is deterministic
    if kind == "bert-ckpt":
        model.gradient_checkpointing_enable()
    batch = _padded_batch([5, 64, 1, 33], 64, pad=pad)
    p = pack_batch(batch, pad_token_id=pad, roberta=(kind == "roberta"))
    logits_a, grads_a = _logits_and_grads(
        model, input_ids=batch["input_ids"],
        attention_mask=batch["attention_mask"],
        token_type_ids=batch["token_type_ids"], labels=batch["label"])
    logits_b, grads_b = _logits_and_grads(
        model, input_ids=p["input_ids"],
        token_type_ids=p["token_type_ids"], labels=p["label"],
        cu_seqlens=p["cu_seqlens"], max_seqlen=p["max_seqlen"],
        position_ids=p["position_ids"])
    torch.testing.assert_close(logits_b, logits_a, rtol=1e-5, atol=1e-5)
    assert grads_a.keys() == grads_b.keys()
    # padding rows get exactly zero gradient in both runs (masked keys have
    # probability exactly 0, so nothing flows back from a CLS row to them):
    # every parameter, embeddings included, is compared in full
    for n in grads_a:
        torch.testing.assert_close(grads_b[n], grads_a[n], rtol=1e-5,
                                   atol=1e-5, msg=lambda m, n=n: f"{n}: {m}")


# ------------------------------------------------- attention_varlen fallback
def test_attention_varlen_cpu_fallback_tail_zero():
    torch.manual_seed(0)
    nh, hd = 2, 16
    H = nh * hd
    cu = torch.tensor([0, 5, 6, 40], dtype=torch.int32)
    T = 64
    qkv = torch.randn(T, 3 * H, requires_grad=True)
    o = ops.attention_varlen(qkv, cu, 34, nh)
    assert o.shape == (T, H)
    assert (o[40:] == 0).all()
    # sequences are independent: each equals attention on its own slice
    ref = ops.attention_packed(qkv[5:6].unsqueeze(0), None, nh)[0]
    torch.testing.assert_close(o[5:6], ref)
    ref = ops.attention_packed(qkv[6:40].unsqueeze(0), None, nh)[0]
    torch.testing.assert_close(o[6:40], ref)
    o.backward(torch.randn(T, H))
    assert (qkv.grad[40:] == 0).all()
    assert torch.isfinite(qkv.grad).all() and qkv.grad[:40].abs().sum() > 0


# ------------------------------------------------------------------ Trainer
class _VarLenDs(Dataset):
    """Tiny pre-tokenized dataset with mixed lengths (1..16) whose label is
    the second token's bucket (learnable)."""

    def __init__(self, n=24, S=16, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for i in range(n):
            L = 1 + int(torch.randint(0, S, (1,), generator=g))
            ids = torch.randint(106, 512, (S,), generator=g)
            ids[0] = 101
            tok = 106 + int(torch.randint(0, 12, (1,), generator=g))
            if L > 1:
                ids[1] = tok
            mask = (torch.arange(S) < L).long()
            self.items.append({
                "input_ids": ids * mask, "attention_mask": mask,
                "token_type_ids": torch.zeros(S, dtype=torch.long),
                "label": torch.tensor((tok - 106) % 6)})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _trainer_args(tmp_path, unpad):
    args = Args()
    args.epochs = 1
    args.do_dev = False
    args.max_seq_len = 16
    args.unpad = unpad
    args.output_dir = str(tmp_path)
    args.ckpt_path = str(tmp_path / f"model_{int(unpad)}.pt")
    return args


def _three_step_losses(tmp_path, unpad, hip_graph=False):
    torch.manual_seed(0)
    args = _trainer_args(tmp_path, unpad)
    args.hip_graph = hip_graph
    model = BertForSequenceClassification(BertConfig.tiny())
    opt = build_optimizer(model, lr=1e-3)
    trainer = Trainer(args, model, opt, torch.device("cpu"))
    loader = DataLoader(_VarLenDs(), batch_size=8, shuffle=False,
                        collate_fn=Collate(None, 16, unpad=unpad))
    losses = []
    orig = trainer.on_step

    def spy(batch):
        assert ("cu_seqlens" in batch) == unpad
        res = orig(batch)
        losses.append(float(res[0].detach()))
        return res

    trainer.on_step = spy
    trainer.train(loader)
    assert trainer.global_step == 3
    return losses, trainer


def test_trainer_unpad_matches_padded(tmp_path):
    padded, _ = _three_step_losses(tmp_path, unpad=False)
    packed, _ = _three_step_losses(tmp_path, unpad=True)
    assert len(padded) == len(packed) == 3
    for a, b in zip(padded, packed):
        assert abs(a - b) < 1e-5, (padded, packed)


def test_trainer_unpad_never_captures_graph(tmp_path, capsys):
    _, trainer = _three_step_losses(tmp_path, unpad=True, hip_graph=True)
    assert trainer._graph is None
    assert capsys.readouterr().out.count("hipGraph capture disabled") == 1


def _accumulated_params(tmp_path, unpad):
    """Three micro-batches accumulated into ONE plain-SGD step."""
    torch.manual_seed(0)
    args = _trainer_args(tmp_path, unpad)
    args.grad_accum_steps = 3
    model = BertForSequenceClassification(BertConfig.tiny())
    opt = build_optimizer(model, lr=0.1, optimizer="sgd", sgd_momentum=0.0)
    trainer = Trainer(args, model, opt, torch.device("cpu"))
    loader = DataLoader(_VarLenDs(), batch_size=8, shuffle=False,
                        collate_fn=Collate(None, 16, unpad=unpad))
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    trainer.train(loader)
    return before, dict(model.named_parameters())


def test_grad_accumulation_unpad_matches_padded(tmp_path):
    before, padded = _accumulated_params(tmp_path, unpad=False)
    _, packed = _accumulated_params(tmp_path, unpad=True)
    assert any(not torch.equal(before[n], padded[n]) for n in padded)
    for n in padded:
        # lr 0.1 x the 1e-5 gradient tolerance of the model test
        torch.testing.assert_close(packed[n], padded[n], rtol=1e-5,
                                   atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


def test_unpad_with_dp_raises(tmp_path):
    args = _trainer_args(tmp_path, unpad=True)
    args.strategy = "dp"
    with pytest.raises(ValueError, match="unpad"):
        build_training(args, model=BertForSequenceClassification(
            BertConfig.tiny()))


def test_cli_flag_parses():
    assert Args().unpad is False
    assert Args().apply_cli(["--unpad", "true"]).unpad is True


# -------------------------------------------------------------- distributed
def _unpad_two_steps(rank, world, out_dir, strategy):
    import torch.distributed as dist
    from pdnlp_amd.data import DistributedSampler

    torch.manual_seed(123)
    args = Args()
    args.epochs = 1
    args.do_dev = False
    args.log_every = 100
    args.max_seq_len = 16
    args.unpad = True
    args.strategy = strategy
    args.local_rank = rank
    args.output_dir = out_dir
    args.ckpt_path = out_dir + "/model.pt"
    model, _, _, trainer = build_training(
        args, model=BertForSequenceClassification(BertConfig.tiny()))
    ds = _VarLenDs(n=16)
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank,
                                 shuffle=False)
    loader = DataLoader(ds, batch_size=4, sampler=sampler,
                        collate_fn=Collate(None, 16, unpad=True))
    before = [p.detach().clone() for p in model.parameters()]
    trainer.train(loader, train_sampler=sampler)
    assert trainer.global_step == 2
    assert any(not torch.equal(b, p.data)
               for b, p in zip(before, model.parameters()))
    for n, p in model.named_parameters():
        t = p.data.clone()
        dist.broadcast(t, src=0)
        assert torch.equal(t, p.data), f"rank divergence in {n}"


@pytest.mark.parametrize("strategy", ["ddp", "zero", "hooks"])
def test_distributed_unpad_world2(tmp_path, strategy):
    """Two steps with unpad at world 2 (ranks see different token counts):
    both ranks end with identical parameters."""
    run_distributed(_unpad_two_steps, world=2,
                    args=(str(tmp_path), strategy))
