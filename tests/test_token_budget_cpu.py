"""Token-budget batching (``--unpad true --max-tokens N``) on CPU: the
batch sampler, fixed-shape ``pack_batch``, ``ops.cross_entropy`` with
``ignore_index``, budgeted-vs-plain packed model equivalence in fp32, the
Trainer wiring (single process and gloo world 2) and the flag validation."""

import math

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from pdnlp_amd import ops
from pdnlp_amd.cli import token_budget_loader
from pdnlp_amd.config import Args, BertConfig
from pdnlp_amd.data import (SEQ_MULTIPLE, Collate, TokenBudgetBatchSampler,
                            pack_batch, sequence_lengths)
from pdnlp_amd.engine.trainer import build_training, graph_key
from pdnlp_amd.models import BertForSequenceClassification
from tests.utils_dist import run_distributed


def lognormal_lengths(n, seed=123, cap=128):
    """The stand-in of tools/bench_unpad.py for the dataset's lengths:
    lognormal with median 15 and mean 20, clipped to [3, cap]."""
    g = torch.Generator().manual_seed(seed)
    mu, sigma = math.log(15.0), math.sqrt(2.0 * math.log(20.0 / 15.0))
    x = torch.exp(mu + sigma * torch.randn(n, generator=g))
    return x.round().clamp(3, cap).long().tolist()


def padded_batch(lens, S, vocab=512, seed=0):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    mask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(5, vocab, (B, S), generator=g) * mask
    types = torch.randint(0, 2, (B, S), generator=g) * mask
    return {"input_ids": ids, "attention_mask": mask,
            "token_type_ids": types,
            "label": torch.randint(0, 6, (B,), generator=g)}


# --------------------------------------------------------------- 1: sampler
def test_sampler_partition():
    lens = lognormal_lengths(1000)
    s = TokenBudgetBatchSampler(lens, 1024, seed=7)
    batches = list(s)
    assert len(batches) == len(s)
    flat = sorted(i for b in batches for i in b)
    assert flat == list(range(1000)), "every index in exactly one batch"
    assert all(sum(lens[i] for i in b) <= 1024 for b in batches)

    capped = TokenBudgetBatchSampler(lens, 1024, max_sentences=40, seed=7)
    assert max(len(b) for b in capped) <= 40
    assert sorted(i for b in capped for i in b) == list(range(1000))

    assert list(TokenBudgetBatchSampler(lens, 1024, seed=7)) == batches
    assert list(TokenBudgetBatchSampler(lens, 1024, seed=8)) != batches

    s.set_epoch(1)
    again = list(s)
    assert again != batches, "set_epoch must change the order of batches"
    assert sorted(map(tuple, again)) == sorted(map(tuple, batches)), \
        "set_epoch must not change what the batches hold"
    assert len(again) == len(batches)

    with pytest.raises(ValueError, match="max_tokens"):
        TokenBudgetBatchSampler(lens + [1025], 1024)


# ----------------------------------------------------------- 2: budget fill
def test_sampler_budget_fill():
    lens = lognormal_lengths(1000)
    s = TokenBudgetBatchSampler(lens, 1024, seed=7)
    fills = [sum(lens[i] for i in b) / 1024 for b in s.batches[:-1]]
    mean = sum(fills) / len(fills)
    print(f"fill over {len(fills)} batches: mean {mean:.4f}, "
          f"worst {min(fills):.4f}")
    assert mean >= 0.95


# ----------------------------------------------------------------- 3: ranks
def test_sampler_ranks():
    lens = lognormal_lengths(1000)
    whole = TokenBudgetBatchSampler(lens, 1024, seed=7)
    ranks = [TokenBudgetBatchSampler(lens, 1024, seed=7, num_replicas=3,
                                     rank=r) for r in range(3)]
    for e in (0, 1):
        for s in ranks:
            s.set_epoch(e)
        per_rank = [list(s) for s in ranks]
        assert len({len(s) for s in ranks}) == 1
        assert all(len(b) == len(ranks[0]) for b in per_rank)
        seen = [tuple(b) for r in per_rank for b in r]
        assert set(seen) == set(map(tuple, whole.batches))
        twice = len(seen) - len(set(seen))
        assert twice <= 2 and twice == 3 * len(ranks[0]) - len(whole.batches)
    with pytest.raises(ValueError, match="rank"):
        TokenBudgetBatchSampler(lens, 1024, num_replicas=3, rank=3)
    # the rank-sharded copy Accelerator.prepare makes of an unsharded sampler
    whole.set_epoch(1)
    for r in range(3):
        assert list(whole.shard(3, r)) == list(ranks[r])


def test_sequence_lengths():
    class Tok:
        def encode(self, text, max_len):
            n = min(len(text), max_len)
            return [1] * max_len, [1] * n + [0] * (max_len - n), [0] * max_len

    assert sequence_lengths([("abc", 0), ("a" * 40, 1)], Tok(), 16) == [3, 16]
    b = padded_batch([1, 7, 16], 16)
    ds = [{k: v[i] for k, v in b.items()} for i in range(3)]
    assert sequence_lengths(ds, None, 16) == [1, 7, 16]


# ------------------------------------------------------------ 4: pack_batch
LENS4 = [1, 64, 65, 17, 40]


def test_pack_batch_fixed_shape():
    batch = padded_batch(LENS4, 128)
    p = pack_batch(batch, total_rows=256, seq_multiple=32)
    assert p["input_ids"].numel() == 256
    assert p["token_type_ids"].numel() == p["position_ids"].numel() == 256
    cu = p["cu_seqlens"]
    assert cu.numel() == 33 and cu.dtype == torch.int32
    assert cu[:6].tolist() == [0, 1, 65, 130, 147, 187]
    assert (cu[-28:] == 187).all()
    assert torch.equal(p["label"][:5], batch["label"])
    assert p["label"].numel() == 32 and (p["label"][5:32] == -100).all()
    assert p["num_seqs"] == 5 and isinstance(p["num_seqs"], int)
    assert p["max_seqlen"] == 65
    assert (p["input_ids"][187:] == 0).all()

    with pytest.raises(ValueError, match="total_rows"):
        pack_batch(padded_batch([128, 128, 1], 128), total_rows=256,
                   seq_multiple=32)

    # another composition, same padded count: one graph key
    q = pack_batch(padded_batch([30, 2, 100, 7, 9, 11, 50], 128, seed=1),
                   total_rows=256, seq_multiple=32)
    assert not torch.equal(q["cu_seqlens"], p["cu_seqlens"])
    assert graph_key(p, 128) == graph_key(q, 128) == ("packed", 256, 32, 128)

    # without the new arguments: today's output
    plain = pack_batch(batch)
    assert plain["input_ids"].numel() == 192
    assert plain["cu_seqlens"].tolist() == [0, 1, 65, 130, 147, 187]
    assert torch.equal(plain["label"], batch["label"])
    assert plain["max_seqlen"] == 65
    for k in ("input_ids", "token_type_ids", "position_ids"):
        assert torch.equal(plain[k], p[k][:192])
        assert (p[k][192:] == 0).all()
    assert torch.equal(plain["cu_seqlens"], cu[:6])


def test_collate_passes_budget_through():
    batch = padded_batch(LENS4, 128)
    samples = [{k: v[i] for k, v in batch.items()} for i in range(5)]
    out = Collate(None, 128, unpad=True, max_tokens=256,
                  seq_multiple=SEQ_MULTIPLE)(samples)
    ref = pack_batch(batch, total_rows=256, seq_multiple=32)
    for k in ("input_ids", "cu_seqlens", "label"):
        assert torch.equal(out[k], ref[k])
    # padded collate ignores the budget
    assert "attention_mask" in Collate(None, 128, max_tokens=256)(samples)


# --------------------------------------------------------- 5: cross_entropy
def test_cross_entropy_ignore_index_cpu():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(12, 6, generator=g)
    labels = torch.randint(0, 6, (12,), generator=g)
    labels[[0, 5, 11]] = -100
    a = logits.clone().requires_grad_()
    b = logits.clone().requires_grad_()
    la = ops.cross_entropy(a, labels, ignore_index=-100)
    lb = F.cross_entropy(b, labels, ignore_index=-100)
    assert torch.equal(la, lb)
    (la * 1.7).backward()
    (lb * 1.7).backward()
    assert torch.equal(a.grad, b.grad)
    assert (a.grad[[0, 5, 11]] == 0).all()

    full = torch.randint(0, 6, (12,), generator=g)
    assert torch.equal(ops.cross_entropy(logits, full, ignore_index=None),
                       ops.cross_entropy(logits, full))


# ----------------------------------------------------- 6: model equivalence
def _logits_and_grads(model, p):
    model.zero_grad(set_to_none=True)
    out = model(input_ids=p["input_ids"], token_type_ids=p["token_type_ids"],
                labels=p["label"], cu_seqlens=p["cu_seqlens"],
                max_seqlen=p["max_seqlen"], position_ids=p["position_ids"])
    out.loss.backward()
    return out.loss.detach(), out.logits.detach(), \
        {n: q.grad.clone() for n, q in model.named_parameters()}


@pytest.mark.parametrize("lens", [LENS4, [128, 64, 64]],
                         ids=["tail-rows", "exact-fill-clamp"])
def test_budgeted_model_matches_plain_packed(lens):
    cfg = BertConfig.tiny()
    cfg.max_position_embeddings = 128
    torch.manual_seed(0)
    model = BertForSequenceClassification(cfg).train()  # dropout is 0
    batch = padded_batch(lens, 128)
    plain = pack_batch(batch)
    budget = pack_batch(batch, total_rows=256, seq_multiple=32)
    if sum(lens) == 256:   # empty sequences start at T: the clamp case
        assert int(budget["cu_seqlens"][-1]) == budget["input_ids"].numel()
    loss_a, logits_a, grads_a = _logits_and_grads(model, plain)
    loss_b, logits_b, grads_b = _logits_and_grads(model, budget)
    n = len(lens)
    assert logits_b.shape[0] == 32 and torch.isfinite(logits_b).all()
    # comparison and tolerance of test_unpad_cpu (packed against padded)
    torch.testing.assert_close(loss_b, loss_a, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(logits_b[:n], logits_a, rtol=1e-5, atol=1e-5)
    assert grads_a.keys() == grads_b.keys()
    for k in grads_a:
        torch.testing.assert_close(grads_b[k], grads_a[k], rtol=1e-5,
                                   atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


# ---------------------------------------------------------------- 7: Trainer
class _MixedDs(Dataset):
    """Pre-tokenized samples of mixed length 1..S."""

    def __init__(self, n=60, S=64, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for _ in range(n):
            L = 1 + int(torch.randint(0, S, (1,), generator=g))
            ids = torch.randint(106, 512, (S,), generator=g)
            ids[0] = 101
            mask = (torch.arange(S) < L).long()
            self.items.append({
                "input_ids": ids * mask, "attention_mask": mask,
                "token_type_ids": torch.zeros(S, dtype=torch.long),
                "label": torch.tensor(int(ids[0 if L == 1 else 1]) % 6)})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _budget_args(out_dir, **kw):
    args = Args()
    args.epochs = 1
    args.do_dev = False
    args.log_every = 100
    args.max_seq_len = 64
    args.unpad = True
    args.max_tokens = 256
    args.num_workers = 0
    args.strategy = "single"
    args.output_dir = str(out_dir)
    args.ckpt_path = str(out_dir) + "/model.pt"
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def _train_one_epoch(args, world=1, rank=0):
    torch.manual_seed(123)
    model, _, _, trainer = build_training(
        args, model=BertForSequenceClassification(BertConfig.tiny()))
    ds = _MixedDs()
    loader, sampler = token_budget_loader(args, ds, Collate(None, 64,
                                                            unpad=True),
                                          world, rank)
    seen = {"samples": 0, "losses": [], "shapes": set()}
    orig = trainer.on_step

    def spy(batch):
        seen["samples"] += batch["num_seqs"]
        seen["shapes"].add((batch["input_ids"].numel(),
                            batch["cu_seqlens"].numel() - 1))
        res = orig(batch)
        seen["losses"].append(float(res[0].detach()))
        return res

    trainer.on_step = spy
    counted = []
    import pdnlp_amd.engine.trainer as tr_mod
    real_timer = tr_mod.StepTimer

    class Timer(real_timer):
        def step(self, n_samples=0):
            counted.append(n_samples)
            super().step(n_samples)

    tr_mod.StepTimer = Timer
    try:
        trainer.train(loader, train_sampler=sampler)
    finally:
        tr_mod.StepTimer = real_timer
    return trainer, sampler, seen, counted, len(ds)


def test_trainer_token_budget(tmp_path):
    trainer, sampler, seen, counted, n = _train_one_epoch(
        _budget_args(tmp_path))
    assert len(sampler) >= 4, "the dataset must give several steps"
    assert trainer.global_step == len(sampler) == len(counted)
    assert sum(counted) == n == seen["samples"]
    assert all(math.isfinite(l) for l in seen["losses"])
    assert seen["shapes"] == {(256, 32)}


def _world2_epoch(rank, world, out_dir):
    import torch.distributed as dist
    args = _budget_args(out_dir, strategy="ddp", local_rank=rank)
    trainer, sampler, seen, counted, n = _train_one_epoch(args, world, rank)
    assert trainer.global_step == len(sampler) == len(counted)
    assert all(math.isfinite(l) for l in seen["losses"])
    steps = torch.tensor([trainer.global_step, seen["samples"]])
    both = [torch.zeros_like(steps) for _ in range(world)]
    dist.all_gather(both, steps)
    assert both[0][0] == both[1][0], "ranks must do the same number of steps"
    # an odd batch count wraps one batch: at most one batch seen twice
    total = int(both[0][1] + both[1][1])
    assert n <= total <= n + max(len(b) for b in sampler.batches)
    # timer.step counts real sentences x world
    assert sum(counted) == seen["samples"] * world
    for name, p in trainer.model.named_parameters():
        t = p.data.clone()
        dist.broadcast(t, src=0)
        assert torch.equal(t, p.data), f"rank divergence in {name}"
    dist.barrier()   # leave together: no rank tears down under a peer's recv


def test_trainer_token_budget_world2(tmp_path):
    run_distributed(_world2_epoch, world=2, args=(str(tmp_path),))


def test_dev_drops_ignored_rows(tmp_path):
    """dev() on budgeted batches: the empty sequences' rows (label -100) do
    not enter the accuracy."""
    args = _budget_args(tmp_path)
    torch.manual_seed(123)
    _, _, _, trainer = build_training(
        args, model=BertForSequenceClassification(BertConfig.tiny()))
    ds = _MixedDs(n=20)
    loader, _ = token_budget_loader(args, ds, Collate(None, 64, unpad=True),
                                    1, 0)
    plain = torch.utils.data.DataLoader(
        ds, batch_size=20, collate_fn=Collate(None, 64, unpad=True))
    _, acc_budget = trainer.dev(loader)
    _, acc_plain = trainer.dev(plain)
    assert abs(acc_budget - acc_plain) < 1e-9


# ------------------------------------------------------------- 8: validation
@pytest.mark.parametrize("kw,match", [
    (dict(unpad=False), "unpad"),
    (dict(strategy="dp"), "dp"),
    (dict(max_tokens=64, max_seq_len=128), "max-seq-len"),
    (dict(max_tokens=200), "multiple of 64"),
])
def test_invalid_configurations_raise(tmp_path, kw, match):
    args = _budget_args(tmp_path, **kw)
    with pytest.raises(ValueError, match=match):
        build_training(args, model=BertForSequenceClassification(
            BertConfig.tiny()))


def test_build_dataloaders_uses_the_budget(tmp_path, capsys):
    from pdnlp_amd.cli import build_dataloaders
    args = _budget_args(tmp_path, model="tiny", data_limit=50,
                        data_path=Args().data_path, dev_batch_size=4)
    train, dev, sampler = build_dataloaders(args, 1, 0)
    assert isinstance(train.batch_sampler, TokenBudgetBatchSampler)
    assert train.batch_sampler is sampler and train.batch_size is None
    assert capsys.readouterr().out.count("train_batch_size is not used") == 1
    b = next(iter(train))
    assert b["input_ids"].numel() == 256
    assert (b["cu_seqlens"].numel() - 1) % SEQ_MULTIPLE == 0
    # the dev loader keeps dev_batch_size and the plain packed collate
    d = next(iter(dev))
    assert dev.batch_size == 4 and d["cu_seqlens"].numel() == 5
    assert (d["label"] != -100).all()
    args.max_tokens = 200
    with pytest.raises(ValueError, match="multiple of 64"):
        build_dataloaders(args, 1, 0)


def test_cli_flags_parse():
    assert Args().max_tokens == 0 and Args().max_sentences == 0
    a = Args().apply_cli(["--max-tokens", "4096", "--max-sentences", "256"])
    assert a.max_tokens == 4096 and a.max_sentences == 256
