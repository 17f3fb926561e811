"""Tile-packed attention (``--attn-tile-pack``) on CPU: the properties of
the tile plan (its Python mirror), its item count on the stand-in
token-budget batches, the flag validation, and the model / Trainer wiring,
where the torch fallback ignores the plan and results are identical."""

import copy
import random

import pytest
import torch
from torch.utils.data import DataLoader

from pdnlp_amd import ops
from pdnlp_amd.config import Args, BertConfig
from pdnlp_amd.data import (Collate, SyntheticClsDataset,
                            TokenBudgetBatchSampler, pack_batch)
from pdnlp_amd.engine.trainer import build_training, check_attn_tile_pack
from pdnlp_amd.models import BertForSequenceClassification
from tests.test_token_budget_cpu import lognormal_lengths, padded_batch


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def _check_plan(lens, T):
    cu = _cu(lens)
    items, bounds = ops.tile_plan_reference(cu, T)
    # every real row is a Q row of exactly one item, no other row of any
    cover = [0] * T
    for row0, n, tile in items:
        assert n >= 1 and row0 >= 0 and row0 + n <= T
        if n <= 64:
            assert tile == 0, "a group has one tile"
        for r in range(row0 + tile * 64, row0 + min(n, tile * 64 + 64)):
            cover[r] += 1
    real = [False] * T
    for s0, s1 in zip(cu[:-1], cu[1:]):
        real[s0:s1] = [True] * (s1 - s0)
    assert cover == [int(x) for x in real]
    # bounds: the row's own sequence, start == end outside every sequence
    for b, n in enumerate(lens):
        assert bounds[cu[b]:cu[b + 1]] == [(cu[b], cu[b + 1])] * n
    assert all(s == e for s, e in bounds[cu[-1]:])
    # no sequence of at most 64 rows is split: it lies inside one item
    for b, n in enumerate(lens):
        if 0 < n <= 64:
            inside = [i for i in items
                      if i[1] <= 64 and i[0] <= cu[b]
                      and cu[b + 1] <= i[0] + i[1]]
            assert len(inside) == 1, (lens, b)
    # groups are whole sequences: they start and end on boundaries
    starts, ends = set(cu[:-1]), set(cu[1:])
    for row0, n, _ in items:
        if n <= 64:
            assert row0 in starts and row0 + n in ends
    # the items of long sequences are the live blocks of the per-sequence grid
    long_items = [i for i in items if i[1] > 64]
    live = [(cu[b], n, t) for b, n in enumerate(lens) if n > 64
            for t in range((n + 63) // 64)]
    assert long_items == live
    # order is the sequence order
    assert [i[0] + i[2] * 64 for i in items] == \
        sorted(i[0] + i[2] * 64 for i in items)
    # greedy: a group and the short sequence that follows it directly do
    # not fit one tile together
    for a, b in zip(items[:-1], items[1:]):
        if a[1] <= 64 and b[1] <= 64 and a[0] + a[1] == b[0]:
            first = next(n for s, n in zip(cu[:-1], lens)
                         if s >= b[0] and n > 0)
            assert a[1] + first > 64
    assert len(items) <= ops.tile_plan_max_items(T, len(lens))
    return items


FIXED = [
    ([20, 30, 14], 64, [(0, 64, 0)]),
    ([40, 30, 10], 128, [(0, 40, 0), (40, 40, 0)]),
    ([1, 1, 1, 1, 1], 64, [(0, 5, 0)]),
    ([5, 100, 7, 64, 3], 192,
     [(0, 5, 0), (5, 100, 0), (5, 100, 1), (105, 7, 0), (112, 64, 0),
      (176, 3, 0)]),
    ([10, 0, 0, 25, 0], 128, [(0, 35, 0)]),
    ([129, 20, 30, 200], 384,
     [(0, 129, 0), (0, 129, 1), (0, 129, 2), (129, 50, 0), (179, 200, 0),
      (179, 200, 1), (179, 200, 2), (179, 200, 3)]),
    ([65, 128, 70], 320,
     [(0, 65, 0), (0, 65, 1), (65, 128, 0), (65, 128, 1), (193, 70, 0),
      (193, 70, 1)]),
    ([0, 0], 64, []),
    ([64, 64], 192, [(0, 64, 0), (64, 64, 0)]),
]


@pytest.mark.parametrize("lens,T,want", FIXED)
def test_plan_fixed_cases(lens, T, want):
    assert _check_plan(lens, T) == want


def test_plan_properties_on_random_lengths():
    rng = random.Random(1234)
    for _ in range(400):
        lens = [rng.choice((0, rng.randint(1, 20), rng.randint(1, 64),
                            rng.randint(0, 200)))
                for _ in range(rng.randint(1, 14))]
        T = (sum(lens) + 63) // 64 * 64 + 64 * rng.randint(0, 3)
        _check_plan(lens, max(T, 64))


def test_item_bound_is_attained_up_to_rounding():
    """The two arms of the bound on their worst patterns: B single-row
    sequences behind long ones (T/64 + B), and a one-row group before every
    65-row sequence (3 items per 66 rows against 3*T/65 + 1)."""
    lens = [65] * 4 + [1]
    T = 320
    assert len(ops.tile_plan_reference(_cu(lens), T)[0]) == 9
    assert ops.tile_plan_max_items(T, len(lens)) == 10
    lens = [1, 65] * 31
    T = (sum(lens) + 63) // 64 * 64
    n = len(ops.tile_plan_reference(_cu(lens), T)[0])
    assert n == 93 and 3 * T // 65 + 1 == 95
    assert ops.tile_plan_max_items(T, len(lens)) == T // 64 + len(lens) == 94
    # many short sequences: the arm that does not grow with B takes over
    assert ops.tile_plan_max_items(4096, 224) == 3 * 4096 // 65 + 1 == 190


def test_item_count_on_stand_in_batches():
    """The 4096-row token-budget batches of the seeded lognormal stand-in:
    81.9 items per batch where the per-sequence grid has 210.0 live blocks
    (and 20.4 against 51.9 at 1024 rows)."""
    lens = lognormal_lengths(9200)
    for budget, want_items, want_live in ((4096, 81.9, 210.0),
                                          (1024, 20.4, 51.9)):
        s = TokenBudgetBatchSampler(lens, budget, seed=7)
        items, live = [], []
        for b in s.batches:
            cu = _cu([lens[i] for i in b])
            got = ops.tile_plan_reference(cu, budget)[0]
            assert len(got) <= ops.tile_plan_max_items(budget, len(b))
            items.append(len(got))
            live.append(sum((lens[i] + 63) // 64 for i in b))
        mean_items = sum(items) / len(items)
        mean_live = sum(live) / len(live)
        print(f"budget {budget}: {mean_items:.2f} items, {mean_live:.2f} "
              f"live per-sequence blocks, most items {max(items)}")
        assert round(mean_items, 1) == want_items
        assert round(mean_live, 1) == want_live


def test_cpu_plan_has_the_device_layout():
    cu = torch.tensor(_cu([5, 100, 7, 64, 3]), dtype=torch.int32)
    plan = ops.varlen_attention_plan(cu, 192)
    items, bounds = ops.tile_plan_reference(cu.tolist(), 192)
    m = ops.tile_plan_max_items(192, 5)
    assert plan.buf.dtype == torch.int32
    assert plan.buf.numel() == 4 + 4 * m + 2 * 192
    assert plan.count.item() == len(items)
    assert plan.items[:len(items), :3].tolist() == [list(i) for i in items]
    assert plan.bounds.tolist() == [list(b) for b in bounds]


# --------------------------------------------------------------- validation
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
    args = _args(tmp_path, attn_tile_pack=True)
    with pytest.raises(ValueError, match="--attn-tile-pack needs --unpad"):
        check_attn_tile_pack(args)
    with pytest.raises(ValueError, match="--attn-tile-pack needs --unpad"):
        build_training(args)
    from pdnlp_amd.cli import build_dataloaders
    with pytest.raises(ValueError, match="--attn-tile-pack needs --unpad"):
        build_dataloaders(args, 1, 0)
    args.unpad = True
    check_attn_tile_pack(args)


def test_option_defaults_and_cli():
    assert Args().attn_tile_pack is False
    assert BertConfig().attn_tile_pack is False
    a = Args().apply_cli(["--unpad", "true", "--attn-tile-pack", "true"])
    assert a.attn_tile_pack is True and a.unpad is True
    from pdnlp_amd.engine.hf_trainer import TrainingArguments
    assert TrainingArguments(output_dir="x").attn_tile_pack is False


# -------------------------------------------------------------------- model
def test_cpu_model_is_identical_with_the_option_on():
    torch.manual_seed(0)
    cfg = BertConfig.tiny()
    off = BertForSequenceClassification(cfg).train()
    on = copy.deepcopy(off)
    on.cfg.attn_tile_pack = True
    assert off.cfg.attn_tile_pack is False
    p = pack_batch(padded_batch([1, 7, 16, 3, 12], 16))
    outs = []
    for model in (off, on):
        out = model(input_ids=p["input_ids"],
                    token_type_ids=p["token_type_ids"], labels=p["label"],
                    cu_seqlens=p["cu_seqlens"], max_seqlen=p["max_seqlen"],
                    position_ids=p["position_ids"])
        out.loss.backward()
        outs.append(out)
    assert torch.equal(outs[0].logits, outs[1].logits)
    assert torch.equal(outs[0].loss, outs[1].loss)
    for (n, a), (_, b) in zip(off.named_parameters(), on.named_parameters()):
        assert torch.equal(a.grad, b.grad), n


def test_layers_receive_one_plan_per_forward(monkeypatch):
    """The model builds the plan once, before the layer loop, and every
    layer (also under activation checkpointing) receives that object."""
    torch.manual_seed(0)
    cfg = BertConfig.tiny()
    cfg.attn_tile_pack = True
    model = BertForSequenceClassification(cfg).train()
    built, seen = [], []
    real_plan, real_attn = ops.varlen_attention_plan, ops.attention_varlen

    def spy_plan(cu, total):
        built.append(real_plan(cu, total))
        return built[-1]

    def spy_attn(*a, plan=None, **kw):
        seen.append(plan)
        return real_attn(*a, plan=plan, **kw)

    monkeypatch.setattr(ops, "varlen_attention_plan", spy_plan)
    monkeypatch.setattr(ops, "attention_varlen", spy_attn)
    p = pack_batch(padded_batch([1, 7, 16, 3, 12], 16))
    kw = dict(input_ids=p["input_ids"], token_type_ids=p["token_type_ids"],
              labels=p["label"], cu_seqlens=p["cu_seqlens"],
              max_seqlen=p["max_seqlen"], position_ids=p["position_ids"])
    model(**kw)
    assert len(built) == 1 and len(seen) == cfg.num_hidden_layers
    assert all(s is built[0] for s in seen)
    model.gradient_checkpointing_enable()
    del built[:], seen[:]
    model(**kw).loss.backward()
    assert len(built) == 1 and len(seen) == 2 * cfg.num_hidden_layers
    assert all(s is built[0] for s in seen)
    cfg.attn_tile_pack = False
    del built[:], seen[:]
    model(**kw)
    assert not built and seen == [None] * cfg.num_hidden_layers


def test_trainer_step_with_the_option_on(tmp_path):
    args = _args(tmp_path, unpad=True, attn_tile_pack=True)
    model, opt, scaler, trainer = build_training(
        args, model=BertForSequenceClassification(BertConfig.tiny()))
    assert model.cfg.attn_tile_pack is True
    ds = SyntheticClsDataset(8, seq_len=16, vocab_size=512, var_len=True)
    loader = DataLoader(ds, batch_size=8, shuffle=False,
                        collate_fn=Collate(None, 16, unpad=True))
    before = [p.detach().clone() for p in model.parameters()]
    trainer.train(loader)
    assert trainer.global_step == 1
    assert any(not torch.equal(b, p.data)
               for b, p in zip(before, model.parameters()))
