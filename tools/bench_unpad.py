#!/usr/bin/env python
"""Padded vs padding-free (``--unpad``) training steps on real-data lengths.

    python tools/bench_unpad.py [--pairs 5] [--steps 30] [--multiple 64]

Eager bf16 BERT-base training steps (forward, backward, fused AdamW) at
batch 32, once on padded [32, 128] batches and once on the same batches
packed by ``pack_batch``. Sequence lengths come from ``data/train.json``
when present (characters after space-strip plus [CLS]/[SEP], capped at
128), otherwise from a seeded synthetic sample clipped to [3, 128] with
median ~15 and mean ~20 — the statistics of the reference dataset's first
10 000 samples.

Method: a fixed pool of seeded batches lives on the device; every batch of
the pool runs once per mode before timing (each distinct packed length T is
a new shape). Timed windows of ``--steps`` steps alternate padded / unpad,
``--pairs`` times, each window closed by a device synchronise. The tool
reports every window, the range per mode and whether the ranges are
disjoint, then ``torch.cuda.memory_reserved()`` after ``--mem-steps`` steps
per mode (allocator cache emptied in between), and one JSON line.

A third mode, ``unpad_graph``, runs the same packed batches through the
Trainer's hipGraph cache (``--unpad true --hip-graph true``) in the same
alternating windows. After the eager pass it passes over the pool twice
more with capture on, so that
every batch key is captured and the timed windows hold replays only, and
reports what the graphs' shared memory pool holds.
"""
import argparse
import gc
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdnlp_amd.config import Args  # noqa: E402
from pdnlp_amd.data import load_data, pack_batch  # noqa: E402
from pdnlp_amd.engine.trainer import Trainer  # noqa: E402
from pdnlp_amd.models import build_model  # noqa: E402
from pdnlp_amd.ops.adamw import build_optimizer  # noqa: E402
from pdnlp_amd.utils import set_seed  # noqa: E402

S, VOCAB = 128, 21128


def lengths(n, seed, data_path):
    if os.path.isfile(data_path):
        data = load_data(data_path, limit=10000)
        lens = [min(len(t.replace(" ", "")) + 2, S) for t, _ in data]
        g = torch.Generator().manual_seed(seed)
        pick = torch.randint(0, len(lens), (n,), generator=g)
        return f"real lengths from {data_path}", [lens[i] for i in pick]
    # lognormal: median exp(mu) = 15, mean exp(mu + sigma^2/2) = 20
    g = torch.Generator().manual_seed(seed)
    mu, sigma = math.log(15.0), math.sqrt(2.0 * math.log(20.0 / 15.0))
    x = torch.exp(mu + sigma * torch.randn(n, generator=g))
    return ("synthetic lognormal lengths (median ~15, mean ~20)",
            x.round().clamp(3, S).long().tolist())


def make_batches(lens, batch, seed):
    g = torch.Generator().manual_seed(seed + 1)
    out = []
    for i in range(0, len(lens), batch):
        ll = torch.tensor(lens[i:i + batch])
        mask = (torch.arange(S)[None, :] < ll[:, None]).long()
        ids = torch.randint(106, VOCAB, (batch, S), generator=g)
        ids[:, 0] = 101
        ids[torch.arange(batch), ll - 1] = 102
        out.append({"input_ids": ids * mask, "attention_mask": mask,
                    "token_type_ids": torch.zeros_like(ids),
                    "label": torch.randint(0, 6, (batch,), generator=g)})
    return out


def to_device(b, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}


class Mode:
    def __init__(self, name, batches, dev, tile_pack=False, cls_only=False):
        set_seed(123)
        self.name = name
        self.model = build_model("bert-base").to(torch.bfloat16).to(dev)
        self.model.train()
        if tile_pack:  # --attn-tile-pack true
            self.model.cfg.attn_tile_pack = True
        if cls_only:   # --cls-only-last-layer true
            self.model.cfg.cls_only_last_layer = True
        self.opt = build_optimizer(self.model, lr=3e-5)
        self.batches = batches
        self.i = 0

    def step(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        if "cu_seqlens" in b:
            out = self.model(
                input_ids=b["input_ids"], token_type_ids=b["token_type_ids"],
                labels=b["label"], cu_seqlens=b["cu_seqlens"],
                max_seqlen=b["max_seqlen"], position_ids=b["position_ids"])
        else:
            out = self.model(
                input_ids=b["input_ids"], attention_mask=b["attention_mask"],
                token_type_ids=b["token_type_ids"], labels=b["label"])
        out.loss.backward()
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        return out.loss

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = None
        for _ in range(steps):
            # an eager step's loss keeps its autograd graph alive, and a
            # graph capture must not find one (Trainer.train_step)
            del loss
            loss = self.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        assert math.isfinite(loss.item()), f"{self.name}: loss {loss.item()}"
        return ms


class GraphMode(Mode):
    """The packed batches through the Trainer's hipGraph cache
    (``--unpad true --hip-graph true``): one captured graph per batch key,
    eager fused AdamW between replays."""

    def __init__(self, name, batches, dev, tile_pack=False, cls_only=False):
        super().__init__(name, batches, dev, tile_pack, cls_only)
        args = Args()
        args.unpad = True
        args.attn_tile_pack = tile_pack
        args.cls_only_last_layer = cls_only
        args.hip_graph = False      # until capture_all()
        args.max_seq_len = S
        self.trainer = Trainer(args, self.model, self.opt, dev)

    def capture_all(self):
        """Two passes over the pool with capture on: a key is captured at
        its second sighting, so every later step is a replay. Returns the
        bytes the graphs' memory pool holds (``empty_cache`` on both sides
        releases what the eager steps cached, never a live graph's pool)."""
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_reserved()
        self.trainer.args.hip_graph = True
        for _ in range(2):
            self.window(len(self.batches))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.memory_reserved() - base

    def step(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        return self.trainer.train_step(b)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--pool", type=int, default=40, help="distinct batches")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--mem-steps", type=int, default=200)
    ap.add_argument("--multiple", type=int, default=64)
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--data-path", default="./data/train.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_unpad.py measures GPU step time: no GPU visible")
    dev = torch.device("cuda:0")

    source, lens = lengths(a.pool * a.batch, a.seed, a.data_path)
    padded = make_batches(lens, a.batch, a.seed)
    packed = [pack_batch(b, multiple=a.multiple) for b in padded]
    toks = [int(b["cu_seqlens"][-1]) for b in packed]
    rows = [b["input_ids"].numel() for b in packed]
    print(f"lengths: {source}; mean {sum(lens) / len(lens):.1f}, median "
          f"{sorted(lens)[len(lens) // 2]}")
    print(f"batch {a.batch}: mean real tokens {sum(toks) / len(toks):.0f}, "
          f"mean packed rows (multiple {a.multiple}) "
          f"{sum(rows) / len(rows):.0f} (max {max(rows)}, "
          f"{len(set(rows))} distinct) vs {a.batch * S} padded rows")

    dev_packed = [to_device(b, dev) for b in packed]
    graph = GraphMode("unpad_graph", dev_packed, dev)
    modes = [Mode("padded", [to_device(b, dev) for b in padded], dev),
             Mode("unpad", dev_packed, dev), graph]
    for m in modes:                      # every shape of the pool, once
        m.window(len(m.batches))
    graph_pool = graph.capture_all()
    keys = {graph.trainer._graph_key(b) for b in graph.batches}
    captured = graph.trainer.graph_stats["captured"]
    print(f"unpad_graph: {captured} graphs captured for {len(keys)} batch "
          f"keys; their memory pool holds {graph_pool / 2**20:.0f} MiB")
    assert captured == len(keys), "timed windows would contain eager steps"
    eager_before = graph.trainer.graph_stats["eager"]
    times = {m.name: [] for m in modes}
    for p in range(a.pairs):
        for m in modes:
            times[m.name].append(m.window(a.steps))
        print(f"pair {p}: padded {times['padded'][-1]:.3f} ms/step, "
              f"unpad {times['unpad'][-1]:.3f} ms/step")
        print(f"pair {p}: unpad_graph {times['unpad_graph'][-1]:.3f} ms/step")
    assert graph.trainer.graph_stats["eager"] == eager_before
    rng = {k: (min(v), max(v)) for k, v in times.items()}
    disjoint = rng["unpad"][1] < rng["padded"][0]
    graph_disjoint = rng["unpad_graph"][1] < rng["unpad"][0]
    for k, (lo, hi) in rng.items():
        print(f"{k}: {lo:.3f} .. {hi:.3f} ms/step over {a.pairs} windows "
              f"of {a.steps} steps")
    print("ranges disjoint in favour of unpad:", disjoint)
    print("ranges disjoint in favour of unpad_graph over unpad:",
          graph_disjoint)

    def measure(m):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_reserved()
        m.window(a.mem_steps // 2)
        mid = torch.cuda.memory_reserved()
        m.window(a.mem_steps - a.mem_steps // 2)
        reserved[m.name] = {"start": base, "half": mid,
                            "end": torch.cuda.memory_reserved()}
        print(f"{m.name}: memory_reserved {base / 2**20:.0f} MiB at start, "
              f"{mid / 2**20:.0f} MiB after {a.mem_steps // 2} steps, "
              f"{reserved[m.name]['end'] / 2**20:.0f} MiB after "
              f"{a.mem_steps}")

    reserved = {}
    # the graph mode first (all three modes resident), then the other two
    # without it: its pool stays reserved for as long as its graphs live
    # and is no part of their figures
    measure(modes.pop())
    del graph, m
    gc.collect()
    for m in modes:
        measure(m)
    print(json.dumps({
        "metric": "bench_unpad", "source": source, "batch": a.batch,
        "multiple": a.multiple, "mean_tokens": sum(toks) / len(toks),
        "mean_rows": sum(rows) / len(rows), "ms_per_step": times,
        "range_ms": rng, "disjoint": disjoint,
        "speedup_of_medians": sorted(times["padded"])[a.pairs // 2]
        / sorted(times["unpad"])[a.pairs // 2],
        "memory_reserved": reserved,
        "graphs_captured": captured, "graph_pool_bytes": graph_pool,
        "graph_disjoint": graph_disjoint,
        "graph_speedup_of_medians": sorted(times["unpad"])[a.pairs // 2]
        / sorted(times["unpad_graph"])[a.pairs // 2]}))


if __name__ == "__main__":
    main()
