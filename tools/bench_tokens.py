#!/usr/bin/env python
"""Sentence-count batches vs token-budget batches on the padding-free path.

    python tools/bench_tokens.py [--budgets 1024,2048,4096] [--pairs 5]
                                 [--steps 30] [--hip-graph true]
                                 [--attn-tile-pack true]
                                 [--cls-only-last-layer true]

Eager bf16 BERT-base training steps (forward, backward, fused AdamW) on the
packed stream: ``--unpad true`` at batch 32 (the baseline) against
``--max-tokens N`` for every N of ``--budgets``, all on the same length
source as tools/bench_unpad.py (``data/train.json`` when present, else the
seeded lognormal stand-in, median ~15 / mean ~20, capped at 128).

Method: ``--samples`` lengths are drawn once. The baseline pool is the
first ``--pool`` batches of 32 of them; each budget's pool is what
TokenBudgetBatchSampler makes of all of them (at most ``--pool`` batches,
the short last batch left out of the timed pool). Every batch of a pool
runs once before timing. Timed windows of ``--steps`` steps alternate over
the modes, ``--pairs`` times, each closed by a device synchronise. Reported
per mode: every window, the ms/step range, real sentences per step,
samples/s (range), and ``memory_reserved`` after ``--mem-steps`` steps from
an emptied allocator cache. Ranges that overlap are reported as such.

With ``--attn-tile-pack true`` every budget also runs with tile-packed
attention (``tokensN_tp``, same batches, same windows), next to the same
build with the option off.

With ``--cls-only-last-layer true`` every budget also runs with the CLS-only
last encoder layer (``tokensN_cls``, or ``tokensN_tp_cls`` on top of
``--attn-tile-pack true``), next to the same build with that option off.

With ``--hip-graph true`` every mode also runs through the Trainer's
hipGraph cache: graphs captured, the share of an epoch's steps that
GraphPolicy replays from a cold start, and replay windows interleaved in
the same run.

Last, ``embedding`` backward (``embedding_ln_bwd``) is timed with device
events on a full 4096-row batch and on a tail batch of the same shape whose
rows are mostly pad tokens with a zero upstream gradient.
"""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_unpad import (GraphMode, Mode, S, VOCAB, lengths,  # noqa: E402
                         to_device)
from pdnlp_amd.data import (SEQ_MULTIPLE, TokenBudgetBatchSampler,  # noqa: E402
                            pack_batch)
from pdnlp_amd.engine.trainer import GraphPolicy, graph_key  # noqa: E402


def padded_samples(lens, seed):
    """One padded row per sample (ids [n, S], mask, types, labels)."""
    g = torch.Generator().manual_seed(seed + 1)
    n = len(lens)
    ll = torch.tensor(lens)
    mask = (torch.arange(S)[None, :] < ll[:, None]).long()
    ids = torch.randint(106, VOCAB, (n, S), generator=g)
    ids[:, 0] = 101
    ids[torch.arange(n), ll - 1] = 102
    return {"input_ids": ids * mask, "attention_mask": mask,
            "token_type_ids": torch.zeros_like(ids),
            "label": torch.randint(0, 6, (n,), generator=g)}


def take(samples, idx):
    idx = torch.tensor(idx)
    return {k: v[idx] for k, v in samples.items()}


def replay_share(batches):
    """Share of one epoch's steps that GraphPolicy replays from a cold
    start, and the number of graphs it captures (host-side rule only)."""
    pol = GraphPolicy()
    replays = sum(pol.decide(graph_key(b, S)) != "eager" for b in batches)
    return replays / len(batches), len(pol.captured)


def embedding_backward_us(dev, rows, real, iters=50):
    """Device-event time of one embedding_ln_bwd on [rows] tokens of which
    the first ``real`` are real; the rest are pad id 0 / position 0 with a
    zero upstream gradient, as in the tail of a budgeted batch."""
    from pdnlp_amd.ops import ext
    e = ext()
    H = 768
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(106, VOCAB, (1, rows), generator=g)
    pos = (torch.arange(rows) % 20)[None, :].clone()
    ids[0, real:] = 0
    pos[0, real:] = 0
    ids, pos = ids.to(dev), pos.to(dev)
    types = torch.zeros_like(ids)
    bf = dict(device=dev, dtype=torch.bfloat16)
    word = torch.randn(VOCAB, H, **bf) * 0.02
    posw = torch.randn(512, H, **bf) * 0.02
    typew = torch.randn(2, H, **bf) * 0.02
    lnw, lnb = torch.ones(H, **bf), torch.zeros(H, **bf)
    y, mean, rstd = e.embedding_ln_fwd(ids, types, pos, word, posw, typew,
                                       lnw, lnb, 1e-12)
    dy = torch.randn_like(y)
    dy[0, real:] = 0
    for _ in range(5):
        e.embedding_ln_bwd(dy, ids, types, pos, word, posw, typew, lnw, mean,
                           rstd)
    t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        e.embedding_ln_bwd(dy, ids, types, pos, word, posw, typew, lnw, mean,
                           rstd)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budgets", default="1024,2048,4096")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=9200)
    ap.add_argument("--pool", type=int, default=40, help="batches per mode")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--mem-steps", type=int, default=200)
    ap.add_argument("--hip-graph", default="false")
    ap.add_argument("--attn-tile-pack", default="false")
    ap.add_argument("--cls-only-last-layer", default="false")
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--data-path", default="./data/train.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tokens.py measures GPU step time: no GPU visible")
    dev = torch.device("cuda:0")
    use_graph = a.hip_graph.lower() in ("1", "true", "yes")
    tile_pack = a.attn_tile_pack.lower() in ("1", "true", "yes")
    cls_only = a.cls_only_last_layer.lower() in ("1", "true", "yes")
    budgets = [int(x) for x in a.budgets.split(",")]
    print(f"device: {torch.cuda.get_device_name(0)}")

    source, lens = lengths(a.samples, a.seed, a.data_path)
    samples = padded_samples(lens, a.seed)
    print(f"lengths: {source}; {len(lens)} samples, mean "
          f"{sum(lens) / len(lens):.1f}, median {sorted(lens)[len(lens) // 2]}")

    # name -> (every batch of one epoch, on the host)
    epochs = {f"unpad{a.batch}": [
        pack_batch(take(samples, list(range(i, min(i + a.batch, len(lens))))))
        for i in range(0, len(lens), a.batch)]}
    for n in budgets:
        sampler = TokenBudgetBatchSampler(lens, n, seed=a.seed)
        epochs[f"tokens{n}"] = [
            pack_batch(take(samples, b), total_rows=n,
                       seq_multiple=SEQ_MULTIPLE) for b in sampler.batches]
    info = {}
    for name, ep in epochs.items():
        share, graphs = replay_share(ep)
        timed = ep[:-1][:a.pool]          # without the short last batch
        seqs = [b["num_seqs"] for b in timed]
        info[name] = {
            "steps_per_epoch": len(ep), "pool": len(timed),
            "sentences_per_step": sum(seqs) / len(seqs),
            "sentences_min_max": [min(seqs), max(seqs)],
            "mean_fill": sum(int(b["cu_seqlens"][-1]) for b in timed)
            / sum(b["input_ids"].numel() for b in timed),
            "graph_keys_per_epoch": len({graph_key(b, S) for b in ep}),
            "policy_graphs_per_epoch": graphs,
            "policy_replay_share_first_epoch": share}
        print(f"{name}: {len(ep)} steps/epoch, {info[name]['sentences_per_step']:.1f} "
              f"sentences/step ({min(seqs)}..{max(seqs)}), rows "
              f"{info[name]['mean_fill'] * 100:.1f} % real, "
              f"{info[name]['graph_keys_per_epoch']} graph keys/epoch; "
              f"GraphPolicy from cold: {graphs} graphs, "
              f"{share * 100:.1f} % of the first epoch's steps replayed")
        epochs[name] = [to_device(b, dev) for b in timed]

    # (mode name, pool name, tile-packed attention, CLS-only last layer)
    runs = [(name, name, False, False) for name in epochs]
    if tile_pack:
        runs += [(name + "_tp", name, True, False) for name in epochs
                 if name.startswith("tokens")]
    if cls_only:   # on top of the tile-packed mode when that is on
        tp_tag = "_tp" if tile_pack else ""
        runs += [(name + tp_tag + "_cls", name, tile_pack, True)
                 for name in epochs if name.startswith("tokens")]
    modes = [Mode(name, epochs[ep], dev, tp, co) for name, ep, tp, co in runs]
    graph_modes = []
    if use_graph:
        graph_modes = [GraphMode(name + "_graph", epochs[ep], dev, tp, co)
                       for name, ep, tp, co in runs]
    for m in modes + graph_modes:            # every batch of the pool, once
        m.window(len(m.batches))
    for m in graph_modes:
        pool = m.capture_all()
        st = m.trainer.graph_stats
        info[m.name] = {"graphs_captured": st["captured"],
                        "graph_pool_bytes": pool}
        print(f"{m.name}: {st['captured']} graphs captured, pool "
              f"{pool / 2**20:.0f} MiB")
        m.eager_before = st["eager"]

    times = {m.name: [] for m in modes + graph_modes}
    for p in range(a.pairs):
        for m in modes + graph_modes:
            times[m.name].append(m.window(a.steps))
        print(f"pair {p}: " + ", ".join(
            f"{k} {v[-1]:.3f}" for k, v in times.items()) + " ms/step")
    for m in graph_modes:
        st = m.trainer.graph_stats
        timed = a.pairs * a.steps
        info[m.name]["timed_replay_share"] = \
            1.0 - (st["eager"] - m.eager_before) / timed

    result = {}
    for name, v in times.items():
        base = name.replace("_graph", "").replace("_tp", "") \
            .replace("_cls", "")
        sps = info[base]["sentences_per_step"]
        result[name] = {
            "ms_per_step": v, "range_ms": [min(v), max(v)],
            "samples_per_s_range": [sps / max(v) * 1e3, sps / min(v) * 1e3]}
        print(f"{name}: {min(v):.3f} .. {max(v):.3f} ms/step over {a.pairs} "
              f"windows of {a.steps} steps; {sps:.1f} sentences/step; "
              f"{sps / max(v) * 1e3:.0f} .. {sps / min(v) * 1e3:.0f} samples/s")
    base = result[f"unpad{a.batch}"]["samples_per_s_range"]
    for name, r in result.items():
        lo, hi = r["samples_per_s_range"]
        r["vs_baseline"] = ("above" if lo > base[1] else
                            "below" if hi < base[0] else "overlapping")
        print(f"{name} samples/s against unpad{a.batch}: {r['vs_baseline']}")
    for name, r in result.items():   # option on against off, same batches
        if "_tp" in name and "_cls" not in name:
            lo, hi = r["range_ms"]
            off = result[name.replace("_tp", "")]["range_ms"]
            r["vs_option_off"] = ("faster" if hi < off[0] else
                                  "slower" if lo > off[1] else "overlapping")
            print(f"{name} ms/step {lo:.3f} .. {hi:.3f} against option off "
                  f"{off[0]:.3f} .. {off[1]:.3f}: {r['vs_option_off']}")

    for name, r in result.items():   # CLS-only last layer on against off
        if "_cls" in name:
            lo, hi = r["range_ms"]
            off = result[name.replace("_cls", "")]["range_ms"]
            r["vs_cls_only_off"] = ("faster" if hi < off[0] else
                                    "slower" if lo > off[1] else
                                    "overlapping")
            print(f"{name} ms/step {lo:.3f} .. {hi:.3f} against "
                  f"cls-only off {off[0]:.3f} .. {off[1]:.3f}: "
                  f"{r['vs_cls_only_off']}")

    # memory: one mode resident at a time would need a rebuild; report the
    # growth of memory_reserved over mem-steps from an emptied cache instead
    del graph_modes
    gc.collect()
    for m in modes:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        start = torch.cuda.memory_reserved()
        m.window(a.mem_steps // 2)
        half = torch.cuda.memory_reserved()
        m.window(a.mem_steps - a.mem_steps // 2)
        end = torch.cuda.memory_reserved()
        result[m.name]["memory_reserved"] = {"start": start, "half": half,
                                             "end": end}
        print(f"{m.name}: memory_reserved {start / 2**20:.0f} MiB at start, "
              f"{half / 2**20:.0f} MiB after {a.mem_steps // 2} steps, "
              f"{end / 2**20:.0f} MiB after {a.mem_steps}")
    del modes, m
    gc.collect()
    torch.cuda.empty_cache()

    rows = max(budgets)
    emb = {"full": embedding_backward_us(dev, rows, rows),
           "tail": embedding_backward_us(dev, rows, 300)}
    print(f"embedding_ln_bwd at {rows} rows: {emb['full']:.1f} us on a full "
          f"batch, {emb['tail']:.1f} us with 300 real rows and "
          f"{rows - 300} pad rows of zero gradient")

    print(json.dumps({"metric": "bench_tokens", "source": source,
                      "device": torch.cuda.get_device_name(0),
                      "pairs": a.pairs, "steps": a.steps, "info": info,
                      "result": result, "embedding_bwd_us": emb}))


if __name__ == "__main__":
    main()
