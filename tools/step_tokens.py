#!/usr/bin/env python
"""A fixed number of eager token-budget training steps, for profilers.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/step_tokens.py --max-tokens 4096 --steps 25 \\
        [--attn-tile-pack true] [--cls-only-last-layer true]
    python tools/step_tokens.py --summarize DIR --steps 25 --title "..."

bf16 BERT-base with fused AdamW on the ``--max-tokens`` batches of
tools/bench_tokens.py (seeded lognormal stand-in unless ``data/train.json``
exists), cycling over the first ``--pool`` batches. Every step is profiled,
the first ones included. ``--summarize`` turns the profiler's
``*kernel_stats.csv`` under DIR into the per-step table kept in profiles/.
"""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def summarize(directory, steps, title):
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"),
                             recursive=True))
    if not paths:
        sys.exit(f"no *kernel_stats.csv under {directory}")
    rows = []
    with open(paths[0], newline="") as f:
        for r in csv.DictReader(f):
            rows.append((r["Name"], int(r["Calls"]),
                         float(r["TotalDurationNs"])))
    total = sum(r[2] for r in rows)
    calls = sum(r[1] for r in rows)
    print(title)
    print(f"{steps} steps profiled; TOTAL {total / 1e6:.1f} ms -> "
          f"{total / 1e6 / steps:.3f} ms/step GPU kernel time; "
          f"{calls / steps:.1f} launches/step")
    print(f"{'kernel':<90} calls/st  us/step      %")
    for name, n, ns in sorted(rows, key=lambda r: -r[2]):
        print(f"{name[:88]:<90} {n / steps:>8.1f} {ns / 1e3 / steps:>8.1f} "
              f"{100 * ns / total:>6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--pool", type=int, default=10)
    ap.add_argument("--attn-tile-pack", default="false")
    ap.add_argument("--cls-only-last-layer", default="false")
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--data-path", default="./data/train.json")
    ap.add_argument("--summarize", metavar="DIR", default=None)
    ap.add_argument("--title", default="")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.steps, a.title)

    import torch
    from bench_tokens import padded_samples, take
    from bench_unpad import Mode, lengths, to_device
    from pdnlp_amd.data import (SEQ_MULTIPLE, TokenBudgetBatchSampler,
                                pack_batch)
    if not torch.cuda.is_available():
        sys.exit("step_tokens.py runs GPU steps: no GPU visible")
    dev = torch.device("cuda:0")
    tile_pack = a.attn_tile_pack.lower() in ("1", "true", "yes")
    cls_only = a.cls_only_last_layer.lower() in ("1", "true", "yes")
    source, lens = lengths(9200, a.seed, a.data_path)
    samples = padded_samples(lens, a.seed)
    sampler = TokenBudgetBatchSampler(lens, a.max_tokens, seed=a.seed)
    pool = [to_device(pack_batch(take(samples, b), total_rows=a.max_tokens,
                                 seq_multiple=SEQ_MULTIPLE), dev)
            for b in sampler.batches[:-1][:a.pool]]
    mode = Mode("tokens", pool, dev, tile_pack, cls_only)
    ms = mode.window(a.steps)
    print(f"{source}; --max-tokens {a.max_tokens}, attn_tile_pack "
          f"{tile_pack}, cls_only_last_layer {cls_only}: {a.steps} steps, {ms:.3f} ms/step wall")


if __name__ == "__main__":
    main()
