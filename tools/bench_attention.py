"""Attention kernel timings.

    python tools/bench_attention.py            # padded kernels, wall clock
    python tools/bench_attention.py --packed   # per-sequence vs tile-packed
    python tools/bench_attention.py --bwd      # fused vs two-kernel backward

``--packed`` times the per-sequence (VARLEN) and the tile-packed kernels,
forward and backward, on one stand-in token-budget batch of ``--rows``
packed rows (tools/bench_unpad.py's seeded lognormal lengths, batched by
TokenBudgetBatchSampler), BERT-base heads, bf16, random data. Device events
around ``--iters`` launches; the modes alternate for ``--rounds`` rounds in
one process and the per-round means are reported with their range. The plan
kernel (once per model forward, not per layer) is timed on its own. The
serving pair rides along: the tile-packed forward at p = 0 (zero-fill launch,
kernel, lse) next to ``flash_attn_tilepack_infer``, which replaces it under
``ops.inference_kernels()``. The one-query-row-per-sequence kernels of the
CLS-only last layer (``cls_attn_fwd`` / ``cls_attn_bwd`` / ``cls_attn_infer``,
``ceil64(slots)`` output rows) are timed on the same batch.

``--bwd`` times the padded backward at (32, 12, 128) and (32, 12, 64), bf16,
p = 0.1, with an additive mask: the fused kernel (one launch) against the
two-kernel path that ``PDNLP_FA_BWD_SPLIT`` keeps, the switch set around the
timed launches, both alternating in one process, device events around
``--iters`` launches, per-round means with their range over ``--rounds``.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pdnlp_amd.ops import ext  # noqa: E402

dev = "cuda:0"


def padded():
    e = ext()
    torch.manual_seed(0)
    for (B, nh, S) in [(16, 16, 512), (32, 12, 128)]:
        H = nh * 64
        qkv = (torch.randn(B, S, 3*H, device=dev) / 28).bfloat16()
        mask = torch.zeros(B, 1, 1, S, device=dev, dtype=torch.bfloat16).reshape(B, S).contiguous()
        o, lse = e.flash_attn_qkv_fwd(qkv, mask, nh, 0.125, 0.0, torch.Tensor(), 0)
        do = torch.randn_like(o)
        def t_fwd():
            return e.flash_attn_qkv_fwd(qkv, mask, nh, 0.125, 0.0, torch.Tensor(), 0)
        def t_bwd():
            return e.flash_attn_qkv_bwd(do, qkv, o, lse, mask, nh, 0.125, 0.0, torch.Tensor(), 0)
        for name, fn in (("fwd", t_fwd), ("bwd", t_bwd)):
            for _ in range(5): fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(30): fn()
            torch.cuda.synchronize()
            us = (time.perf_counter()-t0)/30*1e6
            print(f"B{B} nh{nh} S{S} {name}: {us:.0f} us")


def event_us(fn, iters):
    t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


SPLIT_SWITCH = "PDNLP_FA_BWD_SPLIT"


def bwd(a):
    e = ext()
    torch.manual_seed(0)
    p, sc = 0.1, 0.125
    seed = torch.tensor([1234], dtype=torch.int64, device=dev)
    shapes = {}
    for (B, nh, S) in [(32, 12, 128), (32, 12, 64)]:
        H = nh * 64
        qkv = torch.randn(B, S, 3 * H, device=dev).bfloat16()
        do = torch.randn(B, S, H, device=dev).bfloat16()
        # padded tails of 0 .. S/2 keys, as a collated batch has them
        tails = torch.randint(0, S // 2 + 1, (B, 1), device=dev)
        mask = ((torch.arange(S, device=dev)[None] >= S - tails)
                .to(torch.bfloat16) * -10000.0).contiguous()
        o, lse = e.flash_attn_qkv_fwd(qkv, mask, nh, sc, p, seed, 1)

        def call():
            return e.flash_attn_qkv_bwd(do, qkv, o, lse, mask, nh, sc, p,
                                        seed, 1)

        def timed(split, iters):
            assert SPLIT_SWITCH not in os.environ
            if split:
                os.environ[SPLIT_SWITCH] = "1"
            try:
                return event_us(call, iters)
            finally:
                os.environ.pop(SPLIT_SWITCH, None)

        for split in (False, True):
            timed(split, 10)
        us = {"fused": [], "split": []}
        for _ in range(a.rounds):
            us["fused"].append(timed(False, a.iters))
            us["split"].append(timed(True, a.iters))
        f, s2 = us["fused"], us["split"]
        print(f"B{B} nh{nh} S{S} bwd: fused {min(f):.1f} .. {max(f):.1f} us, "
              f"split {min(s2):.1f} .. {max(s2):.1f} us over {a.rounds} "
              f"rounds of {a.iters} launches (each with its output "
              f"allocation); ranges disjoint in favour of fused: "
              f"{max(f) < min(s2)}; of split: {max(s2) < min(f)}")
        shapes[f"{B}x{nh}x{S}"] = us
    print(json.dumps({"metric": "bench_attention_bwd_fused", "dropout": p,
                      "dtype": "bf16", "us": shapes}))


def packed(a):
    from bench_unpad import lengths
    from pdnlp_amd.data import SEQ_MULTIPLE, TokenBudgetBatchSampler
    from pdnlp_amd.ops import tile_plan_max_items, tile_plan_reference
    e = ext()
    nh, T, p = 12, a.rows, a.dropout
    H = nh * 64
    source, lens = lengths(9200, 123, "./data/train.json")
    batch = TokenBudgetBatchSampler(lens, T, seed=7).batches[a.batch_index]
    bl = [lens[i] for i in batch]
    nseq = (len(bl) + SEQ_MULTIPLE - 1) // SEQ_MULTIPLE * SEQ_MULTIPLE
    cu = [0]
    for n in bl + [0] * (nseq - len(bl)):   # empty sequences, as the collate
        cu.append(cu[-1] + n)
    items, _ = tile_plan_reference(cu, T)
    live = sum((n + 63) // 64 for n in bl)
    grid_ps = (max(bl) + 63) // 64 * nseq
    print(f"{source}: {len(bl)} sentences ({nseq} slots), {cu[-1]} of {T} "
          f"rows real, longest {max(bl)}")
    print(f"per head: per-sequence grid {grid_ps} blocks, {live} live; "
          f"tile-packed grid {tile_plan_max_items(T, nseq)} blocks, "
          f"{len(items)} live")
    torch.manual_seed(0)
    qkv = torch.randn(T, 3 * H, device=dev).bfloat16()
    do = torch.randn(T, H, device=dev).bfloat16()
    cu_t = torch.tensor(cu, dtype=torch.int32, device=dev)
    seed = torch.tensor([1234], dtype=torch.int64, device=dev) if p \
        else torch.Tensor()
    mx, sc = 128, 0.125
    plan = e.flash_attn_tilepack_plan(cu_t, T)
    assert plan[0].item() == len(items)
    o_ps, lse_ps = e.flash_attn_varlen_fwd(qkv, cu_t, mx, nh, sc, p, seed, 1)
    o_tp, lse_tp = e.flash_attn_tilepack_fwd(qkv, plan, mx, nh, sc, p, seed, 1)
    rows_out = (nseq + 63) // 64 * 64
    do_cls = torch.randn(rows_out, H, device=dev).bfloat16()
    o_cls, lse_cls = e.cls_attn_fwd(qkv, cu_t, rows_out, mx, nh, sc, p, seed,
                                    1)
    fns = {
        "per_sequence_fwd": lambda: e.flash_attn_varlen_fwd(
            qkv, cu_t, mx, nh, sc, p, seed, 1),
        "tile_packed_fwd": lambda: e.flash_attn_tilepack_fwd(
            qkv, plan, mx, nh, sc, p, seed, 1),
        "per_sequence_bwd": lambda: e.flash_attn_varlen_bwd(
            do, qkv, o_ps, lse_ps, cu_t, mx, nh, sc, p, seed, 1),
        "tile_packed_bwd": lambda: e.flash_attn_tilepack_bwd(
            do, qkv, o_tp, lse_tp, plan, mx, nh, sc, p, seed, 1),
        "plan": lambda: e.flash_attn_tilepack_plan(cu_t, T),
        "tile_packed_fwd_p0": lambda: e.flash_attn_tilepack_fwd(
            qkv, plan, mx, nh, sc, 0.0, torch.Tensor(), 0),
        "tile_packed_infer": lambda: e.flash_attn_tilepack_infer(
            qkv, plan, mx, nh, sc),
        "cls_fwd": lambda: e.cls_attn_fwd(
            qkv, cu_t, rows_out, mx, nh, sc, p, seed, 1),
        "cls_bwd": lambda: e.cls_attn_bwd(
            do_cls, qkv, o_cls, lse_cls, cu_t, mx, nh, sc, p, seed, 1),
        "cls_infer": lambda: e.cls_attn_infer(
            qkv, cu_t, rows_out, mx, nh, sc),
    }
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            us[k].append(event_us(fn, a.iters))
    for k, v in us.items():
        print(f"{k}: {min(v):.1f} .. {max(v):.1f} us over {a.rounds} rounds "
              f"of {a.iters} launches (each with its output allocation)")
    for d in ("fwd", "bwd"):
        ps, tp = us[f"per_sequence_{d}"], us[f"tile_packed_{d}"]
        print(f"{d}: ranges disjoint in favour of tile-packed: "
              f"{max(tp) < min(ps)}; of per-sequence: {max(ps) < min(tp)}")
    f0, inf = us["tile_packed_fwd_p0"], us["tile_packed_infer"]
    print(f"serving fwd: ranges disjoint in favour of infer: "
          f"{max(inf) < min(f0)}; of the training forward: "
          f"{max(f0) < min(inf)}")
    for d in ("fwd", "bwd"):
        tp, cl = us[f"tile_packed_{d}"], us[f"cls_{d}"]
        print(f"{d}: {rows_out} first-token rows (cls) against all {T} rows "
              f"(tile-packed): ranges disjoint in favour of cls: "
              f"{max(cl) < min(tp)}")
    print(json.dumps({"metric": "bench_attention_packed", "rows": T,
                      "dropout": p, "sentences": len(bl),
                      "live_blocks_per_head": {"per_sequence": live,
                                               "tile_packed": len(items)},
                      "us": us}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--bwd", action="store_true")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--batch-index", type=int, default=0)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attention.py measures GPU kernels: no GPU visible")
    if args.bwd:
        bwd(args)
    elif args.packed:
        packed(args)
    else:
        padded()
