#!/usr/bin/env python
"""Serving latency/throughput across batch sizes (hipGraph engine).

    python tools/serve_bench.py            # padded engine at seq 128
    python tools/serve_bench.py --packed   # padded vs padding-free serving
    python tools/serve_bench.py --packed --cls-only-last-layer

``--packed`` serves the same requests with three engines: the graphed padded
engine (the baseline: every text of a request padded to the power-of-two
bucket of the longest), the packed engine on the training kernels
(``infer_kernels=False``) and the packed engine on the forward-only kernels.
``--cls-only-last-layer`` adds a fourth, ``packed_cls``: the packed engine
whose last encoder layer computes the first-token rows only, reported next
to ``packed`` (at request size 1 the two run the same code: the fallback
rule).
Text lengths come from tools/bench_unpad.py's seeded stand-in (real lengths
when ./data/train.json exists, else lognormal, mean ~20, cap 128); token ids
are random. For request sizes 1, 8 and 64 every engine first serves all
requests once (which captures its graphs), then the engines alternate for
``--windows`` windows over the same requests in one process. A request's
latency runs from its token lists on the host to its logits on the device,
synchronised. Reported per engine: p50, p99 and sequences/s as ranges over
the windows. A last part runs one offline pass of ``--offline`` texts
through ``predict_logits`` (tokenizer included) per engine and window.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pdnlp_amd.engine import InferenceEngine  # noqa: E402
from pdnlp_amd.models import build_model  # noqa: E402
from pdnlp_amd.utils import set_seed  # noqa: E402

S = 128


def padded_only():
    set_seed(5)
    model = build_model("bert-base").to(torch.bfloat16)
    eng = InferenceEngine(model, device="cuda", use_graph=True)
    for b in (1, 8, 64):
        st = eng.latency_bench(batch=b, seq=128, iters=50, warmup=15)
        p50, p99 = st["p50_ms"], st["p99_ms"]
        print(f"serve b{b:<3d}: p50 {p50:6.3f} ms  p99 {p99:6.3f} ms  "
              f"-> {b / p50 * 1000:8.0f} seq/s")


def _requests(lens, size, count, seed):
    g = torch.Generator().manual_seed(seed)
    reqs = []
    for r in range(count):
        ll = lens[r * size:(r + 1) * size]
        reqs.append([([101] + torch.randint(106, 21128, (n - 2,),
                                            generator=g).tolist() + [102]
                      if n > 2 else [101] * n, [0] * n) for n in ll])
    return reqs


def _serve_padded(eng, req):
    """what InferenceEngine._encode + forward_tensors do with a request"""
    from pdnlp_amd.engine.infer import _bucket
    seq = _bucket(max(len(i) for i, _ in req), hi=S)
    ids = torch.tensor([i + [0] * (seq - len(i)) for i, _ in req])
    mask = torch.tensor([[1] * len(i) + [0] * (seq - len(i)) for i, _ in req])
    types = torch.zeros_like(ids)
    return eng.forward_tensors(ids, mask, types, clone=False)


def _window(serve, reqs):
    lat = []
    for req in reqs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        serve(req)
        torch.cuda.synchronize()
        lat.append((time.perf_counter() - t0) * 1e3)
    total = sum(lat)
    lat.sort()
    return (lat[len(lat) // 2], lat[max(int(len(lat) * 0.99) - 1, 0)],
            sum(len(r) for r in reqs) / total * 1e3)


def _rng(v, fmt):
    return f"{min(v):{fmt}} .. {max(v):{fmt}}"


def packed(a):
    from bench_unpad import lengths
    set_seed(5)
    model = build_model("bert-base").to(torch.bfloat16)
    from pdnlp_amd.data import build_tokenizer
    tok = build_tokenizer(None)
    kw = dict(device="cuda", max_seq_len=S, use_graph=True)
    engines = {
        "padded": InferenceEngine(model, tok, **kw),
        "packed_train_kernels": InferenceEngine(
            model, tok, packed=True, infer_kernels=False, **kw),
        "packed": InferenceEngine(model, tok, packed=True, **kw),
    }
    if a.cls_only_last_layer:
        engines["packed_cls"] = InferenceEngine(
            model, tok, packed=True, cls_only_last_layer=True, **kw)
    serve = {k: ((lambda r, e=e: _serve_padded(e, r)) if k == "padded"
                 else e.forward_sequences) for k, e in engines.items()}
    source, lens = lengths(max(a.offline, 64 * a.requests), 123,
                           "./data/train.json")
    print(f"{source}: mean {sum(lens) / len(lens):.1f} tokens")
    out = []
    for size in (1, 8, 64):
        reqs = _requests(lens, size, a.requests, size)
        for fn in serve.values():                 # captures the graphs
            _window(fn, reqs)
        res = {k: [] for k in serve}
        for _ in range(a.windows):
            for k, fn in serve.items():
                res[k].append(_window(fn, reqs))
        for k, v in res.items():
            p50, p99, sps = zip(*v)
            print(f"request size {size:2d} {k:21s}: p50 {_rng(p50, '6.3f')} "
                  f"ms  p99 {_rng(p99, '6.3f')} ms  {_rng(sps, '7.0f')} "
                  f"seq/s", flush=True)
            out.append({"request_size": size, "engine": k,
                        "p50_ms": [round(x, 3) for x in p50],
                        "p99_ms": [round(x, 3) for x in p99],
                        "seq_per_s": [round(x) for x in sps]})
        base = [w[0] for w in res["padded"]]
        for k in ("packed_train_kernels", "packed"):
            mine = [w[0] for w in res[k]]
            print(f"  p50 of {k} against padded: disjointly lower "
                  f"{max(mine) < min(base)}, disjointly higher "
                  f"{min(mine) > max(base)}")
        if "packed_cls" in res:
            base = [w[0] for w in res["packed"]]
            mine = [w[0] for w in res["packed_cls"]]
            print(f"  p50 of packed_cls against packed: disjointly lower "
                  f"{max(mine) < min(base)}, disjointly higher "
                  f"{min(mine) > max(base)}")
    # offline: texts of the stand-in lengths through the tokenizer
    g = torch.Generator().manual_seed(9)
    texts = ["".join(chr(0x4e00 + c) for c in
                     torch.randint(0, 3000, (max(n - 2, 1),),
                                   generator=g).tolist())
             for n in lens[:a.offline]]
    for e in engines.values():
        e.predict_logits(texts)
    off = {k: [] for k in engines}
    for _ in range(a.windows):
        for k, e in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.predict_logits(texts)
            off[k].append(len(texts) / (time.perf_counter() - t0))
    for k, v in off.items():
        print(f"offline {len(texts)} texts {k:21s}: {_rng(v, '7.0f')} seq/s")
        out.append({"offline_texts": len(texts), "engine": k,
                    "seq_per_s": [round(x) for x in v]})
    print({k: e.graph_stats for k, e in engines.items() if e.packed})
    print(json.dumps({"metric": "serve_bench_packed", "results": out}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--cls-only-last-layer", action="store_true",
                    help="with --packed: also the packed engine with the "
                         "CLS-only last encoder layer")
    ap.add_argument("--requests", type=int, default=60,
                    help="requests per size and window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--offline", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("serve_bench.py measures GPU serving: no GPU visible")
    packed(args) if args.packed else padded_only()
