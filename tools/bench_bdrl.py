#!/usr/bin/env python
"""Per-call time of the fused bias + dropout + residual + LayerNorm epilogue.

    python tools/bench_bdrl.py [--rounds 5] [--calls 48] [--shape R H ...]
    python tools/bench_bdrl.py --infer     # serving: forward at p = 0 next
                                           # to bias_dropout_residual_ln_infer

Forward (``bias_dropout_residual_ln_fwd``) and backward
(``bias_dropout_residual_ln_bwd_nodb``, the variant the flagship step runs)
at ``[4096, 768]`` and ``[8192, 1024]``, bf16, p = 0.1, for the one-pass
kernels and for the loop kernels that ``PDNLP_BDRL_2PASS=1`` keeps.
``--shape R H`` (repeatable) times other shapes instead, e.g. an R past
32 rows per CU, where the forward's waves walk rows.

Method: a call is ~10 us, less than its host-side launch, so ``--calls``
calls are captured into one hipGraph per (path, direction) and the replay is
timed with device events, as the training step runs them. The calls of a
graph rotate over four sets of inputs (113 MB at the small shape), so the
8 x 4 MiB of L2 do not hold a call's inputs from the call before; the
256 MiB Infinity Cache may. After a warm-up replay of every graph the two
paths alternate for ``--rounds`` rounds in the one process. Reported: every
round's us/call, the median, and the median as TB/s of unique bytes, those
computed from the shapes (each tensor a call reads or writes counted once;
bias, LayerNorm vectors, row statistics and partial sums left out).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdnlp_amd import ops  # noqa: E402

DEV = "cuda:0"
P, EPS, SALT = 0.1, 1e-12, 7
SETS = 4
SHAPES = [(4096, 768), (8192, 1024)]


def unique_bytes(R, H):
    t, m = R * H * 2, R * H  # one bf16 tensor, the u8 mask
    return {"fwd": 4 * t + m,   # y, res in; xsum, out, mask out
            "bwd": 4 * t + m}   # dout, xsum, mask in; dy, dres out


class _env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            del os.environ[k]


def build_graphs(e, R, H, env, calls):
    """{direction: graph} for one path; the switch is read per call, so it is
    set while the graph is captured"""
    g = torch.Generator(device=DEV).manual_seed(R + H)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).to(torch.bfloat16)
    bias, lnw, lnb = rnd(H), rnd(H), rnd(H)
    seed = torch.tensor([11], dtype=torch.int64, device=DEV)
    sets = [(rnd(R, H), rnd(R, H), rnd(R, H)) for _ in range(SETS)]
    with _env(env):
        saved = [e.bias_dropout_residual_ln_fwd(y, bias, res, lnw, lnb, P, EPS,
                                                seed, SALT)
                 for y, res, _ in sets]
        e.bias_dropout_residual_ln_bwd_nodb(sets[0][2], *saved[0][1:3], lnw,
                                            *saved[0][3:], P)
        torch.cuda.synchronize()
        graphs = {}
        keep = []
        for name in ("fwd", "bwd"):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for i in range(calls):
                    y, res, dout = sets[i % SETS]
                    if name == "fwd":
                        keep.append(e.bias_dropout_residual_ln_fwd(
                            y, bias, res, lnw, lnb, P, EPS, seed, SALT))
                    else:
                        _, xsum, mask, mean, rstd = saved[i % SETS]
                        keep.append(e.bias_dropout_residual_ln_bwd_nodb(
                            dout, xsum, mask, lnw, mean, rstd, P))
            graphs[name] = graph
    return graphs, keep


def build_infer_graphs(e, R, H, calls):
    """{"fwd_p0", "infer"}: the training forward at p = 0 and the forward-only
    op that replaces it under ``ops.inference_kernels()``, same inputs"""
    g = torch.Generator(device=DEV).manual_seed(R + H)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).to(torch.bfloat16)
    bias, lnw, lnb = rnd(H), rnd(H), rnd(H)
    sets = [(rnd(R, H), rnd(R, H)) for _ in range(SETS)]
    calls_of = {
        "fwd_p0": lambda y, res: e.bias_dropout_residual_ln_fwd(
            y, bias, res, lnw, lnb, 0.0, EPS, torch.Tensor(), 0),
        "infer": lambda y, res: e.bias_dropout_residual_ln_infer(
            y, bias, res, lnw, lnb, EPS),
    }
    for fn in calls_of.values():
        fn(*sets[0])
    torch.cuda.synchronize()
    graphs, keep = {}, []
    for name, fn in calls_of.items():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(calls):
                keep.append(fn(*sets[i % SETS]))
        graphs[name] = graph
    return graphs, keep


def bench_infer(rounds, calls, shapes):
    e = ops.ext()
    assert e is not None, "the HIP extension is not built"
    lines = []
    for R, H in shapes:
        graphs, keep = build_infer_graphs(e, R, H, calls)
        for graph in graphs.values():             # warm-up
            time_graph(graph, calls)
        us = {name: [] for name in graphs}
        for _ in range(rounds):
            for name, graph in graphs.items():
                us[name].append(time_graph(graph, calls))
        t = R * H * 2
        nbytes = {"fwd_p0": 4 * t, "infer": 3 * t}   # y, res in; (xsum,) out
        for name, v in us.items():
            med = statistics.median(v)
            lines.append({"shape": [R, H], "path": name,
                          "us_per_call": [round(u, 2) for u in v],
                          "median_us": round(med, 2),
                          "unique_MB": round(nbytes[name] / 1e6, 1)})
            print(f"[{R}, {H}] {name:7s}: {min(v):6.2f} .. {max(v):6.2f} "
                  f"us/call, median {med:6.2f}, "
                  f"{nbytes[name] / 1e6:.1f} MB unique", flush=True)
        print(f"[{R}, {H}] ranges disjoint in favour of infer: "
              f"{max(us['infer']) < min(us['fwd_p0'])}; of the training "
              f"forward: {max(us['fwd_p0']) < min(us['infer'])}")
        del graphs, keep
        torch.cuda.empty_cache()
    print(json.dumps(lines))
    return lines


def time_graph(graph, calls):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    graph.replay()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


def bench(paths, rounds, calls, shapes=SHAPES):
    """paths: {label: env dict}; returns {shape: {label: {dir: [us]}}}"""
    e = ops.ext()
    assert e is not None, "the HIP extension is not built"
    out = {}
    for R, H in shapes:
        built = {label: build_graphs(e, R, H, env, calls)
                 for label, env in paths.items()}
        for graphs, _ in built.values():          # warm-up
            for graph in graphs.values():
                time_graph(graph, calls)
        res = {label: {"fwd": [], "bwd": []} for label in paths}
        for _ in range(rounds):
            for label, (graphs, _) in built.items():
                for name, graph in graphs.items():
                    res[label][name].append(time_graph(graph, calls))
        out[(R, H)] = res
        del built
        torch.cuda.empty_cache()
    return out


def report(out):
    lines = []
    for (R, H), res in out.items():
        nbytes = unique_bytes(R, H)
        for label, dirs in res.items():
            for name, us in dirs.items():
                med = statistics.median(us)
                rec = {"shape": [R, H], "path": label, "dir": name,
                       "us_per_call": [round(u, 2) for u in us],
                       "median_us": round(med, 2),
                       "unique_MB": round(nbytes[name] / 1e6, 1),
                       "TBps": round(nbytes[name] / med / 1e6, 2)}
                lines.append(rec)
                print(f"[{R}, {H}] {label:8s} {name}: "
                      f"{min(us):6.2f} .. {max(us):6.2f} us/call, median "
                      f"{med:6.2f} = {rec['TBps']:.2f} TB/s of "
                      f"{rec['unique_MB']} MB", flush=True)
    print(json.dumps(lines))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=48)
    ap.add_argument("--shape", type=int, nargs=2, action="append",
                    metavar=("R", "H"),
                    help="time this [R, H] instead of the two default "
                         "shapes (repeatable); H a multiple of 256, <= 1024")
    ap.add_argument("--infer", action="store_true",
                    help="time the forward at p = 0 next to the forward-only "
                         "op of serving, at [4096, 768] unless --shape")
    a = ap.parse_args()
    if a.infer:
        bench_infer(a.rounds, a.calls,
                    [tuple(s) for s in a.shape] if a.shape else SHAPES[:1])
        return
    shapes = [tuple(s) for s in a.shape] if a.shape else SHAPES
    report(bench({"onepass": {}, "2pass": {"PDNLP_BDRL_2PASS": "1"}},
                 a.rounds, a.calls, shapes))


if __name__ == "__main__":
    main()
