#!/usr/bin/env python
"""Flagship benchmark: BERT-base classification fine-tuning step throughput.

Measures BASELINE.json's metric — samples/sec (whole-job aggregate) + epoch
wall-clock equivalent — for BERT-base cls seq128 bs32/GPU on 1..8 MI355X,
synthetic data, random-init weights.

    python bench.py --gpus N --steps K --warmup W
    # N>1 is launched by the driver as:
    # python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
    #     --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Timing: W untimed warmup steps, then exactly K steps bracketed by
barrier + torch.cuda.synchronize on both sides; MAX elapsed over ranks;
rank 0 prints ONE JSON line.

A plain run does only that: set up, warm up, time the K steps, print.
``--dump-outputs DIR`` additionally writes the last timed step's loss, logits
and a seeded sample of the updated parameters as ``DIR/<name>.npy`` (model,
batch and dropout are seeded, so equal arguments give equal inputs and two
builds can be compared output for output; on one MI355X two runs were
bit-identical up to 20 steps in all and apart by up to 0.5 in the logits at
40, see README.md). ``--full`` is where secondary
measurements belong; there are none in this file today (sweeps, CPU and
per-kernel figures are separate programs under ``tools/``).

Baseline for ``vs_baseline``: the reference's fastest published number —
HF Trainer fp16, 0.49 min/epoch on 2 GPUs = 312.9 samples/s (BASELINE.md,
reference README.md:23), linearly scaled per GPU: baseline(N) = 156.46 * N.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist

# reference epoch = 9200 train samples; fastest published row:
# HF Trainer fp16 0.49 min on 2 GPUs
_REF_EPOCH_SAMPLES = 9200
_BASELINE_SPS_PER_GPU = _REF_EPOCH_SAMPLES / (0.49 * 60.0) / 2.0  # 156.46


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--model", default="bert-base")
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--seq-len", type=int, default=128)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--bucket-cap-mb", type=float, default=50.0)
    p.add_argument("--zero", action="store_true", help="ZeRO mode instead of DDP")
    p.add_argument("--no-ddp-overlap", action="store_true")
    p.add_argument("--graph", action="store_true",
                   help="hipGraph-capture the fwd+bwd of the step "
                        "(single-GPU; optimizer stays eager)")
    p.add_argument("--no-warmup-floor", action="store_true",
                   help="skip the 2s time-based warmup extension (for "
                        "rocprofv3 --pmc runs: counter collection "
                        "serializes kernels and the floor never finishes)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the LAST timed "
                        "step computed as DIR/<name>.npy (float32): loss, "
                        "logits and a seeded sample of the updated "
                        "parameters. The time-based warmup extension does "
                        "not train in such a run, so the last step is "
                        "exactly step warmup+steps of the seeded start and "
                        "two builds can be compared output for output")
    p.add_argument("--full", action="store_true",
                   help="also run the benchmark's secondary measurements. "
                        "There are none today: every run is the plain "
                        "flagship measurement (CPU baselines, sweeps and "
                        "per-kernel figures live under tools/), so the "
                        "flag changes nothing yet")
    return p.parse_args()


# elements sampled per parameter tensor for --dump-outputs; ~200 tensors in
# bert-base -> < 4 MB of float32, far below the 64 MB a dump may take
_DUMP_PARAM_SAMPLE = 4096


def dump_outputs(out_dir, loss, logits, model):
    """Write the last timed step's results as float32 .npy files.

    ``params_sample`` is, per parameter in ``named_parameters()`` order, the
    elements at a fixed seeded set of flat indices (the whole tensor when it
    is not larger than the sample), concatenated."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    g = torch.Generator().manual_seed(4321)
    parts = []
    with torch.no_grad():
        for _, p in model.named_parameters():
            flat = p.detach().reshape(-1)
            if flat.numel() > _DUMP_PARAM_SAMPLE:
                idx = torch.randint(0, flat.numel(), (_DUMP_PARAM_SAMPLE,),
                                    generator=g)
                flat = flat[idx.to(flat.device)]
            parts.append(flat.float().cpu())
        arrays = {
            "loss": loss.detach().float().reshape(1).cpu(),
            "logits": logits.detach().float().cpu(),
            "params_sample": torch.cat(parts),
        }
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"),
                t.numpy().astype(np.float32, copy=False))


def main():
    ns = parse_args()
    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    use_cuda = torch.cuda.is_available()

    from pdnlp_amd.utils import set_seed
    set_seed(123)

    if world > 1:
        from pdnlp_amd.parallel.bootstrap import init_distributed
        init_distributed()
    dev_idx = local_rank % max(torch.cuda.device_count(), 1) if use_cuda else 0
    device = torch.device(f"cuda:{dev_idx}" if use_cuda else "cpu")
    if use_cuda:
        torch.cuda.set_device(device)

    from pdnlp_amd.models import build_model
    from pdnlp_amd.ops.adamw import build_optimizer
    from pdnlp_amd.parallel.ddp import DistributedDataParallel
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer

    model = build_model(ns.model, model_path=None)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16,
             "fp32": torch.float32}[ns.dtype]
    if dtype != torch.float32:
        model = model.to(dtype)
    model = model.to(device)
    model.train()

    scaler = None
    if ns.dtype == "fp16":
        from pdnlp_amd.amp import GradScaler
        scaler = GradScaler()

    if ns.zero and world > 1:
        optimizer = ZeroRedundancyOptimizer(model, lr=3e-5,
                                            bucket_mb=ns.bucket_cap_mb)
        wrapped = model
    else:
        optimizer = build_optimizer(model, lr=3e-5)
        wrapped = model
        if world > 1:
            wrapped = DistributedDataParallel(
                model, bucket_cap_mb=ns.bucket_cap_mb,
                overlap_comm=not ns.no_ddp_overlap)

    # synthetic batch of the reference shape, resident on device
    g = torch.Generator().manual_seed(1234 + rank)
    vocab = model.config.vocab_size if hasattr(model, "config") else 21128
    ids = torch.randint(106, vocab, (ns.batch_size, ns.seq_len), generator=g)
    ids[:, 0] = 101
    ids = ids.to(device)
    mask = torch.ones_like(ids)
    type_ids = torch.zeros_like(ids)
    labels = torch.randint(0, 6, (ns.batch_size,), generator=g).to(device)

    def fwd_bwd():
        out = wrapped(input_ids=ids, attention_mask=mask,
                      token_type_ids=type_ids, labels=labels)
        loss = out.loss
        if scaler is not None:
            loss = scaler.scale(loss)
        loss.backward()
        return out.loss, out.logits

    def opt_step(zero: bool = True):
        if isinstance(wrapped, DistributedDataParallel):
            wrapped.finalize_backward()
        if scaler is not None:
            scaler.step(optimizer)
            scaler.update()
        else:
            optimizer.step()
        if isinstance(wrapped, DistributedDataParallel):
            wrapped.zero_grad_buffers()
        elif zero:
            # set_to_none: AccumulateGrad steals the produced grad tensor —
            # no per-param fill and no per-param add kernels
            optimizer.zero_grad(set_to_none=True)

    graph = None
    if ns.graph and use_cuda and world == 1:
        from pdnlp_amd.ops import reseed_dropout
        # warm up allocator + autograd on a side stream, then capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                fwd_bwd()
                opt_step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        # capture with grads None: AccumulateGrad *assigns* inside the graph,
        # so every replay overwrites the same grad blocks — no zero_grad and
        # no accumulate-adds, ever (valid because each param has exactly one
        # grad contribution in this model)
        optimizer.zero_grad(set_to_none=True)
        with torch.cuda.graph(graph):
            static_out = fwd_bwd()

        def step():
            reseed_dropout()
            graph.replay()
            opt_step(zero=False)
            return static_out
    else:
        def step():
            out = fwd_bwd()
            opt_step()
            return out

    # W contractual warmup steps, extended to >=2s of wall time so a FRESH
    # box's clock ramp-up doesn't leak into the timed region (a cold MI355X
    # measured ~30% low with 10 warmup steps = 0.1 s of load).
    # Multi-rank: the extension is decided by RANK 0 and broadcast, so every
    # rank runs the SAME number of warmup steps — per-rank time-based exits
    # would mismatch the collectives inside step() and deadlock RCCL.
    # With --dump-outputs the extension must not train: the last timed step
    # has to be exactly step W+K of the seeded start whatever the clock says,
    # so there it is filled with eval-mode no-grad forwards, which keep the
    # GPU loaded but touch neither weights, optimizer nor dropout state.
    def floor_step():
        if not ns.dump_outputs:
            step()
            return
        model.eval()
        with torch.no_grad():
            model(input_ids=ids, attention_mask=mask, token_type_ids=type_ids)
        model.train()

    t_w = time.perf_counter()
    for _ in range(ns.warmup):
        step()
    w = ns.warmup
    while use_cuda and not ns.no_warmup_floor and w < ns.warmup + 2000:
        more = 1.0 if time.perf_counter() - t_w < 2.0 else 0.0
        if world > 1:
            t = torch.tensor([more], device=device if use_cuda else "cpu")
            dist.broadcast(t, src=0)
            more = float(t.item())
        if more == 0.0:
            break
        for _ in range(10):
            floor_step()
        w += 10

    if world > 1:
        dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for _ in range(ns.steps):
        last = step()
    if world > 1:
        dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    if ns.dump_outputs and rank == 0 and last is not None:
        dump_outputs(ns.dump_outputs, last[0], last[1], model)

    if world > 1:
        t = torch.tensor([elapsed], device=device if use_cuda else "cpu",
                         dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    n_gpus = world if world > 1 else 1
    total_samples = ns.batch_size * n_gpus * ns.steps
    sps = total_samples / elapsed
    ms_per_step = elapsed / ns.steps * 1000.0
    baseline = _BASELINE_SPS_PER_GPU * n_gpus
    if rank == 0:
        # "weak" is derived, not assumed: per-GPU work (batch_size x seq_len
        # per rank) is fixed as N grows in this harness — there is no
        # strong-scaling mode (total work would have to shrink per rank)
        zero_active = ns.zero and world > 1
        par = (("zero%d" % n_gpus) if zero_active else f"dp{n_gpus}")
        backend = dist.get_backend() if world > 1 else None
        n_phys = torch.cuda.device_count() if use_cuda else 0
        result = {
            "metric": "samples_per_sec",
            "value": round(sps, 2),
            "unit": "samples/s",
            "n_gpus": n_gpus,
            "steps": ns.steps,
            "warmup": ns.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(sps / baseline, 3),
            "dtype": ns.dtype,
            "data": "synthetic",
            "config": {
                "model": ns.model,
                "global_batch": ns.batch_size * n_gpus,
                "seq_len": ns.seq_len,
                "parallelism": par,
                "backend": backend,
                "physical_gpus": n_phys,
                "oversubscribed": bool(world > 1 and n_phys < world),
                "epoch_equiv_min": round(_REF_EPOCH_SAMPLES / sps / 60.0, 4),
                "baseline_source": "reference README.md:23 HF-Trainer fp16 "
                                   "0.49 min/epoch on 2 rented 2022 GPUs, "
                                   "scaled per GPU (other hardware — see "
                                   "BASELINE.md caveat)",
            },
        }
        print(json.dumps(result))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
