#!/usr/bin/env python
"""Cost of global-norm gradient clipping in the training step.

    python tools/bench_clip.py [--windows 5] [--steps 30] [--max-norm 1.0]

Eager bf16 BERT-base training steps (forward, backward, fused AdamW) at
batch 32 x seq 128 on one GPU, in three modes:

  none   no clipping;
  torch  ``torch.nn.utils.clip_grad_norm_`` on the gradients, then
         ``step()`` — what the Trainer did before the fused path (foreach
         norm kernels, then every gradient rewritten);
  fused  ``ops.grad_clip_coef`` (one read pass, csrc/grad_clip.hip) and
         ``step(grad_coef=coef)`` — the coefficient is applied inside the
         AdamW kernels, gradients are not rewritten.

Method: one model + optimizer per mode from the same seed, a fixed pool of
seeded batches on the device, a warm-up window per mode, then ``--windows``
rounds in which the three modes run one timed window of ``--steps`` steps
each, interleaved, every window closed by a device synchronise. Reports
every window, the range and median per mode, the kernel launches the fused
clip adds per step, the norm each clipping mode saw at step 1 (same weights
and batch but different dropout masks, and torch's is rounded to bf16, so
the two agree to a few percent only), and one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdnlp_amd import ops  # noqa: E402
from pdnlp_amd.models import build_model  # noqa: E402
from pdnlp_amd.ops.adamw import build_optimizer  # noqa: E402
from pdnlp_amd.utils import set_seed  # noqa: E402

S, VOCAB = 128, 21128
MAXT = 32  # tensors per stage-1 launch (csrc/grad_clip.hip)


def make_batches(n, batch, seed, dev):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        ids = torch.randint(106, VOCAB, (batch, S), generator=g)
        ids[:, 0] = 101
        out.append({"input_ids": ids.to(dev),
                    "attention_mask": torch.ones_like(ids).to(dev),
                    "token_type_ids": torch.zeros_like(ids).to(dev),
                    "label": torch.randint(0, 6, (batch,),
                                           generator=g).to(dev)})
    return out


class Mode:
    def __init__(self, name, batches, dev, max_norm):
        set_seed(123)
        self.name = name
        self.max_norm = max_norm
        self.model = build_model("bert-base").to(torch.bfloat16).to(dev)
        self.model.train()
        self.opt = build_optimizer(self.model, lr=3e-5)
        self.params = [p for p in self.model.parameters() if p.requires_grad]
        self.batches = batches
        self.i = 0
        self.norm = None
        self.first_norm = None   # step 1: same weights and batch in all modes

    def step(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        out = self.model(
            input_ids=b["input_ids"], attention_mask=b["attention_mask"],
            token_type_ids=b["token_type_ids"], labels=b["label"])
        out.loss.backward()
        if self.name == "torch":
            self.norm = torch.nn.utils.clip_grad_norm_(self.params,
                                                       self.max_norm)
            self.opt.step()
        elif self.name == "fused":
            coef, self.norm = ops.grad_clip_coef(
                [p.grad for p in self.params], self.max_norm)
            self.opt.step(grad_coef=coef)
        else:
            self.opt.step()
        if self.first_norm is None:
            self.first_norm = self.norm
        self.opt.zero_grad(set_to_none=True)
        return out.loss

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = self.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        assert math.isfinite(loss.item()), f"{self.name}: loss {loss.item()}"
        return ms


def fused_launches(params):
    """Launches ``grad_clip_coef`` adds: per dtype, one stage-1 launch per
    MAXT non-empty tensors and one fold (which also writes coef and norm)."""
    by_dtype = {}
    for p in params:
        if p.numel():
            by_dtype[p.dtype] = by_dtype.get(p.dtype, 0) + 1
    return sum((n + MAXT - 1) // MAXT + 1 for n in by_dtype.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--pool", type=int, default=8, help="distinct batches")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=123)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clip.py measures GPU step time: no GPU visible")
    dev = torch.device("cuda:0")

    batches = make_batches(a.pool, a.batch, a.seed, dev)
    modes = [Mode(n, batches, dev, a.max_norm)
             for n in ("none", "torch", "fused")]
    for m in modes:
        m.window(10)
    times = {m.name: [] for m in modes}
    for w in range(a.windows):
        for m in modes:
            times[m.name].append(m.window(a.steps))
        print(f"window {w}: " + ", ".join(
            f"{k} {v[-1]:.3f}" for k, v in times.items()) + " ms/step")
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k, v in times.items():
        print(f"{k}: {min(v):.3f} .. {max(v):.3f} ms/step, median "
              f"{med[k]:.3f}, over {a.windows} windows of {a.steps} steps")
    norms = {m.name: float(m.first_norm.item()) for m in modes
             if m.first_norm is not None}
    launches = fused_launches(modes[2].params)
    nbytes = sum(p.numel() * p.element_size() for p in modes[2].params)
    print(f"fused clip: {launches} launches per step over "
          f"{len(modes[2].params)} gradient tensors, {nbytes / 1e6:.0f} MB "
          f"read; norm of step 1 {norms}")
    print(f"fused - none: {med['fused'] - med['none']:+.3f} ms/step; "
          f"torch - none: {med['torch'] - med['none']:+.3f} ms/step "
          "(medians)")
    print("fused median <= torch median:", med["fused"] <= med["torch"])
    print(json.dumps({
        "metric": "bench_clip", "batch": a.batch, "seq": S,
        "max_norm": a.max_norm, "ms_per_step": times, "median_ms": med,
        "fused_launches": launches, "grad_bytes": nbytes,
        "first_norm": norms,
        "fused_not_slower_than_torch": med["fused"] <= med["torch"]}))


if __name__ == "__main__":
    main()
