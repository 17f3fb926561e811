"""The Trainer loop (layer L4) — one engine with strategy modes, replacing the
reference's per-script Trainer copies (canonical:
multi-gpu-distributed-cls.py:113-239).

Behavioral parity with the reference:
- epoch loop → ``sampler.set_epoch`` → step loop → forward/loss → backward →
  step → reduced global-mean loss → rank-0 ``【train】 epoch：e/E step：s/S
  loss：x`` print → periodic dev() with best-acc checkpoint save.
- dev/test: per-batch loss all-reduce + logits/labels all-gather, CPU argmax
  accuracy, final sklearn classification_report in test().

Deliberate deviations (SURVEY.md §2.2 notes):
- no per-step ``dist.barrier()`` in the hot loop (correctness does not need
  it; ``barrier_per_step`` flag restores reference semantics for debugging);
- the loss scalar all-reduce can be batched (``loss_reduce_every``);
- checkpoints are saved UNWRAPPED (no ``module.`` prefix);
- the AMP path calls ``zero_grad`` every step (the reference's AMP script
  forgot it — SURVEY.md §3.2 — we fix, not replicate).
"""

from __future__ import annotations

import time


import numpy as np
import torch
import torch.distributed as dist

from ..parallel.ddp import DistributedDataParallel
from ..parallel.zero import ZeroRedundancyOptimizer
from ..utils.checkpoint import save_checkpoint
from ..utils.logging import rank0_print
from ..utils.metrics import MetricsWriter, StepTimer, TraceRange


MAX_GRAPHS = 32        # captured graphs kept; further batch keys run eager
GRAPH_EAGER_STEPS = 3  # eager steps that must have run before any capture


def graph_key(batch, max_seq_len: int):
    """Batch signature under which a captured fwd+bwd graph is replayed.

    Padded batches: ``("padded", B, S)``. Packed batches
    (``pack_batch``): ``("packed", T, B, ms)`` with ``ms`` the batch's
    ``max_seqlen`` rounded up to 128 and capped at ``max_seq_len`` — the
    graph is captured with ``max_seqlen=ms``, so the attention grid and
    the PRELOAD/streamed choice hold for every batch of the key, whatever
    its sequence boundaries. ``None``: the batch cannot be replayed (a
    sequence longer than ``max_seq_len``)."""
    ids = batch["input_ids"]
    if "cu_seqlens" not in batch:
        return ("padded", int(ids.shape[0]), int(ids.shape[1]))
    longest = int(batch["max_seqlen"])
    if longest > max_seq_len:
        return None
    ms = min(int(max_seq_len), (longest + 127) // 128 * 128)
    return ("packed", int(ids.numel()),
            int(batch["cu_seqlens"].numel()) - 1, ms)


class GraphPolicy:
    """When a batch key gets a graph (no device involved): on its second
    or later sighting, once ``eager_steps`` eager steps have run, while
    fewer than ``max_graphs`` graphs exist. ``decide`` returns "replay",
    "capture" (capture now, then replay) or "eager"."""

    def __init__(self, max_graphs: int = MAX_GRAPHS,
                 eager_steps: int = GRAPH_EAGER_STEPS):
        self.max_graphs = max_graphs
        self.eager_steps = eager_steps
        self.seen = set()
        self.captured = set()
        self.eager = 0

    def decide(self, key) -> str:
        if key in self.captured:
            return "replay"
        if (key is not None and key in self.seen
                and self.eager >= self.eager_steps
                and len(self.captured) < self.max_graphs):
            self.captured.add(key)
            return "capture"
        self.seen.add(key)
        self.eager += 1
        return "eager"


class _GraphEntry:
    """One captured fwd+bwd graph: its static input buffers, the gradient
    tensors its backward assigns (in ``model.parameters()`` order) and its
    outputs. All of them stay referenced for the life of the entry, so
    later captures into the shared pool cannot reuse their memory."""

    def __init__(self, static, label_key):
        self.static = static
        self.label_key = label_key
        self.graph = None
        self.grads = self.loss = self.logits = None

    def run(self, batch):
        """Copy ``batch`` into the static buffers and replay. The caller
        reseeds dropout and owns what happens to ``grads``."""
        for k, t in self.static.items():
            t.copy_(batch[k], non_blocking=True)
        self.graph.replay()
        return self.loss, self.logits, self.static[self.label_key]


class Trainer:
    def __init__(self, args, model, optimizer, device,
                 scaler=None, lr_scheduler=None, label_key: str = "label"):
        self.args = args
        self.model = model
        self.optimizer = optimizer
        self.device = torch.device(device)
        self.scaler = scaler
        self.lr_scheduler = lr_scheduler
        self.label_key = label_key
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.metrics = MetricsWriter(getattr(args, "metrics_jsonl", None),
                                     rank=self.rank)
        self.best_acc = -1.0  # first dev eval always checkpoints
        self.global_step = 0
        self._resume_skip = 0  # batches to fast-forward after load_state
        # hipGraph replay (args.hip_graph): batch key -> _GraphEntry, all
        # captured into one memory pool; _graph_bound is the entry whose
        # gradient tensors the parameters' .grad currently point at
        self._graphs = {}
        self._graph_policy = GraphPolicy()
        self._graph_pool = None
        self._graph_bound = None
        self.graph_stats = {"captured": 0, "replayed": 0, "eager": 0}
        # global gradient norm of the last optimizer step as an fp32[1]
        # DEVICE tensor (None while max_grad_norm is off); read on logged
        # steps only, where the loss .item() syncs anyway
        self.last_grad_norm = None
        mgn = float(getattr(args, "max_grad_norm", 0.0) or 0.0)
        if mgn > 0 and getattr(optimizer, "max_grad_norm", None) == 0.0:
            # ZeRO / hooks clip inside step(): hand them the bound when the
            # optimizer was built without build_training
            optimizer.max_grad_norm = mgn
        # optional per-step hook: fn(trainer) called after every global step
        # (HFStyleTrainer uses it for checkpoint-N dirs)
        self.step_callback = None
        apply_attn_tile_pack(args, model)
        apply_cls_only_last_layer(args, model)

    # ------------------------------------------------------------------
    def on_step(self, batch):
        """H2D copy + forward (reference: multi-gpu-distributed-cls.py:126-137)."""
        input_ids = batch["input_ids"].to(self.device, non_blocking=True)
        token_type_ids = batch["token_type_ids"].to(self.device, non_blocking=True)
        labels = batch[self.label_key].to(self.device, non_blocking=True)
        if "cu_seqlens" in batch:  # packed stream from Collate(unpad=True)
            out = self.model(
                input_ids=input_ids, token_type_ids=token_type_ids,
                labels=labels,
                cu_seqlens=batch["cu_seqlens"].to(self.device,
                                                  non_blocking=True),
                max_seqlen=int(batch["max_seqlen"]),
                position_ids=batch["position_ids"].to(self.device,
                                                      non_blocking=True))
            return out.loss, out.logits, labels
        attention_mask = batch["attention_mask"].to(self.device, non_blocking=True)
        out = self.model(input_ids=input_ids, attention_mask=attention_mask,
                         token_type_ids=token_type_ids, labels=labels)
        return out.loss, out.logits, labels

    def loss_reduce(self, loss: torch.Tensor) -> torch.Tensor:
        """Global mean loss (reference: multi-gpu-distributed-cls.py:139-143)."""
        if self.world > 1:
            loss = loss.detach().clone()
            dist.all_reduce(loss, op=dist.ReduceOp.SUM)
            loss = loss / self.world
        return loss

    def output_reduce(self, logits: torch.Tensor, labels: torch.Tensor):
        """All-gather eval logits+labels (reference:
        multi-gpu-distributed-cls.py:145-155)."""
        if self.world == 1:
            return logits, labels
        lg = [torch.zeros_like(logits) for _ in range(self.world)]
        lb = [torch.zeros_like(labels) for _ in range(self.world)]
        dist.all_gather(lg, logits.contiguous())
        dist.all_gather(lb, labels.contiguous())
        return torch.cat(lg, dim=0), torch.cat(lb, dim=0)

    # ------------------------------------------------------------------
    def _backward_and_step(self, loss, accum_boundary: bool):
        from ..parallel.dp import DataParallel
        args = self.args
        scale_accum = 1.0 / max(args.grad_accum_steps, 1)
        is_ddp = isinstance(self.model, DistributedDataParallel)
        is_zero = isinstance(self.optimizer, ZeroRedundancyOptimizer)

        def _bw(l):
            l = l * scale_accum
            if self.scaler is not None:
                l = self.scaler.scale(l)
            with TraceRange("backward"):
                l.backward()
            if isinstance(self.model, DataParallel):
                # fold replica grads into the primary (single-process DP)
                self.model.sync_replica_grads()

        if not accum_boundary:
            # micro-step: gradients only accumulate — no sync, no clip, no
            # optimizer step until the boundary
            if is_ddp:
                with self.model.no_sync():
                    _bw(loss)
            else:
                _bw(loss)
            return False
        _bw(loss)
        if is_ddp:
            self.model.finalize_backward()
        with TraceRange("optimizer"):
            if self.scaler is not None and not is_zero:
                if self._clips_here():
                    # the clip must see unscaled gradients
                    self.scaler.unscale_(self.optimizer)
                coef = self._grad_coef()
                if coef is not None:
                    self.scaler.step(self.optimizer, grad_coef=coef)
                else:
                    self.scaler.step(self.optimizer)
                self.scaler.update()
            elif self.scaler is not None and is_zero:
                # grads were unscaled rank-LOCALLY (before reduce-scatter),
                # so the overflow flag must be all-reduced; on the device
                # path both the reduce and the skip stay on-GPU (no .item())
                self.scaler.unscale_(self.optimizer)
                self.scaler.sync_found_inf()
                if self.scaler._found_async:
                    self.optimizer.step(found_inf=self.scaler._found_dev)
                elif not self.scaler._found_inf:
                    self.optimizer.step()
                self.scaler.update()
            else:
                self._optimizer_step()
        if not self._clips_here():
            # ZeRO / hooks clip inside step(), after their own reduction
            self.last_grad_norm = getattr(self.optimizer, "last_grad_norm",
                                          None)
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        self._zero_grad()
        return True

    # ---- global-norm gradient clipping (ops/grad_clip.py) ----
    def _clips_here(self) -> bool:
        """True when the Trainer itself computes the clip coefficient.
        Optimizers that reduce gradients inside ``step()`` (ZeRO, hooks)
        carry ``max_grad_norm`` themselves and clip after the reduction."""
        mgn = getattr(self.args, "max_grad_norm", 0.0)
        return bool(mgn and mgn > 0
                    and not hasattr(self.optimizer, "max_grad_norm"))

    def _grad_coef(self):
        """Device clip coefficient for the gradients as they stand (already
        synchronized and unscaled), or None when there is nothing to pass
        on. Fused optimizers take the coefficient into their kernels, so the
        gradients are read once and never rewritten; any other optimizer
        gets them scaled in place."""
        if not self._clips_here():
            return None
        from ..ops.adamw import FusedAdamW, FusedSGD
        from ..ops.grad_clip import grad_clip_coef, scale_
        grads = [p.grad for p in self.model.parameters()
                 if p.grad is not None]
        if not grads:
            return None
        coef, norm = grad_clip_coef(grads, self.args.max_grad_norm)
        self.last_grad_norm = norm
        if isinstance(self.optimizer, (FusedAdamW, FusedSGD)):
            return coef
        scale_(grads, coef)
        return None

    def _optimizer_step(self):
        coef = self._grad_coef()
        if coef is not None:
            self.optimizer.step(grad_coef=coef)
        else:
            self.optimizer.step()

    def _zero_grad(self):
        if isinstance(self.model, DistributedDataParallel):
            self.model.zero_grad_buffers()
        else:
            self.optimizer.zero_grad(set_to_none=True)

    # ---- hipGraph-replayed training steps (single GPU, SURVEY.md §5.1+) ----
    # One graph of fwd+bwd per batch key (graph_key), padded and packed
    # batches alike; the optimizer, the clip and dropout reseeding stay
    # eager between replays. DESIGN.md "hipGraph replay per batch key".
    @property
    def _graph(self):
        """The graph cache once any graph exists, else None."""
        return self._graphs or None

    def _graph_capable(self) -> bool:
        a = self.args
        return (self.device.type == "cuda" and self.world == 1
                and getattr(a, "grad_accum_steps", 1) <= 1
                and self.scaler is None
                and not getattr(a, "activation_checkpointing", False)
                and not isinstance(self.model, DistributedDataParallel)
                and not isinstance(self.optimizer, ZeroRedundancyOptimizer))

    def _graph_key(self, batch):
        return graph_key(batch, int(getattr(self.args, "max_seq_len", 128)))

    def _maybe_capture_graph(self, batch):
        """True when ``batch`` has a graph to replay, capturing one first
        where GraphPolicy says so. Enabled by ``args.hip_graph`` on a
        single GPU without grad accumulation, fp16 scaling or activation
        checkpointing."""
        if not getattr(self.args, "hip_graph", False):
            return False
        if not self._graph_capable():
            if getattr(self.args, "unpad", False) \
                    and not getattr(self, "_unpad_graph_noted", False):
                self._unpad_graph_noted = True
                rank0_print("[pdnlp] --unpad with --hip-graph needs one GPU, "
                            "no grad accumulation, no fp16 scaler and no "
                            "activation checkpointing: hipGraph capture "
                            "disabled (eager steps)")
            return False
        key = self._graph_key(batch)
        what = self._graph_policy.decide(key)
        if what == "capture":
            self._graphs[key] = self._capture_graph(batch, key)
            self.graph_stats["captured"] += 1
            rank0_print(f"[pdnlp] hipGraph captured for {key}: replaying "
                        f"fwd+bwd ({len(self._graphs)} graphs)")
        return what != "eager"

    def _model_inputs(self, static, key):
        kw = dict(input_ids=static["input_ids"],
                  token_type_ids=static["token_type_ids"],
                  labels=static[self.label_key])
        if key[0] == "packed":
            # max_seqlen is the key's bound, not the batch's own maximum:
            # the captured attention launch must cover every batch of the key
            kw.update(cu_seqlens=static["cu_seqlens"], max_seqlen=key[3],
                      position_ids=static["position_ids"])
        else:
            kw.update(attention_mask=static["attention_mask"])
        return kw

    def _release_graph_grads(self):
        """Unbind .grad from a replayed graph's tensors, so that an eager
        backward (or a capture) assigns fresh gradients instead of
        accumulating onto the last replay's."""
        if self._graph_bound is not None:
            self._graph_bound = None
            for p in self.model.parameters():
                p.grad = None

    def _capture_graph(self, batch, key=None):
        """Capture fwd+bwd on ``batch`` into a new _GraphEntry. The caller
        holds no autograd references of an earlier step (see the note at
        ``del out``). Gradients are captured with .grad = None, so the
        backward ASSIGNS them: every replay overwrites the entry's own
        gradient tensors (no zero_grad, no accumulate-adds)."""
        key = key or self._graph_key(batch)
        names = ["input_ids", "token_type_ids", self.label_key]
        names += ["cu_seqlens", "position_ids"] if key[0] == "packed" \
            else ["attention_mask"]
        entry = _GraphEntry({k: batch[k].to(self.device).clone()
                             for k in names}, self.label_key)
        inputs = self._model_inputs(entry.static, key)
        params = list(self.model.parameters())
        self._release_graph_grads()
        # warm-up: forward and backward only — an optimizer step here would
        # be an update on this batch that no step counter sees
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                out = self.model(**inputs)
                out.loss.backward()
        del out  # a live autograd graph from before the capture pins
        #          default/side-stream AccumulateGrad nodes and SEGFAULTS
        #          hipGraph instantiation (torch input_buffer stream check)
        torch.cuda.current_stream().wait_stream(s)
        for p in params:
            p.grad = None
        if self._graph_pool is None:
            self._graph_pool = torch.cuda.graph_pool_handle()
        entry.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(entry.graph, pool=self._graph_pool):
            out = self.model(**inputs)
            out.loss.backward()
        # detached: the outputs must not keep the captured autograd graph
        # (and its AccumulateGrad nodes) alive into the next capture
        entry.loss, entry.logits = out.loss.detach(), out.logits.detach()
        del out
        entry.grads = [p.grad for p in params]
        for p in params:   # bound again by the first replay
            p.grad = None
        return entry

    def _graph_step(self, batch):
        """Replay the graph of ``batch``'s key and step the optimizer;
        None when the key has no graph (the caller runs the step eager).
        .grad stays bound to the entry's gradients afterwards."""
        from ..ops import reseed_dropout
        entry = self._graphs.get(self._graph_key(batch))
        if entry is None:
            return None
        reseed_dropout()
        res = entry.run(batch)
        if self._graph_bound is not entry:
            for p, g in zip(self.model.parameters(), entry.grads):
                p.grad = g
            self._graph_bound = entry
        # the clip runs eagerly between replay and step, like the optimizer
        self._optimizer_step()
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        self.graph_stats["replayed"] += 1
        return res

    def train_step(self, batch, accum_boundary: bool = True):
        """One training step on ``batch``: a graph replay where its key has
        a graph, an eager step otherwise. Returns (loss, logits, labels,
        stepped). The caller drops the previous step's loss/logits first:
        a capture must not find their autograd graph alive."""
        if self._maybe_capture_graph(batch):
            res = self._graph_step(batch)
            if res is not None:
                return (*res, True)
        self._release_graph_grads()
        with TraceRange("forward"):
            loss, logits, labels = self.on_step(batch)
        if self.args.barrier_per_step and self.world > 1:
            dist.barrier()
        stepped = self._backward_and_step(loss, accum_boundary)
        self.graph_stats["eager"] += 1
        return loss, logits, labels, stepped

    def _state_path(self) -> str:
        import os
        p = getattr(self.args, "save_state_path", "") or ""
        if not p:
            p = os.path.join(getattr(self.args, "output_dir", "."),
                             "train_state.pt")
        os.makedirs(os.path.dirname(p) or ".", exist_ok=True)
        return p

    # ---- resume (a capability the reference lacks — SURVEY.md §5.4) ----
    def save_state(self, path: str) -> None:
        """Full training state: model + optimizer + step counters (+ scale,
        + LR-scheduler position)."""
        extra = {"global_step": self.global_step, "best_acc": self.best_acc}
        if self.scaler is not None:
            extra["scaler_scale"] = self.scaler.get_scale()
        if self.lr_scheduler is not None and hasattr(self.lr_scheduler,
                                                     "state_dict"):
            extra["lr_scheduler"] = self.lr_scheduler.state_dict()
        save_checkpoint(self.model, path, optimizer=self.optimizer,
                        extra=extra, rank=self.rank)
        if self.world > 1:
            dist.barrier()  # nobody resumes from a half-written file

    def load_state(self, path: str) -> None:
        from ..utils.checkpoint import load_checkpoint
        extra = load_checkpoint(self.model, path,
                                map_location=self.device,
                                optimizer=self.optimizer)
        self.global_step = int(extra.get("global_step", 0))
        self.best_acc = float(extra.get("best_acc", -1.0))
        if self.scaler is not None and "scaler_scale" in extra:
            self.scaler._scale = float(extra["scaler_scale"])
        if (self.lr_scheduler is not None and "lr_scheduler" in extra
                and hasattr(self.lr_scheduler, "load_state_dict")):
            self.lr_scheduler.load_state_dict(extra["lr_scheduler"])
        self._resume_skip = self.global_step

    # ------------------------------------------------------------------
    def train(self, train_loader, dev_loader=None, train_sampler=None):
        args = self.args
        total_step = len(train_loader) * args.epochs
        args.total_step = total_step
        self.model.train()
        timer = StepTimer(self.device)
        t_start = time.time()
        micro = 0
        prof = None
        if getattr(args, "torch_profile_steps", 0) > 0 and self.rank == 0:
            # first-class tracing the reference lacks:
            # kernel-level chrome trace for a few steps, written to
            # output_dir/trace.json
            import os
            from torch.profiler import (ProfilerActivity, profile, schedule,
                                        tensorboard_trace_handler)  # noqa: F401
            out = os.path.join(getattr(args, "output_dir", "."),
                               "trace.json")

            def _export(p):
                p.export_chrome_trace(out)
                rank0_print(f"[pdnlp] torch.profiler trace -> {out}")

            prof = profile(
                activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA],
                schedule=schedule(wait=1, warmup=2,
                                  active=args.torch_profile_steps),
                on_trace_ready=_export)
            prof.__enter__()
        self._prof = prof
        for epoch in range(1, args.epochs + 1):
            if train_sampler is not None and hasattr(train_sampler, "set_epoch"):
                train_sampler.set_epoch(epoch)
            for step, batch in enumerate(train_loader, start=1):
                if self._resume_skip > 0:
                    # fast-forward the data order to the restored step;
                    # micro advances too so grad-accumulation boundaries
                    # stay aligned with the original run
                    self._resume_skip -= 1
                    micro += 1
                    continue
                micro += 1
                accum_boundary = (micro % max(args.grad_accum_steps, 1) == 0)
                # drop the previous step's autograd references BEFORE any
                # capture attempt (see note in _capture_graph)
                loss = logits = None
                loss, logits, labels, stepped = self.train_step(
                    batch, accum_boundary)
                self.global_step += 1
                # budgeted batches round the sequence count up with empty
                # sequences: count the real ones
                timer.step(int(batch.get("num_seqs", labels.shape[0]))
                           * self.world)
                self._after_step(epoch, total_step, loss, timer, dev_loader,
                                 stepped)
        if prof is not None:
            prof.__exit__(None, None, None)
        self._prof = None
        if getattr(args, "save_state_every", 0) > 0:
            self.save_state(self._state_path())
        if not (args.do_dev and dev_loader is not None):
            save_checkpoint(self.model, args.ckpt_path, rank=self.rank)
        mins = (time.time() - t_start) / 60.0
        rank0_print(f"耗时：{mins:.4f}分钟 (wall-clock minutes)")
        self.metrics.write(phase="train_end", minutes=mins,
                           samples_per_sec=timer.samples_per_sec(sync=True),
                           graph_stats=dict(self.graph_stats))
        return mins

    def _after_step(self, epoch, total_step, loss, timer, dev_loader,
                    stepped):
        args = self.args
        if getattr(self, "_prof", None) is not None:
            self._prof.step()
        if self.global_step % args.log_every == 0:
            # the .item() device sync happens only on logged steps
            if self.global_step % args.loss_reduce_every == 0:
                printed_loss = self.loss_reduce(loss).item()
            else:
                printed_loss = loss.item()
            rank0_print(
                f"【train】 epoch：{epoch}/{args.epochs} "
                f"step：{self.global_step}/{total_step} "
                f"loss：{printed_loss:.6f}")
            extra = {}
            if self.last_grad_norm is not None:
                extra["grad_norm"] = float(self.last_grad_norm.item())
            self.metrics.write(
                phase="train", epoch=epoch, step=self.global_step,
                loss=printed_loss, **extra,
                lr=self.optimizer.param_groups[0]["lr"]
                if hasattr(self.optimizer, "param_groups") else args.learning_rate,
                samples_per_sec=timer.samples_per_sec(),
                stepped=stepped)
        if self.step_callback is not None:
            self.step_callback(self)
        if (getattr(args, "save_state_every", 0) > 0
                and self.global_step % args.save_state_every == 0):
            self.save_state(self._state_path())
        if (dev_loader is not None and args.do_dev
                and self.global_step % args.eval_step == 0):
            dev_loss, acc = self.dev(dev_loader)
            rank0_print(f"【dev】 loss：{dev_loss:.6f} accuracy：{acc:.4f}")
            self.metrics.write(phase="dev", step=self.global_step,
                               loss=dev_loss, accuracy=acc)
            if acc > self.best_acc:
                self.best_acc = acc
                save_checkpoint(self.model, args.ckpt_path, rank=self.rank)
                rank0_print(f"【best】 accuracy：{acc:.4f} → saved "
                            f"{args.ckpt_path}")
            self.model.train()

    # ------------------------------------------------------------------
    @torch.no_grad()
    def dev(self, loader):
        """Eval loop (reference: multi-gpu-distributed-cls.py:199-220)."""
        self.model.eval()
        total_loss = 0.0
        preds, trues = [], []
        for batch in loader:
            loss, logits, labels = self.on_step(batch)
            total_loss += self.loss_reduce(loss).item()
            g_logits, g_labels = self.output_reduce(logits.float(), labels)
            real = g_labels != -100  # empty sequences of a budgeted batch
            preds.append(g_logits[real].argmax(-1).cpu().numpy())
            trues.append(g_labels[real].cpu().numpy())
        preds = np.concatenate(preds)
        trues = np.concatenate(trues)
        acc = float((preds == trues).mean()) if len(trues) else 0.0
        return total_loss, acc

    @torch.no_grad()
    def test(self, loader, label_names=None):
        """Test with classification report (reference:
        multi-gpu-distributed-cls.py:222-239)."""
        self.model.eval()
        total_loss = 0.0
        preds, trues = [], []
        for batch in loader:
            loss, logits, labels = self.on_step(batch)
            total_loss += self.loss_reduce(loss).item()
            g_logits, g_labels = self.output_reduce(logits.float(), labels)
            real = g_labels != -100  # empty sequences of a budgeted batch
            preds.append(g_logits[real].argmax(-1).cpu().numpy())
            trues.append(g_labels[real].cpu().numpy())
        preds = np.concatenate(preds)
        trues = np.concatenate(trues)
        report = classification_report_text(trues, preds, label_names)
        if self.rank == 0:
            print(report)
        acc = float((preds == trues).mean()) if len(trues) else 0.0
        return total_loss, acc, report


class _LambdaLR:
    """Minimal LambdaLR that also works for optimizers that are not
    torch.optim.Optimizer subclasses (ZeroRedundancyOptimizer)."""

    def __init__(self, optimizer, fn):
        self.optimizer = optimizer
        self.fn = fn
        self._step = 0
        self._base = [g["lr"] for g in optimizer.param_groups]

    def step(self):
        self._step += 1
        for g, b in zip(self.optimizer.param_groups, self._base):
            g["lr"] = b * self.fn(self._step)

    def state_dict(self):
        return {"step": self._step, "base": self._base}

    def load_state_dict(self, sd):
        self._step = sd["step"]
        self._base = sd["base"]


def classification_report_text(trues, preds, label_names=None) -> str:
    try:
        from sklearn.metrics import classification_report
        labels = list(range(len(label_names))) if label_names else None
        return classification_report(trues, preds, labels=labels,
                                     target_names=label_names,
                                     zero_division=0)
    except ImportError:
        # minimal fallback: per-class P/R/F1
        lines = ["label\tprec\trecall\tf1\tsupport"]
        classes = sorted(set(list(trues) + list(preds)))
        for c in classes:
            tp = int(((preds == c) & (trues == c)).sum())
            fp = int(((preds == c) & (trues != c)).sum())
            fn = int(((preds != c) & (trues == c)).sum())
            p = tp / (tp + fp) if tp + fp else 0.0
            r = tp / (tp + fn) if tp + fn else 0.0
            f1 = 2 * p * r / (p + r) if p + r else 0.0
            name = label_names[c] if label_names else str(c)
            lines.append(f"{name}\t{p:.2f}\t{r:.2f}\t{f1:.2f}\t{tp + fn}")
        return "\n".join(lines)


def check_token_budget(args) -> None:
    """Reject configurations ``--max-tokens`` cannot serve (ValueError)."""
    max_tokens = int(getattr(args, "max_tokens", 0) or 0)
    if max_tokens > 0:
        if not getattr(args, "unpad", False):
            raise ValueError(
                "--max-tokens needs --unpad true: a token budget batches the "
                "packed stream, which padded [B, S] batches do not have.")
        if args.strategy == "dp":
            raise ValueError(
                "--max-tokens cannot be combined with strategy=dp (packed "
                "batches have no dim 0 to split). Use strategy=ddp.")
        if max_tokens < args.max_seq_len:
            raise ValueError(
                f"--max-tokens {max_tokens} is below --max-seq-len "
                f"{args.max_seq_len}: the longest sentence must fit a batch.")
        if max_tokens % 64:
            raise ValueError(
                f"--max-tokens {max_tokens} must be a multiple of 64, the "
                f"row granule of the packed stream.")


def check_attn_tile_pack(args) -> None:
    """Reject ``--attn-tile-pack true`` without the packed stream."""
    if getattr(args, "attn_tile_pack", False) \
            and not getattr(args, "unpad", False):
        raise ValueError(
            "--attn-tile-pack needs --unpad true: it packs the short "
            "sequences of the packed stream into shared attention tiles, "
            "which padded [B, S] batches do not have.")


def apply_attn_tile_pack(args, model) -> None:
    """Hand ``args.attn_tile_pack`` to the (unwrapped) model's config. The
    model builds the tile plan itself, once per forward, so nothing else in
    the step (batch dict, graph key, strategy wrappers) knows about it."""
    check_attn_tile_pack(args)
    if getattr(args, "attn_tile_pack", False):
        inner = getattr(model, "module", model)
        cfg = getattr(inner, "cfg", None)
        if cfg is None or not hasattr(cfg, "attn_tile_pack"):
            raise ValueError("--attn-tile-pack: the model has no "
                             "attn_tile_pack config field")
        cfg.attn_tile_pack = True


def check_cls_only_last_layer(args) -> None:
    """Reject ``--cls-only-last-layer true`` without the packed stream."""
    if getattr(args, "cls_only_last_layer", False) \
            and not getattr(args, "unpad", False):
        raise ValueError(
            "--cls-only-last-layer needs --unpad true: it runs the last "
            "encoder layer on the first-token rows of the packed stream, "
            "which padded [B, S] batches do not have.")


def apply_cls_only_last_layer(args, model) -> None:
    """Hand ``args.cls_only_last_layer`` to the (unwrapped) model's config.
    The model decides per forward from (T, B) alone, so the batch dict, the
    graph key and the strategy wrappers know nothing about it."""
    check_cls_only_last_layer(args)
    if getattr(args, "cls_only_last_layer", False):
        inner = getattr(model, "module", model)
        cfg = getattr(inner, "cfg", None)
        if cfg is None or not hasattr(cfg, "cls_only_last_layer"):
            raise ValueError("--cls-only-last-layer: the model has no "
                             "cls_only_last_layer config field")
        cfg.cls_only_last_layer = True


def build_training(args, model=None, label_key: str = "label"):
    """Assemble (model, optimizer, scaler, trainer) for a strategy mode.

    Strategy seam L3 of SURVEY.md §1: "single" | "dp" | "ddp" | "zero" |
    "hooks" — one engine, per-mode wiring.
    """
    from ..amp import GradScaler, cast_model_to
    from ..models import build_model
    from ..ops.adamw import build_optimizer
    from ..parallel import (DataParallel, DistributedOptimizer,
                            broadcast_optimizer_state, broadcast_parameters)

    # rank -> device modulo the visible count: ranks beyond the device
    # count share GPUs (oversubscribed world-2 runs on a 1-GPU box) instead
    # of crashing with "invalid device ordinal"
    if getattr(args, "unpad", False) and args.strategy == "dp":
        raise ValueError(
            "--unpad true cannot be combined with strategy=dp: single-process "
            "DataParallel splits the batch on dim 0, which a packed token "
            "stream does not have. Use strategy=ddp (one process per GPU).")
    check_token_budget(args)
    check_attn_tile_pack(args)
    check_cls_only_last_layer(args)
    ndev = max(torch.cuda.device_count(), 1)
    device = torch.device(f"cuda:{args.local_rank % ndev}"
                          if torch.cuda.is_available() else "cpu")
    args.device = str(device)
    if model is None:
        model = build_model(getattr(args, "model", "bert-base"),
                            model_path=args.model_path)
    if args.amp:
        model = cast_model_to(model, args.amp_dtype)
    model = model.to(device)
    if getattr(args, "activation_checkpointing", False):
        model.gradient_checkpointing_enable(
            cpu_offload=getattr(args, "checkpoint_cpu_offload", False))

    scaler = None
    if args.amp and args.amp_dtype == "fp16":
        scaler = GradScaler(init_scale=args.init_scale)

    if args.strategy == "zero":
        optimizer = ZeroRedundancyOptimizer(
            model, lr=args.learning_rate,
            betas=(args.adam_beta1, args.adam_beta2), eps=args.adam_eps,
            weight_decay=args.weight_decay, bucket_mb=args.bucket_cap_mb)
        optimizer.max_grad_norm = float(getattr(args, "max_grad_norm", 0.0)
                                        or 0.0)
        wrapped = model
    else:
        optimizer = build_optimizer(
            model, lr=args.learning_rate, weight_decay=args.weight_decay,
            betas=(args.adam_beta1, args.adam_beta2), eps=args.adam_eps,
            optimizer=args.optimizer, sgd_momentum=args.sgd_momentum)
        if args.strategy == "ddp" and dist.is_initialized():
            wrapped = DistributedDataParallel(
                model, bucket_cap_mb=args.bucket_cap_mb,
                grad_compression=args.grad_compression,
                overlap_comm=args.overlap_comm)
        elif args.strategy == "hooks" and dist.is_initialized():
            broadcast_parameters(model)
            comp = {"none": None, "bf16": torch.bfloat16,
                    "fp16": torch.float16}[args.grad_compression]
            optimizer = DistributedOptimizer(optimizer, compression=comp,
                                             fusion_mb=args.bucket_cap_mb)
            optimizer.max_grad_norm = float(
                getattr(args, "max_grad_norm", 0.0) or 0.0)
            broadcast_optimizer_state(optimizer.optimizer)
            wrapped = model
        elif args.strategy == "dp":
            wrapped = DataParallel(model)
        else:
            wrapped = model

    lr_scheduler = None
    if args.lr_scheduler != "none":
        base = optimizer.optimizer if isinstance(optimizer, DistributedOptimizer) \
            else optimizer
        total = max(getattr(args, "total_step", 0), 1) or 1000
        if args.lr_scheduler == "cosine" and isinstance(base, torch.optim.Optimizer):
            lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(
                base, T_max=total)
        elif args.lr_scheduler == "warmup_linear":
            # linear warmup over warmup_ratio of the run, then linear decay —
            # what a from-scratch deep transformer needs to move at all
            # (pretrained fine-tuning, the reference's setting, does not).
            # total_step is only known once train() sees the loader, so the
            # lambda reads it lazily.
            def lam(step):
                tot = max(getattr(args, "total_step", 0), 1) or 1000
                warm = max(int(tot * getattr(args, "warmup_ratio", 0.1)), 1)
                if step < warm:
                    return (step + 1) / warm
                return max(0.0, (tot - step) / max(tot - warm, 1))

            if isinstance(base, torch.optim.Optimizer) or hasattr(
                    base, "param_groups"):
                lr_scheduler = _LambdaLR(base, lam)

    trainer = Trainer(args, wrapped, optimizer, device, scaler=scaler,
                      lr_scheduler=lr_scheduler, label_key=label_key)
    return wrapped, optimizer, scaler, trainer
