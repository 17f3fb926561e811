"""HF-Trainer-style fully-delegated API (SURVEY.md §2.1 HF Trainer row).

Reference ergonomics (multi-gpu-transformers-cls.py:150-181):
``TrainingArguments`` (fp16, steps-based eval/save, load-best-at-end) +
``Trainer(model, args, datasets, collator, compute_metrics).train()``.
Same surface here, delegating to our engine; collator uses the ``labels``
key like the reference's HF-Trainer variant
(multi-gpu-transformers-cls.py:86).
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, Optional

import torch
from torch.utils.data import DataLoader

from ..config import Args
from ..data.sampler import DistributedSampler
from ..parallel.bootstrap import get_rank, init_distributed
from ..utils.checkpoint import save_checkpoint, load_checkpoint
from ..utils.logging import rank0_print
from .trainer import Trainer, build_training


@dataclass
class TrainingArguments:
    output_dir: str = "./output"
    per_device_train_batch_size: int = 32
    per_device_eval_batch_size: int = 32
    num_train_epochs: int = 1
    learning_rate: float = 3e-5
    weight_decay: float = 0.01
    fp16: bool = False
    bf16: bool = False
    evaluation_strategy: str = "steps"   # "no" | "steps"
    eval_steps: int = 100
    save_steps: int = 100
    save_strategy: str = "steps"
    load_best_model_at_end: bool = True
    metric_for_best_model: str = "accuracy"
    logging_steps: int = 10
    seed: int = 123
    gradient_accumulation_steps: int = 1
    dataloader_num_workers: int = 2
    unpad: bool = False   # the data_collator packs (Collate(unpad=True))
    max_tokens: int = 0   # with unpad: token-budget train batches of this
                          # many packed rows (per_device_train_batch_size
                          # is then not used); 0 = off
    attn_tile_pack: bool = False  # with unpad: tile-packed attention
    cls_only_last_layer: bool = False  # with unpad: last encoder layer on
                                       # the first-token rows only
    # global-norm gradient clipping, 0 = off. HF's own default is 1.0 (so
    # the reference's transformers run clips); set 1.0 to reproduce it.
    max_grad_norm: float = 0.0


class HFStyleTrainer:
    def __init__(self, model, args: TrainingArguments,
                 train_dataset=None, eval_dataset=None,
                 data_collator: Optional[Callable] = None,
                 compute_metrics: Optional[Callable] = None):
        self.hf_args = args
        self.model = model
        self.train_dataset = train_dataset
        self.eval_dataset = eval_dataset
        self.data_collator = data_collator
        self.compute_metrics = compute_metrics

        eargs = Args()
        eargs.train_batch_size = args.per_device_train_batch_size
        eargs.dev_batch_size = args.per_device_eval_batch_size
        eargs.epochs = int(args.num_train_epochs)
        eargs.learning_rate = args.learning_rate
        eargs.weight_decay = args.weight_decay
        eargs.amp = args.fp16 or args.bf16
        eargs.amp_dtype = "fp16" if args.fp16 else "bf16"
        eargs.eval_step = args.eval_steps
        eargs.do_dev = args.evaluation_strategy != "no"
        eargs.log_every = args.logging_steps
        eargs.grad_accum_steps = args.gradient_accumulation_steps
        eargs.seed = args.seed
        eargs.unpad = args.unpad
        eargs.max_tokens = args.max_tokens
        eargs.attn_tile_pack = args.attn_tile_pack
        eargs.cls_only_last_layer = args.cls_only_last_layer
        eargs.max_grad_norm = args.max_grad_norm
        eargs.output_dir = args.output_dir
        eargs.ckpt_path = os.path.join(args.output_dir, "best_model.pt")
        eargs.local_rank = init_distributed()
        eargs.strategy = "ddp"
        self.args = eargs
        (self.wrapped, self.optimizer, self.scaler,
         self.engine) = build_training(eargs, model=model, label_key="labels")
        # HF-style checkpoint-N dirs every save_steps (reference:
        # multi-gpu-transformers-cls.py:154-156; test.py:93 loads
        # output/checkpoint-100)
        if args.save_strategy == "steps" and args.save_steps > 0:
            def _save_cb(engine):
                if engine.global_step % args.save_steps == 0:
                    self._save_checkpoint_dir(engine.global_step)
            self.engine.step_callback = _save_cb

    def _save_checkpoint_dir(self, step: int) -> str:
        """Write ``output_dir/checkpoint-{step}/`` in HF dir layout
        (config.json + pytorch_model.bin with unwrapped HF keys)."""
        import json
        d = os.path.join(self.hf_args.output_dir, f"checkpoint-{step}")
        if get_rank() == 0:
            os.makedirs(d, exist_ok=True)
            torch.save(self.model.state_dict(),
                       os.path.join(d, "pytorch_model.bin"))
            cfg = getattr(self.model, "config", None)
            if cfg is not None and hasattr(cfg, "to_dict"):
                with open(os.path.join(d, "config.json"), "w") as f:
                    json.dump(cfg.to_dict(), f, indent=1)
        import torch.distributed as dist
        if dist.is_initialized():
            dist.barrier()
        return d

    def _loader(self, dataset, batch_size, shuffle):
        sampler = None
        import torch.distributed as dist
        if dist.is_initialized():
            sampler = DistributedSampler(dataset, shuffle=shuffle)
        return DataLoader(dataset, batch_size=batch_size,
                          sampler=sampler, shuffle=(sampler is None and shuffle),
                          collate_fn=self.data_collator,
                          num_workers=self.hf_args.dataloader_num_workers), sampler

    def _budget_loader(self):
        """Train loader of ``max_tokens``: a rank-sharded batch sampler and
        the data_collator's fixed-shape variant."""
        from ..cli import token_budget_loader
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_initialized() else 1
        rank = dist.get_rank() if dist.is_initialized() else 0
        self.args.num_workers = self.hf_args.dataloader_num_workers
        return token_budget_loader(self.args, self.train_dataset,
                                   self.data_collator, world, rank)

    def train(self):
        if self.hf_args.max_tokens > 0:
            loader, sampler = self._budget_loader()
        else:
            loader, sampler = self._loader(
                self.train_dataset,
                self.hf_args.per_device_train_batch_size, True)
        eval_loader = None
        if self.eval_dataset is not None:
            eval_loader, _ = self._loader(
                self.eval_dataset, self.hf_args.per_device_eval_batch_size, False)
        minutes = self.engine.train(loader, eval_loader, sampler)
        if (self.hf_args.load_best_model_at_end
                and os.path.isfile(self.args.ckpt_path)):
            load_checkpoint(self.model, self.args.ckpt_path,
                            map_location=self.engine.device)
        return {"train_runtime_min": minutes}

    def evaluate(self):
        if self.eval_dataset is None:
            raise ValueError("evaluate() needs an eval_dataset")
        eval_loader, _ = self._loader(
            self.eval_dataset, self.hf_args.per_device_eval_batch_size, False)
        loss, acc = self.engine.dev(eval_loader)
        # engine.dev returns the reference's sum-of-batch-mean losses
        # (SURVEY.md §2.2); HF Trainer reports the MEAN eval loss
        metrics = {"eval_loss": loss / max(len(eval_loader), 1),
                   "eval_accuracy": acc}
        rank0_print(metrics)
        return metrics

    def predict(self, dataset):
        loader, _ = self._loader(
            dataset, self.hf_args.per_device_eval_batch_size, False)
        self.engine.model.eval()
        outs = []
        with torch.no_grad():
            for batch in loader:
                _, logits, _ = self.engine.on_step(batch)
                outs.append(logits.float().cpu())
        return torch.cat(outs, dim=0)

    def save_model(self, path: Optional[str] = None):
        save_checkpoint(self.model,
                        path or os.path.join(self.hf_args.output_dir, "model.pt"),
                        rank=get_rank())
