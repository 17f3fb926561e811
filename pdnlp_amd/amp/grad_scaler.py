"""Dynamic-loss-scaling GradScaler for the fp16 AMP path (K13).

Reference: ``torch.cuda.amp.GradScaler`` — ``scaler.scale(loss).backward();
scaler.step(optimizer); scaler.update()``
(multi-gpu-distributed-mp-amp-cls.py:161,173-175). Same API here.

MI355X design: the unscale + non-finite check runs on the HIP multi-tensor
kernel (device-side found-inf flag), and with a ``FusedAdamW`` the overflow
SKIP also happens device-side (the AdamW kernel reads the flag) — the step
never synchronizes the host. Scale bookkeeping (2x growth per
``growth_interval`` good steps, 0.5 backoff on overflow) consumes the flag
ONE STEP LATE through an async pinned-memory copy, so the launch pipeline
stays deep; a per-step ``found_inf.item()`` (what a naive port does) was
measured to cost ~35% of fp16 step time by draining the queue. Non-fused
optimizers and the CPU path keep the synchronous semantics.
"""

from __future__ import annotations

from typing import Iterable, Optional

import torch

from ..ops import ext, hip_enabled


class GradScaler:
    def __init__(self, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000,
                 enabled: bool = True):
        self._scale = float(init_scale)
        self.growth_factor = growth_factor
        self.backoff_factor = backoff_factor
        self.growth_interval = growth_interval
        self.enabled = enabled
        self._good_steps = 0
        self._unscaled = False
        # device-flag plumbing
        self._found_dev: Optional[torch.Tensor] = None
        self._found_async = False           # flag lives on-device this step
        self._found_val: Optional[bool] = None  # host value once known
        self._pinned: Optional[torch.Tensor] = None
        self._prev_ev = None                # event guarding the async copy

    def get_scale(self) -> float:
        return self._scale if self.enabled else 1.0

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        if not self.enabled:
            return loss
        return loss * self._scale

    def _grads(self, optimizer) -> Iterable[torch.Tensor]:
        for group in optimizer.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    yield p.grad

    def unscale_(self, optimizer) -> None:
        if not self.enabled or self._unscaled:
            return
        inv = 1.0 / self._scale
        grads = list(self._grads(optimizer))
        if grads and hip_enabled(grads[0]):
            dev = grads[0].device
            if self._found_dev is None or self._found_dev.device != dev:
                self._found_dev = torch.zeros(1, dtype=torch.float32,
                                              device=dev)
            else:
                self._found_dev.zero_()
            for i in range(0, len(grads), 512):
                ext().multi_tensor_unscale(grads[i:i + 512], self._found_dev,
                                           inv)
            self._found_async = True
            self._found_val = None          # only known after a sync
        else:
            found = False
            for g in grads:
                g.mul_(inv)
                if not found and not torch.isfinite(g).all():
                    found = True
            self._found_async = False
            self._found_val = bool(found)
        self._unscaled = True

    def sync_found_inf(self, group=None) -> None:
        """Make the overflow flag globally consistent across ranks.

        Needed whenever unscale_ ran on rank-LOCAL gradients (ZeRO: grads
        are unscaled before the reduce-scatter) — without it, ranks can
        disagree on the skip and shard states diverge. On the async/device
        path this is a device-side all-reduce (MAX), no host sync; on the
        sync path it reduces the host boolean."""
        import torch.distributed as dist
        if not (dist.is_initialized() and dist.get_world_size(group) > 1):
            return
        if self._found_async:
            dist.all_reduce(self._found_dev, op=dist.ReduceOp.MAX,
                            group=group)
        else:
            dev = ("cuda" if dist.get_backend(group) == "nccl"
                   and torch.cuda.is_available() else "cpu")
            t = torch.tensor([1.0 if self._found_val else 0.0], device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            self._found_val = bool(t.item() != 0)

    @property
    def _found_inf(self) -> bool:
        """Host view of the overflow flag; synchronizes if it only exists on
        the device (non-fused optimizers, ZeRO)."""
        if self._found_val is None and self._found_async:
            self._found_val = bool(self._found_dev.item() != 0)
        return bool(self._found_val)

    def step(self, optimizer, *args, grad_coef=None, **kwargs):
        """``grad_coef``: optional fp32[1] device clip coefficient, computed
        by the caller on the UNSCALED gradients (``unscale_`` first) and
        forwarded to the optimizer on both paths."""
        if grad_coef is not None:
            kwargs["grad_coef"] = grad_coef
        if not self.enabled:
            return optimizer.step(*args, **kwargs)
        self.unscale_(optimizer)
        if self._found_async:
            from ..ops.adamw import FusedAdamW
            if isinstance(optimizer, FusedAdamW):
                # overflow skip happens INSIDE the AdamW kernel — no sync
                if grad_coef is not None:
                    return optimizer.step(found_inf=self._found_dev,
                                          grad_coef=grad_coef)
                return optimizer.step(found_inf=self._found_dev)
        if self._found_inf:
            return None  # skip the step on overflow
        return optimizer.step(*args, **kwargs)

    def update(self) -> None:
        if not self.enabled:
            return
        if self._found_async and self._found_val is None:
            # async bookkeeping: consume LAST step's flag (its copy finished
            # long ago), enqueue this step's — scale adjustments land one
            # step late, the pipeline never drains
            if self._pinned is None:
                self._pinned = torch.zeros(1, dtype=torch.float32,
                                           pin_memory=True)
            if self._prev_ev is not None:
                self._prev_ev.synchronize()
                self._apply(bool(self._pinned.item() != 0))
            self._pinned.copy_(self._found_dev, non_blocking=True)
            self._prev_ev = torch.cuda.Event()
            self._prev_ev.record()
        else:
            self._apply(self._found_inf)
        self._found_val = None
        self._found_async = False
        self._unscaled = False

    def _apply(self, found: bool) -> None:
        if found:
            self._scale = max(self._scale * self.backoff_factor, 1.0)
            self._good_steps = 0
        else:
            self._good_steps += 1
            if self._good_steps >= self.growth_interval:
                self._scale *= self.growth_factor
                self._good_steps = 0
