"""Global-norm gradient clipping on device scalars (no host sync).

``torch.nn.utils.clip_grad_norm_`` semantics — ``norm = ||g||_2`` over every
gradient, ``coef = min(1, max_norm / (norm + 1e-6))``, a non-finite norm
propagates — split so the training step never rewrites the gradients:

- ``grad_sumsq``      one deterministic read pass (csrc/grad_clip.hip);
- ``grad_clip_coef``  sumsq -> ``(coef, norm)`` as fp32[1] device tensors; the
  fused optimizers take ``grad_coef=coef`` and multiply it into the gradient
  scale they apply anyway. ``extra_sumsq_reduce`` lets a sharded optimizer
  all-reduce the scalar between the two (ZeRO);
- ``clip_grad_norm_`` the in-place form for non-fused optimizers and the
  wrapper APIs.

The torch path (CPU, ``PDNLP_FORCE_TORCH=1``) computes the same with fp32
torch ops and is the numerics reference.
"""

from __future__ import annotations

from typing import Callable, Iterable, List, Optional, Tuple, Union

import torch

from . import ext, hip_enabled

CHUNK = 512  # tensors per extension call


def _grad_list(tensors_or_params) -> List[torch.Tensor]:
    """Gradients of parameters (``None`` grads skipped), tensors as given."""
    if isinstance(tensors_or_params, torch.Tensor):
        tensors_or_params = [tensors_or_params]
    out = []
    for t in tensors_or_params:
        if isinstance(t, torch.nn.Parameter):
            if t.grad is not None:
                out.append(t.grad)
        elif t is not None:
            out.append(t)
    return out


def _device_of(tensors: List[torch.Tensor], out: Optional[torch.Tensor]):
    if out is not None:
        return out.device
    return tensors[0].device if tensors else torch.device("cpu")


def _flat(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _by_dtype(tensors: List[torch.Tensor]) -> List[List[torch.Tensor]]:
    """Same-dtype call lists of at most CHUNK tensors."""
    groups = {}
    for t in tensors:
        groups.setdefault(t.dtype, []).append(t)
    calls = []
    for ts in groups.values():
        for i in range(0, len(ts), CHUNK):
            calls.append(ts[i:i + CHUNK])
    return calls


def grad_sumsq(tensors: Iterable[torch.Tensor],
               out: Optional[torch.Tensor] = None,
               accumulate: bool = False) -> torch.Tensor:
    """fp32[1] sum of squares over ``tensors`` (fp32/bf16/fp16, any mix).

    ``out``: write into this fp32[1] tensor; with ``accumulate=True`` add to
    what it holds, so several lists fold into one scalar. An empty list gives
    0 (or leaves ``out`` unchanged when accumulating)."""
    tensors = _grad_list(tensors)
    dev = _device_of(tensors, out)
    if out is None:
        out = torch.zeros(1, dtype=torch.float32, device=dev)
        accumulate = False
    if out.is_cuda and hip_enabled(out):
        calls = _by_dtype([_flat(t) for t in tensors]) or [[]]
        for i, ts in enumerate(calls):
            ext().multi_tensor_sumsq(ts, out, accumulate or i > 0)
        return out
    with torch.no_grad():
        s = torch.zeros(1, dtype=torch.float32, device=dev)
        for t in tensors:
            s += t.float().pow(2).sum()
        if accumulate:
            out += s
        else:
            out.copy_(s)
    return out


def clip_coef_from_sumsq(sumsq: torch.Tensor, max_norm: float
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(coef, norm)`` fp32[1] from an fp32[1] sum of squares."""
    if sumsq.is_cuda and hip_enabled(sumsq):
        coef = torch.empty_like(sumsq)
        norm = torch.empty_like(sumsq)
        ext().clip_coef_from_sumsq(sumsq, float(max_norm), coef, norm)
        return coef, norm
    norm = sumsq.sqrt()
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return coef, norm


def grad_clip_coef(tensors: Iterable[torch.Tensor], max_norm: float, *,
                   extra_sumsq_reduce: Optional[
                       Callable[[torch.Tensor], None]] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Clip coefficient and global norm of ``tensors`` as fp32[1] device
    tensors. ``extra_sumsq_reduce(sumsq)`` may reduce the fp32[1] sum of
    squares in place (e.g. an all-reduce over disjoint shards) before the
    norm is taken."""
    tensors = _grad_list(tensors)
    dev = _device_of(tensors, None)
    if extra_sumsq_reduce is None and dev.type == "cuda" \
            and hip_enabled(tensors[0]):
        # single process: the finalisation rides on the last fold launch
        sumsq = torch.empty(1, dtype=torch.float32, device=dev)
        coef = torch.empty_like(sumsq)
        norm = torch.empty_like(sumsq)
        calls = _by_dtype([_flat(t) for t in tensors])
        for i, ts in enumerate(calls):
            if i + 1 < len(calls):
                ext().multi_tensor_sumsq(ts, sumsq, i > 0)
            else:
                ext().multi_tensor_sumsq(ts, sumsq, i > 0, float(max_norm),
                                         coef, norm)
        return coef, norm
    sumsq = grad_sumsq(tensors)
    if extra_sumsq_reduce is not None:
        extra_sumsq_reduce(sumsq)
    return clip_coef_from_sumsq(sumsq, max_norm)


def scale_(tensors: Iterable[torch.Tensor], coef: torch.Tensor) -> None:
    """``t *= coef`` for every tensor, ``coef`` an fp32[1] device scalar."""
    tensors = _grad_list(tensors)
    if not tensors:
        return
    if tensors[0].is_cuda and hip_enabled(tensors[0]):
        for t in tensors:
            if not t.is_contiguous():
                raise ValueError("scale_: gradients must be contiguous")
        for ts in _by_dtype(tensors):
            ext().multi_tensor_scale_(ts, coef)
        return
    with torch.no_grad():
        for t in tensors:
            t.mul_(coef.to(t.device))


def clip_grad_norm_(tensors_or_params: Union[torch.Tensor, Iterable],
                    max_norm: float) -> torch.Tensor:
    """In-place global-norm clip; returns the (pre-clip) norm, fp32[1].

    Accepts parameters (their ``.grad`` is clipped) or gradient tensors."""
    grads = _grad_list(tensors_or_params)
    if not grads:
        return torch.zeros(1, dtype=torch.float32)
    coef, norm = grad_clip_coef(grads, max_norm)
    scale_(grads, coef)
    return norm
