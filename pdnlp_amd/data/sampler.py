"""Our own DistributedSampler-equivalent.

Shards a dataset across ranks with per-epoch shuffling via ``set_epoch``
(reference uses torch's DistributedSampler: multi-gpu-distributed-cls.py:313-331
and calls ``set_epoch`` at :164). Behavior: pad-to-even with wrapped samples so
every rank sees the same number of batches (no rank hangs a collective), then
take rank::world_size strided.
"""

from __future__ import annotations

import math
from typing import Iterator, Optional

import torch
import torch.distributed as dist
from torch.utils.data import Sampler


class DistributedSampler(Sampler):
    def __init__(self, dataset, num_replicas: Optional[int] = None,
                 rank: Optional[int] = None, shuffle: bool = True,
                 seed: int = 0, drop_last: bool = False):
        if num_replicas is None:
            num_replicas = dist.get_world_size() if dist.is_initialized() else 1
        if rank is None:
            rank = dist.get_rank() if dist.is_initialized() else 0
        if not (0 <= rank < num_replicas):
            raise ValueError(f"rank {rank} out of range for {num_replicas} replicas")
        self.dataset = dataset
        self.num_replicas = num_replicas
        self.rank = rank
        self.shuffle = shuffle
        self.seed = seed
        self.drop_last = drop_last
        self.epoch = 0
        n = len(dataset)
        if drop_last and n % num_replicas:
            self.num_samples = n // num_replicas
        else:
            self.num_samples = math.ceil(n / num_replicas)
        self.total_size = self.num_samples * num_replicas

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __iter__(self) -> Iterator[int]:
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            indices = torch.randperm(n, generator=g).tolist()
        else:
            indices = list(range(n))
        if not self.drop_last:
            pad = self.total_size - len(indices)
            if pad > 0:
                indices += (indices * math.ceil(pad / max(len(indices), 1)))[:pad]
        else:
            indices = indices[: self.total_size]
        assert len(indices) == self.total_size
        return iter(indices[self.rank:: self.num_replicas])

    def __len__(self) -> int:
        return self.num_samples


class TokenBudgetBatchSampler(Sampler):
    """Batch sampler of the padding-free path: each batch takes as many
    sentences as fit into ``max_tokens`` real tokens (``--max-tokens``), so
    every step runs at the packed shape the GEMMs were tuned for.

    Batches are formed ONCE, here: the indices are permuted with ``seed``
    (when ``shuffle``) and filled greedily in that order; a batch closes
    when the next sentence would take it past ``max_tokens`` tokens, or past
    ``max_sentences`` sentences when that is > 0. There is no sorting by
    length — without padding there is nothing to gain from it, and it would
    bias the batches. ``set_epoch(e)`` permutes the ORDER of the batches
    with ``seed + e``; their composition, and so ``len()``, stays fixed
    (step counts, LR schedules and resume depend on that).

    With ``num_replicas > 1`` the ordered batch list is extended by wrapping
    from its start to a multiple of ``num_replicas`` and rank r takes
    ``order[r::num_replicas]``: every rank runs the same number of steps.
    """

    def __init__(self, lengths, max_tokens: int, max_sentences: int = 0,
                 shuffle: bool = True, seed: int = 0, num_replicas: int = 1,
                 rank: int = 0):
        if not (0 <= rank < num_replicas):
            raise ValueError(f"rank {rank} out of range for {num_replicas} replicas")
        lengths = [int(n) for n in lengths]
        if not lengths:
            raise ValueError("TokenBudgetBatchSampler: no samples")
        longest = max(lengths)
        if longest > max_tokens:
            raise ValueError(f"TokenBudgetBatchSampler: a sample of {longest} "
                             f"tokens exceeds max_tokens={max_tokens}")
        self.lengths = lengths
        self.max_tokens = int(max_tokens)
        self.max_sentences = int(max_sentences)
        self.shuffle = shuffle
        self.seed = seed
        self.num_replicas = num_replicas
        self.rank = rank
        self.epoch = 0
        n = len(lengths)
        if shuffle:
            g = torch.Generator()
            g.manual_seed(seed)
            indices = torch.randperm(n, generator=g).tolist()
        else:
            indices = list(range(n))
        self.batches = []
        cur, tokens = [], 0
        for i in indices:
            full = tokens + lengths[i] > self.max_tokens or \
                (self.max_sentences > 0 and len(cur) >= self.max_sentences)
            if cur and full:
                self.batches.append(cur)
                cur, tokens = [], 0
            cur.append(i)
            tokens += lengths[i]
        self.batches.append(cur)
        self.num_batches = math.ceil(len(self.batches) / num_replicas)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def shard(self, num_replicas: int, rank: int) -> "TokenBudgetBatchSampler":
        """The same batches, sharded for ``rank`` of ``num_replicas``."""
        s = TokenBudgetBatchSampler(
            self.lengths, self.max_tokens, self.max_sentences, self.shuffle,
            self.seed, num_replicas, rank)
        s.epoch = self.epoch
        return s

    def _order(self):
        n = len(self.batches)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        pad = self.num_batches * self.num_replicas - n
        if pad > 0:
            order += (order * math.ceil(pad / n))[:pad]
        return order[self.rank:: self.num_replicas]

    def __iter__(self):
        return iter([list(self.batches[b]) for b in self._order()])

    def __len__(self) -> int:
        return self.num_batches


def sequence_lengths(dataset, tokenizer, max_seq_len: int):
    """Real token count of every sample, computed once up front:
    ``attention_mask.sum()`` of pre-tokenized dict samples, ``sum(mask)`` of
    ``tokenizer.encode`` for (text, label) samples."""
    out = []
    for i in range(len(dataset)):
        sample = dataset[i]
        if isinstance(sample, dict):
            out.append(int(sample["attention_mask"].sum()))
        else:
            _, mask, _ = tokenizer.encode(sample[0], max_seq_len)
            out.append(int(sum(mask)))
    return out
