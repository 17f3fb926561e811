"""Batch collation: text → fixed-length int64 tensors.

Reference equivalent: ``Collate.collate_fn`` (single-gpu-cls.py:44-84) runs
``tokenizer.encode_plus`` per sample in a Python loop — the CPU-side hot spot
SURVEY.md §2.2 flags. Here encoding happens per sample too (tokenization is
inherently per-text) but tensorization is one ``torch.tensor`` call per batch,
and pre-tokenized dict samples (SyntheticClsDataset) pass through with a
single stack.
"""

from __future__ import annotations

import torch

# sequence-count granule of token-budget batches (``--max-tokens``): the
# count is rounded up to it with empty sequences, so an epoch has two or
# three hipGraph keys instead of one per distinct count
SEQ_MULTIPLE = 32
IGNORE_LABEL = -100  # label of an empty sequence; the loss skips the row


def pack_batch(batch, multiple: int = 64, label_key: str = "label",
               pad_token_id: int = 0, roberta: bool = False,
               total_rows=None, seq_multiple=None):
    """Padded batch dict ([B, S] ids/mask/types + labels) -> packed token
    stream for the padding-free path (``--unpad``).

    Real tokens (``attention_mask == 1``, which must be a prefix of ones in
    every row) are concatenated row after row; the stream is padded to a
    multiple of ``multiple`` rows (the GEMM row granule) with
    ``pad_token_id`` / type 0 / position 0. ``cu_seqlens`` [B+1] int32 holds
    the sequence boundaries, ``max_seqlen`` the longest sequence (a host int,
    so the attention launch needs no device sync). Position ids restart per
    sequence; RoBERTa's are ``pad_token_id + 1 + i`` as on the padded path.

    Fixed shapes (token-budget batching): ``total_rows=N`` pads the stream
    to exactly N rows and raises ``ValueError`` when the batch holds more
    real tokens. ``seq_multiple=m`` rounds the sequence count up to a
    multiple of m with EMPTY sequences: ``cu_seqlens`` repeats the total for
    them (length 0: the attention kernels exit at once) and their labels
    are -100 (the loss ignores them). ``max_seqlen`` stays the longest real
    sequence; ``num_seqs`` is the count of real sequences (a host int).
    """
    mask = batch["attention_mask"]
    B, S = mask.shape
    lens = mask.sum(-1)
    prefix = (torch.arange(S)[None, :] < lens[:, None]).to(mask.dtype)
    if not torch.equal(mask, prefix):
        raise ValueError("pack_batch: every attention_mask row must be a "
                         "prefix of ones followed by zeros")
    if int(lens.min()) < 1:
        raise ValueError("pack_batch: every sequence needs >= 1 real token")
    Bp = B if not seq_multiple else \
        (B + seq_multiple - 1) // seq_multiple * seq_multiple
    cu = torch.zeros(Bp + 1, dtype=torch.int32)
    cu[1:B + 1] = lens.cumsum(0)
    total = int(cu[B])
    cu[B + 1:] = total
    if total_rows is None:
        T = (total + multiple - 1) // multiple * multiple
    else:
        T = int(total_rows)
        if total > T:
            raise ValueError(f"pack_batch: {total} real tokens do not fit "
                             f"into total_rows={T}")
    labels = batch[label_key]
    if Bp > B:
        labels = torch.cat([labels, labels.new_full((Bp - B,), IGNORE_LABEL)])
    keep = mask.bool()
    pos = torch.arange(S)[None, :].expand(B, S)[keep]
    if roberta:
        pos = pos + pad_token_id + 1
    input_ids = torch.full((T,), pad_token_id, dtype=torch.long)
    token_type_ids = torch.zeros(T, dtype=torch.long)
    position_ids = torch.zeros(T, dtype=torch.long)
    input_ids[:total] = batch["input_ids"][keep]
    token_type_ids[:total] = batch["token_type_ids"][keep]
    position_ids[:total] = pos
    return {
        "input_ids": input_ids,
        "token_type_ids": token_type_ids,
        "position_ids": position_ids,
        "cu_seqlens": cu,
        "max_seqlen": int(lens.max()),
        "num_seqs": B,
        label_key: labels,
    }


class Collate:
    def __init__(self, tokenizer, max_seq_len: int = 128,
                 label_key: str = "label", unpad: bool = False,
                 pad_token_id: int = 0, roberta: bool = False,
                 max_tokens=None, seq_multiple=None):
        self.tokenizer = tokenizer
        self.max_seq_len = max_seq_len
        self.label_key = label_key  # HF-Trainer mode uses "labels"
        self.unpad = unpad          # emit the packed stream (pack_batch)
        self.pad_token_id = pad_token_id
        self.roberta = roberta
        # fixed-shape packed batches (token-budget batching); unpad only
        self.max_tokens = max_tokens or None
        self.seq_multiple = seq_multiple or None

    def __call__(self, batch):
        out = self.collate_fn(batch)
        if self.unpad:
            out = pack_batch(out, label_key=self.label_key,
                             pad_token_id=self.pad_token_id,
                             roberta=self.roberta,
                             total_rows=self.max_tokens,
                             seq_multiple=self.seq_multiple)
        return out

    def collate_fn(self, batch):
        if isinstance(batch[0], dict):  # pre-tokenized
            out = {
                "input_ids": torch.stack([b["input_ids"] for b in batch]),
                "attention_mask": torch.stack([b["attention_mask"] for b in batch]),
                "token_type_ids": torch.stack([b["token_type_ids"] for b in batch]),
                self.label_key: torch.stack([b.get("label", b.get("labels")) for b in batch]),
            }
            return out
        ids_l, mask_l, type_l, labels = [], [], [], []
        for text, label in batch:
            ids, mask, type_ids = self.tokenizer.encode(text, self.max_seq_len)
            ids_l.append(ids)
            mask_l.append(mask)
            type_l.append(type_ids)
            labels.append(int(label))
        return {
            "input_ids": torch.tensor(ids_l, dtype=torch.long),
            "attention_mask": torch.tensor(mask_l, dtype=torch.long),
            "token_type_ids": torch.tensor(type_l, dtype=torch.long),
            self.label_key: torch.tensor(labels, dtype=torch.long),
        }
