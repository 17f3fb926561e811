"""Latency-oriented inference engine — the serving path grown from the
reference's ``predict.py`` (single-text, batch-1 inference across
checkpoints; reference predict.py:104-136).

MI355X design: batch-1 BERT forward is LAUNCH-bound (hundreds of small
kernels, each ~2-20 us); the whole forward is captured once per input shape
into a hipGraph and replayed into pinned static buffers afterwards — one
launch per request. Shapes are bucketed to the next power-of-two sequence
length so a handful of graphs serve arbitrary inputs. Falls back to plain
eager forward on CPU or when capture is unavailable.

``packed=True`` is the padding-free serving path: a request of any number of
texts is cut into consecutive ranges under a token budget
(``split_by_budget``), each range becomes one packed token stream
(``pack_batch``) whose row and sequence counts are bucketed
(``serve_bucket``), and one hipGraph per bucket key ``(T, B, ms)`` is
replayed whatever the sequence boundaries are: the tile plan of tile-packed
attention is built inside the graph from the contents of ``cu_seqlens``.
The forward runs the forward-only kernel instantiations
(``ops.inference_kernels``).
"""

from __future__ import annotations

import contextlib
import copy
import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import ops
from ..data.collate import pack_batch

MAX_PLAN_SEQS = 4096   # sequences per packed stream: the plan kernel's limit


def _bucket(n: int, lo: int = 32, hi: int = 512) -> int:
    b = lo
    while b < n and b < hi:
        b *= 2
    return b


def _ceil64(n: int) -> int:
    return (int(n) + 63) // 64 * 64


def serve_ladder(limit: int) -> List[int]:
    """Packed row counts that get a graph, up to ``limit``: every multiple of
    64 up to 512, above that the values 2^k and 3*2^(k-1). Consecutive values
    above 512 are at most 3/2 apart, so bucketing adds less than T/3 rows."""
    out = list(range(64, min(512, limit) + 1, 64))
    k = 9
    while True:
        for v in (3 << (k - 1), 2 << k):   # 768, 1024, 1536, 2048, ...
            if v > limit:
                return out
            out.append(v)
        k += 1


def serve_bucket(rows: int, nseq: int, longest: int,
                 max_seq_len: int) -> Tuple[int, int, int]:
    """Graph key ``(T, B, ms)`` of a packed range with ``rows`` real tokens
    in ``nseq`` sequences, the longest of ``longest`` tokens. ``T``: the
    smallest ladder value (``serve_ladder``) that holds ``rows`` rounded up
    to 64; ``B``: the smallest power of two >= ``nseq``; ``ms``: as in the
    Trainer's ``graph_key``, ``longest`` rounded up to 128 and capped at
    ``max_seq_len``. No device involved."""
    need = max(64, _ceil64(rows))
    if need <= 512:
        T = need
    else:
        T = 1 << (need - 1).bit_length()          # 2^k >= need
        if 3 * (T // 4) >= need:                  # 3*2^(k-2) sits below it
            T = 3 * (T // 4)
    B = 1
    while B < nseq:
        B *= 2
    ms = min(int(max_seq_len), (max(int(longest), 1) + 127) // 128 * 128)
    return T, B, ms


def split_by_budget(lengths: Sequence[int], max_tokens: int,
                    max_seqs: int) -> List[Tuple[int, int]]:
    """Consecutive index ranges ``[(start, end), ...]`` over ``lengths`` in
    input order, filled greedily: a range closes only when the next text
    would take it past ``max_tokens`` real tokens or ``max_seqs`` texts.
    Texts are never sorted or reordered (a packed stream has no padding for
    sorting to save). No device involved."""
    if max_tokens <= 0 or max_tokens % 64:
        raise ValueError("split_by_budget: max_tokens must be a positive "
                         f"multiple of 64, got {max_tokens}")
    if not 1 <= max_seqs <= MAX_PLAN_SEQS:
        raise ValueError(f"split_by_budget: max_seqs must be in [1, "
                         f"{MAX_PLAN_SEQS}], got {max_seqs}")
    ranges, start, tokens = [], 0, 0
    for i, n in enumerate(lengths):
        n = int(n)
        if n < 1 or n > max_tokens:
            raise ValueError(f"split_by_budget: text {i} has {n} tokens; "
                             f"every text needs 1..{max_tokens}")
        if i > start and (tokens + n > max_tokens or i - start >= max_seqs):
            ranges.append((start, i))
            start, tokens = i, 0
        tokens += n
    if len(lengths) > start:
        ranges.append((start, len(lengths)))
    return ranges


class _Graphed:
    """One captured forward for a fixed (batch, seq) shape."""

    def __init__(self, model, batch: int, seq: int, device):
        self.ids = torch.zeros(batch, seq, dtype=torch.long, device=device)
        self.mask = torch.zeros(batch, seq, dtype=torch.long, device=device)
        self.type_ids = torch.zeros(batch, seq, dtype=torch.long, device=device)
        # warm up on a side stream, then capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(input_ids=self.ids, attention_mask=self.mask,
                      token_type_ids=self.type_ids)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            out = model(input_ids=self.ids, attention_mask=self.mask,
                        token_type_ids=self.type_ids)
            self.logits = out.logits

    def run(self, ids, mask, type_ids):
        self.ids.copy_(ids, non_blocking=True)
        self.mask.copy_(mask, non_blocking=True)
        self.type_ids.copy_(type_ids, non_blocking=True)
        self.graph.replay()
        return self.logits


class _PackedInputs:
    """Inputs of one packed forward in ONE int64 buffer, so that a request
    costs one host-to-device copy: ids | type_ids | position_ids (T each),
    then cu_seqlens (B + 1 int32, two per word)."""

    def __init__(self, T: int, B: int, device, pin: bool = False):
        self.T, self.B = T, B
        self.buf = torch.zeros(3 * T + (B + 2) // 2, dtype=torch.long,
                               device=device, pin_memory=pin)
        self.ids = self.buf[:T]
        self.type_ids = self.buf[T:2 * T]
        self.position_ids = self.buf[2 * T:3 * T]
        self.cu_seqlens = self.buf[3 * T:].view(torch.int32)[:B + 1]

    def fill(self, packed):
        self.ids.copy_(packed["input_ids"])
        self.type_ids.copy_(packed["token_type_ids"])
        self.position_ids.copy_(packed["position_ids"])
        self.cu_seqlens.copy_(packed["cu_seqlens"])


class _GraphedPacked:
    """One captured packed forward for a key ``(T, B, ms)``: static ids,
    type_ids, position_ids, cu_seqlens and logits. Captured with
    ``max_seqlen = ms``; the tile-plan kernel sits inside the capture and
    reads only the contents of cu_seqlens, so the graph serves any sequence
    boundaries of its key. As _Graphed: two warm-up runs on a side stream,
    then the capture, into the engine's one memory pool."""

    def __init__(self, forward, key, device, pool):
        T, B, ms = key
        self.static = _PackedInputs(T, B, device)
        self.stage = _PackedInputs(T, B, "cpu", pin=True)
        self.staged = None  # event: the last copy out of ``stage`` is done
        # valid boundaries for the warm-up and the capture: B empty sequences
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                forward(self.static, ms)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, pool=pool):
            self.logits = forward(self.static, ms)

    def run(self, packed):
        if self.staged is not None:
            self.staged.synchronize()  # the pinned buffer is free again
        self.stage.fill(packed)
        self.static.buf.copy_(self.stage.buf, non_blocking=True)
        self.staged = torch.cuda.Event()
        self.staged.record()
        self.graph.replay()
        return self.logits


class InferenceEngine:
    """``engine = InferenceEngine(model, tokenizer); engine.predict(texts)``.

    On GPU, each (bucketed) input shape gets a hipGraph-captured forward;
    on CPU it is a plain no-grad forward.

    ``packed=True``: padding-free serving (see the module docstring) on a
    copy of the model whose config has ``attn_tile_pack=True``. A request
    of any size is cut into ranges of at most ``max_tokens`` real tokens and
    ``max_seqs`` texts; at most ``max_graphs`` keys get a graph, further
    keys run eager; ``infer_kernels`` selects the forward-only kernels.
    ``cls_only_last_layer=True`` (packed only) also sets that config field
    on the copy: the last encoder layer computes the first-token rows only.
    ``graph_stats`` counts packed forwards: ``captured`` graphs, and each
    forward under ``replayed`` or ``eager`` (the forward that triggers a
    capture is replayed from the new graph and counts as replayed; the
    warm-up runs of a capture are not counted). ``forward_tensors`` and
    ``latency_bench`` keep their padded meaning in either mode.
    """

    def __init__(self, model, tokenizer=None, device: Optional[str] = None,
                 max_seq_len: int = 128, use_graph: bool = True,
                 packed: bool = False, max_tokens: int = 4096,
                 max_seqs: int = 1024, max_graphs: int = 32,
                 infer_kernels: bool = True,
                 cls_only_last_layer: bool = False):
        self.device = torch.device(
            device or ("cuda" if torch.cuda.is_available() else "cpu"))
        self.packed = bool(packed)
        if cls_only_last_layer and not self.packed:
            raise ValueError("InferenceEngine: cls_only_last_layer needs "
                             "packed=True (padded batches have no packed "
                             "stream to take the first-token rows from)")
        if self.packed:
            if max_tokens % 64 or max_tokens < max_seq_len:
                raise ValueError("InferenceEngine: max_tokens must be a "
                                 "multiple of 64 and at least max_seq_len")
            if not 1 <= max_seqs <= MAX_PLAN_SEQS:
                raise ValueError("InferenceEngine: max_seqs must be in "
                                 f"[1, {MAX_PLAN_SEQS}]")
            if max_graphs < 0:
                raise ValueError("InferenceEngine: max_graphs must be >= 0")
            # the engine's own copy: the caller's model keeps its config
            model = copy.deepcopy(model)
            old = model.config
            cfg = dataclasses.replace(
                old, attn_tile_pack=True,
                cls_only_last_layer=bool(cls_only_last_layer))
            for m in model.modules():
                for name in ("cfg", "config"):
                    if getattr(m, name, None) is old:
                        setattr(m, name, cfg)
        self.model = model.to(self.device).eval()
        self.tokenizer = tokenizer
        self.max_seq_len = max_seq_len
        self.use_graph = use_graph and self.device.type == "cuda"
        self._graphs: Dict[Tuple[int, int], _Graphed] = {}
        self.max_tokens = max_tokens
        self.max_seqs = max_seqs
        self.max_graphs = max_graphs
        self.infer_kernels = bool(infer_kernels)
        self._packed_graphs: Dict[Tuple[int, int, int], _GraphedPacked] = {}
        self._graph_pool = None
        self._eager_noted = False
        self.graph_stats = {"captured": 0, "replayed": 0, "eager": 0}

    # ---- padding-free serving (packed=True) ------------------------------

    def _packed_forward(self, inp: _PackedInputs, ms: int) -> torch.Tensor:
        ctx = ops.inference_kernels() if self.infer_kernels \
            else contextlib.nullcontext()
        with ctx:
            out = self.model(input_ids=inp.ids, token_type_ids=inp.type_ids,
                             position_ids=inp.position_ids,
                             cu_seqlens=inp.cu_seqlens, max_seqlen=ms)
        return out.logits

    def _capture_packed(self, key) -> _GraphedPacked:
        if self._graph_pool is None:
            self._graph_pool = torch.cuda.graph_pool_handle()
        g = _GraphedPacked(self._packed_forward, key, self.device,
                           self._graph_pool)
        self._packed_graphs[key] = g
        self.graph_stats["captured"] += 1
        return g

    @torch.no_grad()
    def warmup(self, keys) -> None:
        """Capture the graphs of the given ``(T, B, ms)`` keys (the values of
        ``serve_bucket``) ahead of traffic. Keys past ``max_graphs`` are
        left to run eager."""
        assert self.packed, "warmup(keys) is for packed=True"
        if not self.use_graph:
            return
        for key in keys:
            key = tuple(int(k) for k in key)
            if key not in self._packed_graphs \
                    and len(self._packed_graphs) < self.max_graphs:
                self._capture_packed(key)

    def _run_range(self, seqs) -> torch.Tensor:
        """Logits [n, C] (a fresh tensor) of one range of (ids, type_ids)."""
        n = len(seqs)
        lens = [len(ids) for ids, _ in seqs]
        longest = max(lens)
        key = serve_bucket(sum(lens), n, longest, self.max_seq_len)
        T, B, ms = key
        cfg = self.model.config
        ids = torch.full((n, longest), cfg.pad_token_id, dtype=torch.long)
        types = torch.zeros(n, longest, dtype=torch.long)
        mask = torch.zeros(n, longest, dtype=torch.long)
        for i, (a, t) in enumerate(seqs):
            ids[i, :lens[i]] = torch.as_tensor(a, dtype=torch.long)
            types[i, :lens[i]] = torch.as_tensor(t, dtype=torch.long)
            mask[i, :lens[i]] = 1
        packed = pack_batch(
            {"input_ids": ids, "attention_mask": mask,
             "token_type_ids": types,
             "label": torch.zeros(n, dtype=torch.long)},
            pad_token_id=cfg.pad_token_id,
            roberta=cfg.model_type == "roberta", total_rows=T,
            seq_multiple=B)
        if self.use_graph:
            g = self._packed_graphs.get(key)
            if g is None and len(self._packed_graphs) < self.max_graphs:
                g = self._capture_packed(key)
            if g is not None:
                self.graph_stats["replayed"] += 1
                return g.run(packed)[:n].clone()
            if not self._eager_noted:
                self._eager_noted = True
                print(f"[pdnlp] InferenceEngine: {self.max_graphs} graphs "
                      f"captured; key {key} and further new keys run eager",
                      flush=True)
        inp = _PackedInputs(T, B, "cpu")
        inp.fill(packed)
        if self.device.type != "cpu":
            dev = _PackedInputs(T, B, self.device)
            dev.buf.copy_(inp.buf)
            inp = dev
        self.graph_stats["eager"] += 1
        return self._packed_forward(inp, ms)[:n]

    @torch.no_grad()
    def forward_sequences(self, seqs) -> torch.Tensor:
        """Logits [N, C] on the engine's device, in input order, for already
        tokenized texts: ``seqs`` is a list of ``(ids, type_ids)`` lists of
        1..max_seq_len real tokens each (no padding)."""
        assert self.packed, "forward_sequences needs packed=True"
        seqs = list(seqs)
        lens = [len(ids) for ids, _ in seqs]
        if any(n < 1 or n > self.max_seq_len for n in lens):
            raise ValueError("forward_sequences: every text needs 1.."
                             f"{self.max_seq_len} tokens")
        outs = [self._run_range(seqs[a:b]) for a, b in
                split_by_budget(lens, self.max_tokens, self.max_seqs)]
        if not outs:
            return torch.empty(0, self.model.config.num_labels,
                               device=self.device)
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _tokenize(self, texts: List[str]):
        assert self.tokenizer is not None, "predict(texts) needs a tokenizer"
        seqs = []
        for t in texts:
            ids, mask, type_ids = self.tokenizer.encode(t, self.max_seq_len)
            n = int(sum(mask))
            seqs.append((ids[:n], type_ids[:n]))
        return seqs

    @torch.no_grad()
    def predict_logits(self, texts: List[str]) -> torch.Tensor:
        """float32 logits [N, C] on the host for any number of texts."""
        if self.packed:
            return self.forward_sequences(self._tokenize(texts)).float().cpu()
        ids, mask, type_ids = self._encode(texts)
        return self.forward_tensors(ids, mask, type_ids).float().cpu()

    # ---- padded serving ----------------------------------------------------

    def _encode(self, texts: List[str]):
        assert self.tokenizer is not None, "predict(texts) needs a tokenizer"
        ids_l, mask_l, type_l = [], [], []
        maxlen = 0
        enc = []
        for t in texts:
            ids, mask, type_ids = self.tokenizer.encode(t, self.max_seq_len)
            n = int(sum(mask))
            maxlen = max(maxlen, n)
            enc.append((ids, mask, type_ids))
        seq = _bucket(maxlen, hi=self.max_seq_len)
        for ids, mask, type_ids in enc:
            ids_l.append(ids[:seq])
            mask_l.append(mask[:seq])
            type_l.append(type_ids[:seq])
        return (torch.tensor(ids_l, dtype=torch.long),
                torch.tensor(mask_l, dtype=torch.long),
                torch.tensor(type_l, dtype=torch.long))

    @torch.no_grad()
    def forward_tensors(self, ids, mask, type_ids,
                        clone: bool = True) -> torch.Tensor:
        """Logits for already-tokenized fixed-shape inputs.

        On the graph path the result is cloned out of the static replay
        buffer by default (the next ``replay()`` overwrites it); pass
        ``clone=False`` for zero-copy access when the caller consumes the
        tensor before issuing another request (latency_bench does)."""
        ids = ids.to(self.device, non_blocking=True)
        mask = mask.to(self.device, non_blocking=True)
        type_ids = type_ids.to(self.device, non_blocking=True)
        if self.use_graph:
            key = (ids.shape[0], ids.shape[1])
            g = self._graphs.get(key)
            if g is None:
                g = _Graphed(self.model, *key, device=self.device)
                self._graphs[key] = g
            out = g.run(ids, mask, type_ids)
            return out.clone() if clone else out
        out = self.model(input_ids=ids, attention_mask=mask,
                         token_type_ids=type_ids)
        return out.logits

    @torch.no_grad()
    def predict(self, texts: List[str], id2label: Optional[dict] = None):
        if self.packed:   # any number of texts, cut into ranges
            pred = self.predict_logits(texts).argmax(-1).tolist()
        else:
            ids, mask, type_ids = self._encode(texts)
            logits = self.forward_tensors(ids, mask, type_ids)
            pred = logits.float().argmax(-1).cpu().tolist()
        if id2label:
            return [id2label[int(p)] for p in pred]
        return pred

    @torch.no_grad()
    def latency_bench(self, batch: int = 1, seq: Optional[int] = None,
                      iters: int = 100, warmup: int = 20) -> dict:
        """Measure request latency for a fixed shape; returns ms stats."""
        import time
        seq = seq or self.max_seq_len
        vocab = getattr(self.model.config, "vocab_size", 21128)
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(106, vocab, (batch, seq), generator=g)
        mask = torch.ones_like(ids)
        type_ids = torch.zeros_like(ids)
        lat = []
        for i in range(warmup + iters):
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.forward_tensors(ids, mask, type_ids, clone=False)
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                lat.append(dt)
        lat.sort()
        return {
            "batch": batch, "seq": seq, "iters": iters,
            "p50_ms": round(lat[len(lat) // 2], 3),
            "p99_ms": round(lat[int(len(lat) * 0.99) - 1], 3),
            "mean_ms": round(sum(lat) / len(lat), 3),
            "graph": self.use_graph,
        }
