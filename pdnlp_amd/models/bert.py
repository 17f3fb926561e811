"""BERT / RoBERTa sequence classifiers with HF checkpoint layout, computed
through pdnlp_amd.ops (hand-written CDNA4 kernels on GPU).

State-dict keys match HF ``BertForSequenceClassification`` exactly
(``bert.embeddings.word_embeddings.weight`` …
``bert.encoder.layer.N.attention.self.query.weight`` … ``classifier.weight``)
so checkpoints interchange with the reference workflow
(BASELINE.json: "the same HF BertForSequenceClassification checkpoint
layout"; reference model build at multi-gpu-distributed-cls.py:336-338).

Parameters live in standard ``nn.Linear``/``nn.Embedding``/``nn.LayerNorm``
containers (for the key names); forward bypasses their ``forward`` and calls
the fused ops directly: embedding+LN (K1), fused-QKV GEMM (K2), attention
(K3-K5), GEMM+bias+GELU (K7), GEMM + bias+dropout+residual+LN epilogues
(K6/K8), pooler/classifier (K9), CE (K10).
"""

from __future__ import annotations


from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..config import BertConfig


@dataclass
class SequenceClassifierOutput:
    loss: Optional[torch.Tensor]
    logits: torch.Tensor

    def __getitem__(self, i):  # reference indexes output[1] for logits
        return (self.loss, self.logits)[i]

    def __iter__(self):
        return iter((self.loss, self.logits))


class BertEmbeddings(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.cfg = cfg
        self.word_embeddings = nn.Embedding(cfg.vocab_size, cfg.hidden_size,
                                            padding_idx=cfg.pad_token_id)
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings,
                                                cfg.hidden_size)
        self.token_type_embeddings = nn.Embedding(cfg.type_vocab_size,
                                                  cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.register_buffer(
            "position_ids",
            torch.arange(cfg.max_position_embeddings).unsqueeze(0),
            persistent=False)

    def forward(self, input_ids, token_type_ids, training: bool,
                position_ids=None):
        # a packed stream brings its own per-sequence position_ids
        if position_ids is not None:
            pass
        elif self.cfg.model_type == "roberta":
            # HF roberta: position ids from non-pad positions, offset by pad id
            mask = (input_ids != self.cfg.pad_token_id).long()
            position_ids = mask.cumsum(-1) * mask + self.cfg.pad_token_id
        else:
            B, S = input_ids.shape
            position_ids = self.position_ids[:, :S].expand(B, S)
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        h = ops.embedding_layernorm(
            input_ids, token_type_ids, position_ids,
            self.word_embeddings.weight, self.position_embeddings.weight,
            self.token_type_embeddings.weight,
            self.LayerNorm.weight, self.LayerNorm.bias, self.cfg.layer_norm_eps)
        return ops.dropout(h, self.cfg.hidden_dropout_prob, training)


class BertSelfAttention(nn.Module):
    """Q/K/V projections stored as ONE fused [3H, H] parameter (single MFMA
    GEMM per layer, no per-step torch.cat, gradients land fused) while the
    state dict still presents the HF keys ``query.weight``/``key.bias``/…
    via save/load hooks."""

    def __init__(self, cfg: BertConfig):
        super().__init__()
        H = cfg.hidden_size
        self.hidden = H
        self.qkv_weight = nn.Parameter(torch.empty(3 * H, H))
        self.qkv_bias = nn.Parameter(torch.zeros(3 * H))
        nn.init.normal_(self.qkv_weight, std=cfg.initializer_range)
        self._register_state_dict_hook(_qkv_save_hook)
        self._register_load_state_dict_pre_hook(self._qkv_load_hook,
                                                with_module=False)

    def _qkv_load_hook(self, state_dict, prefix, *args):
        H = self.hidden
        names = [("query", 0), ("key", 1), ("value", 2)]
        if prefix + "qkv_weight" in state_dict:
            return
        ws, bs = [], []
        for name, _ in names:
            wk, bk = prefix + name + ".weight", prefix + name + ".bias"
            if wk not in state_dict:
                return  # let load_state_dict report what is missing
            ws.append(state_dict.pop(wk))
            bs.append(state_dict.pop(bk))
        state_dict[prefix + "qkv_weight"] = torch.cat(ws, dim=0)
        state_dict[prefix + "qkv_bias"] = torch.cat(bs, dim=0)


def _qkv_save_hook(module, state_dict, prefix, local_metadata):
    H = module.hidden
    w = state_dict.pop(prefix + "qkv_weight")
    b = state_dict.pop(prefix + "qkv_bias")
    for i, name in enumerate(("query", "key", "value")):
        state_dict[prefix + name + ".weight"] = w[i * H:(i + 1) * H]
        state_dict[prefix + name + ".bias"] = b[i * H:(i + 1) * H]
    return state_dict


class BertSelfOutput(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class BertAttention(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.self = BertSelfAttention(cfg)
        self.output = BertSelfOutput(cfg)


class BertIntermediate(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.intermediate_size)


class BertOutput(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.dense = nn.Linear(cfg.intermediate_size, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class BertLayer(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.cfg = cfg
        self.attention = BertAttention(cfg)
        self.intermediate = BertIntermediate(cfg)
        self.output = BertOutput(cfg)

    def forward(self, h: torch.Tensor, attn_mask: Optional[torch.Tensor],
                training: bool, cu_seqlens: Optional[torch.Tensor] = None,
                max_seqlen: Optional[int] = None,
                attn_plan=None,
                cls_rows: Optional[int] = None) -> torch.Tensor:
        """``cls_rows`` (packed streams only; the last layer under
        ``cfg.cls_only_last_layer``): after the QKV projection over all T
        rows, everything runs on the ``cls_rows`` first-token rows alone and
        the layer returns [1, cls_rows, H] in place of [1, T, H]."""
        cfg = self.cfg
        nh = cfg.num_attention_heads
        a = self.attention.self
        # fused QKV projection: one [H, 3H] GEMM (K2), then fused flash
        # attention straight on the packed projection (K3-K5 + K16).
        # linear_fork routes the residual stream through the projection
        # node so the residual-grad fan-in add fuses into the dX GEMM
        # epilogue (ops/functional.py _LinearForkHipFn)
        qkv, h_res = ops.linear_fork(h, a.qkv_weight, a.qkv_bias)
        if cls_rows is not None:
            # K and V need every row, the query side only the first token
            # of each sequence: one attention row per sequence, and the
            # residual gathered from the same rows. The gather's backward
            # scatters into the dpass of the projection node above.
            ctx = ops.cls_attention(
                qkv[0], cu_seqlens, cls_rows, max_seqlen, nh,
                cfg.attention_probs_dropout_prob, training).unsqueeze(0)
            h_res = _first_token_rows(h_res, cu_seqlens, cls_rows)
        elif cu_seqlens is not None:
            # packed stream h [1, T, H]: sequence-boundary-aware attention
            ctx = ops.attention_varlen(
                qkv[0], cu_seqlens, max_seqlen, nh,
                cfg.attention_probs_dropout_prob, training,
                plan=attn_plan).unsqueeze(0)
        else:
            ctx = ops.attention_packed(
                qkv, attn_mask, nh, cfg.attention_probs_dropout_prob,
                training)
        # attention output projection + fused bias/dropout/residual/LN (K6);
        # the bias gradient comes out of the projection's dW GEMM
        ao = self.attention.output
        h = ops.linear_bias_dropout_residual_layernorm(
            ctx, ao.dense.weight, ao.dense.bias, h_res, ao.LayerNorm.weight,
            ao.LayerNorm.bias, cfg.hidden_dropout_prob, training,
            cfg.layer_norm_eps)
        # FFN: GEMM + fused GELU (K7), GEMM + fused epilogue (K8)
        inter, h_res2 = ops.linear_fork(h, self.intermediate.dense.weight,
                                        self.intermediate.dense.bias,
                                        act="gelu")
        h = ops.linear_bias_dropout_residual_layernorm(
            inter, self.output.dense.weight, self.output.dense.bias, h_res2,
            self.output.LayerNorm.weight, self.output.LayerNorm.bias,
            cfg.hidden_dropout_prob, training, cfg.layer_norm_eps)
        return h


class BertEncoder(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.layer = nn.ModuleList(BertLayer(cfg)
                                   for _ in range(cfg.num_hidden_layers))


class BertPooler(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.hidden_size)


class BertModel(nn.Module):
    def __init__(self, cfg: BertConfig, add_pooler: bool = True):
        super().__init__()
        self.cfg = cfg
        self.embeddings = BertEmbeddings(cfg)
        self.encoder = BertEncoder(cfg)
        self.pooler = BertPooler(cfg) if add_pooler else None
        self._grad_ckpt = False
        self._ckpt_cpu_offload = False

    def forward(self, input_ids, attention_mask=None, token_type_ids=None,
                cu_seqlens=None, max_seqlen=None, position_ids=None):
        """Padded: ``input_ids`` [B, S] + ``attention_mask``. Packed
        (``cu_seqlens`` given): ``input_ids``/``token_type_ids``/
        ``position_ids`` are the 1-D token stream [T] of ``pack_batch``,
        ``attention_mask`` is ignored, and the hidden states come back as
        the packed [1, T, H] stream. With ``cfg.cls_only_last_layer`` (and
        ``cls_only_rows`` not None) the last layer computes the first-token
        rows only, and the hidden states come back as that first-token
        stream [1, R, H] instead: row i < B belongs to sequence i, rows of
        empty sequences and rows B..R hold finite values nothing reads."""
        training = self.training
        attn_plan = None
        cls_rows = None
        if cu_seqlens is not None:
            assert input_ids.dim() == 1 and position_ids is not None \
                and max_seqlen is not None, \
                "packed input needs 1-D input_ids, position_ids, max_seqlen"
            tt = token_type_ids.unsqueeze(0) \
                if token_type_ids is not None else None
            h = self.embeddings(input_ids.unsqueeze(0), tt, training,
                                position_ids.unsqueeze(0))
            addmask = None
            # tile-packed attention: one plan per forward, shared by every
            # layer; a function of the contents of cu_seqlens alone
            if self.cfg.attn_tile_pack:
                attn_plan = ops.varlen_attention_plan(cu_seqlens,
                                                      input_ids.numel())
            cls_rows = cls_only_rows(self.cfg, input_ids.numel(),
                                     cu_seqlens.numel() - 1)
        else:
            if attention_mask is None:
                attention_mask = torch.ones_like(input_ids)
            # additive mask in compute dtype: 0 keep / -10000 drop (HF
            # convention)
            dtype = self.embeddings.word_embeddings.weight.dtype
            addmask = (1.0 - attention_mask[:, None, None, :].to(dtype)) \
                * -10000.0
            h = self.embeddings(input_ids, token_type_ids, training)
        last = len(self.encoder.layer) - 1
        for n, layer in enumerate(self.encoder.layer):
            rows = cls_rows if n == last else None
            if self._grad_ckpt and training:
                h = _checkpoint_layer(layer, h, addmask, training,
                                      self._ckpt_cpu_offload, cu_seqlens,
                                      max_seqlen, attn_plan, rows)
            else:
                h = layer(h, addmask, training, cu_seqlens, max_seqlen,
                          attn_plan, rows)
        if cls_rows is not None:
            # h is already the first-token stream: no second gather
            cls = h[0, :cu_seqlens.numel() - 1]
        elif cu_seqlens is not None:
            cls = _packed_cls(h, cu_seqlens)
        else:
            cls = h[:, 0]
        pooled = None
        if self.pooler is not None:
            pooled = ops.linear(cls, self.pooler.dense.weight,
                                self.pooler.dense.bias, act="tanh")
        return h, pooled

    def gradient_checkpointing_enable(self, cpu_offload: bool = False):
        self._grad_ckpt = True
        self._ckpt_cpu_offload = cpu_offload

    def gradient_checkpointing_disable(self):
        self._grad_ckpt = False


def _packed_cls(h, cu_seqlens):
    """[B, H] first-token rows of a packed hidden stream h [1, T, H]. An
    empty sequence (``pack_batch(seq_multiple=...)``) starts at the total,
    which is T when the stream is filled exactly: the clamp makes it gather
    some finite row, which the loss ignores (label -100)."""
    idx = cu_seqlens[:-1].long().clamp(max=h.shape[1] - 1)
    return h[0].index_select(0, idx)


def cls_only_rows(cfg, total_rows: int, num_seqs: int) -> Optional[int]:
    """Row count R = ceil64(B) of the last layer's first-token stream under
    ``cfg.cls_only_last_layer``, or None when the layer runs as usual: the
    option is off, or R >= T and there is nothing to save (one text in a
    64-row stream). Host integers only and a function of (T, B), so every
    batch of a graph key decides the same way. A multiple of 64 keeps the
    first-party GEMMs and the deferred-bias path engaged."""
    if not getattr(cfg, "cls_only_last_layer", False):
        return None
    rows = -(-int(num_seqs) // 64) * 64
    return rows if rows < int(total_rows) else None


def _first_token_rows(h, cu_seqlens, rows: int):
    """[1, rows, H] first-token rows of a packed stream h [1, T, H], with no
    host sync. Clamped as ``_packed_cls`` clamps; the rows past the batch
    gather row 0. Those and the rows of empty sequences are real, finite
    rows whose outputs nothing reads, so their gradients are exactly zero."""
    idx = torch.nn.functional.pad(cu_seqlens[:-1].long(),
                                  (0, rows - (cu_seqlens.numel() - 1)))
    return h[0].index_select(0, idx.clamp(max=h.shape[1] - 1)).unsqueeze(0)


def _cls_loss(logits, labels, cu_seqlens):
    """Packed batches may carry empty sequences labelled -100; padded
    batches take the plain mean."""
    if labels is None:
        return None
    if cu_seqlens is not None:
        return ops.cross_entropy(logits, labels, ignore_index=-100)
    return ops.cross_entropy(logits, labels)


def _checkpoint_layer(layer, h, mask, training, cpu_offload,
                      cu_seqlens=None, max_seqlen=None, attn_plan=None,
                      cls_rows=None):
    """Activation checkpointing (deepspeed-capability equivalent,
    reference config: multi-gpu-deepspeed-cls.py:240-244), optional CPU
    offload of the saved input over PCIe."""
    import torch.utils.checkpoint as cp
    if cpu_offload:
        ctx = torch.autograd.graph.save_on_cpu(pin_memory=True)
        with ctx:
            return cp.checkpoint(layer, h, mask, training, cu_seqlens,
                                 max_seqlen, attn_plan, cls_rows,
                                 use_reentrant=False)
    return cp.checkpoint(layer, h, mask, training, cu_seqlens, max_seqlen,
                         attn_plan, cls_rows, use_reentrant=False)


class BertForSequenceClassification(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.cfg = self.config = cfg
        self.bert = BertModel(cfg, add_pooler=True)
        self.dropout = nn.Dropout(cfg.hidden_dropout_prob)
        self.classifier = nn.Linear(cfg.hidden_size, cfg.num_labels)
        self.apply(_init_weights(cfg))

    def forward(self, input_ids, attention_mask=None, token_type_ids=None,
                labels=None, cu_seqlens=None, max_seqlen=None,
                position_ids=None):
        _, pooled = self.bert(input_ids, attention_mask, token_type_ids,
                              cu_seqlens, max_seqlen, position_ids)
        pooled = ops.dropout(pooled, self.cfg.hidden_dropout_prob, self.training)
        logits = ops.linear(pooled, self.classifier.weight, self.classifier.bias)
        loss = _cls_loss(logits, labels, cu_seqlens)
        return SequenceClassifierOutput(loss=loss, logits=logits)

    def gradient_checkpointing_enable(self, cpu_offload: bool = False):
        self.bert.gradient_checkpointing_enable(cpu_offload)

    @staticmethod
    def from_pretrained(path: str, cfg: Optional[BertConfig] = None):
        return _from_pretrained(BertForSequenceClassification, path, cfg)


class RobertaClassificationHead(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.out_proj = nn.Linear(cfg.hidden_size, cfg.num_labels)


class RobertaForSequenceClassification(nn.Module):
    """RoBERTa-base variant (BASELINE.json config 5): HF ``roberta.*`` keys,
    no pooler, CLS-token classification head."""

    def __init__(self, cfg: Optional[BertConfig] = None):
        super().__init__()
        cfg = cfg or BertConfig.roberta_base()
        assert cfg.model_type == "roberta"
        self.cfg = self.config = cfg
        self.roberta = BertModel(cfg, add_pooler=False)
        self.classifier = RobertaClassificationHead(cfg)
        self.apply(_init_weights(cfg))

    def forward(self, input_ids, attention_mask=None, token_type_ids=None,
                labels=None, cu_seqlens=None, max_seqlen=None,
                position_ids=None):
        h, _ = self.roberta(input_ids, attention_mask, token_type_ids,
                            cu_seqlens, max_seqlen, position_ids)
        if cu_seqlens is None:
            cls = h[:, 0]
        elif cls_only_rows(self.cfg, input_ids.numel(),
                           cu_seqlens.numel() - 1) is not None:
            cls = h[0, :cu_seqlens.numel() - 1]  # h: first-token stream
        else:
            cls = _packed_cls(h, cu_seqlens)
        x = ops.dropout(cls, self.cfg.hidden_dropout_prob, self.training)
        x = ops.linear(x, self.classifier.dense.weight,
                       self.classifier.dense.bias, act="tanh")
        x = ops.dropout(x, self.cfg.hidden_dropout_prob, self.training)
        logits = ops.linear(x, self.classifier.out_proj.weight,
                            self.classifier.out_proj.bias)
        loss = _cls_loss(logits, labels, cu_seqlens)
        return SequenceClassifierOutput(loss=loss, logits=logits)

    def gradient_checkpointing_enable(self, cpu_offload: bool = False):
        self.roberta.gradient_checkpointing_enable(cpu_offload)

    @staticmethod
    def from_pretrained(path: str, cfg: Optional[BertConfig] = None):
        return _from_pretrained(RobertaForSequenceClassification, path,
                                cfg or BertConfig.roberta_base())


def _init_weights(cfg: BertConfig):
    def fn(m):
        if isinstance(m, nn.Linear):
            m.weight.data.normal_(0.0, cfg.initializer_range)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.Embedding):
            m.weight.data.normal_(0.0, cfg.initializer_range)
            if m.padding_idx is not None:
                m.weight.data[m.padding_idx].zero_()
        elif isinstance(m, nn.LayerNorm):
            m.weight.data.fill_(1.0)
            m.bias.data.zero_()
    return fn


def _from_pretrained(cls, path: str, cfg: Optional[BertConfig]):
    """Load from an HF checkpoint dir (config.json + pytorch_model.bin /
    model.safetensors) or a bare state-dict .pt file."""
    import json
    import os

    if os.path.isdir(path):
        cfg_file = os.path.join(path, "config.json")
        if cfg is None and os.path.isfile(cfg_file):
            with open(cfg_file) as f:
                cfg = BertConfig.from_dict(json.load(f))
        model = cls(cfg or BertConfig())
        sd = None
        st = os.path.join(path, "model.safetensors")
        pt = os.path.join(path, "pytorch_model.bin")
        if os.path.isfile(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        elif os.path.isfile(pt):
            sd = torch.load(pt, map_location="cpu", weights_only=False)
        if sd is not None:
            from ..utils.checkpoint import strip_module_prefix
            missing, unexpected = model.load_state_dict(
                strip_module_prefix(sd), strict=False)
            dropped = [k for k in unexpected if "position_ids" not in k]
            if dropped:
                raise RuntimeError(f"unexpected checkpoint keys: {dropped[:8]}")
        return model
    model = cls(cfg or BertConfig())
    if os.path.isfile(path):
        from ..utils.checkpoint import load_checkpoint
        load_checkpoint(model, path)
    return model


def build_model(name: str = "bert-base", num_labels: int = 6,
                model_path: Optional[str] = None):
    """Model factory by preset name (bench + CLI entrypoints)."""
    import os
    if name in ("bert-base", "bert-base-chinese"):
        cfg = BertConfig.bert_base_chinese(num_labels)
        cls = BertForSequenceClassification
    elif name == "bert-large":
        cfg = BertConfig.bert_large(num_labels)
        cls = BertForSequenceClassification
    elif name == "bert-small":
        cfg = BertConfig.bert_small(num_labels)
        cls = BertForSequenceClassification
    elif name == "roberta-base":
        cfg = BertConfig.roberta_base(num_labels)
        cls = RobertaForSequenceClassification
    elif name == "tiny":
        cfg = BertConfig.tiny(num_labels)
        cls = BertForSequenceClassification
    else:
        raise ValueError(f"unknown model preset {name}")
    if model_path and os.path.exists(model_path):
        return cls.from_pretrained(model_path, cfg)
    return cls(cfg)
