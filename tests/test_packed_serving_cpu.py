"""Padding-free serving without a GPU: the two pure functions behind the
packed InferenceEngine (``serve_bucket``, ``split_by_budget``), the engine's
packed forward on the CPU against the model's padded forward, the graph cap
and ``predict.py --engine packed``."""

import os
import subprocess
import sys

import pytest
import torch

from pdnlp_amd.config import BertConfig

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [5, 64, 1, 33, 128, 70, 2, 17]
TOL = dict(rtol=1e-5, atol=1e-5)   # as tests/test_unpad_cpu.py

# every multiple of 64 up to 512 (8 values), then 768, 1024, 1536, 2048,
# 3072, 4096 (2^k and 3 * 2^(k-1))
LADDER_4096 = 14


def _ceil64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------ serve_bucket
def test_serve_bucket_properties():
    from pdnlp_amd.engine.infer import serve_bucket, serve_ladder
    ts, prev_t = set(), 0
    for rows in range(1, 4097):
        T, _, _ = serve_bucket(rows, 1, 1, 128)
        assert T % 64 == 0 and T >= rows
        assert 3 * (T - _ceil64(rows)) < T
        assert T >= prev_t                       # monotone in rows
        prev_t = T
        ts.add(T)
    assert len(ts) == LADDER_4096
    assert sorted(ts) == serve_ladder(4096)
    assert sorted(ts)[:8] == list(range(64, 513, 64))
    assert sorted(ts)[8:] == [768, 1024, 1536, 2048, 3072, 4096]
    prev_b = 0
    for nseq in range(1, 4097):
        _, B, _ = serve_bucket(64, nseq, 1, 128)
        assert B >= nseq and B & (B - 1) == 0 and B < 2 * nseq
        assert B >= prev_b                       # monotone in nseq
        prev_b = B
    # T depends on rows alone, B on nseq alone
    for rows in (1, 64, 65, 513, 1025, 3073, 4096):
        for nseq in (1, 3, 64, 1000):
            T, B, _ = serve_bucket(rows, nseq, 1, 128)
            assert T == serve_bucket(rows, 1, 1, 128)[0]
            assert B == serve_bucket(64, nseq, 1, 128)[1]


def test_serve_bucket_ms_follows_graph_key():
    from pdnlp_amd.engine.infer import serve_bucket
    from pdnlp_amd.engine.trainer import graph_key
    for max_seq_len in (128, 192, 512):
        for longest in (1, 127, 128, 129, 192, 256, 257, 512):
            if longest > max_seq_len:
                continue
            batch = {"input_ids": torch.zeros(64, dtype=torch.long),
                     "cu_seqlens": torch.zeros(2, dtype=torch.int32),
                     "max_seqlen": longest}
            assert serve_bucket(longest, 1, longest, max_seq_len)[2] \
                == graph_key(batch, max_seq_len)[3]


# --------------------------------------------------------- split_by_budget
@pytest.mark.parametrize("max_tokens,max_seqs", [(128, 1024), (256, 3),
                                                 (4096, 1024), (128, 1)])
def test_split_by_budget(max_tokens, max_seqs):
    from pdnlp_amd.engine.infer import split_by_budget
    g = torch.Generator().manual_seed(max_tokens + max_seqs)
    lens = torch.randint(1, 129, (200,), generator=g).tolist() + LENS
    ranges = split_by_budget(lens, max_tokens, max_seqs)
    assert ranges[0][0] == 0 and ranges[-1][1] == len(lens)
    for (a, b), nxt in zip(ranges, ranges[1:] + [None]):
        assert a < b
        assert sum(lens[a:b]) <= max_tokens and b - a <= max_seqs
        if nxt is not None:
            assert nxt[0] == b                   # consecutive, input order
            # closed only because the next text would not fit
            assert sum(lens[a:b]) + lens[b] > max_tokens \
                or b - a == max_seqs
    assert split_by_budget([], max_tokens, max_seqs) == []


def test_split_by_budget_bad_arguments():
    from pdnlp_amd.engine.infer import split_by_budget
    for bad in (0, 100, -64):
        with pytest.raises(ValueError):
            split_by_budget([5], bad, 8)
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            split_by_budget([5], 128, bad)
    with pytest.raises(ValueError):
        split_by_budget([5, 129], 128, 8)        # can never fit
    with pytest.raises(ValueError):
        split_by_budget([5, 0], 128, 8)


def test_engine_bad_arguments():
    from pdnlp_amd.engine import InferenceEngine
    from pdnlp_amd.models import BertForSequenceClassification
    model = BertForSequenceClassification(BertConfig.tiny())
    for kw in (dict(max_tokens=100), dict(max_tokens=64, max_seq_len=128),
               dict(max_seqs=4097), dict(max_seqs=0)):
        with pytest.raises(ValueError):
            InferenceEngine(model, device="cpu", packed=True, **kw)


# ------------------------------------------------------------------ engine
def _model(kind):
    from pdnlp_amd.models import (BertForSequenceClassification,
                                  RobertaForSequenceClassification)
    cfg = BertConfig.tiny()
    cfg.max_position_embeddings = 128    # tiny() stops at 64 positions
    torch.manual_seed(11)
    if kind == "roberta":
        cfg.model_type, cfg.pad_token_id = "roberta", 1
        cfg.type_vocab_size, cfg.max_position_embeddings = 1, 130
        return RobertaForSequenceClassification(cfg).eval()
    return BertForSequenceClassification(cfg).eval()


def _seqs(vocab):
    g = torch.Generator().manual_seed(3)
    return [(torch.randint(5, vocab, (n,), generator=g).tolist(), [0] * n)
            for n in LENS]


def _padded_logits(model, seqs):
    pad = model.config.pad_token_id
    ids = torch.full((len(seqs), 128), pad, dtype=torch.long)
    mask = torch.zeros_like(ids)
    for i, (t, _) in enumerate(seqs):
        ids[i, :len(t)] = torch.tensor(t)
        mask[i, :len(t)] = 1
    with torch.no_grad():
        return model(input_ids=ids, attention_mask=mask,
                     token_type_ids=torch.zeros_like(ids)).logits


@pytest.mark.parametrize("max_tokens,n_ranges", [(4096, 1), (128, 3)])
@pytest.mark.parametrize("kind", ["bert", "roberta"])
def test_engine_cpu_matches_padded_forward(kind, max_tokens, n_ranges):
    """One range, and ``max_tokens=128``: several ranges, empty slots (three
    texts in a four-slot range) and the input order restored."""
    from pdnlp_amd.engine import InferenceEngine
    from pdnlp_amd.engine.infer import split_by_budget
    model = _model(kind)
    seqs = _seqs(model.config.vocab_size)
    ref = _padded_logits(model, seqs)
    assert len(split_by_budget(LENS, max_tokens, 1024)) == n_ranges
    eng = InferenceEngine(model, device="cpu", max_seq_len=128, packed=True,
                          max_tokens=max_tokens)
    got = eng.forward_sequences(seqs)
    assert got.shape == ref.shape
    torch.testing.assert_close(got, ref, **TOL)
    assert eng.graph_stats == {"captured": 0, "replayed": 0,
                               "eager": n_ranges}
    # the caller's model keeps its config; the engine's copy is tile-packed
    assert model.config.attn_tile_pack is False
    assert eng.model.config.attn_tile_pack is True
    # without the forward-only kernel selection nothing changes on the CPU
    eng2 = InferenceEngine(model, device="cpu", max_seq_len=128, packed=True,
                           max_tokens=max_tokens, infer_kernels=False)
    assert torch.equal(eng2.forward_sequences(seqs), got)


def test_engine_predict_any_number_of_texts():
    from pdnlp_amd.data import build_tokenizer
    from pdnlp_amd.engine import InferenceEngine
    model = _model("bert")
    tok = build_tokenizer(None, vocab_size=model.config.vocab_size)
    texts = ["你好世界", "今天天气不错", "我", "这部电影太让人失望了"] * 5
    eng = InferenceEngine(model, tok, device="cpu", max_seq_len=64,
                          packed=True, max_tokens=64, max_seqs=3)
    logits = eng.predict_logits(texts)
    assert logits.shape == (20, model.config.num_labels)
    assert logits.dtype == torch.float32
    assert eng.graph_stats["eager"] >= 7         # 20 texts, 3 per range
    for i in range(4, 20):                       # same text, same logits
        torch.testing.assert_close(logits[i], logits[i % 4], **TOL)
    padded = InferenceEngine(model, tok, device="cpu", max_seq_len=64)
    torch.testing.assert_close(logits, padded.predict_logits(texts), **TOL)
    assert eng.predict(texts) == logits.argmax(-1).tolist()
    labels = eng.predict(texts[:2], id2label={i: f"L{i}" for i in range(6)})
    assert all(lab.startswith("L") for lab in labels)


def test_max_graphs_zero_runs_eager():
    """``max_graphs=0``: every request is counted under ``eager`` (on the
    CPU nothing is ever captured either)."""
    from pdnlp_amd.engine import InferenceEngine
    model = _model("bert")
    eng = InferenceEngine(model, device="cpu", max_seq_len=128, packed=True,
                          max_graphs=0)
    seqs = _seqs(model.config.vocab_size)
    for _ in range(3):
        eng.forward_sequences(seqs)
    eng.warmup([(64, 1, 128)])
    assert eng.graph_stats == {"captured": 0, "replayed": 0, "eager": 3}


def test_inference_kernels_flag_is_scoped():
    from pdnlp_amd import ops
    from pdnlp_amd.ops import functional as Fn
    assert not Fn._infer_active()
    with ops.inference_kernels():
        assert not Fn._infer_active()            # autograd is on
        with torch.no_grad():
            assert Fn._infer_active()
            with ops.inference_kernels(False):
                assert not Fn._infer_active()
            assert Fn._infer_active()
    with torch.no_grad():
        assert not Fn._infer_active()            # never set implicitly


def test_cli_predict_packed(tmp_path):
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "predict.py"), "--engine",
         "packed", "--text", "今天天气真好", "--model", "tiny",
         "--max-seq-len", "16", "--output-dir", str(tmp_path)],
        cwd=REPO, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "predicted:" in r.stdout and "packed" in r.stdout
