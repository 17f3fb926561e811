"""Padding-free serving on the GPU: the forward-only (INFER) instantiations
of tile-packed attention and of the fused bias+residual+LN epilogue against
the training forwards they replace, bit for bit; the packed InferenceEngine
replaying one graph per key ``(T, B, ms)`` against its eager and its
training-kernel twins, bit for bit; and its distance from the fp32 CPU padded
model next to the padded engine's.

Accuracy rule (that of tests/test_attn_tilepack_gpu.py): in the metric
``max|x - ref| / max(std(ref), 1)`` the packed engine may be at most twice as
far from the fp32 reference as the padded engine on the same texts. Both make
the same roundings and differ in the order of fp32 sums. Measured figures
(MI355X) are recorded in DESIGN.md "Padding-free serving".
"""

import copy
import functools
import math
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = "cuda:0"
NH, HD = 2, 64
H = NH * HD
SCALE = 1.0 / math.sqrt(HD)
EPS = 1e-12

# the lengths of tests/test_attn_tilepack_gpu.py, plus two whole stripes
# outside every sequence and a stream without a free row
ATTN_CASES = {
    "full-tile-of-three": ([20, 30, 14], None),
    "five-singles": ([1, 1, 1, 1, 1], None),
    "groups-around-long": ([5, 100, 7, 64, 3], None),
    "empties-and-tail-tile": ([10, 0, 0, 25, 0], 128),
    "streamed-next-to-group": ([129, 20, 30, 200], None),
    "two-free-stripes": ([20, 30, 14], 192),
    "no-free-row": ([64, 64], None),
}
_ids = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


def ext():
    from pdnlp_amd.ops import ext as _ext
    e = _ext()
    assert e is not None, "HIP extension must be built on the GPU box"
    return e


# ------------------------------------------------------------ attention op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=_ids.get)
@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_attention_infer_equals_training_forward(case, dtype):
    from pdnlp_amd import ops
    e = ext()
    lens, T = ATTN_CASES[case]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    T = T or (cu[-1] + 63) // 64 * 64
    torch.manual_seed(len(lens) * 1000 + T)
    qkv = torch.randn(T, 3 * H, device=DEV, dtype=dtype)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    plan = ops.varlen_attention_plan(cu_t, T)
    mx = max(lens)
    ref, _ = e.flash_attn_tilepack_fwd(qkv, plan.buf, mx, NH, SCALE, 0.0,
                                       torch.Tensor(), 0)
    free = torch.ones(T, dtype=torch.bool)
    free[:cu[-1]] = False
    assert not ref[free.to(DEV)].any()          # the reference's own zeros

    out = torch.full((T, H), float("nan"), device=DEV, dtype=dtype)
    got = e.flash_attn_tilepack_infer(qkv, plan.buf, mx, NH, SCALE, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got, ref)

    # no ``out``: the allocator tends to hand back the NaN block just freed
    del got, out
    x = torch.full((T, H), float("nan"), device=DEV, dtype=dtype)
    del x
    got = e.flash_attn_tilepack_infer(qkv, plan.buf, mx, NH, SCALE)
    assert got.shape == (T, H) and got.dtype == dtype
    assert torch.equal(got, ref)


def test_attention_infer_rejects_bad_out():
    from pdnlp_amd import ops
    e = ext()
    T = 64
    qkv = torch.randn(T, 3 * H, device=DEV, dtype=torch.bfloat16)
    cu_t = torch.tensor([0, 20], dtype=torch.int32, device=DEV)
    plan = ops.varlen_attention_plan(cu_t, T)
    for bad in (torch.empty(T, H, device=DEV, dtype=torch.float16),
                torch.empty(T + 64, H, device=DEV, dtype=torch.bfloat16),
                torch.empty(T, 2 * H, device=DEV,
                            dtype=torch.bfloat16)[:, :H]):
        with pytest.raises(RuntimeError, match="out must be"):
            e.flash_attn_tilepack_infer(qkv, plan.buf, 20, NH, SCALE,
                                        out=bad)


def test_inference_kernels_selects_infer_attention(monkeypatch):
    """Only inside the context manager and with autograd off."""
    from pdnlp_amd import ops
    e = ext()
    T = 64
    qkv = torch.randn(T, 3 * H, device=DEV, dtype=torch.bfloat16)
    cu_t = torch.tensor([0, 20, 50], dtype=torch.int32, device=DEV)
    plan = ops.varlen_attention_plan(cu_t, T)
    calls = []
    real = e.flash_attn_tilepack_infer
    monkeypatch.setattr(e, "flash_attn_tilepack_infer",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    base = ops.attention_varlen(qkv, cu_t, 30, NH, plan=plan)
    with ops.inference_kernels():
        ops.attention_varlen(qkv, cu_t, 30, NH, plan=plan)  # grad mode on
        assert not calls
        with torch.no_grad():
            got = ops.attention_varlen(qkv, cu_t, 30, NH, plan=plan)
        assert len(calls) == 1
    with torch.no_grad():
        ops.attention_varlen(qkv, cu_t, 30, NH, plan=plan)
    assert len(calls) == 1
    assert torch.equal(got, base)


# ------------------------------------------------------------- epilogue op
def _bdrl_inputs(R, Hh, dtype):
    g = torch.Generator(device=DEV).manual_seed(1000 * R + Hh)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).to(dtype)
    return rnd(R, Hh), rnd(Hh), rnd(R, Hh), rnd(Hh), rnd(Hh)


def _bdrl_check(R, Hh, dtype):
    e = ext()
    y, bias, res, lnw, lnb = _bdrl_inputs(R, Hh, dtype)
    for two_pass in (False, True):
        assert "PDNLP_BDRL_2PASS" not in os.environ
        if two_pass:
            os.environ["PDNLP_BDRL_2PASS"] = "1"
        try:
            ref = e.bias_dropout_residual_ln_fwd(
                y, bias, res, lnw, lnb, 0.0, EPS, torch.Tensor(), 0)[0]
            x = torch.full((R, Hh), float("nan"), device=DEV, dtype=dtype)
            del x
            got = e.bias_dropout_residual_ln_infer(y, bias, res, lnw, lnb,
                                                   EPS)
        finally:
            os.environ.pop("PDNLP_BDRL_2PASS", None)
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert torch.equal(got, ref), f"two_pass={two_pass}"


@pytest.mark.parametrize("dtype", list(_ids), ids=_ids.get)
@pytest.mark.parametrize("R", [1, 64, 200])
@pytest.mark.parametrize("Hh", [256, 512, 768, 1024])
def test_epilogue_infer_equals_training_forward(Hh, R, dtype):
    _bdrl_check(R, Hh, dtype)


@pytest.mark.parametrize("dtype", list(_ids), ids=_ids.get)
@pytest.mark.parametrize("Hh", [256, 768])
def test_epilogue_infer_walks_rows(Hh, dtype):
    """R past 32 * CUs: 37 waves of the one-pass forward walk a second row
    (the shape of tests/test_bdrl_onepass_gpu.py)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _bdrl_check(32 * cus + 37, Hh, dtype)


# ------------------------------------------------------------------ engine
def _seqs(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(106, 1024, (n,), generator=g).tolist(), [0] * n)
            for n in lens]


@functools.lru_cache(maxsize=None)
def _model():
    from tests.test_unpad_gpu import _model_cfg
    from pdnlp_amd.models import BertForSequenceClassification
    torch.manual_seed(123)
    return BertForSequenceClassification(_model_cfg()).to(torch.bfloat16)


ENGINE_CASES = {
    "preload": (128, [5, 64, 1, 33, 128, 70], [70, 20, 100, 3, 64, 40]),
    "streamed": (192, [129, 70, 64, 40], [100, 129, 3, 70]),
}


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_replays_one_graph_per_key(case):
    """Three requests of one key: one capture, three replays (the request
    that triggers the capture is replayed from the new graph), and the bits
    of the eager packed forward and of the training-kernel forward."""
    from pdnlp_amd.engine import InferenceEngine
    from pdnlp_amd.engine.infer import serve_bucket
    S, lens_a, lens_b = ENGINE_CASES[case]
    a, b = _seqs(lens_a, 5), _seqs(lens_b, 6)
    assert serve_bucket(sum(lens_a), len(lens_a), max(lens_a), S) \
        == serve_bucket(sum(lens_b), len(lens_b), max(lens_b), S)
    kw = dict(device=DEV, max_seq_len=S, packed=True)
    graphed = InferenceEngine(_model(), infer_kernels=True, use_graph=True,
                              **kw)
    eager = InferenceEngine(_model(), infer_kernels=True, use_graph=False,
                            **kw)
    train_k = InferenceEngine(_model(), infer_kernels=False, use_graph=True,
                              **kw)
    for req in (a, b, a):
        got = graphed.forward_sequences(req)
        assert got.shape == (len(req), 6) and torch.isfinite(got).all()
        assert torch.equal(got, eager.forward_sequences(req))
        assert torch.equal(got, train_k.forward_sequences(req))
    assert graphed.graph_stats == {"captured": 1, "replayed": 3, "eager": 0}
    assert train_k.graph_stats == {"captured": 1, "replayed": 3, "eager": 0}
    assert eager.graph_stats == {"captured": 0, "replayed": 0, "eager": 3}


def test_engine_warmup_and_graph_cap():
    from pdnlp_amd.engine import InferenceEngine
    eng = InferenceEngine(_model(), device=DEV, packed=True, max_graphs=1)
    eng.warmup([(64, 1, 128)])
    assert eng.graph_stats == {"captured": 1, "replayed": 0, "eager": 0}
    one = eng.forward_sequences(_seqs([20], 1))           # the warmed key
    two = eng.forward_sequences(_seqs([20, 100], 1))      # a second key
    assert eng.graph_stats == {"captured": 1, "replayed": 1, "eager": 1}
    assert torch.equal(one[0], two[0])   # a sequence's logits are its own


def _err(x, ref):
    return (x.double() - ref.double()).abs().max().item() \
        / max(ref.double().std().item(), 1.0)


def test_engine_accuracy_next_to_padded_engine():
    from pdnlp_amd.engine import InferenceEngine
    lens = [5, 64, 1, 33, 128, 70]
    S = 128
    seqs = _seqs(lens, 5)
    ids = torch.zeros(len(lens), S, dtype=torch.long)
    mask = torch.zeros_like(ids)
    for i, (t, _) in enumerate(seqs):
        ids[i, :len(t)] = torch.tensor(t)
        mask[i, :len(t)] = 1
    types = torch.zeros_like(ids)
    cpu_model = copy.deepcopy(_model()).float().eval()
    with torch.no_grad():
        ref = cpu_model(input_ids=ids, attention_mask=mask,
                        token_type_ids=types).logits
    padded = InferenceEngine(_model(), device=DEV, max_seq_len=S)
    packed = InferenceEngine(_model(), device=DEV, max_seq_len=S,
                             packed=True)
    e_pad = _err(padded.forward_tensors(ids, mask, types).float().cpu(), ref)
    e_pack = _err(packed.forward_sequences(seqs).float().cpu(), ref)
    print(f"serving accuracy vs fp32 CPU: padded {e_pad:.3e}, "
          f"packed {e_pack:.3e}")
    assert e_pack <= 2 * e_pad
