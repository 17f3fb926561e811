"""CLS-only last encoder layer (``--cls-only-last-layer``) on the GPU: the
one-query-row-per-sequence attention kernels (cls_attention.hip) against an
fp32 torch reference, against fp64 next to the per-sequence flash kernels on
the same input, their zeros, the serving form, dropout masks shared with the
flash kernels; then the model, one graph serving other boundaries, a
token-budget batch, activation checkpointing and the packed engine.

Accuracy rule (that of tests/test_attn_tilepack_gpu.py): in the metric
``max|x - ref| / max(std(ref), 1)`` the new path may be at most twice as far
from its reference as the existing path on the same input. The new kernel
keeps P in fp32 where the MFMA kernels round it to 16 bits, so it makes a
subset of their roundings. Measured figures (MI355X) are recorded in DESIGN.md
"CLS-only last layer".
"""

import copy
import functools
import math

import pytest
import torch

from tests.test_attn_tilepack_gpu import (LENS_A, LENS_B, _graph_args,
                                          _model_cfg, _packed_in,
                                          _padded_batch, _plain_sgd, _rel,
                                          _replay, _run)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = "cuda:0"
NH, HD = 2, 64
H = NH * HD
ROWS = 64
SCALE = 1.0 / math.sqrt(HD)
FWD_TOL = dict(rtol=3e-2, atol=3e-2)   # as tests/test_unpad_gpu.py
BWD_TOL = dict(rtol=5e-2, atol=5e-2)

# name -> (lengths, T or None for the next multiple of 64)
CASES = {
    "three-short": ([20, 30, 14], None),
    "five-singles": ([1, 1, 1, 1, 1], None),
    "short-and-long": ([5, 100, 7, 64, 3], None),
    "empties-and-tail": ([10, 0, 0, 25, 0], 128),
    "past-128-keys": ([129, 20, 30, 200], None),
    "512-keys": ([512, 1], None),
}
FP16_CASES = ("three-short", "past-128-keys")


def ext():
    from pdnlp_amd.ops import ext as _ext
    e = _ext()
    assert e is not None, "HIP extension must be built on the GPU box"
    return e


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def _nan_prefill(*shape, dtype):
    """As tests/test_attn_tilepack_gpu.py: the caching allocator tends to
    hand the freed NaN block to the next request of that size, so an output
    that is neither written nor zero-filled shows up as NaN."""
    x = torch.full(shape, float("nan"), device=DEV, dtype=dtype)
    del x


def _inputs(lens, T, dtype, seed):
    cu = _cu(lens)
    T = T or (cu[-1] + 63) // 64 * 64
    torch.manual_seed(seed)
    qkv = torch.randn(T, 3 * H, device=DEV, dtype=dtype)
    dout = torch.randn(ROWS, H, device=DEV, dtype=dtype)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    return cu, T, qkv, dout, cu_t


def _ref_cls(qkv, cu, keep=None, p=0.0):
    """[ROWS, H] first-token attention per sequence in qkv's dtype (fp32 or
    fp64), zero rows elsewhere. ``keep`` (per sequence [NH, n]) applies a
    given dropout mask."""
    rows = []
    for b, (s0, s1) in enumerate(zip(cu[:-1], cu[1:])):
        n = s1 - s0
        if n == 0:
            rows.append(qkv.new_zeros(1, H))
            continue
        q, k, v = (t.reshape(n, NH, HD).transpose(0, 1)
                   for t in qkv[s0:s1].split(H, dim=-1))
        pr = torch.softmax(q[:, :1] @ k.transpose(-1, -2) * SCALE, dim=-1)
        if keep is not None:
            pr = pr * keep[b].to(pr.dtype)[:, None, :] / (1.0 - p)
        rows.append((pr @ v).transpose(0, 1).reshape(1, H))
    rows.append(qkv.new_zeros(ROWS - len(rows), H))
    return torch.cat(rows, dim=0)


def _err64(x, ref):
    return (x.double() - ref).abs().max().item() / max(ref.std().item(), 1.0)


def _cls_fwd_bwd(e, qkv, dout, cu_t, mx, p=0.0, seed=None, salt=0):
    seed = torch.Tensor() if seed is None else seed
    _nan_prefill(ROWS, H, dtype=qkv.dtype)
    o, lse = e.cls_attn_fwd(qkv, cu_t, ROWS, mx, NH, SCALE, p, seed, salt)
    _nan_prefill(*qkv.shape, dtype=qkv.dtype)
    dqkv = e.cls_attn_bwd(dout, qkv, o, lse, cu_t, mx, NH, SCALE, p, seed,
                          salt)
    return o, lse, dqkv


def _flash_first_rows(e, qkv, dout, cu, cu_t, mx):
    """The per-sequence flash kernels on the same input: their first-token
    rows of o as [ROWS, H], and their dqkv for a dout that is zero except at
    those rows."""
    T = qkv.shape[0]
    none = torch.Tensor()
    live = [i for i in range(len(cu) - 1) if cu[i + 1] > cu[i]]
    first = torch.tensor([cu[i] for i in live], device=DEV)
    o, lse = e.flash_attn_varlen_fwd(qkv, cu_t, mx, NH, SCALE, 0.0, none, 0)
    dfull = torch.zeros(T, H, device=DEV, dtype=qkv.dtype)
    dfull[first] = dout[torch.tensor(live, device=DEV)]
    dqkv = e.flash_attn_varlen_bwd(dfull, qkv, o, lse, cu_t, mx, NH, SCALE,
                                   0.0, none, 0)
    rows = torch.zeros(ROWS, H, device=DEV, dtype=qkv.dtype)
    rows[torch.tensor(live, device=DEV)] = o[first]
    return rows, dqkv


# ----------------------------------------------------------------- kernels
@pytest.mark.parametrize("case,dtype", [
    (c, torch.bfloat16) for c in CASES] + [
    (c, torch.float16) for c in FP16_CASES])
def test_cls_kernel_fwd_bwd(case, dtype):
    e = ext()
    lens, T = CASES[case]
    cu, T, qkv, dout, cu_t = _inputs(lens, T, dtype, seed=0)
    B, total, mx = len(lens), cu[-1], max(lens)

    o, lse, dqkv = _cls_fwd_bwd(e, qkv, dout, cu_t, mx)
    assert o.shape == (ROWS, H) and o.dtype == dtype
    assert lse.shape == (NH, ROWS) and lse.dtype == torch.float32
    assert dqkv.shape == (T, 3 * H)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert torch.isfinite(dqkv).all()

    # structure: the exact zeros
    assert (o[B:] == 0).all(), "rows past the batch"
    for i, n in enumerate(lens):
        if n == 0:
            assert (o[i] == 0).all(), "row of an empty sequence"
    assert (dqkv[total:] == 0).all(), "rows outside the sequences"
    first = torch.zeros(T, dtype=torch.bool, device=DEV)
    first[[cu[i] for i, n in enumerate(lens) if n > 0]] = True
    assert (dqkv[~first, :H] == 0).all(), "q columns of non-first rows"
    assert dqkv[first, :H].abs().sum() > 0 or mx == 1

    # the infer form: the same output bits, no lse
    _nan_prefill(ROWS, H, dtype=dtype)
    assert torch.equal(e.cls_attn_infer(qkv, cu_t, ROWS, mx, NH, SCALE), o)

    # bit-reproducible
    o2, lse2, dqkv2 = _cls_fwd_bwd(e, qkv, dout, cu_t, mx)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    assert torch.equal(dqkv, dqkv2)

    q32 = qkv.float().requires_grad_()
    ref = _ref_cls(q32, cu)
    ref.backward(dout.float())
    torch.testing.assert_close(o.float(), ref.detach(), **FWD_TOL)
    torch.testing.assert_close(dqkv.float(), q32.grad, **BWD_TOL)

    # against fp64, next to the per-sequence flash kernels on the same input
    q64 = qkv.double().requires_grad_()
    ref64 = _ref_cls(q64, cu)
    ref64.backward(dout.double())
    o_ps, dqkv_ps = _flash_first_rows(e, qkv, dout, cu, cu_t, mx)
    new = (_err64(o, ref64.detach()), _err64(dqkv, q64.grad))
    old = (_err64(o_ps, ref64.detach()), _err64(dqkv_ps, q64.grad))
    print(f"{case} {str(dtype)[6:]}: o cls {new[0]:.3e} flash {old[0]:.3e}; "
          f"dqkv cls {new[1]:.3e} flash {old[1]:.3e}")
    assert new[0] <= 2 * old[0] and new[1] <= 2 * old[1]


def test_cls_op_routes_and_differentiates():
    """ops.cls_attention: the autograd function under autograd, the infer
    kernel under ops.inference_kernels() with autograd off."""
    from pdnlp_amd import ops
    lens = [20, 30, 14]
    cu, T, qkv, dout, cu_t = _inputs(lens, None, torch.bfloat16, seed=1)
    x = qkv.clone().requires_grad_()
    o = ops.cls_attention(x, cu_t, ROWS, 30, NH)
    o.backward(dout)
    o_k, lse, dqkv = _cls_fwd_bwd(ext(), qkv, dout, cu_t, 30)
    assert torch.equal(o, o_k) and torch.equal(x.grad, dqkv)
    with torch.no_grad(), ops.inference_kernels():
        assert torch.equal(ops.cls_attention(qkv, cu_t, ROWS, 30, NH), o_k)


def test_cls_kernel_rejects_bad_arguments():
    e = ext()
    qkv = torch.randn(64, 3 * H, device=DEV, dtype=torch.bfloat16)
    cu = torch.tensor([0, 10, 20, 30], dtype=torch.int32, device=DEV)
    none = torch.Tensor()
    with pytest.raises(RuntimeError, match="bf16/fp16"):
        e.cls_attn_fwd(qkv.float(), cu, ROWS, 10, NH, SCALE, 0.0, none, 0)
    with pytest.raises(RuntimeError, match="rows_out"):
        e.cls_attn_fwd(qkv, cu, 2, 10, NH, SCALE, 0.0, none, 0)
    with pytest.raises(RuntimeError, match="int32"):
        e.cls_attn_fwd(qkv, cu.long(), ROWS, 10, NH, SCALE, 0.0, none, 0)
    odd = torch.randn(64, 3 * 96, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="head_dim"):
        e.cls_attn_fwd(odd, cu, ROWS, 10, 1, SCALE, 0.0, none, 0)
    with pytest.raises(RuntimeError, match="bf16/fp16"):
        e.cls_attn_infer(qkv.float(), cu, ROWS, 10, NH, SCALE)
    with pytest.raises(RuntimeError, match="rows_out"):
        e.cls_attn_infer(qkv, cu, 2, 10, NH, SCALE)
    o, lse = e.cls_attn_fwd(qkv, cu, ROWS, 10, NH, SCALE, 0.0, none, 0)
    with pytest.raises(RuntimeError, match="dout"):
        e.cls_attn_bwd(o.float(), qkv, o, lse, cu, 10, NH, SCALE, 0.0, none,
                       0)
    with pytest.raises(RuntimeError, match="seed"):
        e.cls_attn_fwd(qkv, cu, ROWS, 10, NH, SCALE, 0.1, none, 0)


# ----------------------------------------------------------------- dropout
def test_cls_dropout_keeps_what_the_flash_kernel_keeps():
    e = ext()
    p = 0.1
    lens = [20, 30, 14, 64, 1, 50, 64, 64, 33, 60, 64, 47]   # all <= 64 keys
    cu, T, qkv, dout, cu_t = _inputs(lens, None, torch.bfloat16, seed=2)
    mx, none = max(lens), torch.Tensor()
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    seed2 = torch.tensor([4321], dtype=torch.int64, device=DEV)

    def cls(x, p_, s_, salt):
        return e.cls_attn_fwd(x, cu_t, ROWS, mx, NH, SCALE, p_, s_, salt)

    o1, lse = cls(qkv, p, seed, 7)
    assert torch.equal(o1, cls(qkv, p, seed, 7)[0])       # same (seed, salt)
    assert not torch.equal(o1, cls(qkv, p, seed2, 7)[0])  # a reseed
    assert not torch.equal(o1, cls(qkv, p, seed, 8)[0])   # another salt
    assert (o1[len(lens):] == 0).all()

    # V = unit vectors: o[d] is the kept probability of key d
    probe = qkv.clone()
    probe[:, 2 * H:] = 0
    eye = torch.eye(64, device=DEV, dtype=qkv.dtype)
    for s0, s1 in zip(cu[:-1], cu[1:]):
        for h in range(NH):
            probe[s0:s1, 2 * H + h * HD:2 * H + (h + 1) * HD] = eye[:s1 - s0]
    first = torch.tensor(cu[:-1], device=DEV)

    def flash(x, p_, s_, salt):
        o = e.flash_attn_varlen_fwd(x, cu_t, mx, NH, SCALE, p_, s_, salt)[0]
        return o[first]

    def kept(fn):
        pd = fn(probe, p, seed, 7)
        p0 = fn(probe, 0.0, none, 0)
        return [((pd[i] != 0) | (p0[i] == 0)).reshape(NH, HD)[:, :n]
                for i, n in enumerate(lens)]

    keep = kept(lambda *a: cls(*a)[0][:len(lens)])
    keep_flash = kept(flash)
    for a, b in zip(keep, keep_flash):
        assert torch.equal(a, b), "the kept set of flash_attn_varlen_fwd"
    n_all = sum(k.numel() for k in keep)
    drop_rate = 1.0 - sum(k.sum().item() for k in keep) / n_all
    print(f"cls dropout: drop rate {drop_rate:.4f} over {n_all}")
    assert abs(drop_rate - p) < 0.05

    # forward and backward at p against fp32 with the recovered mask
    q32 = qkv.float().requires_grad_()
    ref = _ref_cls(q32, cu, keep=[k.float() for k in keep], p=p)
    torch.testing.assert_close(o1.float(), ref.detach(), **FWD_TOL)
    dqkv = e.cls_attn_bwd(dout, qkv, o1, lse, cu_t, mx, NH, SCALE, p, seed, 7)
    ref.backward(dout.float())
    assert torch.isfinite(dqkv).all() and (dqkv[cu[-1]:] == 0).all()
    torch.testing.assert_close(dqkv.float(), q32.grad, **BWD_TOL)


# ------------------------------------------------------------------- model
@functools.lru_cache(maxsize=None)
def _models():
    from pdnlp_amd.models import BertForSequenceClassification
    torch.manual_seed(123)
    gpu_model = BertForSequenceClassification(_model_cfg()).to(torch.bfloat16)
    cpu_model = copy.deepcopy(gpu_model).float().train()
    return cpu_model, gpu_model.to(DEV).train()


def _set(model, on, tile_pack=False):
    model.cfg.cls_only_last_layer = on
    model.cfg.attn_tile_pack = tile_pack


@functools.lru_cache(maxsize=None)
def _model_runs(which):
    """(packed batch, fp32 CPU padded reference, HIP option off, HIP option
    on) for length list A or B; logits, loss and every gradient."""
    from pdnlp_amd.data import pack_batch
    cpu_model, gpu_model = _models()
    lens, seed = {"A": (LENS_A, 5), "B": (LENS_B, 6)}[which]
    b = _padded_batch(lens, 128, seed)
    p = pack_batch(b)
    assert p["input_ids"].numel() == 320
    ref = _run(cpu_model, "cpu", input_ids=b["input_ids"],
               attention_mask=b["attention_mask"],
               token_type_ids=b["token_type_ids"], labels=b["label"])
    try:
        _set(gpu_model, False)
        off = _run(gpu_model, DEV, **_packed_in(p))
        _set(gpu_model, True)
        on = _run(gpu_model, DEV, **_packed_in(p))
    finally:
        _set(gpu_model, False)
    return p, ref, off, on


def test_model_within_twice_the_option_off_distance():
    _, ref, off, on = _model_runs("A")
    keys = [k for k in ref if k != "loss"]
    for k in keys:
        print(f"{k}: on-vs-fp32 {_rel(on[k], ref[k], ref[k]):.3e}  "
              f"off-vs-fp32 {_rel(off[k], ref[k], ref[k]):.3e}")
    d_on = max(_rel(on[k], ref[k], ref[k]) for k in keys)
    d_off = max(_rel(off[k], ref[k], ref[k]) for k in keys)
    print(f"WORST option on {d_on:.3e}  option off {d_off:.3e}")
    assert all(torch.isfinite(on[k]).all() for k in keys)
    assert on["logits"].shape == off["logits"].shape
    assert d_on <= 2 * d_off


def test_option_selects_the_cls_kernel(monkeypatch):
    """One cls_attn forward for the last layer and num_layers - 1 varlen (or
    tile-packed) forwards with the option on; no cls_attn forward with it
    off."""
    e = ext()
    _, model = _models()
    p = _model_runs("A")[0]
    n = model.cfg.num_hidden_layers
    calls = {"cls": 0, "varlen": 0, "tp": 0}

    def counted(name, key):
        real = getattr(e, name)

        def fn(*a):
            calls[key] += 1
            return real(*a)
        monkeypatch.setattr(e, name, fn)

    counted("cls_attn_fwd", "cls")
    counted("flash_attn_varlen_fwd", "varlen")
    counted("flash_attn_tilepack_fwd", "tp")
    kw = {k: (v.to(DEV) if torch.is_tensor(v) else v)
          for k, v in _packed_in(p).items()}
    try:
        with torch.no_grad():
            _set(model, True)
            model(**kw)
            assert calls == {"cls": 1, "varlen": n - 1, "tp": 0}
            _set(model, True, tile_pack=True)
            model(**kw)
            assert calls == {"cls": 2, "varlen": n - 1, "tp": n - 1}
            _set(model, False)
            model(**kw)
            assert calls == {"cls": 2, "varlen": 2 * n - 1, "tp": n - 1}
    finally:
        _set(model, False)


def test_one_graph_serves_other_boundaries():
    """Capture on A, replay A, B, A: the same (T, B, ms), other boundaries.
    cu_seqlens is read on the device only, so every replay is the eager
    option-on run of that batch."""
    from pdnlp_amd.engine.trainer import Trainer, graph_key
    _, model = _models()
    runs = {w: _model_runs(w) for w in "AB"}
    pa, pb = runs["A"][0], runs["B"][0]
    assert graph_key(pa, 128) == graph_key(pb, 128)
    args = _graph_args(attn_tile_pack=False, cls_only_last_layer=True)
    tr = Trainer(args, model, _plain_sgd(model), DEV)
    assert model.cfg.cls_only_last_layer and not model.cfg.attn_tile_pack
    try:
        entry = tr._capture_graph(pa)
        for which in "ABA":
            got = _replay(entry, model, runs[which][0])
            eager = runs[which][3]
            for k in eager:
                assert torch.equal(got[k], eager[k]), (which, k)
    finally:
        _set(model, False)


def test_token_budget_batch_under_one_graph():
    """A budgeted batch ([256 rows, 32 sequences], most of them empty) under
    one graph with the option on (and tile-packed attention on the other
    layer). Its loss matches the option-off loss within the model bound:
    twice the option-off run's distance from the fp32 CPU reference, worst of
    loss, logits and gradients."""
    from pdnlp_amd.data import pack_batch
    from pdnlp_amd.engine.trainer import Trainer
    cpu_model, model = _models()
    lens = [1, 64, 65, 17, 40]
    budget = pack_batch(_padded_batch(lens, 128, seed=5), total_rows=256,
                        seq_multiple=32)
    assert budget["input_ids"].numel() == 256
    assert budget["cu_seqlens"].numel() == 33
    ref = _run(cpu_model, "cpu", **_packed_in(budget))
    _set(model, False)
    off = _run(model, DEV, **_packed_in(budget))
    n = len(lens)
    for r in (ref, off):
        r["logits"] = r["logits"][:n]
    bound = 2 * max(_rel(off[k], ref[k], ref[k]) for k in ref)
    tr = Trainer(_graph_args(cls_only_last_layer=True), model,
                 _plain_sgd(model), DEV)
    assert model.cfg.cls_only_last_layer and model.cfg.attn_tile_pack
    try:
        entry = tr._capture_graph(budget)
        loss = entry.run(budget)[0].float().cpu().reshape(1)
    finally:
        _set(model, False)
    print(f"budgeted loss: option on (graph) {loss.item():.6f}  option off "
          f"{off['loss'].item():.6f}  fp32 {ref['loss'].item():.6f}  bound "
          f"{bound:.3e}")
    assert torch.isfinite(loss).all()
    assert (loss - off["loss"]).abs().item() <= bound


def test_activation_checkpointing_gives_the_same_gradients():
    _, model = _models()
    p, _, _, on = _model_runs("A")
    try:
        _set(model, True)
        model.gradient_checkpointing_enable()
        ck = _run(model, DEV, **_packed_in(p))
    finally:
        model.bert.gradient_checkpointing_disable()
        _set(model, False)
    for k in on:
        assert torch.equal(ck[k], on[k]), k


# ------------------------------------------------------------------ engine
def _err(x, ref):
    return (x.double() - ref.double()).abs().max().item() \
        / max(ref.double().std().item(), 1.0)


def test_packed_engine_with_the_option_on():
    """The rule of test_engine_accuracy_next_to_padded_engine: packed at most
    2 x padded from the fp32 CPU padded model. A single short text falls
    under the fallback rule and equals the option-off engine to the bit."""
    from pdnlp_amd.engine import InferenceEngine
    from tests.test_packed_serving_gpu import _model, _seqs
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
    off = InferenceEngine(_model(), device=DEV, max_seq_len=S, packed=True)
    on = InferenceEngine(_model(), device=DEV, max_seq_len=S, packed=True,
                         cls_only_last_layer=True)
    assert on.model.config.cls_only_last_layer
    assert not _model().config.cls_only_last_layer
    e_pad = _err(padded.forward_tensors(ids, mask, types).float().cpu(), ref)
    e_off = _err(off.forward_sequences(seqs).float().cpu(), ref)
    got = on.forward_sequences(seqs)
    assert got.shape == ref.shape
    e_on = _err(got.float().cpu(), ref)
    print(f"serving accuracy vs fp32 CPU: padded {e_pad:.3e}, packed "
          f"{e_off:.3e}, packed + cls-only {e_on:.3e}")
    assert e_on <= 2 * e_pad
    # a replay of the captured graph returns the same bits
    assert torch.equal(on.forward_sequences(seqs), got)
    one = _seqs([9], 7)
    assert torch.equal(on.forward_sequences(one), off.forward_sequences(one))
