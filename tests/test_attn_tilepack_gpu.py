"""Tile-packed attention (``--attn-tile-pack``) on the GPU: the device plan
against its Python mirror, the tile-packed kernel instantiations against an
fp32 per-sequence reference, against fp64 next to the per-sequence kernels,
and against those kernels bit for bit where the plan holds only their
blocks; dropout masks shared by the two modes; the model, one graph serving
other groupings, and a token-budget batch.

fp64 figures (``max|x - ref| / max(std(ref), 1)``, MI355X) are recorded in
DESIGN.md "Tile-packed attention".
"""

import copy
import functools
import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = "cuda:0"
NH, HD = 2, 64
H = NH * HD
SCALE = 1.0 / math.sqrt(HD)
FWD_TOL = dict(rtol=3e-2, atol=3e-2)   # as tests/test_unpad_gpu.py
BWD_TOL = dict(rtol=5e-2, atol=5e-2)

# name -> (lengths, T or None for the next multiple of 64)
CASES = {
    "full-tile-of-three": ([20, 30, 14], None),
    "closes-on-overflow": ([40, 30, 10], None),
    "five-singles": ([1, 1, 1, 1, 1], None),
    "groups-around-long": ([5, 100, 7, 64, 3], None),
    "empties-and-tail-tile": ([10, 0, 0, 25, 0], 128),
    "streamed-next-to-group": ([129, 20, 30, 200], None),
}
FP16_CASES = ("full-tile-of-three", "streamed-next-to-group")


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


def _round64(n):
    return (n + 63) // 64 * 64


def _nan_prefill(*shape, dtype):
    """Allocate and free a NaN block of the output's size: the caching
    allocator tends to hand the same block to the next request, so an output
    that is not zero-filled shows up as NaN."""
    x = torch.full(shape, float("nan"), device=DEV, dtype=dtype)
    del x


def _ref_attn(qkv, cu, keep=None, p=0.0):
    """Per-sequence attention on a packed [T, 3H] stream in qkv's dtype
    (fp32 or fp64); rows outside the sequences are 0. ``keep`` (per sequence
    [NH, n, n]) applies a given dropout mask."""
    T = qkv.shape[0]
    out = qkv.new_zeros(T, H)
    for b, (s0, s1) in enumerate(zip(cu[:-1], cu[1:])):
        n = s1 - s0
        if n == 0:
            continue
        q, k, v = (t.reshape(n, NH, HD).transpose(0, 1)
                   for t in qkv[s0:s1].split(H, dim=-1))
        pr = torch.softmax(q @ k.transpose(-1, -2) * SCALE, dim=-1)
        if keep is not None:
            pr = pr * keep[b].to(pr.dtype) / (1.0 - p)
        out[s0:s1] = (pr @ v).transpose(0, 1).reshape(n, H)
    return out


def _inputs(lens, T, dtype, seed):
    cu = _cu(lens)
    T = T or _round64(cu[-1])
    torch.manual_seed(seed)
    qkv = torch.randn(T, 3 * H, device=DEV, dtype=dtype)
    dout = torch.randn(T, H, device=DEV, dtype=dtype)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    return cu, T, qkv, dout, cu_t


def _err64(x, ref):
    return (x.double() - ref).abs().max().item() / max(ref.std().item(), 1.0)


# -------------------------------------------------------------------- plan
@pytest.mark.parametrize("case", list(CASES) + ["all-long"])
def test_device_plan_equals_mirror(case):
    from pdnlp_amd import ops
    lens, T = CASES.get(case, ([65, 128, 70], None))
    cu = _cu(lens)
    T = T or _round64(cu[-1])
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    plan = ops.varlen_attention_plan(cu_t, T)
    items, bounds = ops.tile_plan_reference(cu, T)
    m = ops.tile_plan_max_items(T, len(lens))
    assert ext().flash_attn_tilepack_max_items(T, len(lens)) == m
    assert plan.items.shape == (m, 4) and plan.bounds.shape == (T, 2)
    assert plan.count.is_cuda and plan.count.item() == len(items) <= m
    assert plan.items[:len(items), :3].tolist() == [list(i) for i in items]
    assert (plan.items[len(items):] == 0).all()
    assert plan.bounds.tolist() == [list(b) for b in bounds]


# ----------------------------------------------------------------- kernels
def _tp_fwd_bwd(e, qkv, dout, cu_t, T, mx, p=0.0, seed=None, salt=0):
    seed = torch.Tensor() if seed is None else seed
    plan = e.flash_attn_tilepack_plan(cu_t, T)
    _nan_prefill(T, H, dtype=qkv.dtype)
    o, lse = e.flash_attn_tilepack_fwd(qkv, plan, mx, NH, SCALE, p, seed,
                                       salt)
    _nan_prefill(T, 3 * H, dtype=qkv.dtype)
    dqkv = e.flash_attn_tilepack_bwd(dout, qkv, o, lse, plan, mx, NH, SCALE,
                                     p, seed, salt)
    return o, lse, dqkv


def _ps_fwd_bwd(e, qkv, dout, cu_t, mx, p=0.0, seed=None, salt=0):
    seed = torch.Tensor() if seed is None else seed
    o, lse = e.flash_attn_varlen_fwd(qkv, cu_t, mx, NH, SCALE, p, seed, salt)
    dqkv = e.flash_attn_varlen_bwd(dout, qkv, o, lse, cu_t, mx, NH, SCALE, p,
                                   seed, salt)
    return o, lse, dqkv


@pytest.mark.parametrize("case,dtype", [
    (c, torch.bfloat16) for c in CASES] + [
    (c, torch.float16) for c in FP16_CASES])
def test_tilepack_kernel_fwd_bwd(case, dtype):
    e = ext()
    lens, T = CASES[case]
    cu, T, qkv, dout, cu_t = _inputs(lens, T, dtype, seed=0)
    total, mx = cu[-1], max(lens)

    o, lse, dqkv = _tp_fwd_bwd(e, qkv, dout, cu_t, T, mx)
    assert o.shape == (T, H) and lse.shape == (NH, T)
    assert dqkv.shape == (T, 3 * H)
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all()
    assert (o[total:] == 0).all() and (dqkv[total:] == 0).all(), \
        "rows outside the sequences must be 0"
    for h in range(NH):
        assert torch.isfinite(lse[h, :total]).all()

    q32 = qkv.float().requires_grad_()
    ref = _ref_attn(q32, cu)
    ref.backward(dout.float())
    torch.testing.assert_close(o.float(), ref.detach(), **FWD_TOL)
    torch.testing.assert_close(dqkv.float(), q32.grad, **BWD_TOL)

    # against fp64, next to the per-sequence kernels on the same input: both
    # make the same roundings (bf16 P, fp32 sums) in another order, and a
    # maximum over a few thousand elements moves by that much
    q64 = qkv.double().requires_grad_()
    ref64 = _ref_attn(q64, cu)
    ref64.backward(dout.double())
    o_ps, _, dqkv_ps = _ps_fwd_bwd(e, qkv, dout, cu_t, mx)
    new = (_err64(o, ref64.detach()), _err64(dqkv, q64.grad))
    old = (_err64(o_ps, ref64.detach()), _err64(dqkv_ps, q64.grad))
    print(f"{case} {str(dtype)[6:]}: o tile-packed {new[0]:.3e} "
          f"per-sequence {old[0]:.3e}; dqkv tile-packed {new[1]:.3e} "
          f"per-sequence {old[1]:.3e}")
    assert new[0] <= 2 * old[0] and new[1] <= 2 * old[1]


def test_all_long_batch_is_bit_equal():
    """Every item of [65, 128, 70] is a live block of the per-sequence grid
    and takes its code path, arithmetic included."""
    e = ext()
    cu, T, qkv, dout, cu_t = _inputs([65, 128, 70], None, torch.bfloat16, 3)
    o, lse, dqkv = _tp_fwd_bwd(e, qkv, dout, cu_t, T, 128)
    o_ps, lse_ps, dqkv_ps = _ps_fwd_bwd(e, qkv, dout, cu_t, 128)
    total = cu[-1]
    assert torch.equal(o, o_ps)
    assert torch.equal(lse[:, :total], lse_ps[:, :total])
    assert torch.equal(dqkv, dqkv_ps)


def test_cross_mode_forward_and_backward():
    """lse and dvec are [nh, T] by packed row in both modes, so a forward of
    one mode feeds a backward of the other."""
    e = ext()
    lens = [5, 100, 7, 64, 3]
    cu, T, qkv, dout, cu_t = _inputs(lens, None, torch.bfloat16, seed=4)
    mx, none = max(lens), torch.Tensor()
    plan = e.flash_attn_tilepack_plan(cu_t, T)
    q32 = qkv.float().requires_grad_()
    _ref_attn(q32, cu).backward(dout.float())

    o, lse = e.flash_attn_tilepack_fwd(qkv, plan, mx, NH, SCALE, 0.0, none, 0)
    d1 = e.flash_attn_varlen_bwd(dout, qkv, o, lse, cu_t, mx, NH, SCALE, 0.0,
                                 none, 0)
    o, lse = e.flash_attn_varlen_fwd(qkv, cu_t, mx, NH, SCALE, 0.0, none, 0)
    d2 = e.flash_attn_tilepack_bwd(dout, qkv, o, lse, plan, mx, NH, SCALE,
                                   0.0, none, 0)
    for d in (d1, d2):
        assert torch.isfinite(d).all() and (d[cu[-1]:] == 0).all()
        torch.testing.assert_close(d.float(), q32.grad, **BWD_TOL)


def test_tilepack_rejects_bad_arguments():
    e = ext()
    qkv = torch.randn(64, 3 * H, device=DEV, dtype=torch.bfloat16)
    cu = torch.tensor([0, 10], dtype=torch.int32, device=DEV)
    none = torch.Tensor()
    plan = e.flash_attn_tilepack_plan(cu, 64)
    with pytest.raises(RuntimeError, match="int32"):
        e.flash_attn_tilepack_plan(cu.long(), 64)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        e.flash_attn_tilepack_plan(cu, 32)
    with pytest.raises(RuntimeError, match="max_seqlen"):
        e.flash_attn_tilepack_fwd(qkv, plan, 1025, NH, SCALE, 0.0, none, 0)
    with pytest.raises(RuntimeError, match="total_rows"):
        e.flash_attn_tilepack_fwd(qkv, cu, 10, NH, SCALE, 0.0, none, 0)
    with pytest.raises(RuntimeError, match="total_rows"):
        e.flash_attn_tilepack_fwd(qkv, e.flash_attn_tilepack_plan(cu, 128),
                                  10, NH, SCALE, 0.0, none, 0)
    with pytest.raises(RuntimeError, match="bf16/fp16"):
        e.flash_attn_tilepack_fwd(qkv.float(), plan, 10, NH, SCALE, 0.0,
                                  none, 0)


# ----------------------------------------------------------------- dropout
def _recover_probs(fwd, qkv, cu):
    """Per sequence [NH, n, n]: the (dropped, rescaled) probabilities the
    kernel applies, read out by running ``fwd`` with V = basis vectors of
    one 64-key chunk at a time (then O = P[:, chunk])."""
    out = []
    for s0, s1 in zip(cu[:-1], cu[1:]):
        n = s1 - s0
        pm = torch.zeros(NH, n, n, device=DEV)
        for c in range((n + 63) // 64):
            k0, k1 = c * 64, min(c * 64 + 64, n)
            probe = qkv.clone()
            probe[:, 2 * H:] = 0
            eye = torch.eye(64, device=DEV, dtype=qkv.dtype)[:k1 - k0]
            for h in range(NH):
                probe[s0 + k0:s0 + k1,
                      2 * H + h * HD:2 * H + (h + 1) * HD] = eye
            o = fwd(probe)
            pm[:, :, k0:k1] = o[s0:s1].float().reshape(
                n, NH, HD).transpose(0, 1)[:, :, :k1 - k0]
        out.append(pm)
    return out


def test_tilepack_dropout():
    e = ext()
    p, lens = 0.1, [20, 30, 14, 65, 17]
    cu, T, qkv, dout, cu_t = _inputs(lens, None, torch.bfloat16, seed=2)
    total, mx, none = cu[-1], max(lens), torch.Tensor()
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    seed2 = torch.tensor([4321], dtype=torch.int64, device=DEV)
    plan = e.flash_attn_tilepack_plan(cu_t, T)

    def tp(x, p_, s_, salt):
        return e.flash_attn_tilepack_fwd(x, plan, mx, NH, SCALE, p_, s_, salt)

    def ps(x, p_, s_, salt):
        return e.flash_attn_varlen_fwd(x, cu_t, mx, NH, SCALE, p_, s_, salt)

    o1, lse = tp(qkv, p, seed, 7)
    assert torch.equal(o1, tp(qkv, p, seed, 7)[0])       # same (seed, salt)
    assert not torch.equal(o1, tp(qkv, p, seed2, 7)[0])  # a reseed
    assert (o1[total:] == 0).all()

    keeps = []
    for fn in (tp, ps):
        pd = _recover_probs(lambda x: fn(x, p, seed, 7)[0], qkv, cu)
        p0 = _recover_probs(lambda x: fn(x, 0.0, none, 0)[0], qkv, cu)
        keeps.append([(a != 0) | (b0 == 0) for a, b0 in zip(pd, p0)])
    for k_tp, k_ps in zip(*keeps):
        assert torch.equal(k_tp, k_ps), "the two modes must drop the same"
    keep = keeps[0]
    n_all = sum(k.numel() for k in keep)
    drop_rate = 1.0 - sum(k.sum().item() for k in keep) / n_all
    print(f"tile-packed dropout: drop rate {drop_rate:.4f} over {n_all}")
    assert abs(drop_rate - p) < 0.05

    q32 = qkv.float().requires_grad_()
    ref = _ref_attn(q32, cu, keep=[k.float() for k in keep], p=p)
    torch.testing.assert_close(o1.float(), ref.detach(), **FWD_TOL)
    dqkv = e.flash_attn_tilepack_bwd(dout, qkv, o1, lse, plan, mx, NH, SCALE,
                                     p, seed, 7)
    ref.backward(dout.float())
    assert torch.isfinite(dqkv).all() and (dqkv[total:] == 0).all()
    torch.testing.assert_close(dqkv.float(), q32.grad, **BWD_TOL)


# ------------------------------------------------------------------- model
LENS_A = [5, 64, 1, 33, 128, 70]
LENS_B = [70, 20, 100, 3, 64, 40]   # same (T, B, ms), another grouping


def _model_cfg(tile_pack=False):
    from pdnlp_amd.config import BertConfig
    return BertConfig(vocab_size=1024, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, intermediate_size=1024,
                      hidden_dropout_prob=0.0,
                      attention_probs_dropout_prob=0.0,
                      attn_tile_pack=tile_pack)


def _padded_batch(lens, S, seed):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(106, 1024, (len(lens), S), generator=g) * mask
    return {"input_ids": ids, "attention_mask": mask,
            "token_type_ids": torch.zeros_like(ids),
            "label": torch.randint(0, 6, (len(lens),), generator=g)}


def _packed_in(p):
    return dict(input_ids=p["input_ids"], token_type_ids=p["token_type_ids"],
                labels=p["label"], cu_seqlens=p["cu_seqlens"],
                max_seqlen=p["max_seqlen"], position_ids=p["position_ids"])


def _run(model, device, **inputs):
    model.zero_grad(set_to_none=True)
    out = model(**{k: (v.to(device) if torch.is_tensor(v) else v)
                   for k, v in inputs.items()})
    out.loss.backward()
    res = {"loss": out.loss.detach().float().cpu().reshape(1),
           "logits": out.logits.detach().float().cpu()}
    for n, p in model.named_parameters():
        res[n] = p.grad.detach().float().cpu()
    model.zero_grad(set_to_none=True)
    return res


def _rel(a, b, ref):
    return (a - b).abs().max().item() / max(ref.abs().std().item(), 1.0) \
        if ref.numel() > 1 else (a - b).abs().max().item()


@functools.lru_cache(maxsize=None)
def _models():
    from pdnlp_amd.models import BertForSequenceClassification
    torch.manual_seed(123)
    gpu_model = BertForSequenceClassification(_model_cfg()).to(torch.bfloat16)
    cpu_model = copy.deepcopy(gpu_model).float().train()
    return cpu_model, gpu_model.to(DEV).train()


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
    gpu_model.cfg.attn_tile_pack = False
    off = _run(gpu_model, DEV, **_packed_in(p))
    gpu_model.cfg.attn_tile_pack = True
    on = _run(gpu_model, DEV, **_packed_in(p))
    gpu_model.cfg.attn_tile_pack = False
    return p, ref, off, on


def test_model_tile_packed_within_twice_the_per_sequence_distance():
    _, ref, off, on = _model_runs("A")
    keys = [k for k in ref if k != "loss"]
    for k in keys:
        print(f"{k}: on-vs-fp32 {_rel(on[k], ref[k], ref[k]):.3e}  "
              f"off-vs-fp32 {_rel(off[k], ref[k], ref[k]):.3e}")
    d_on = max(_rel(on[k], ref[k], ref[k]) for k in keys)
    d_off = max(_rel(off[k], ref[k], ref[k]) for k in keys)
    print(f"WORST option on {d_on:.3e}  option off {d_off:.3e}")
    assert all(torch.isfinite(on[k]).all() for k in keys)
    assert d_on <= 2 * d_off


def test_option_selects_the_tile_packed_kernels(monkeypatch):
    """One plan launch per forward and one tile-packed attention launch per
    layer with the option on, none with it off. (The outputs cannot tell:
    both modes round alike and mostly agree to the bit.)"""
    e = ext()
    _, model = _models()
    p = _model_runs("A")[0]
    calls = {"plan": 0, "fwd": 0, "varlen": 0}

    def counted(name, key):
        real = getattr(e, name)

        def fn(*a):
            calls[key] += 1
            return real(*a)
        monkeypatch.setattr(e, name, fn)

    counted("flash_attn_tilepack_plan", "plan")
    counted("flash_attn_tilepack_fwd", "fwd")
    counted("flash_attn_varlen_fwd", "varlen")
    kw = {k: (v.to(DEV) if torch.is_tensor(v) else v)
          for k, v in _packed_in(p).items()}
    try:
        with torch.no_grad():
            model.cfg.attn_tile_pack = True
            model(**kw)
            assert calls == {"plan": 1, "fwd": 2, "varlen": 0}
            model.cfg.attn_tile_pack = False
            model(**kw)
            assert calls == {"plan": 1, "fwd": 2, "varlen": 2}
    finally:
        model.cfg.attn_tile_pack = False


def _graph_args(**kw):
    from pdnlp_amd.config import Args
    args = Args()
    args.strategy = "single"
    args.unpad = args.hip_graph = args.attn_tile_pack = True
    args.amp, args.amp_dtype = True, "bf16"
    args.epochs, args.do_dev, args.log_every = 1, False, 1000
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def _plain_sgd(model):
    from pdnlp_amd.ops.adamw import FusedSGD
    return FusedSGD(model.parameters(), lr=0.1, momentum=0.0)


def _replay(entry, model, batch):
    loss, logits, _ = entry.run(batch)
    res = {"loss": loss.float().cpu().reshape(1),
           "logits": logits.float().cpu()}
    for (n, _), g in zip(model.named_parameters(), entry.grads):
        res[n] = g.float().cpu()
    return res


def test_one_graph_serves_another_grouping():
    """Capture on A, replay A, B, A: B has the same (T, B, ms) but another
    grouping and item count. The plan is rebuilt on the device inside the
    graph, so every replay is the eager option-on run of that batch."""
    from pdnlp_amd import ops
    from pdnlp_amd.engine.trainer import Trainer, graph_key
    _, model = _models()
    runs = {w: _model_runs(w) for w in "AB"}
    pa, pb = runs["A"][0], runs["B"][0]
    assert graph_key(pa, 128) == graph_key(pb, 128)
    counts = [len(ops.tile_plan_reference(p["cu_seqlens"].tolist(), 320)[0])
              for p in (pa, pb)]
    assert counts[0] != counts[1], counts
    tr = Trainer(_graph_args(), model, _plain_sgd(model), DEV)
    assert model.cfg.attn_tile_pack
    try:
        entry = tr._capture_graph(pa)
        for which in "ABA":
            got = _replay(entry, model, runs[which][0])
            eager = runs[which][3]
            for k in eager:
                assert torch.equal(got[k], eager[k]), (which, k)
    finally:
        model.cfg.attn_tile_pack = False


def test_token_budget_batch_under_one_graph():
    """A budgeted batch ([256 rows, 32 sequences], most of them empty) under
    one graph with the option on. Its loss matches the option-off loss
    within the model bound: twice the option-off run's distance from the
    fp32 CPU reference, worst of loss, logits and gradients."""
    from pdnlp_amd.data import pack_batch
    from pdnlp_amd.engine.trainer import Trainer
    cpu_model, model = _models()
    lens = [1, 64, 65, 17, 40]
    budget = pack_batch(_padded_batch(lens, 128, seed=5), total_rows=256,
                        seq_multiple=32)
    assert budget["input_ids"].numel() == 256
    assert budget["cu_seqlens"].numel() == 33
    ref = _run(cpu_model, "cpu", **_packed_in(budget))
    off = _run(model, DEV, **_packed_in(budget))
    n = len(lens)
    for r in (ref, off):
        r["logits"] = r["logits"][:n]
    bound = 2 * max(_rel(off[k], ref[k], ref[k]) for k in ref)
    tr = Trainer(_graph_args(), model, _plain_sgd(model), DEV)
    try:
        entry = tr._capture_graph(budget)
        loss = entry.run(budget)[0].float().cpu().reshape(1)
    finally:
        model.cfg.attn_tile_pack = False
    print(f"budgeted loss: option on (graph) {loss.item():.6f}  option off "
          f"{off['loss'].item():.6f}  fp32 {ref['loss'].item():.6f}  bound "
          f"{bound:.3e}")
    assert torch.isfinite(loss).all()
    assert (loss - off["loss"]).abs().item() <= bound
