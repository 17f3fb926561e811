"""Global-norm gradient clipping on the HIP path (csrc/grad_clip.hip and
the ``grad_coef`` argument of the optimizer kernels).

Tolerance of the norm: the kernel's fp32 rounding depth is L + D = 117
adds (see grad_clip.hip), (L + D) * 2^-24 = 7e-6 <= 1e-5 relative on the sum
of squares; the norm, its square root, is held to the same 1e-5.

End-to-end checks observe quantities LINEAR in the clip coefficient (SGD
parameters / master weights, the norm itself) — an AdamW update would
cancel a uniform gradient scale. Every clipping case asserts that the norm
is at least twice ``max_norm``.
"""

import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NUMELS = [1, 3, 5, 1023, 1024, 1025, 0, 300_001]
LOOSE = 1e6


def ext():
    from pdnlp_amd.ops import ext as _ext
    return _ext()


def _lists(dtype):
    """name -> tensor list, built once per dtype (never modified)."""
    g = torch.Generator().manual_seed(11)
    out = {}
    out["sizes"] = [torch.randn(n, generator=g).to(dtype).to(DEV)
                    for n in NUMELS]
    # views at odd element offsets of one flat buffer: unaligned pointers
    flat = torch.randn(1 + sum(NUMELS) + len(NUMELS), generator=g
                       ).to(dtype).to(DEV)
    views, off = [], 1
    for n in NUMELS:
        views.append(flat[off:off + n])
        off += n + (n % 2)          # keep every start odd
    assert all(v.numel() == 0 or (v.storage_offset() % 2 == 1) for v in views)
    out["odd_views"] = views
    for k in (33, 65):               # cross the 32-tensor launch chunk
        out[f"many{k}"] = [torch.randn(7 + i, generator=g).to(dtype).to(DEV)
                           for i in range(k)]
    return out


_CACHE = {}


def _case(dtype, name):
    if dtype not in _CACHE:
        _CACHE[dtype] = _lists(dtype)
    return _CACHE[dtype][name]


def _norm64(tensors):
    s = sum((t.double().pow(2).sum() for t in tensors),
            torch.zeros((), dtype=torch.float64, device=DEV))
    return math.sqrt(s.item())


def _sumsq(tensors, out=None, accumulate=False):
    if out is None:
        out = torch.full((1,), 123.0, device=DEV)   # must be overwritten
    ext().multi_tensor_sumsq(list(tensors), out, accumulate)
    return out


# ---- sumsq numerics ----------------------------------------------------------
@pytest.mark.parametrize("name", ["sizes", "odd_views", "many33", "many65"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_sumsq_matches_fp64(dtype, name):
    ts = _case(dtype, name)
    ref = _norm64(ts)
    a = _sumsq(ts)
    b = _sumsq(ts)
    got = math.sqrt(a.item())
    print(f"sumsq {name} {dtype}: norm {got!r} ref {ref!r} "
          f"rel {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= 1e-5 * ref
    assert torch.equal(a, b), "two calls must be bit-identical"
    # accumulate over two lists == one call over both
    half = len(ts) // 2
    acc = _sumsq(ts[:half])
    _sumsq(ts[half:], out=acc, accumulate=True)
    assert abs(math.sqrt(acc.item()) - ref) <= 1e-5 * ref
    # the ops entry point agrees with the raw kernel
    from pdnlp_amd import ops
    assert torch.equal(ops.grad_sumsq(ts), a)


def test_sumsq_accumulates_in_fp32_not_in_the_input_dtype():
    t = torch.full((4096,), 1e4, dtype=torch.float16, device=DEV)
    out = _sumsq([t])                       # 1e8 per square: inf in fp16
    assert out.item() == pytest.approx(4096 * 1e8, rel=1e-5)


def test_sumsq_empty_and_zero_size():
    assert _sumsq([]).item() == 0.0
    z = torch.empty(0, device=DEV)
    assert _sumsq([z, z]).item() == 0.0
    keep = torch.full((1,), 5.0, device=DEV)
    _sumsq([], out=keep, accumulate=True)
    _sumsq([z], out=keep, accumulate=True)
    assert keep.item() == 5.0
    from pdnlp_amd import ops
    assert ops.grad_sumsq([z]).item() == 0.0


def test_sumsq_mixed_dtypes_through_ops():
    from pdnlp_amd import ops
    ts = _case(torch.float32, "sizes") + _case(torch.bfloat16, "many33")
    ref = _norm64(ts)
    got = math.sqrt(ops.grad_sumsq(ts).item())
    assert abs(got - ref) <= 1e-5 * ref


# ---- coefficient and in-place clip ----------------------------------------
def _ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of ``dtype`` at |x| (x fp32), normal range."""
    bits = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}[dtype]
    _, e = torch.frexp(x.abs().float())
    tiny = torch.finfo(dtype).tiny
    return torch.maximum(torch.ldexp(torch.ones_like(x), e - 1 - bits),
                         torch.full_like(x, tiny * 2.0 ** -bits))


@pytest.mark.parametrize("name", ["sizes", "odd_views", "many65"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_coef_norm_and_inplace_clip(dtype, name):
    from pdnlp_amd import ops
    src = _case(dtype, name)
    # fp32 torch reference (clip_grad_norm_ semantics)
    norm_ref = torch.sqrt(sum(t.float().pow(2).sum() for t in src)).item()
    max_norm = norm_ref / 4
    assert norm_ref >= 2 * max_norm
    coef_ref = min(1.0, max_norm / (norm_ref + 1e-6))
    coef, norm = ops.grad_clip_coef(src, max_norm)
    assert coef.dtype == norm.dtype == torch.float32
    assert coef.numel() == norm.numel() == 1 and coef.is_cuda
    assert abs(norm.item() - norm_ref) <= 1e-5 * norm_ref
    assert abs(coef.item() - coef_ref) <= 1e-5 * coef_ref
    # stand-alone finaliser == the one folded into the last stage
    c2, n2 = ops.clip_coef_from_sumsq(ops.grad_sumsq(src), max_norm)
    assert torch.equal(c2, coef) and torch.equal(n2, norm)

    # in place, on copies that keep the (mis)alignment of the originals
    if name == "odd_views":
        flat = torch.empty(1 + sum(t.numel() + 1 for t in src), dtype=dtype,
                           device=DEV)
        work, off = [], 1
        for t in src:
            v = flat[off:off + t.numel()]
            v.copy_(t)
            work.append(v)
            off += t.numel() + (t.numel() % 2)
    else:
        work = [t.clone() for t in src]
    out = ops.clip_grad_norm_(work, max_norm)
    assert torch.equal(out, norm)
    for w, t in zip(work, src):
        want = t.float() * coef
        err = (w.float() - want).abs()
        assert bool((err <= _ulp(want, dtype)).all()), (name, t.numel())
    # loose bound: coefficient exactly 1, nothing rewritten
    before = [w.clone() for w in work]
    ops.clip_grad_norm_(work, LOOSE)
    assert all(torch.equal(a, b) for a, b in zip(work, before))


def test_nonfinite_norm_propagates():
    from pdnlp_amd import ops
    bad = [torch.tensor([1.0, float("inf")], device=DEV)]
    coef, norm = ops.grad_clip_coef(bad, 1.0)
    assert math.isinf(norm.item()) and coef.item() == 0.0
    bad = [torch.tensor([1.0, float("nan")], device=DEV)]
    coef, norm = ops.grad_clip_coef(bad, 1.0)
    assert math.isnan(norm.item()) and math.isnan(coef.item())


# ---- optimizer kernels -------------------------------------------------------
def _opt_state(dtype, master):
    g = torch.Generator().manual_seed(5)
    shapes = [(1025,), (64, 33), (7,)]
    p = [torch.randn(*s, generator=g).to(dtype).to(DEV) for s in shapes]
    gr = [(torch.randn(*s, generator=g) * 0.1).to(dtype).to(DEV)
          for s in shapes]
    m = [torch.zeros(*s, device=DEV) for s in shapes]
    v = [torch.zeros(*s, device=DEV) for s in shapes]
    mw = [t.float().clone() for t in p] if master else []
    return p, gr, m, v, mw


@pytest.mark.parametrize("dtype,master", [(torch.float32, False),
                                          (torch.bfloat16, True),
                                          (torch.float16, True)],
                         ids=["fp32", "bf16-master", "fp16-master"])
def test_adamw_grad_coef_bitwise(dtype, master):
    c = 0.37
    cdev = torch.tensor([c], device=DEV)
    c32 = cdev.item()
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001)
    none = torch.Tensor()

    def run(gsi, **kw):
        p, g, m, v, mw = _opt_state(dtype, master)
        ext().multi_tensor_adamw(p, g, m, v, mw, *hp, gsi, none, **kw)
        return p + m + v + mw

    with_coef = run(1.0, grad_coef=cdev)
    with_gsi = run(c32)
    for a, b in zip(with_coef, with_gsi):
        assert torch.equal(a, b)
    plain = run(1.0)                      # the existing 14-argument form
    explicit_none = run(1.0, grad_coef=None)
    for a, b in zip(plain, explicit_none):
        assert torch.equal(a, b)
    assert not torch.equal(plain[len(plain) // 2], with_coef[len(plain) // 2])


@pytest.mark.parametrize("dtype,master", [(torch.float32, False),
                                          (torch.bfloat16, True)],
                         ids=["fp32", "bf16-master"])
def test_sgd_grad_coef_bitwise(dtype, master):
    cdev = torch.tensor([0.37], device=DEV)
    c32 = cdev.item()
    none = torch.Tensor()

    def run(gsi, **kw):
        p, g, buf, _, mw = _opt_state(dtype, master)
        ext().multi_tensor_sgd(p, g, buf, mw, 0.1, 0.9, 0.01, gsi, none, **kw)
        return p + buf + mw

    for a, b in zip(run(1.0, grad_coef=cdev), run(c32)):
        assert torch.equal(a, b)
    for a, b in zip(run(1.0), run(1.0, grad_coef=None)):
        assert torch.equal(a, b)


def test_clip_and_fused_step_never_sync_the_host():
    from pdnlp_amd import ops
    from pdnlp_amd.ops.adamw import FusedAdamW
    params = [torch.nn.Parameter(t.clone())
              for t in _case(torch.bfloat16, "many33")]
    for p in params:
        p.grad = torch.ones_like(p)
    opt = FusedAdamW(params, lr=1e-3)
    opt.step()                             # allocate the state up front
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        coef, norm = ops.grad_clip_coef([p.grad for p in params], 0.5)
        opt.step(grad_coef=coef)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert norm.item() > 1.0 and coef.item() < 1.0


# ---- Trainer ----------------------------------------------------------------
def _tiny_bf16(seed=123):
    from pdnlp_amd.config import BertConfig
    from pdnlp_amd.models import BertForSequenceClassification
    from pdnlp_amd.utils import set_seed
    set_seed(seed)
    m = BertForSequenceClassification(BertConfig.tiny())
    return m.to(torch.bfloat16).to(DEV)


def _loader(n, bs=8):
    from torch.utils.data import DataLoader
    from pdnlp_amd.config import BertConfig
    from pdnlp_amd.data import Collate, SyntheticClsDataset
    ds = SyntheticClsDataset(n, seq_len=16,
                             vocab_size=BertConfig.tiny().vocab_size)
    return DataLoader(ds, batch_size=bs, shuffle=False,
                      collate_fn=Collate(None, 16))


def _args(tmp_path, **kw):
    from pdnlp_amd.config import Args
    args = Args()
    args.epochs = 1
    args.do_dev = False
    args.log_every = 100
    args.output_dir = str(tmp_path)
    args.ckpt_path = str(tmp_path / "model.pt")
    for k, v in kw.items():
        setattr(args, k, v)
    return args


LR = 0.1


def _plain_sgd(model):
    from pdnlp_amd.ops.adamw import FusedSGD
    return FusedSGD(model.parameters(), lr=LR, momentum=0.0)


def _masters(opt):
    return [opt.state[p]["master"].clone()
            for g in opt.param_groups for p in g["params"]]


def _delta_norm(after, before):
    return math.sqrt(sum((a.double() - b.double()).pow(2).sum().item()
                         for a, b in zip(after, before)))


def _trainer_run(tmp_path, max_grad_norm, n=24):
    from pdnlp_amd.engine.trainer import Trainer
    model = _tiny_bf16()
    opt = _plain_sgd(model)
    tr = Trainer(_args(tmp_path, max_grad_norm=max_grad_norm), model, opt, DEV)
    tr.train(_loader(n))
    return model, opt, tr


def test_trainer_sgd_matches_fp32_torch_clip(tmp_path):
    max_norm = 0.25
    # reference: same seeds, same kernels, the clip done with fp32 torch ops
    ref = _tiny_bf16()
    ref.train()
    ropt = _plain_sgd(ref)
    start = [p.detach().float().clone() for p in ref.parameters()]
    norms = []
    for batch in _loader(24):
        ref(input_ids=batch["input_ids"].to(DEV),
            attention_mask=batch["attention_mask"].to(DEV),
            token_type_ids=batch["token_type_ids"].to(DEV),
            labels=batch["label"].to(DEV)).loss.backward()
        grads = [p.grad for p in ref.parameters()]
        norm = torch.sqrt(sum(g.float().pow(2).sum() for g in grads))
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        for p in ref.parameters():
            p.grad = (p.grad.float() * coef).to(p.grad.dtype)
        norms.append(norm.item())
        ropt.step()
        ropt.zero_grad(set_to_none=True)
    assert len(norms) == 3 and min(norms) >= 2 * max_norm, norms

    model, opt, tr = _trainer_run(tmp_path, max_norm)
    for (n, p), rp in zip(model.named_parameters(), ref.parameters()):
        torch.testing.assert_close(p.data.float(), rp.data.float(),
                                   rtol=2e-2, atol=2e-2, msg=n)
    print("last_grad_norm", tr.last_grad_norm.item(), "ref", norms[-1])
    assert abs(tr.last_grad_norm.item() - norms[-1]) <= 1e-2 * norms[-1]
    # three clipped plain-SGD steps cannot move the weights further than
    # 3 * lr * max_norm (fp32 masters; 1% slack for the bf16 gradients)
    moved = _delta_norm(_masters(opt), start)
    print("moved", moved, "bound", 3 * LR * max_norm)
    assert 0 < moved <= 3 * LR * max_norm * (1 + 1e-2)


def test_trainer_loose_bound_bit_identical(tmp_path):
    free, _, tr0 = _trainer_run(tmp_path, 0.0)
    model, _, tr = _trainer_run(tmp_path, LOOSE)
    assert tr0.last_grad_norm is None and tr.last_grad_norm is not None
    for (n, p), q in zip(model.named_parameters(), free.parameters()):
        assert torch.equal(p.data, q.data), n


def test_trainer_hip_graph_clips(tmp_path):
    """hip_graph=True used to ignore max_grad_norm: after capture, one
    replayed step may move the weights by at most lr * max_norm."""
    from pdnlp_amd.engine.trainer import Trainer
    max_norm = 0.05
    model = _tiny_bf16()
    opt = _plain_sgd(model)
    tr = Trainer(_args(tmp_path, max_grad_norm=max_norm, hip_graph=True),
                 model, opt, DEV)
    tr.train(_loader(40))                  # 3 eager steps, capture, replays
    assert tr._graph is not None, "graph was never captured"
    batch = next(iter(_loader(8)))
    before = _masters(opt)
    assert tr._graph_step(batch) is not None
    torch.cuda.synchronize()
    gnorm = _norm64([p.grad for p in model.parameters()])
    assert gnorm >= 2 * max_norm, gnorm
    moved = _delta_norm(_masters(opt), before)
    print("graph step: moved", moved, "lr*max_norm", LR * max_norm,
          "unclipped", LR * gnorm, "last_grad_norm", tr.last_grad_norm.item())
    assert moved <= LR * max_norm * (1 + 1e-2)
    assert moved < LR * gnorm
    assert abs(tr.last_grad_norm.item() - gnorm) <= 1e-2 * gnorm


def test_unpad_trainer_clips(tmp_path):
    """--unpad needs nothing new: one packed step is clipped like any."""
    from torch.utils.data import DataLoader
    from pdnlp_amd.config import BertConfig
    from pdnlp_amd.data import Collate, SyntheticClsDataset
    from pdnlp_amd.engine.trainer import build_training
    from pdnlp_amd.models import BertForSequenceClassification
    from pdnlp_amd.utils import set_seed
    set_seed(123)
    max_norm = 0.05
    cfg = BertConfig(vocab_size=1024, hidden_size=256, num_hidden_layers=2,
                     num_attention_heads=4, intermediate_size=1024,
                     hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0)
    args = _args(tmp_path, strategy="single", unpad=True, amp=True,
                 amp_dtype="bf16", optimizer="sgd", sgd_momentum=0.0,
                 weight_decay=0.0, learning_rate=LR, max_grad_norm=max_norm)
    model, opt, _, trainer = build_training(
        args, model=BertForSequenceClassification(cfg))
    before = [p.detach().float().clone() for g in opt.param_groups
              for p in g["params"]]
    ds = SyntheticClsDataset(16, seq_len=128, vocab_size=cfg.vocab_size,
                             var_len=True)
    trainer.train(DataLoader(ds, batch_size=16, shuffle=False,
                             collate_fn=Collate(None, 128, unpad=True)))
    norm = trainer.last_grad_norm.item()
    assert math.isfinite(norm) and norm >= 2 * max_norm, norm
    moved = _delta_norm(_masters(opt), before)
    assert 0 < moved <= LR * max_norm * (1 + 1e-2), moved


# ---- ZeRO on GPU tensors, world 2 ---------------------------------------------
def _zero_world2_clip_gpu(rank, world):
    """Sharded AdamW moments are linear in the coefficient: a clipped step's
    ``m_shard`` is ``coef`` times the unclipped one, with ``coef`` from the
    norm of the full averaged gradient (all shards of all groups)."""
    import torch.distributed as dist
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer
    dev = torch.device(f"cuda:{rank % torch.cuda.device_count()}")
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, 512, (8, 16), generator=g).to(dev)
    mask = torch.ones(8, 16, dtype=torch.long, device=dev)
    labels = torch.randint(0, 6, (8,), generator=g).to(dev)
    lo, hi = rank * 4, rank * 4 + 4

    def run(max_grad_norm):
        model = _tiny_bf16().to(dev)
        zopt = ZeroRedundancyOptimizer(model, lr=1e-3)
        zopt.max_grad_norm = max_grad_norm
        model(input_ids=ids[lo:hi], attention_mask=mask[lo:hi],
              labels=labels[lo:hi]).loss.backward()
        zopt.step()
        torch.cuda.synchronize()
        return model, zopt

    m0, z0 = run(0.0)
    sq = sum(g_.m_shard.double().pow(2).sum() for g_ in z0.groups)
    dist.all_reduce(sq)                   # shards are disjoint
    norm_ref = math.sqrt(sq.item()) / (1 - 0.9)   # m = (1 - beta1) * g
    max_norm = norm_ref / 4
    assert norm_ref >= 2 * max_norm
    coef_ref = max_norm / (norm_ref + 1e-6)
    m1, z1 = run(max_norm)
    assert abs(z1.last_grad_norm.item() - norm_ref) <= 1e-4 * norm_ref
    for a, b in zip(z0.groups, z1.groups):
        torch.testing.assert_close(b.m_shard, a.m_shard * coef_ref,
                                   rtol=1e-4, atol=1e-9)
    # loose bound == off, bit for bit, and ranks stay identical
    m2, z2 = run(LOOSE)
    for (n, p), q in zip(m2.named_parameters(), m0.parameters()):
        assert torch.equal(p.data, q.data), n
        t = p.data.clone()
        dist.broadcast(t, src=0)
        assert torch.equal(t, p.data), f"rank divergence in {n}"


def test_zero_world2_clips_on_gpu():
    from tests.utils_dist import run_distributed_gpu
    run_distributed_gpu(_zero_world2_clip_gpu, world=2)
