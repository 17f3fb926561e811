"""Global-norm gradient clipping on the CPU (torch) path: every strategy
must clip the gradient the optimizer actually applies — the averaged one
under ZeRO / hooks, the unscaled one under fp16, the summed one under
accumulation — with torch ``clip_grad_norm_`` semantics.

An AdamW update is nearly invariant to a uniform gradient scale, so every
check observes something LINEAR in the coefficient: SGD parameters, AdamW
``exp_avg``, or the norm itself. Every clipping case asserts that the
reference norm is at least twice ``max_norm`` (the clip engages); the
"loose" cases use a ``max_norm`` above the norm and must be bit-identical to
an unclipped run.
"""

import json

import pytest
import torch
from torch.utils.data import DataLoader

from tests.utils_dist import run_distributed

pytestmark = pytest.mark.timeout(300)

LOOSE = 1e6  # a max_norm far above any gradient norm here


# ---------------------------------------------------------------------------
def _fresh_model(seed=123):
    from pdnlp_amd.config import BertConfig
    from pdnlp_amd.models import BertForSequenceClassification
    from pdnlp_amd.utils import set_seed
    set_seed(seed)
    return BertForSequenceClassification(BertConfig.tiny())


def _batches(n=12, bs=4):
    from pdnlp_amd.config import BertConfig
    from pdnlp_amd.data import Collate, SyntheticClsDataset
    ds = SyntheticClsDataset(n, seq_len=16,
                             vocab_size=BertConfig.tiny().vocab_size)
    return DataLoader(ds, batch_size=bs, shuffle=False,
                      collate_fn=Collate(None, 16))


def _loss(model, batch, label_key="label"):
    return model(input_ids=batch["input_ids"],
                 attention_mask=batch["attention_mask"],
                 token_type_ids=batch["token_type_ids"],
                 labels=batch[label_key]).loss


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


def _sgd(model, lr=0.1):
    from pdnlp_amd.ops.adamw import build_optimizer
    return build_optimizer(model, lr=lr, optimizer="sgd")


def _adamw(model, lr=1e-3):
    from pdnlp_amd.ops.adamw import build_optimizer
    return build_optimizer(model, lr=lr)


def _reference_run(make_opt, loader, max_norm, accum=1):
    """The plain loop with torch's own clip: forward, backward, (at the
    accumulation boundary) clip_grad_norm_, step, zero_grad."""
    model = _fresh_model()
    model.train()
    opt = make_opt(model)
    norms = []
    for i, batch in enumerate(loader):
        (_loss(model, batch) / accum).backward()
        if (i + 1) % accum:
            continue
        if max_norm:
            norms.append(torch.nn.utils.clip_grad_norm_(
                model.parameters(), max_norm).item())
        opt.step()
        opt.zero_grad(set_to_none=True)
    return model, opt, norms


def _trainer_run(make_opt, loader, tmp_path, scaler=None, **argkw):
    from pdnlp_amd.engine.trainer import Trainer
    model = _fresh_model()
    opt = make_opt(model)
    tr = Trainer(_args(tmp_path, **argkw), model, opt, "cpu", scaler=scaler)
    tr.train(loader)
    return model, opt, tr


def _assert_params(model, ref, **tol):
    for (n, p), (_, rp) in zip(model.named_parameters(),
                               ref.named_parameters()):
        if tol:
            torch.testing.assert_close(p.data, rp.data, msg=f"param {n}",
                                       **tol)
        else:
            assert torch.equal(p.data, rp.data), f"param {n} differs"


def _full_norm(grads):
    return float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads)))


# ---- ops layer, torch path -------------------------------------------------
def test_ops_match_torch_clip():
    from pdnlp_amd import ops
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(n, generator=g) for n in (1, 5, 1023, 0, 4097)]
    ref = [t.clone() for t in grads]
    total = torch.sqrt(sum(t.double().pow(2).sum() for t in ref)).item()
    max_norm = total / 4
    assert total >= 2 * max_norm
    coef, norm = ops.grad_clip_coef(grads, max_norm)
    assert coef.dtype == norm.dtype == torch.float32
    assert coef.numel() == norm.numel() == 1
    torch.testing.assert_close(norm.item(), total, rtol=1e-5, atol=0)
    torch.testing.assert_close(coef.item(), max_norm / (total + 1e-6),
                               rtol=1e-5, atol=0)
    params = [torch.nn.Parameter(t.clone()) for t in ref]
    for p, t in zip(params, ref):
        p.grad = t.clone()
    tnorm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    out = ops.clip_grad_norm_(grads, max_norm)
    torch.testing.assert_close(out.item(), tnorm.item(), rtol=1e-5, atol=0)
    for t, p in zip(grads, params):
        torch.testing.assert_close(t, p.grad, rtol=1e-5, atol=1e-8)
    # accumulate, empty list, zero-size
    s = ops.grad_sumsq(ref[:2])
    ops.grad_sumsq(ref[2:], out=s, accumulate=True)
    torch.testing.assert_close(s.item(), total * total, rtol=1e-5, atol=0)
    assert ops.grad_sumsq([]).item() == 0.0
    # loose bound: coefficient exactly 1, gradients untouched
    before = [t.clone() for t in grads]
    ops.clip_grad_norm_(grads, LOOSE)
    assert all(torch.equal(a, b) for a, b in zip(grads, before))
    # a non-finite norm propagates, as in torch (error_if_nonfinite=False)
    bad = [torch.tensor([1.0, float("nan")])]
    coef, norm = ops.grad_clip_coef(bad, 1.0)
    assert torch.isnan(norm).all() and torch.isnan(coef).all()


def test_optimizers_take_grad_coef():
    """FusedSGD / FusedAdamW with grad_coef=c == the same step on c*g."""
    from pdnlp_amd.ops.adamw import FusedAdamW, FusedSGD
    c = torch.tensor([0.25])
    for cls, kw in ((FusedSGD, dict(lr=0.1, momentum=0.9)),
                    (FusedAdamW, dict(lr=1e-2))):
        torch.manual_seed(0)
        a = [torch.nn.Parameter(torch.randn(7, 3))]
        b = [torch.nn.Parameter(a[0].detach().clone())]
        g = torch.randn(7, 3)
        a[0].grad = g.clone()
        b[0].grad = g * 0.25   # exact: power of two
        oa, ob = cls(a, **kw), cls(b, **kw)
        oa.step(grad_coef=c)
        ob.step()
        assert torch.equal(a[0].data, b[0].data), cls.__name__
        assert torch.equal(a[0].grad, g), "grad_coef must not rewrite grads"


# ---- Trainer, single process -------------------------------------------------
def test_trainer_sgd_matches_torch_clip(tmp_path):
    max_norm = 0.25
    ref, _, norms = _reference_run(_sgd, _batches(), max_norm)
    assert len(norms) == 3 and min(norms) >= 2 * max_norm, norms
    model, _, tr = _trainer_run(_sgd, _batches(), tmp_path,
                                max_grad_norm=max_norm)
    _assert_params(model, ref, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(tr.last_grad_norm.item(), norms[-1],
                               rtol=1e-5, atol=0)
    # and the clip really moved the result: the unclipped run differs
    free, _, _ = _reference_run(_sgd, _batches(), 0.0)
    assert not all(torch.equal(p, q) for p, q in zip(
        model.parameters(), free.parameters()))


def test_trainer_loose_bound_is_bit_identical(tmp_path):
    free, _, _ = _reference_run(_sgd, _batches(), 0.0)
    model, _, tr = _trainer_run(_sgd, _batches(), tmp_path,
                                max_grad_norm=LOOSE)
    _assert_params(model, free)
    assert tr.last_grad_norm is not None


def test_trainer_grad_accum_clips_once_on_the_sum(tmp_path):
    max_norm = 0.25
    ref, _, norms = _reference_run(_sgd, _batches(n=16), max_norm, accum=2)
    assert len(norms) == 2 and min(norms) >= 2 * max_norm, norms
    model, _, tr = _trainer_run(_sgd, _batches(n=16), tmp_path,
                                max_grad_norm=max_norm, grad_accum_steps=2)
    _assert_params(model, ref, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(tr.last_grad_norm.item(), norms[-1],
                               rtol=1e-5, atol=0)


def test_trainer_fp16_scaler_clips_unscaled_grads(tmp_path):
    """Sync GradScaler path: the norm is the UNSCALED gradient's, the update
    is the clipped one, and an injected inf still skips the step."""
    from pdnlp_amd.amp import GradScaler
    from pdnlp_amd.engine.trainer import Trainer
    max_norm = 0.25
    loader = _batches(n=4)
    ref, _, norms = _reference_run(_sgd, loader, max_norm)
    assert norms[0] >= 2 * max_norm
    scaler = GradScaler(init_scale=8.0)
    model, _, tr = _trainer_run(_sgd, loader, tmp_path, scaler=scaler,
                                max_grad_norm=max_norm)
    torch.testing.assert_close(tr.last_grad_norm.item(), norms[0],
                               rtol=1e-5, atol=0)
    _assert_params(model, ref, rtol=1e-5, atol=1e-7)
    assert scaler.get_scale() == 8.0

    # overflow: the step is skipped, the scale backs off
    before = [p.detach().clone() for p in model.parameters()]
    batch = next(iter(loader))
    loss, _, _ = tr.on_step(batch)
    assert tr._backward_and_step(loss * float("inf"), True)
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p.data, q)
    assert scaler.get_scale() == 4.0


def test_grad_norm_in_metrics_on_logged_steps_only(tmp_path):
    path = tmp_path / "m.jsonl"
    _trainer_run(_sgd, _batches(n=16), tmp_path, max_grad_norm=0.25,
                 log_every=2, metrics_jsonl=str(path))
    recs = [json.loads(line) for line in open(path)]
    train = [r for r in recs if r.get("phase") == "train"]
    assert [r["step"] for r in train] == [2, 4]
    for r in train:
        assert r["grad_norm"] >= 0.5
    assert all("grad_norm" not in r for r in recs if r.get("phase") != "train")
    # off: the record is what it was
    path0 = tmp_path / "m0.jsonl"
    _trainer_run(_sgd, _batches(n=16), tmp_path, max_grad_norm=0.0,
                 log_every=2, metrics_jsonl=str(path0))
    assert all("grad_norm" not in json.loads(line) for line in open(path0))


# ---- off switch -------------------------------------------------------------
def test_off_switch_adamw_bit_identical(tmp_path):
    ref, ropt, _ = _reference_run(_adamw, _batches(), 0.0)
    model, opt, tr = _trainer_run(_adamw, _batches(), tmp_path,
                                  max_grad_norm=0.0)
    _assert_params(model, ref)
    assert tr.last_grad_norm is None


def test_off_switch_zero_world1_bit_identical(tmp_path):
    from pdnlp_amd.engine.trainer import Trainer
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer
    ref = _fresh_model()
    ref.train()
    ropt = ZeroRedundancyOptimizer(ref, lr=1e-3)
    for batch in _batches():
        _loss(ref, batch).backward()
        ropt.step()
        ropt.zero_grad()
    model = _fresh_model()
    zopt = ZeroRedundancyOptimizer(model, lr=1e-3)
    assert zopt.max_grad_norm == 0.0
    tr = Trainer(_args(tmp_path, max_grad_norm=0.0), model, zopt, "cpu")
    tr.train(_batches())
    _assert_params(model, ref)
    # a loose bound goes through the clipped path and must agree bit for bit
    model2 = _fresh_model()
    zopt2 = ZeroRedundancyOptimizer(model2, lr=1e-3)
    zopt2.max_grad_norm = LOOSE
    tr2 = Trainer(_args(tmp_path, max_grad_norm=LOOSE), model2, zopt2, "cpu")
    tr2.train(_batches())
    _assert_params(model2, ref)
    assert tr2.last_grad_norm is zopt2.last_grad_norm is not None


# ---- wrapper APIs -----------------------------------------------------------
def _one_batch_reference(max_norm, label_key="label", bs=4):
    """Gradients, norm and coefficient of the first batch on a fresh model."""
    from pdnlp_amd.data import Collate, SyntheticClsDataset
    from pdnlp_amd.config import BertConfig
    ds = SyntheticClsDataset(bs, seq_len=16,
                             vocab_size=BertConfig.tiny().vocab_size)
    batch = Collate(None, 16, label_key=label_key)([ds[i] for i in range(bs)])
    ref = _fresh_model()
    ref.train()
    _loss(ref, batch, label_key).backward()
    grads = {n: p.grad.clone() for n, p in ref.named_parameters()}
    norm = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm).item()
    assert norm >= 2 * max_norm
    clipped = {n: p.grad.clone() for n, p in ref.named_parameters()}
    return ds, batch, grads, clipped, norm


def test_accelerator_clip_grad_norm(tmp_path):
    from pdnlp_amd.engine import Accelerator
    max_norm = 0.25
    _, batch, _, clipped, norm_ref = _one_batch_reference(max_norm)
    acc = Accelerator()
    model = _fresh_model()
    opt = _sgd(model)
    model, opt = acc.prepare(model, opt)
    acc.backward(_loss(model, batch))
    norm = acc.clip_grad_norm_(model.parameters(), max_norm)
    assert isinstance(norm, torch.Tensor) and norm.numel() == 1
    torch.testing.assert_close(norm.item(), norm_ref, rtol=1e-5, atol=0)
    for n, p in model.named_parameters():
        torch.testing.assert_close(p.grad, clipped[n], rtol=1e-5, atol=1e-9,
                                   msg=n)
    acc.step(opt, model)


def test_accelerator_fp16_unscales_before_clip(tmp_path):
    from pdnlp_amd.amp import GradScaler
    from pdnlp_amd.engine import Accelerator
    max_norm = 0.25
    _, batch, _, clipped, norm_ref = _one_batch_reference(max_norm)
    acc = Accelerator()
    acc.scaler = GradScaler(init_scale=8.0)   # fp32 model, scaled loss
    from pdnlp_amd.ops.adamw import FusedSGD
    model = _fresh_model()
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.0)
    acc.backward(_loss(model, batch))
    norm = acc.clip_grad_norm_(model.parameters(), max_norm)
    torch.testing.assert_close(norm.item(), norm_ref, rtol=1e-5, atol=0)
    for n, p in model.named_parameters():
        torch.testing.assert_close(p.grad, clipped[n], rtol=1e-5, atol=1e-9,
                                   msg=n)
    acc.step(opt, model)   # must not unscale a second time
    ref = _fresh_model()
    for (n, p), rp in zip(model.named_parameters(), ref.parameters()):
        torch.testing.assert_close(p.data, rp.data - 0.1 * clipped[n],
                                   rtol=1e-5, atol=1e-7, msg=n)


def test_fabric_clip_gradients(tmp_path):
    from pdnlp_amd.engine import Fabric
    max_norm = 0.25
    _, batch, _, clipped, norm_ref = _one_batch_reference(max_norm)
    fabric = Fabric(devices=1, precision="32-true")
    fabric.launch()
    model = _fresh_model()
    opt = _sgd(model)
    model, opt = fabric.setup(model, opt)
    fabric.backward(_loss(model, batch))
    norm = fabric.clip_gradients(model, opt, max_norm=max_norm)
    torch.testing.assert_close(norm.item(), norm_ref, rtol=1e-5, atol=0)
    for n, p in model.named_parameters():
        torch.testing.assert_close(p.grad, clipped[n], rtol=1e-5, atol=1e-9,
                                   msg=n)
    fabric.optimizer_step(opt, model)


def test_hf_trainer_max_grad_norm(tmp_path):
    """TrainingArguments.max_grad_norm reaches the engine: the norm is the
    reference's and AdamW's first moment is (1-b1) * coef * g."""
    from pdnlp_amd.data import Collate
    from pdnlp_amd.engine import HFStyleTrainer, TrainingArguments
    max_norm = 0.25
    ds, _, _, clipped, norm_ref = _one_batch_reference(max_norm,
                                                       label_key="labels")
    assert TrainingArguments().max_grad_norm == 0.0
    args = TrainingArguments(output_dir=str(tmp_path), save_strategy="no",
                             save_steps=0, evaluation_strategy="no",
                             per_device_train_batch_size=4, logging_steps=100,
                             load_best_model_at_end=False,
                             dataloader_num_workers=0,
                             max_grad_norm=max_norm)
    tr = HFStyleTrainer(_fresh_model(), args, train_dataset=ds,
                        data_collator=Collate(None, 16, label_key="labels"))
    assert tr.args.max_grad_norm == max_norm
    tr.train()
    torch.testing.assert_close(tr.engine.last_grad_norm.item(), norm_ref,
                               rtol=1e-5, atol=0)
    named = dict(tr.model.named_parameters())
    for n, g in clipped.items():
        m = tr.optimizer.state[named[n]]["exp_avg"]
        torch.testing.assert_close(m, 0.1 * g, rtol=1e-4, atol=1e-9, msg=n)


# ---- multi-process (gloo) ---------------------------------------------------
def _world2_reference(model_init, ids, mask, labels):
    """Single-process gradient of the averaged full batch."""
    ref = _fresh_model()
    ref.load_state_dict(model_init)
    ref.train()
    l0 = ref(ids[:4], mask[:4], labels=labels[:4]).loss
    l1 = ref(ids[4:], mask[4:], labels=labels[4:]).loss
    ((l0 + l1) / 2).backward()
    return ref


def _data():
    from pdnlp_amd.config import BertConfig
    cfg = BertConfig.tiny()
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, cfg.vocab_size, (8, 16), generator=g)
    mask = torch.ones(8, 16, dtype=torch.long)
    labels = torch.randint(0, cfg.num_labels, (8,), generator=g)
    return ids, mask, labels


def _zero_world2_clip(rank, world):
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer
    ids, mask, labels = _data()
    lo, hi = rank * 4, rank * 4 + 4
    model = _fresh_model()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    ref = _world2_reference(init, ids, mask, labels)
    g_ref = {n: p.grad.clone() for n, p in ref.named_parameters()}
    norm_ref = _full_norm(g_ref.values())
    max_norm = norm_ref / 4
    assert norm_ref >= 2 * max_norm
    coef_ref = max_norm / (norm_ref + 1e-6)

    zopt = ZeroRedundancyOptimizer(model, lr=1e-3)
    zopt.max_grad_norm = max_norm
    model(ids[lo:hi], mask[lo:hi], labels=labels[lo:hi]).loss.backward()
    zopt.step()
    torch.testing.assert_close(zopt.last_grad_norm.item(), norm_ref,
                               rtol=1e-4, atol=0)
    for g in zopt.groups:
        flat = torch.zeros(g.numel_padded)
        for n, off in zip(g.names, g.offsets):
            flat[off:off + g_ref[n].numel()] = g_ref[n].reshape(-1)
        shard = flat[rank * g.shard_size:(rank + 1) * g.shard_size]
        torch.testing.assert_close(
            g.m_shard, (1 - 0.9) * coef_ref * shard, rtol=1e-4, atol=1e-7,
            msg=f"m_shard rank {rank}")

    # loose bound == unclipped, bit for bit (parameters and moments)
    def run(max_grad_norm):
        m = _fresh_model()
        m.load_state_dict(init)
        z = ZeroRedundancyOptimizer(m, lr=1e-3)
        z.max_grad_norm = max_grad_norm
        m(ids[lo:hi], mask[lo:hi], labels=labels[lo:hi]).loss.backward()
        z.step()
        return m, z
    m0, z0 = run(0.0)
    m1, z1 = run(LOOSE)
    _assert_params(m1, m0)
    for a, b in zip(z0.groups, z1.groups):
        assert torch.equal(a.m_shard, b.m_shard)
        assert torch.equal(a.v_shard, b.v_shard)


def test_zero_world2_clips_the_averaged_gradient():
    run_distributed(_zero_world2_clip, world=2)


def _hooks_world2_clip(rank, world):
    from pdnlp_amd.ops.adamw import FusedSGD
    from pdnlp_amd.parallel.hooks import DistributedOptimizer
    ids, mask, labels = _data()
    lo, hi = rank * 4, rank * 4 + 4
    model = _fresh_model()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    ref = _world2_reference(init, ids, mask, labels)
    norm_ref = _full_norm(p.grad for p in ref.parameters())
    max_norm = norm_ref / 4
    assert norm_ref >= 2 * max_norm
    tnorm = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
    torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9).step()

    def run(max_grad_norm):
        m = _fresh_model()
        m.load_state_dict(init)
        opt = DistributedOptimizer(
            FusedSGD(m.parameters(), lr=0.1, momentum=0.9))
        opt.max_grad_norm = max_grad_norm
        m(ids[lo:hi], mask[lo:hi], labels=labels[lo:hi]).loss.backward()
        opt.step()
        return m, opt

    model, opt = run(max_norm)
    torch.testing.assert_close(opt.last_grad_norm.item(), tnorm.item(),
                               rtol=1e-4, atol=0)
    _assert_params(model, ref, rtol=1e-4, atol=1e-7)
    m0, _ = run(0.0)
    m1, _ = run(LOOSE)
    _assert_params(m1, m0)
    assert not all(torch.equal(p, q) for p, q in zip(
        model.parameters(), m0.parameters()))


def test_hooks_world2_clips_the_averaged_gradient():
    run_distributed(_hooks_world2_clip, world=2)
