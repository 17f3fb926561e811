"""ZeRO sharded optimizer tests: single-process equivalence to AdamW,
2-rank (gloo) parity with DDP+AdamW, sharded checkpoint consolidation."""

import pytest
import torch

from tests.utils_dist import run_distributed

pytestmark = pytest.mark.timeout(300)


def _model_and_data(seed=123):
    from pdnlp_amd.config import BertConfig
    from pdnlp_amd.models import BertForSequenceClassification
    from pdnlp_amd.utils import set_seed
    set_seed(seed)
    cfg = BertConfig.tiny()
    model = BertForSequenceClassification(cfg)
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, cfg.vocab_size, (8, 16), generator=g)
    mask = torch.ones(8, 16, dtype=torch.long)
    labels = torch.randint(0, cfg.num_labels, (8,), generator=g)
    return cfg, model, ids, mask, labels


def test_zero_world1_matches_adamw():
    from pdnlp_amd.ops.adamw import build_optimizer
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer
    cfg, model, ids, mask, labels = _model_and_data()
    init = {k: v.clone() for k, v in model.state_dict().items()}

    zopt = ZeroRedundancyOptimizer(model, lr=1e-3)
    for _ in range(3):
        out = model(ids, mask, labels=labels)
        out.loss.backward()
        zopt.step()
        zopt.zero_grad()

    cfg2, ref, _, _, _ = _model_and_data()
    ref.load_state_dict(init)
    ropt = build_optimizer(ref, lr=1e-3)
    for _ in range(3):
        out = ref(ids, mask, labels=labels)
        ropt.zero_grad(set_to_none=False)
        out.loss.backward()
        ropt.step()

    for (n, p), (_, rp) in zip(model.named_parameters(), ref.named_parameters()):
        torch.testing.assert_close(p.data, rp.data, rtol=1e-4, atol=1e-6,
                                   msg=f"param {n}")


def _zero_world2_parity(rank, world):
    from pdnlp_amd.ops.adamw import build_optimizer
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer
    cfg, model, ids, mask, labels = _model_and_data()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    lo, hi = rank * 4, rank * 4 + 4

    zopt = ZeroRedundancyOptimizer(model, lr=1e-3)
    for _ in range(2):
        out = model(ids[lo:hi], mask[lo:hi], labels=labels[lo:hi])
        out.loss.backward()
        zopt.step()
        zopt.zero_grad()

    _, ref, _, _, _ = _model_and_data()
    ref.load_state_dict(init)
    ropt = build_optimizer(ref, lr=1e-3)
    for _ in range(2):
        l0 = ref(ids[:4], mask[:4], labels=labels[:4]).loss
        l1 = ref(ids[4:], mask[4:], labels=labels[4:]).loss
        ropt.zero_grad(set_to_none=False)
        ((l0 + l1) / 2).backward()
        ropt.step()

    for (n, p), (_, rp) in zip(model.named_parameters(), ref.named_parameters()):
        torch.testing.assert_close(p.data, rp.data, rtol=2e-3, atol=1e-5,
                                   msg=f"param {n} rank {rank}")


def test_zero_world2_parity():
    run_distributed(_zero_world2_parity, world=2)


def _zero_ckpt(rank, world, tmpdir):
    from pdnlp_amd.parallel.zero import (ZeroRedundancyOptimizer,
                                         consolidate_zero_checkpoint)
    cfg, model, ids, mask, labels = _model_and_data()
    zopt = ZeroRedundancyOptimizer(model, lr=1e-3)
    out = model(ids, mask, labels=labels)
    out.loss.backward()
    zopt.step()
    zopt.zero_grad()
    zopt.save_checkpoint(tmpdir)
    torch.distributed.barrier()
    if rank == 0:
        sd = consolidate_zero_checkpoint(tmpdir)
        for n, p in model.named_parameters():
            torch.testing.assert_close(sd[n], p.data.float(), rtol=1e-5,
                                       atol=1e-6, msg=n)
    torch.distributed.barrier()
    # resume round-trip
    zopt2 = ZeroRedundancyOptimizer(model, lr=1e-3)
    zopt2.load_checkpoint(tmpdir)
    assert zopt2.step_count == 1


def test_zero_sharded_checkpoint(tmp_path):
    run_distributed(_zero_ckpt, world=2, args=(str(tmp_path),))


def test_zero_with_grad_scaler_world1():
    """AMP + ZeRO: GradScaler.unscale_ walks optimizer.param_groups —
    regression test for the missing attribute."""
    import torch
    from pdnlp_amd.amp import GradScaler
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(16, 16), torch.nn.Linear(16, 4))
    opt = ZeroRedundancyOptimizer(model, lr=1e-2)
    scaler = GradScaler(init_scale=8.0)
    x = torch.randn(4, 16)
    loss = model(x).square().mean()
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    assert not scaler._found_inf
    scaler.step(opt)
    scaler.update()
    opt.zero_grad()
    # LR scheduler contract: mutating param_groups["lr"] must take effect
    for pg in opt.param_groups:
        pg["lr"] = 5e-3
    loss = model(x).square().mean()
    loss.backward()
    opt.step()


def _zero_overflow_sync(rank, world):
    """Rank-divergent overflow: only rank 0's local grads contain inf.
    sync_found_inf must make BOTH ranks skip the step, keeping shard
    states identical."""
    import torch.distributed as dist
    from pdnlp_amd.amp import GradScaler
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer

    cfg, model, ids, mask, labels = _model_and_data()
    zopt = ZeroRedundancyOptimizer(model, lr=1e-3)
    scaler = GradScaler(init_scale=8.0)
    before = {k: v.clone() for k, v in model.state_dict().items()}

    out = model(ids, mask, labels=labels)
    scaler.scale(out.loss).backward()
    if rank == 0:  # poison ONE rank's local grads
        p0 = next(model.parameters())
        p0.grad.view(-1)[0] = float("inf")
    scaler.unscale_(zopt)
    scaler.sync_found_inf()
    assert scaler._found_inf, f"rank {rank} must see the global flag"
    if not scaler._found_inf:
        zopt.step()
    scaler.update()
    assert scaler.get_scale() == 4.0, "backoff applied on both ranks"

    # params unchanged and identical across ranks
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
        t = v.clone()
        dist.broadcast(t, src=0)
        assert torch.equal(t, v), f"rank divergence in {k}"


def test_zero_overflow_sync_world2():
    run_distributed(_zero_overflow_sync, world=2)


def _zero_fp16_through_trainer(rank, world, out_dir):
    """The Trainer's ZeRO+scaler branch (unscale -> sync_found_inf ->
    device/sync skip -> update) end-to-end at world=2 on gloo."""
    from torch.utils.data import DataLoader
    from pdnlp_amd.amp import GradScaler
    from pdnlp_amd.config import Args
    from pdnlp_amd.data import Collate, SyntheticClsDataset
    from pdnlp_amd.engine.trainer import Trainer
    from pdnlp_amd.parallel.zero import ZeroRedundancyOptimizer

    cfg, model, *_ = _model_and_data()
    args = Args()
    args.epochs = 1
    args.do_dev = False
    args.log_every = 100
    # the end-of-training checkpoint goes to the test's tmp dir, not to the
    # default ./output/model.pt of whatever directory pytest runs from
    args.output_dir = out_dir
    args.ckpt_path = out_dir + "/model.pt"
    zopt = ZeroRedundancyOptimizer(model, lr=1e-3)
    scaler = GradScaler(init_scale=8.0)
    ds = SyntheticClsDataset(16, seq_len=16, vocab_size=cfg.vocab_size)
    loader = DataLoader(ds, batch_size=4, shuffle=False,
                        collate_fn=Collate(None, 16))
    tr = Trainer(args, model, zopt, "cpu", scaler=scaler)
    tr.train(loader)
    assert tr.global_step == len(loader)
    # ranks identical after sharded fp16 steps
    import torch.distributed as dist
    for n, p in model.named_parameters():
        t = p.data.clone()
        dist.broadcast(t, src=0)
        assert torch.equal(t, p.data), f"rank divergence in {n}"
    # scale bookkeeping ran (no overflow in this clean run -> unchanged)
    assert scaler.get_scale() == 8.0


def test_zero_fp16_through_trainer_world2(tmp_path):
    run_distributed(_zero_fp16_through_trainer, world=2,
                    args=(str(tmp_path),))
