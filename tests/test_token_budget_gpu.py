"""Token-budget batching (``--unpad true --max-tokens N``) on the GPU: the
``ignore_index`` cross-entropy kernels against torch in fp64, empty
sequences in the variable-length attention kernels, budgeted-vs-plain packed
model equivalence on the HIP path, and one hipGraph serving every budgeted
batch of a Trainer run."""

import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_unpad_gpu import PACKED_VS_PADDED_BOUND, _model_cfg, ext
from tests.test_unpad_gpu import _rel as _rel_tensor

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = "cuda:0"
NH, HD = 2, 64
H = NH * HD
SCALE = 1.0 / math.sqrt(HD)
CE_TOL = dict(rtol=1e-5, atol=1e-6)   # as test_kernels_gpu::test_cross_entropy


def _rel(a, b, ref):
    """The metric of test_unpad_gpu; the scalar loss has no spread, so its
    denominator is that metric's floor of 1."""
    if ref.numel() == 1:
        return (a - b).abs().max().item()
    return _rel_tensor(a, b, ref)


# ------------------------------------------------------- 9: cross-entropy
def _ce_ref64(logits, labels, scale, **kw):
    lr = logits.double().detach().requires_grad_()
    loss = F.cross_entropy(lr, labels, **kw)
    (loss * scale).backward()
    return loss.float(), lr.grad.float()


@pytest.mark.parametrize("C", [6, 130])
def test_cross_entropy_ignore_index_kernels(C):
    from pdnlp_amd import ops
    B = 70
    torch.manual_seed(9)
    logits = torch.randn(B, C, device=DEV) * 3
    labels = torch.randint(0, C, (B,), device=DEV)
    ignored = torch.arange(B, device=DEV) % 3 == 0    # rows 0, 3, ..., 69
    assert ignored[0] and ignored[69] and 20 <= int(ignored.sum()) <= 26
    labels[ignored] = -100

    lg = logits.clone().requires_grad_()
    loss = ops.cross_entropy(lg, labels, ignore_index=-100)
    (loss * 1.7).backward()
    ref_loss, ref_grad = _ce_ref64(logits, labels, 1.7, ignore_index=-100)
    print(f"C={C}: loss {loss.item():.7f} ref {ref_loss.item():.7f}; dlogits "
          f"max err {(lg.grad - ref_grad).abs().max().item():.3e}")
    torch.testing.assert_close(loss, ref_loss, **CE_TOL)
    torch.testing.assert_close(lg.grad, ref_grad, **CE_TOL)
    assert (lg.grad[ignored] == 0).all(), "ignored rows: exactly zero gradient"
    assert (lg.grad[~ignored] != 0).any()

    # the raw binding: the valid-row count is a device tensor
    e = ext()
    l2, logprobs, nvalid = e.cross_entropy_ignore_fwd(logits, labels, -100)
    assert nvalid.is_cuda and nvalid.item() == int((~ignored).sum())
    assert torch.equal(l2, loss.detach())   # deterministic reduction
    torch.testing.assert_close(logprobs.double(),
                               F.log_softmax(logits.double(), -1),
                               rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("C", [6, 130])
def test_cross_entropy_ignore_index_without_ignored_rows(C):
    from pdnlp_amd import ops
    B = 70
    torch.manual_seed(10)
    logits = torch.randn(B, C, device=DEV) * 3
    labels = torch.randint(0, C, (B,), device=DEV)
    a = logits.clone().requires_grad_()
    b = logits.clone().requires_grad_()
    la = ops.cross_entropy(a, labels, ignore_index=-100)
    lb = ops.cross_entropy(b, labels)
    (la * 1.7).backward()
    (lb * 1.7).backward()
    torch.testing.assert_close(la, lb, **CE_TOL)
    torch.testing.assert_close(a.grad, b.grad, **CE_TOL)
    ref_loss, ref_grad = _ce_ref64(logits, labels, 1.7)
    torch.testing.assert_close(la, ref_loss, **CE_TOL)
    torch.testing.assert_close(a.grad, ref_grad, **CE_TOL)


# ------------------------------------------ 10: empty sequences in attention
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_varlen_attention_empty_sequences_are_free(p):
    e = ext()
    T, mx = 192, 128
    torch.manual_seed(4)
    qkv = torch.randn(T, 3 * H, device=DEV, dtype=torch.bfloat16)
    dout = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV) if p \
        else torch.Tensor()
    res = []
    for cu in ([0, 5, 5, 70, 70, 70, 133], [0, 5, 70, 133]):
        cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
        o, lse = e.flash_attn_varlen_fwd(qkv, cu_t, mx, NH, SCALE, p, seed, 7)
        dqkv = e.flash_attn_varlen_bwd(dout, qkv, o, lse, cu_t, mx, NH, SCALE,
                                       p, seed, 7)
        assert torch.isfinite(o).all() and torch.isfinite(dqkv).all()
        assert (o[133:] == 0).all() and (dqkv[133:] == 0).all()
        res.append((o, dqkv))
    assert res[0][0][:133].abs().sum() > 0
    assert torch.equal(res[0][0], res[1][0]), "context must be bit-equal"
    assert torch.equal(res[0][1], res[1][1]), "dqkv must be bit-equal"


# ------------------------------------------------ 11: model equivalence (HIP)
BUDGET_LENGTHS = {"tail-rows": [1, 64, 65, 17, 40],
                  "exact-fill-clamp": [128, 64, 64]}
# budgeted against plain packed, in the metric of test_unpad_gpu (max|a-b| /
# max(std|ref|, 1), ref = the fp32 CPU run): its packed-vs-padded bound, the
# tighter of its two length sets. The two runs here differ in less than
# those do (same kernels per row; only T, the block count of the attention
# grid and the loss reduction change).
BUDGET_BOUND = min(PACKED_VS_PADDED_BOUND.values())


def _padded_batch(lens, S, seed):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(106, 1024, (len(lens), S), generator=g) * mask
    return {"input_ids": ids, "attention_mask": mask,
            "token_type_ids": torch.zeros_like(ids),
            "label": torch.randint(0, 6, (len(lens),), generator=g)}


def _packed_inputs(p, device):
    return dict(input_ids=p["input_ids"].to(device),
                token_type_ids=p["token_type_ids"].to(device),
                labels=p["label"].to(device),
                cu_seqlens=p["cu_seqlens"].to(device),
                max_seqlen=p["max_seqlen"],
                position_ids=p["position_ids"].to(device))


def _run_packed(model, device, p, n_real):
    model.zero_grad(set_to_none=True)
    out = model(**_packed_inputs(p, device))
    out.loss.backward()
    res = {"loss": out.loss.detach().float().cpu().reshape(1),
           "logits": out.logits.detach().float().cpu()[:n_real]}
    assert torch.isfinite(out.logits).all()
    for n, q in model.named_parameters():
        res[n] = q.grad.detach().float().cpu()
    model.zero_grad(set_to_none=True)
    return res


@functools.lru_cache(maxsize=None)
def _budget_runs(name):
    """(fp32 CPU plain packed reference, HIP plain packed, HIP budgeted)."""
    from pdnlp_amd.data import pack_batch
    from pdnlp_amd.models import BertForSequenceClassification
    lens = BUDGET_LENGTHS[name]
    torch.manual_seed(123)
    gpu_model = BertForSequenceClassification(_model_cfg()).to(torch.bfloat16)
    cpu_model = copy.deepcopy(gpu_model).float().train()
    gpu_model = gpu_model.to(DEV).train()
    batch = _padded_batch(lens, 128, seed=5)
    plain = pack_batch(batch)
    budget = pack_batch(batch, total_rows=256, seq_multiple=32)
    assert budget["input_ids"].numel() == 256
    assert budget["cu_seqlens"].numel() == 33
    n = len(lens)
    return (_run_packed(cpu_model, "cpu", plain, n),
            _run_packed(gpu_model, DEV, plain, n),
            _run_packed(gpu_model, DEV, budget, n))


@pytest.mark.parametrize("name", list(BUDGET_LENGTHS))
def test_budgeted_model_matches_plain_packed_hip(name):
    ref, plain, budget = _budget_runs(name)
    worst_ref = worst = 0.0
    for k in ref:
        e_ref = _rel(plain[k], ref[k], ref[k])
        e_bd = _rel(budget[k], plain[k], ref[k])
        worst_ref, worst = max(worst_ref, e_ref), max(worst, e_bd)
        print(f"{name} {k}: plain-vs-fp32 {e_ref:.3e}  budgeted-vs-plain "
              f"{e_bd:.3e}")
    print(f"{name} WORST plain-vs-fp32 {worst_ref:.3e}  budgeted-vs-plain "
          f"{worst:.3e}  bound {BUDGET_BOUND:.3e}")
    for k in ref:
        assert torch.isfinite(budget[k]).all(), k
        assert _rel(budget[k], plain[k], ref[k]) <= BUDGET_BOUND, k


# ----------------------------------------------------------- 12: graph replay
class _LengthsDs(torch.utils.data.Dataset):
    def __init__(self, lens, S=128):
        b = _padded_batch(lens, S, seed=9)
        self.items = [{k: v[i] for k, v in b.items()}
                      for i in range(len(lens))]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_one_graph_replays_every_budgeted_batch(tmp_path):
    """Every batch of the run is [256 rows, 32 sequences, ms 128]: one key,
    whatever the composition. Steps 1-3 are eager (GraphPolicy), step 4
    captures and replays, every later step replays. A replay of a batch
    then gives the loss, logits and gradients of an eager step on that
    batch from the same weights, within the bound of test_unpad_graph_gpu
    (the eager run's distance from the fp32 CPU reference)."""
    from pdnlp_amd.cli import token_budget_loader
    from pdnlp_amd.config import Args
    from pdnlp_amd.data import Collate
    from pdnlp_amd.engine.trainer import build_training, graph_key
    from pdnlp_amd.models import BertForSequenceClassification
    from pdnlp_amd.utils import set_seed
    set_seed(123)
    args = Args()
    args.strategy = "single"
    args.unpad, args.max_tokens, args.hip_graph = True, 256, True
    args.amp, args.amp_dtype = True, "bf16"
    args.epochs, args.do_dev, args.log_every = 1, False, 1000
    args.learning_rate = 5e-4
    args.num_workers = 0
    args.output_dir = str(tmp_path)
    args.ckpt_path = str(tmp_path / "model.pt")
    model, opt, scaler, trainer = build_training(
        args, model=BertForSequenceClassification(_model_cfg()))
    g = torch.Generator().manual_seed(11)
    lens = torch.randint(9, 100, (40,), generator=g).tolist()
    loader, sampler = token_budget_loader(
        args, _LengthsDs(lens), Collate(None, 128, unpad=True), 1, 0)
    steps = len(sampler)
    assert 7 <= steps <= 12, steps
    batches = list(loader)
    assert {graph_key(b, 128) for b in batches} == {("packed", 256, 32, 128)}
    assert len({tuple(b["cu_seqlens"].tolist()) for b in batches}) == steps
    assert len({b["num_seqs"] for b in batches}) > 1

    losses = []
    orig = trainer.train_step

    def spy(batch, accum_boundary=True):
        res = orig(batch, accum_boundary)
        losses.append(res[0].detach().clone())   # a replay's loss is reused
        return res

    trainer.train_step = spy
    trainer.train(loader, train_sampler=sampler)
    print("graph_stats", trainer.graph_stats)
    assert scaler is None and trainer.global_step == steps
    assert trainer.graph_stats == {"captured": 1, "replayed": steps - 3,
                                   "eager": 3}
    assert len(trainer._graph) == 1
    assert all(math.isfinite(l.item()) for l in losses)

    # replay against eager on the same batch, from the weights as they stand
    (entry,) = trainer._graph.values()
    cpu_model = copy.deepcopy(model).cpu().float().train()
    for batch in (batches[0], batches[-1]):
        n = batch["num_seqs"]
        ref = _run_packed(cpu_model, "cpu", batch, n)
        loss, logits, _ = entry.run(batch)
        got = {"loss": loss.float().cpu().reshape(1),
               "logits": logits.float().cpu()[:n]}
        for (name, _), gr in zip(model.named_parameters(), entry.grads):
            got[name] = gr.float().cpu()
        trainer._release_graph_grads()
        eager = _run_packed(model, DEV, batch, n)
        bound = max(_rel(eager[k], ref[k], ref[k]) for k in ref)
        worst = max(_rel(got[k], eager[k], ref[k]) for k in ref)
        print(f"replay-vs-eager {worst:.3e}  bound (eager-vs-fp32) "
              f"{bound:.3e}; loss replay {got['loss'].item():.6f} eager "
              f"{eager['loss'].item():.6f}")
        for k in ref:
            assert torch.isfinite(got[k]).all(), k
            assert _rel(got[k], eager[k], ref[k]) <= bound, k
