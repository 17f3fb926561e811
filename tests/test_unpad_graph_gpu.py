"""hipGraph replay per batch key on the GPU (``--unpad true --hip-graph
true`` and the padded graph path): one captured graph serves batches with
other sequence boundaries, dropout reseeds per replay, and the Trainer
captures, replays, clips and keeps training across eager tail batches.

Bound of replay against eager: both run the same kernels on the same
inputs, so what separates them is the run-to-run order of the fp32 atomics
in the LayerNorm and embedding backward. The bound is computed per case:
the distance of that eager run from the fp32 CPU padded reference on the
same inputs, worst tensor, in the metric ``_rel`` of test_unpad_gpu.py.
Measured on an MI355X: see DESIGN.md "hipGraph replay per batch key".
"""

import copy
import functools
import math

import pytest
import torch

from tests.test_unpad_gpu import _model_cfg, _rel, _run

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = "cuda:0"
LR = 0.1

# name -> (max_seq_len, lengths A, lengths B); A and B pack to T = 320 with
# the same number of sequences, so they share one graph. "streamed": a
# 129-token sequence at max_seq_len 192 gives ms = 192, the attention
# kernels that stream K/V tiles instead of preloading them.
CASES = {
    "preload": (128, [5, 64, 1, 33, 128, 70], [70, 20, 100, 3, 64, 40]),
    "streamed": (192, [129, 70, 64, 40], [100, 129, 3, 70]),
}


def _padded_batch(lens, S, seed):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(106, 1024, (len(lens), S), generator=g) * mask
    return {"input_ids": ids, "attention_mask": mask,
            "token_type_ids": torch.zeros_like(ids),
            "label": torch.randint(0, 6, (len(lens),), generator=g)}


def _args(tmp_path=None, **kw):
    from pdnlp_amd.config import Args
    args = Args()
    args.strategy = "single"
    args.unpad = True
    args.hip_graph = True
    args.amp, args.amp_dtype = True, "bf16"
    args.epochs = 1
    args.do_dev = False
    args.log_every = 1000
    if tmp_path is not None:
        args.output_dir = str(tmp_path)
        args.ckpt_path = str(tmp_path / "model.pt")
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def _plain_sgd(model):
    from pdnlp_amd.ops.adamw import FusedSGD
    return FusedSGD(model.parameters(), lr=LR, momentum=0.0)


def _masters(opt):
    return [opt.state[p]["master"].clone()
            for g in opt.param_groups for p in g["params"]]


def _checksum(opt):
    ms = [opt.state[p]["master"] for g in opt.param_groups
          for p in g["params"]]
    return (sum(m.double().sum().item() for m in ms),
            sum(m.double().abs().sum().item() for m in ms))


@functools.lru_cache(maxsize=None)
def _case(name):
    """Model (bf16, on the GPU, never stepped), the packed batches A and B,
    and per batch the fp32 CPU padded reference and the eager packed HIP
    run: logits and every parameter gradient."""
    from pdnlp_amd.data import pack_batch
    from pdnlp_amd.models import BertForSequenceClassification
    S, lens_a, lens_b = CASES[name]
    torch.manual_seed(123)
    gpu_model = BertForSequenceClassification(_model_cfg()).to(torch.bfloat16)
    cpu_model = copy.deepcopy(gpu_model).float().train()
    gpu_model = gpu_model.to(DEV).train()
    packed, ref, eager = [], [], []
    for seed, lens in ((5, lens_a), (6, lens_b)):
        b = _padded_batch(lens, S, seed)
        p = pack_batch(b)
        assert p["input_ids"].numel() == 320
        ref.append(_run(cpu_model, "cpu", input_ids=b["input_ids"],
                        attention_mask=b["attention_mask"],
                        token_type_ids=b["token_type_ids"],
                        labels=b["label"]))
        eager.append(_run(gpu_model, DEV, input_ids=p["input_ids"],
                          token_type_ids=p["token_type_ids"],
                          labels=p["label"], cu_seqlens=p["cu_seqlens"],
                          max_seqlen=p["max_seqlen"],
                          position_ids=p["position_ids"]))
        packed.append(p)
    gpu_model.zero_grad(set_to_none=True)
    return gpu_model, packed, ref, eager


def _bound(ref, eager):
    return max(_rel(eager[k], ref[k], ref[k]) for k in ref)


def _replay(entry, model, batch):
    _, logits, _ = entry.run(batch)
    res = {"logits": logits.float().cpu()}
    for (n, _), g in zip(model.named_parameters(), entry.grads):
        res[n] = g.float().cpu()
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_one_graph_serves_other_boundaries(name):
    """Capture on A; replay A, B, A. Rows [297, 320) (preload) of B are
    padding that follows a replay of A with real tokens there: nothing of
    A may survive in the static buffers or the zero-filled outputs."""
    from pdnlp_amd.engine.trainer import Trainer, graph_key
    S = CASES[name][0]
    model, packed, ref, eager = _case(name)
    tr = Trainer(_args(max_seq_len=S), model, _plain_sgd(model), DEV)
    assert graph_key(packed[0], S) == graph_key(packed[1], S) \
        == ("packed", 320, len(CASES[name][1]), S)
    assert not torch.equal(packed[0]["cu_seqlens"], packed[1]["cu_seqlens"])
    entry = tr._capture_graph(packed[0])
    for which in (0, 1, 0):
        got = _replay(entry, model, packed[which])
        bound = _bound(ref[which], eager[which])
        worst = max(_rel(got[k], eager[which][k], ref[which][k])
                    for k in got)
        print(f"{name} replay of {'AB'[which]}: replay-vs-eager "
              f"{worst:.3e}  bound (eager-vs-fp32) {bound:.3e}")
        for k in got:
            assert torch.isfinite(got[k]).all(), k
            assert _rel(got[k], eager[which][k], ref[which][k]) <= bound, k


def test_replay_dropout_follows_the_device_seed():
    from pdnlp_amd.engine.trainer import Trainer
    from pdnlp_amd.models import BertForSequenceClassification
    from pdnlp_amd.ops import reseed_dropout
    _, packed, _, _ = _case("preload")
    cfg = _model_cfg()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.1
    torch.manual_seed(123)
    model = BertForSequenceClassification(cfg).to(torch.bfloat16).to(DEV)
    model.train()
    tr = Trainer(_args(), model, _plain_sgd(model), DEV)
    entry = tr._capture_graph(packed[0])
    losses = []
    for seed in (7, 7, 8):
        reseed_dropout(seed)
        losses.append(entry.run(packed[0])[0].item())
    print("replay losses under seeds 7, 7, 8:", losses)
    assert all(math.isfinite(l) for l in losses)
    assert losses[0] == losses[1]
    assert losses[2] != losses[0]


class _LengthsDs(torch.utils.data.Dataset):
    def __init__(self, lens, S=128):
        b = _padded_batch(lens, S, seed=9)
        self.items = [{k: v[i] for k, v in b.items()}
                      for i in range(len(lens))]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_trainer_captures_per_key_and_keeps_training(tmp_path):
    """Five batches per epoch: keys K1 (T 320), K2 (T 384), K1, K2 and a
    3-sequence tail (T 64). Under the capture rule K2 is captured at step
    4, K1 at step 6 and the tail at step 10 (seen in epoch 1, repeated in
    epoch 2): 3 graphs, 4 eager steps (1, 2, 3, 5), 11 replays."""
    from torch.utils.data import DataLoader
    from pdnlp_amd.data import Collate
    from pdnlp_amd.engine.trainer import build_training
    from pdnlp_amd.models import BertForSequenceClassification
    from pdnlp_amd.utils import set_seed
    set_seed(123)
    k1a, k1b = CASES["preload"][1:]
    k2a, k2b = [5, 64, 1, 33, 128, 128], [100, 90, 80, 30, 20, 10]
    lens = k1a + k2a + k1b + k2b + [10, 20, 30]
    args = _args(tmp_path, epochs=3, learning_rate=5e-4)
    model, opt, scaler, trainer = build_training(
        args, model=BertForSequenceClassification(_model_cfg()))
    loader = DataLoader(_LengthsDs(lens), batch_size=6, shuffle=False,
                        collate_fn=Collate(None, 128, unpad=True))
    assert [b["input_ids"].numel() for b in loader] == [320, 384, 320, 384,
                                                        64]
    sums, losses = [], []
    trainer.step_callback = lambda t: sums.append(_checksum(opt))
    orig = trainer.train_step

    def spy(batch, accum_boundary=True):
        res = orig(batch, accum_boundary)
        losses.append(res[0].detach().clone())   # a replay's loss is reused
        return res

    trainer.train_step = spy
    trainer.train(loader)
    print("graph_stats", trainer.graph_stats)
    assert scaler is None and trainer.global_step == 15
    assert trainer.graph_stats == {"captured": 3, "replayed": 11, "eager": 4}
    assert trainer._graph is not None and len(trainer._graph) == 3
    assert len(sums) == 15 and len(set(sums)) == 15, \
        "the master weights must change on every step"
    assert all(a != b for a, b in zip(sums, sums[1:]))
    assert all(math.isfinite(l.item()) for l in losses) and len(losses) == 15


def _sgd_trainers(tmp_path, **kw):
    """(replaying trainer, eager trainer) on deep copies of the never
    stepped model of the preload case, plain SGD with fp32 masters."""
    from pdnlp_amd.engine.trainer import Trainer
    model, packed, ref, eager = _case("preload")
    out = []
    for hip_graph in (True, False):
        m = copy.deepcopy(model)
        opt = _plain_sgd(m)
        out.append((Trainer(_args(tmp_path, hip_graph=hip_graph, **kw), m,
                            opt, DEV), m, opt))
    return out, packed, ref, eager


def _capture_without_training(tr, batch):
    # the warm-up passes take no optimizer step, so a graph can be captured
    # on untouched weights
    key = tr._graph_key(batch)
    tr._graphs[key] = tr._capture_graph(batch, key)


def test_one_replayed_step_equals_one_eager_step(tmp_path):
    """w1 = w0 - lr * g: the applied update (w0 - w1) / lr of a replayed
    step against that of an eager step, held to the replay-vs-eager bound
    of the gradients. fp32 masters: recovering g costs 2^-24 * |w| / lr,
    below 1e-6 here."""
    (rep, eag), packed, ref, eager = _sgd_trainers(tmp_path)
    bound = _bound(ref[0], eager[0])
    start = [p.detach().float().clone() for p in rep[1].parameters()]
    _capture_without_training(rep[0], packed[0])
    for p, q in zip(rep[1].parameters(), start):
        assert torch.equal(p.detach().float(), q), "capture moved the weights"
    assert rep[0]._graph_step(packed[0]) is not None
    res = eag[0].train_step(packed[0])
    assert res[3] and eag[0]._graph is None
    worst = 0.0
    for (n, _), w0, a, b in zip(rep[1].named_parameters(), start,
                                _masters(rep[2]), _masters(eag[2])):
        ua, ub = (w0 - a).cpu() / LR, (w0 - b).cpu() / LR
        assert ub.abs().max() > 0 or ref[0][n].abs().max() == 0, n
        err = _rel(ua, ub, ref[0][n])
        worst = max(worst, err)
        assert err <= bound, n
    print(f"replayed-vs-eager step, update/lr: {worst:.3e}  bound "
          f"{bound:.3e}")


def test_replayed_packed_step_is_clipped(tmp_path):
    max_norm = 0.05
    (rep, _), packed, _, _ = _sgd_trainers(tmp_path, max_grad_norm=max_norm)
    tr, model, opt = rep
    _capture_without_training(tr, packed[0])
    tr._graph_step(packed[1])          # creates the masters (first step)
    before = _masters(opt)
    assert tr._graph_step(packed[0]) is not None
    torch.cuda.synchronize()
    gnorm = math.sqrt(sum(p.grad.double().pow(2).sum().item()
                          for p in model.parameters()))
    assert gnorm >= 2 * max_norm, gnorm
    moved = math.sqrt(sum((a.double() - b.double()).pow(2).sum().item()
                          for a, b in zip(_masters(opt), before)))
    print("replayed packed step: moved", moved, "lr*max_norm", LR * max_norm,
          "grad norm", gnorm, "last_grad_norm", tr.last_grad_norm.item())
    assert 0 < moved <= LR * max_norm * (1 + 1e-2)
    assert abs(tr.last_grad_norm.item() - gnorm) <= 1e-2 * gnorm


def test_padded_replays_keep_training_after_an_eager_tail(tmp_path):
    """Padded batches of 16, 16, 8 over 3 epochs. The 8-batch is new at
    step 3 (eager) and gets its own graph at step 6; steps 7 and 8 are
    replays that follow it. With one graph and an eager tail that ended in
    zero_grad(set_to_none), those replays wrote gradients nobody read and
    the optimizer skipped every parameter."""
    from torch.utils.data import DataLoader
    from pdnlp_amd.config import BertConfig
    from pdnlp_amd.data import Collate, SyntheticClsDataset
    from pdnlp_amd.engine.trainer import Trainer
    from pdnlp_amd.models import BertForSequenceClassification
    from pdnlp_amd.ops.adamw import build_optimizer
    from pdnlp_amd.utils import set_seed
    set_seed(123)
    cfg = BertConfig.tiny()
    model = BertForSequenceClassification(cfg).to(torch.bfloat16).to(DEV)
    opt = build_optimizer(model, lr=1e-3)
    tr = Trainer(_args(tmp_path, unpad=False, epochs=3), model, opt, DEV)
    ds = SyntheticClsDataset(40, seq_len=16, vocab_size=cfg.vocab_size)
    sums = []
    tr.step_callback = lambda t: sums.append(_checksum(opt))
    tr.train(DataLoader(ds, batch_size=16, shuffle=False,
                        collate_fn=Collate(None, 16)))
    assert tr.global_step == 9 and len(sums) == 9
    assert tr._graph is not None, "graph was never captured"
    assert sums[6] != sums[5], "step 7 (replay after the tail) did not train"
    assert sums[7] != sums[6], "step 8 did not train"
    assert len(set(sums)) == 9
    # steps 1-3 eager, the 16-batch captured at 4, the 8-batch at 6
    assert tr.graph_stats == {"captured": 2, "replayed": 6, "eager": 3}
