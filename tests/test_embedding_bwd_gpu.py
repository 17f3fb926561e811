"""``embedding_ln_bwd`` without float atomics: every table row is the sum of
its contribution rows in a fixed order, so the five gradients are accurate
against fp64, repeat bit for bit, and untouched rows are exact zeros."""

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

FP32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPS = 1e-12
# tolerances of the two existing embedding tests (tests/test_kernels_gpu.py,
# tests/test_kernels_training_gpu.py)
LN_TOL = {FP32: (1e-5, 1e-5), BF16: (2e-2, 2e-2)}
MULT = [20, 20, 50, 50, 50]
NAMES = ["dword", "dpos", "dtype", "dlnw", "dlnb"]


def ext():
    from pdnlp_amd.ops import ext as _ext
    e = _ext()
    assert e is not None, "HIP extension must be built on the GPU box"
    return e


def _uniform(dtype):
    torch.manual_seed(1)
    B, S, H, V = 4, 32, 768, 1000
    ids = torch.randint(0, V, (B, S), device=DEV)
    tids = torch.randint(0, 2, (B, S), device=DEV)
    pids = torch.arange(S, device=DEV).repeat(B, 1).contiguous()
    return ids, tids, pids, (V, S, 2), H


def _padded_packed(dtype):
    """mostly id 0, positions that restart inside a row"""
    torch.manual_seed(28)
    B, S, H, V = 3, 11, 128, 16
    ids = torch.randint(1, V, (B, S), device=DEV)
    ids[torch.rand(B, S, device=DEV) < 0.8] = 0
    pids = torch.tensor(list(range(5)) + list(range(6)),
                        device=DEV).repeat(B, 1).contiguous()
    tids = (torch.arange(B * S, device=DEV) % 2).reshape(B, S).contiguous()
    return ids, tids, pids, (V, 8, 2), H


def _skewed(dtype):
    """A destination is summed in row ranges by separate workgroups once it
    has more than 128 rows (for R <= 4096). R = 160 is the smallest round
    batch that splits at 90 % id 0: 144 rows on word row 0, in ranges of 128
    and 32 rows. Token type 0 (136 rows) splits too; type 1 and the positions
    stay single lists."""
    torch.manual_seed(29)
    B, S, H, V = 4, 40, 256, 64
    ids = torch.randint(1, V, (B * S,), device=DEV)
    ids[torch.randperm(B * S, device=DEV)[:144]] = 0
    ids = ids.reshape(B, S).contiguous()
    tids = torch.zeros(B * S, dtype=torch.long, device=DEV)
    tids[torch.randperm(B * S, device=DEV)[:24]] = 1
    tids = tids.reshape(B, S).contiguous()
    pids = torch.arange(S, device=DEV).repeat(B, 1).contiguous()
    return ids, tids, pids, (V, S, 2), H


CASES = {"uniform": _uniform, "padded_packed": _padded_packed,
         "skewed": _skewed}


def _run(case, dtype):
    e = ext()
    ids, tids, pids, (V, P, T), H = CASES[case](dtype)
    word = torch.randn(V, H, device=DEV, dtype=dtype)
    pos = torch.randn(P, H, device=DEV, dtype=dtype)
    typ = torch.randn(T, H, device=DEV, dtype=dtype)
    lnw = torch.randn(H, device=DEV, dtype=dtype)
    lnb = torch.randn(H, device=DEV, dtype=dtype)
    y, mean, rstd = e.embedding_ln_fwd(ids, tids, pids, word, pos, typ, lnw,
                                       lnb, EPS)
    dy = torch.randn(*ids.shape, H, device=DEV, dtype=dtype)
    args = (dy, ids, tids, pids, word, pos, typ, lnw, mean, rstd)
    return e, args, (V, P, T)


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_embedding_bwd_against_fp64(case, dtype):
    e, args, (V, P, T) = _run(case, dtype)
    dy, ids, tids, pids, word, pos, typ, lnw, mean, rstd = args
    grads = e.embedding_ln_bwd(*args)
    wr, pr, tr, lw = (t.to(F64).detach().requires_grad_()
                      for t in (word, pos, typ, lnw))
    lb = torch.zeros_like(lw).requires_grad_()
    emb = F.embedding(ids, wr) + F.embedding(pids, pr) + F.embedding(tids, tr)
    F.layer_norm(emb, (emb.shape[-1],), lw, lb, EPS).backward(dy.to(F64))

    def count(idx, n):
        return torch.bincount(idx.flatten(), minlength=n).clamp(min=1).to(F64)

    R = ids.numel()
    rtol, atol = LN_TOL[dtype]
    # uniform: the fixed multipliers of test_embedding_ln for both dtypes.
    # The other two: the rule of test_embedding_ln_padded_packed_ids, where
    # an fp32 sum adds no error beyond its length and bf16 keeps the
    # multipliers.
    dup = [count(ids, V)[:, None], count(pids, P)[:, None],
           count(tids, T)[:, None], float(R), float(R)]
    by_length = dtype == FP32 and case != "uniform"
    for name, got, want, d, k in zip(NAMES, grads, (wr, pr, tr, lw, lb), dup,
                                     MULT):
        tol = atol * (d if by_length else k)
        err = (got.to(F64) - want.grad).abs()
        bound = tol + rtol * want.grad.abs()
        print(f"{case} {name}: max err {float(err.max()):.3e}, "
              f"worst err/bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), name


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_embedding_bwd_repeats_and_zero_rows(case, dtype):
    e, args, (V, P, T) = _run(case, dtype)
    ids, tids, pids = args[1], args[2], args[3]
    first = e.embedding_ln_bwd(*args)
    second = e.embedding_ln_bwd(*args)
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), name
    for got, idx, n in zip(first[:3], (ids, pids, tids), (V, P, T)):
        untouched = torch.bincount(idx.flatten(), minlength=n) == 0
        assert not bool(got[untouched].any())
        assert bool(torch.isfinite(got).all())
    assert bool((torch.bincount(ids.flatten(), minlength=V) == 0).any())
