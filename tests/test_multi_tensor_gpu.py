"""Multi-tensor kernels at their packing boundaries, and the two vectorized
epilogue kernels at sizes that end inside a vector.

A multi-tensor op packs 32 tensors per launch, 1024 elements per block and 4
elements per vector. Each element's result depends on its own inputs only, so
one call over n tensors must equal n calls over one tensor BIT FOR BIT,
whatever the packing: the expected difference is zero by construction.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = "cuda:0"
F64 = torch.float64
FP32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
# 1024 is one block, 4 one vector
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4097]
NTENSORS = 65
BITS = {FP32: torch.int32, BF16: torch.int16, FP16: torch.int16}


def ext():
    from pdnlp_amd.ops import ext as _ext
    e = _ext()
    assert e is not None, "HIP extension must be built on the GPU box"
    return e


def _ids(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


class TList:
    """65 tensors whose sizes cycle through SIZES. Every third one is a view
    at element offset 1 of a flat buffer two elements longer, so its address
    is not 8- or 16-byte aligned and one guard element lies on either side;
    the others are their own buffer."""

    def __init__(self, flats):
        self.flats = flats
        self.tensors = [f[1:-1] if i % 3 == 2 else f
                        for i, f in enumerate(flats)]

    @classmethod
    def make(cls, dtype, seed, fn=torch.randn):
        g = torch.Generator().manual_seed(seed)
        return cls([fn(SIZES[i % len(SIZES)] + (2 if i % 3 == 2 else 0),
                       generator=g).to(dtype).to(DEV)
                    for i in range(NTENSORS)])

    def clone(self):
        return TList([f.clone() for f in self.flats])


def _same_bits(a, b):
    return torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


def _scalar(v):
    return torch.full((1,), float(v), device=DEV)


def _state(op, dtype):
    """name -> TList of every list the op works on: "g" and "p" of ``dtype``,
    "m", "v", "buf" and "master" fp32"""
    lists = {"g": TList.make(dtype, 1)}
    if op.startswith(("adamw", "sgd")):
        lists["p"] = TList.make(dtype, 2)
        if op.startswith("adamw"):
            lists["m"] = TList.make(FP32, 3)
            lists["v"] = TList.make(FP32, 4, torch.rand)
        else:
            lists["buf"] = TList.make(FP32, 5)
        if op.endswith("_master"):
            lists["master"] = TList.make(FP32, 6)
    return lists


def _run(op, lists, sl):
    """one extension call over the tensors ``sl`` of every list"""
    e = ext()
    t = {k: v.tensors[sl] for k, v in lists.items() if k != "found_inf"}
    if op.startswith("adamw"):
        e.multi_tensor_adamw(t["p"], t["g"], t["m"], t["v"],
                             t.get("master", []), 1e-2, 0.9, 0.999, 1e-8,
                             0.01, 0.1, 0.001, 0.5, _scalar(0), _scalar(0.75))
    elif op.startswith("sgd"):
        e.multi_tensor_sgd(t["p"], t["g"], t["buf"], t.get("master", []),
                           1e-2, 0.9, 0.01, 0.5, _scalar(0), _scalar(0.75))
    elif op == "unscale":
        e.multi_tensor_unscale(t["g"], lists["found_inf"], 2.0 ** -10)
    else:
        e.multi_tensor_scale_(t["g"], _scalar(0.37))


def _clone(lists):
    out = {k: v.clone() for k, v in lists.items()}
    out["found_inf"] = _scalar(0)
    return out


@functools.lru_cache(maxsize=None)
def _one_by_one(op, dtype):
    """(pristine inputs, the result of one call per tensor); never modified"""
    start = _state(op, dtype)
    ref = _clone(start)
    for i in range(NTENSORS):
        _run(op, ref, slice(i, i + 1))
    return start, ref


OPS = ["adamw", "adamw_master", "sgd", "sgd_master", "unscale", "scale"]


@pytest.mark.parametrize("n", [1, 32, 33, 65])
@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_ids)
@pytest.mark.parametrize("op", OPS)
def test_packing_is_bitwise_neutral(op, dtype, n):
    start, ref = _one_by_one(op, dtype)
    got = _clone(start)
    _run(op, got, slice(0, n))
    torch.cuda.synchronize()
    for name, tl in start.items():
        for i in range(NTENSORS):
            what = f"{name}[{i}] ({tl.tensors[i].numel()} elements)"
            # tensors past n were not passed: whole buffer as it was
            want = ref[name].flats[i] if i < n else tl.flats[i]
            assert _same_bits(got[name].flats[i], want), what
            if i % 3 == 2:   # elements of the flat buffer outside the view
                for edge in (0, -1):
                    assert _same_bits(got[name].flats[i][edge:][:1],
                                      tl.flats[i][edge:][:1]), what + " guard"
    assert got["found_inf"].item() == 0.0
    # the op did something: the last tensor passed has changed (an fp32
    # state where there is one; a one-element bf16 param may round back)
    changed = {"ad": "m", "sg": "buf"}.get(op[:2], "g")
    assert not _same_bits(got[changed].flats[n - 1],
                          start[changed].flats[n - 1])


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_ids)
def test_unscale_flag_across_chunks(dtype):
    start, _ = _one_by_one("unscale", dtype)
    clean = _clone(start)
    _run("unscale", clean, slice(0, NTENSORS))
    assert clean["found_inf"].item() == 0.0
    bad = _clone(start)
    bad["g"].tensors[-1][-1] = float("inf")
    _run("unscale", bad, slice(0, NTENSORS))
    assert bad["found_inf"].item() == 1.0
    assert torch.isinf(bad["g"].tensors[-1][-1])
    bad["g"].tensors[-1][-1] = clean["g"].tensors[-1][-1]
    for i in range(NTENSORS):
        # 2^-10 is a power of two: the scaled value is exact in every dtype
        want = (start["g"].flats[i].double() * 2.0 ** -10).to(dtype)
        if i % 3 == 2:
            want[0], want[-1] = start["g"].flats[i][0], start["g"].flats[i][-1]
        assert _same_bits(bad["g"].flats[i], want), f"g[{i}]"
        assert _same_bits(clean["g"].flats[i], want), f"g[{i}] (no inf)"


def _sumsq(tensors):
    out = torch.full((1,), 123.0, device=DEV)   # must be overwritten
    ext().multi_tensor_sumsq(list(tensors), out, False)
    return out.item()


def _sumsq64(tensors):
    return sum(t.to(F64).pow(2).sum().item() for t in tensors)


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_ids)
def test_sumsq_across_chunks(dtype):
    """1e-5 relative: the rounding depth grad_clip.hip derives in its header,
    (L + D) * 2^-24 = 7e-6, rounded up; every term is non-negative, so the
    bound on the sum is relative."""
    ts = TList.make(dtype, 7).tensors
    for name, lst in (("65 tensors", ts),
                      # all head, no body: one element at an odd address
                      ("head-only first", [TList.make(dtype, 8).flats[2][1:2]]
                       + ts[:4])):
        addr = lst[0].data_ptr()
        if name != "65 tensors":
            assert lst[0].numel() == 1 and addr % 16 != 0
        got, ref = _sumsq(lst), _sumsq64(lst)
        print(f"sumsq {name} {dtype}: {got!r} ref {ref!r} "
              f"rel {abs(got - ref) / ref:.3e}")
        assert abs(got - ref) <= 1e-5 * ref, name


# (rtol, atol) of test_act_bwd_odd_sizes for 16-bit dtypes
ELT_TOL = (2e-2, 2e-2)


def _close(got, ref, rtol, atol, what):
    got, ref = got.to(F64), ref.to(F64)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    excess = (got - ref).abs() - (rtol * ref.abs() + atol)
    assert (excess <= 0).all(), (
        f"{what}: max excess {excess.max().item():.3e}, "
        f"max|err|={(got - ref).abs().max().item():.3e}")


@pytest.mark.parametrize("n", [1025, 1031])   # a tail of 1 and of 7
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=_ids)
def test_gelu_bwd_tail_inside_vector(dtype, n):
    torch.manual_seed(31)
    pre = (torch.randn(n, device=DEV) * 2).to(dtype)
    dy = torch.randn(n, device=DEV).to(dtype)
    dx = ext().gelu_bwd(dy, pre)
    pr = pre.to(F64).requires_grad_()
    F.gelu(pr).backward(dy.to(F64))
    _close(dx, pr.grad, *ELT_TOL, "dx")


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=_ids)
def test_col_sum_partial_group(dtype):
    """[257, 68]: the last 64-column group holds 4 columns and the rows are
    no multiple of the 16 row strips. rtol, atol of test_col_sum, with the
    atol scaled from its 2048 rows down to the 257 used here."""
    torch.manual_seed(32)
    x = torch.randn(257, 68, device=DEV).to(dtype)
    cs = ext().col_sum(x)
    assert cs.shape == (68,) and cs.dtype == dtype
    _close(cs, x.to(F64).sum(0), 2e-2, 2e-1 * 257 / 2048, "col_sum")
