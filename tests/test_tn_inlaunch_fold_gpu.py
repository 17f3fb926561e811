"""The split-M fold inside the dW GEMM launch (``gemm_tn_sk_kernel``'s FOLD
path) against the two-launch fold it replaces, which ``PDNLP_TN_FOLD2`` keeps:
both add the fp32 slices in slice order, so ``C`` and the column sums must be
bit-identical, whichever workgroup folds and wherever the slices ran."""

import os

import pytest
import torch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

# (M, N, K): one tile at sm 4 with one 64-row chunk per slice; 6 tiles at
# sm 4 (24 workgroups over the XCDs); 110 tiles at sm 2; sm falls to 1
SHAPES = [(256, 128, 128), (512, 256, 384), (128, 1408, 1280), (64, 128, 128)]
SM4, SM2 = SHAPES[1], SHAPES[2]
DTYPES = [torch.bfloat16, torch.float16]


def ext():
    from pdnlp_amd.ops import ext as _ext
    e = _ext()
    assert e is not None, "HIP extension must be built on the GPU box"
    return e


def _inputs(shape, seed, dtype):
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = (torch.randn(M, N, device=DEV, generator=g) / 4).to(dtype)
    B = torch.randn(M, K, device=DEV, generator=g).to(dtype)
    return A, B


def _two_launch(fn, *args):
    """the same call with the fold in a launch of its own"""
    os.environ["PDNLP_TN_FOLD2"] = "1"
    try:
        return fn(*args)
    finally:
        del os.environ["PDNLP_TN_FOLD2"]


def _same(e, A, B):
    assert "PDNLP_TN_FOLD2" not in os.environ
    C, cs = e.gemm_tn_colsum(A, B)
    Cp = e.gemm_tn(A, B)
    C2, cs2 = _two_launch(e.gemm_tn_colsum, A, B)
    Cp2 = _two_launch(e.gemm_tn, A, B)
    assert torch.equal(C, C2), "colsum C"
    assert torch.equal(cs, cs2), "colsum CS"
    assert torch.equal(Cp, Cp2), "plain C"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fold_bit_identical(shape, dtype):
    _same(ext(), *_inputs(shape, 1, dtype))


def test_fold_against_fp64():
    e = ext()
    A, B = _inputs(SM4, 2, torch.bfloat16)
    C, cs = e.gemm_tn_colsum(A, B)
    ref_c = (A.double().t() @ B.double()).float()
    ref_cs = A.double().sum(0).float()
    torch.testing.assert_close(cs.float(), ref_cs, rtol=2e-2, atol=2e-1)
    torch.testing.assert_close(C.float(), ref_c, rtol=3e-2, atol=3e-1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fold_stale_lines(dtype):
    """Three calls back to back on fresh inputs: the allocator hands back the
    same partials workspace, so the folding workgroup's CU may hold lines of
    the call before."""
    e = ext()
    cases = [_inputs(SM4, 10 + i, dtype) for i in range(3)]
    want = [_two_launch(e.gemm_tn_colsum, A, B) for A, B in cases]
    got = [e.gemm_tn_colsum(A, B) for A, B in cases]
    for (C, cs), (C2, cs2) in zip(got, want):
        assert torch.equal(C, C2) and torch.equal(cs, cs2)


def test_fold_counter_reuse_across_sm():
    e = ext()
    for i, shape in enumerate((SM4, SM2, SM4)):
        _same(e, *_inputs(shape, 20 + i, torch.bfloat16))


def test_fold_forced_splits(monkeypatch):
    """every depth PDNLP_TN_SM can ask for, in turn on the same counters"""
    e = ext()
    for sm in ("3", "8", "2", "1", "4"):
        monkeypatch.setenv("PDNLP_TN_SM", sm)
        _same(e, *_inputs((1536, 256, 384), 30, torch.bfloat16))


def test_fold_graph_replay():
    e = ext()
    A, B = _inputs(SM4, 40, torch.bfloat16)
    for _ in range(2):
        e.gemm_tn_colsum(A, B)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        C, cs = e.gemm_tn_colsum(A, B)
    for i in range(3):
        A2, B2 = _inputs(SM4, 41 + i, torch.bfloat16)
        A.copy_(A2)
        B.copy_(B2)
        graph.replay()
        C2, cs2 = _two_launch(e.gemm_tn_colsum, A, B)
        assert torch.equal(C, C2) and torch.equal(cs, cs2), i
