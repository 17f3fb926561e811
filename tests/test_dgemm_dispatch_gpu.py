"""Which extension functions the backward of ``linear``, ``linear_fork`` and
``linear_bias_dropout_residual_layernorm`` calls, per PDNLP_DGEMM mode and
shape — the dispatch policy pinned as an exact ordered list — plus the
x/w/b gradients of three of those cases against an fp32 torch reference."""

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
DTYPE = torch.bfloat16
gpu = pytest.mark.gpu


class _RecordingExt:
    """Forwards to the real extension; while ``armed`` it appends the name
    of every extension function that is CALLED (attribute look-ups alone do
    not count)."""

    def __init__(self, real):
        self._real = real
        self.armed = False
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args, **kwargs):
            if self.armed:
                self.calls.append(name)
            return fn(*args, **kwargs)
        return call


@pytest.fixture
def rec(monkeypatch):
    from pdnlp_amd.ops import ext, functional as Fops
    real = ext()
    assert real is not None, "HIP extension must be built on the GPU box"
    proxy = _RecordingExt(real)
    monkeypatch.setattr(Fops, "ext", lambda: proxy)
    return proxy


def _inputs(M, n_in, n_out, bias=True):
    """x[M, in], w[out, in], b[out], upstream gradients dout[M, out] and
    dpass[M, in]; one generator per shape, so every user of a shape sees the
    same values. The LN weight is near 1 and dout/dpass are small (1/128) —
    see the tolerance note on ``test_grads_match_fp32_reference``."""
    g = torch.Generator().manual_seed(31 + M + n_in + n_out)
    mk = lambda *s: torch.randn(*s, generator=g)
    t = {
        "x": mk(M, n_in) / 16.0, "w": mk(n_out, n_in) / 16.0, "b": mk(n_out),
        "res": mk(M, n_out), "lnw": 1.0 + 0.1 * mk(n_out), "lnb": mk(n_out),
        "dout": mk(M, n_out) / 128.0, "dpass": mk(M, n_in) / 128.0,
    }
    t = {k: v.to(DTYPE).to(DEV) for k, v in t.items()}
    if not bias:
        t["b"] = None
    return t


def _leaves(t, names):
    return {k: t[k].clone().requires_grad_(True) for k in names
            if t[k] is not None}


def _backward(call, t, rec=None, **kw):
    """Forward unrecorded, then backward with the recorder armed. Returns
    the x/w/b gradients."""
    from pdnlp_amd.ops import functional as Fops

    if call == "composite":
        v = _leaves(t, ("x", "w", "b", "res", "lnw", "lnb"))
        out = Fops.linear_bias_dropout_residual_layernorm(
            v["x"], v["w"], v["b"], v["res"], v["lnw"], v["lnb"], 0.0, True,
            1e-12)
        outs, grads = [out], [t["dout"]]
    elif call == "linear_fork":
        v = _leaves(t, ("x", "w", "b"))
        y, xp = Fops.linear_fork(v["x"], v["w"], v.get("b"), **kw)
        outs, grads = [y, xp], [t["dout"], t["dpass"]]
    else:
        v = _leaves(t, ("x", "w", "b"))
        outs = [Fops.linear(v["x"], v["w"], v.get("b"), **kw)]
        grads = [t["dout"]]
    if rec is not None:
        rec.armed = True
    try:
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
    finally:
        if rec is not None:
            rec.armed = False
    return {k: v[k].grad for k in ("x", "w", "b") if k in v}


# (id, call, kwargs, bias, mode, (M, in, out), expected backward calls)
CASES = [
    ("linear-bias-auto", "linear", {}, True, "auto", (256, 128, 128),
     ["gemm_nn", "gemm_tn_colsum"]),
    ("linear-bias-gelu-hip", "linear", {"act": "gelu"}, True, "hip",
     (256, 128, 128), ["gelu_bwd", "gemm_nn", "gemm_tn_colsum"]),
    ("linear-nobias-auto", "linear", {}, False, "auto", (256, 128, 128),
     ["gemm_nn", "gemm_tn"]),
    ("linear-bias-auto-m16", "linear", {}, True, "auto", (16, 128, 128),
     ["gemm_nn"]),
    ("linear-bias-blas", "linear", {}, True, "blas", (256, 128, 128),
     ["col_sum"]),
    ("linear-bias-blas-m64", "linear", {}, True, "blas", (64, 128, 128), []),
    ("linear-bias-auto-in3072", "linear", {}, True, "auto", (64, 3072, 64),
     ["gemm_tn_colsum"]),
    ("linear-bias-hip-in3072", "linear", {}, True, "hip", (64, 3072, 64),
     ["gemm_nn", "gemm_tn_colsum"]),
    ("fork-bias-auto", "linear_fork", {}, True, "auto", (256, 128, 128),
     ["gemm_nn_add", "gemm_tn_colsum"]),
    ("fork-bias-auto-in3072", "linear_fork", {}, True, "auto", (64, 3072, 64),
     ["gemm_tn_colsum"]),
    ("composite-auto", "composite", {}, True, "auto", (64, 256, 256),
     ["bias_dropout_residual_ln_bwd_nodb", "gemm_nn", "gemm_tn_colsum"]),
    ("composite-blas", "composite", {}, True, "blas", (64, 256, 256),
     ["bias_dropout_residual_ln_bwd"]),
    ("composite-auto-rows16", "composite", {}, True, "auto", (16, 256, 256),
     ["bias_dropout_residual_ln_bwd", "gemm_nn"]),
]


@gpu
@pytest.mark.parametrize("call,kw,bias,mode,shape,expected",
                         [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_backward_extension_calls(monkeypatch, rec, call, kw, bias, mode,
                                  shape, expected):
    monkeypatch.setenv("PDNLP_DGEMM", mode)
    monkeypatch.delenv("PDNLP_DW_STREAM", raising=False)
    monkeypatch.delenv("PDNLP_FWD", raising=False)
    grads = _backward(call, _inputs(*shape, bias=bias), rec, **kw)
    print(f"{call} {mode} {shape}: {rec.calls}")
    assert rec.calls == expected
    assert all(g is not None for g in grads.values())


def _reference_grads(call, t):
    """The same function in fp32 torch ops on the bf16 input values."""
    v = {k: t[k].float().requires_grad_(True) for k in ("x", "w", "b")}
    y = F.linear(v["x"], v["w"], v["b"])
    if call == "composite":
        h = y + t["res"].float()
        out = F.layer_norm(h, (h.shape[-1],), t["lnw"].float(),
                           t["lnb"].float(), 1e-12)
        out.backward(t["dout"].float())
    elif call == "linear_fork":
        torch.autograd.backward([y, v["x"] * 1.0],
                                [t["dout"].float(), t["dpass"].float()])
    else:
        y.backward(t["dout"].float())
    return {k: v[k].grad for k in v}


@gpu
@pytest.mark.parametrize("call,shape", [("linear", (256, 128, 128)),
                                        ("linear_fork", (256, 128, 128)),
                                        ("composite", (64, 256, 256))])
def test_grads_match_fp32_reference(monkeypatch, call, shape):
    """First, ninth and eleventh dispatch cases: x, w and b gradients
    against fp32 torch, at the rtol=5e-2 / atol=5e-4 that
    test_bias_grad_fusion_gpu.py uses for these quantities.

    Both sides get the SAME bf16 upstream gradients, so for the two linear
    cases the only differences are fp32 summation order and one final bf16
    rounding (2^-9 relative). The composite also rounds its intermediate dy
    to bf16, which the fp32 reference does not, and that noise is absolute:
    dy[r, j] ~ lnw[j] * rstd * dout (rstd ~ 0.7 here), each element off by
    up to 2^-9 relative (rms ~0.6 * 2^-9), and db[j] sums 64 of them, so
    sigma(db[j]) ~ |lnw[j]| * 0.7 * std(dout) * 0.6 * 2^-9 * 8. The inputs
    are scaled so that this stays well inside atol for every column: with
    |lnw| <= ~1.4 and std(dout) = 1/128 it is <= 7e-5, i.e. atol is 7
    sigma (dx and dw, scaled by |w|, |x| ~ 1/16, get ~1e-5). The gradients
    themselves have std 0.005 (dx), 0.0026 (dw) and 0.04 (db), 5-80x atol,
    so a wrong path still shows. (With lnw ~ N(0, 1) and dout/64 the
    columns with |lnw| ~ 3 have sigma 3e-4, and one db element of 256 was
    measured 7.4e-4 off: rounding noise, not a dispatch error.)"""
    monkeypatch.setenv("PDNLP_DGEMM", "auto")
    monkeypatch.delenv("PDNLP_DW_STREAM", raising=False)
    monkeypatch.delenv("PDNLP_FWD", raising=False)
    t = _inputs(*shape)
    got = _backward(call, t)
    ref = _reference_grads(call, t)
    for k in ("x", "w", "b"):
        err = (got[k].float() - ref[k]).abs().max().item()
        print(f"{call} d{k}: max|err| {err:.3e}, "
              f"ref std {ref[k].std().item():.3e}")
    for k in ("x", "w", "b"):
        torch.testing.assert_close(got[k].float(), ref[k],
                                   rtol=5e-2, atol=5e-4)
