"""GPU tests of the fused attention backward (``fa_bwd_fused_kernel``: one
workgroup per head for sequences of at most 128 rows) against fp64 and
against the two-kernel backward that ``PDNLP_FA_BWD_SPLIT`` keeps.

Shapes are B = 2 (padded) or up to six sequences (packed), two heads of 64.
Every reference is plain torch in float64 from the dtype-rounded inputs the
kernel receives, under the kernel's own dropout mask, read out of the forward
with V = identity on one 64-key chunk at a time. Gates, as in
test_kernels_training_gpu.py: ``assert_close`` at 5e-2, and
``max|x - ref64| / max(std(ref64), 1)`` at most twice the error of the same
composition in plain torch ops of the kernel's dtype, measured in the same
run (the factor 2 is for summation order)."""

import contextlib
import functools
import math
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = "cuda:0"
F64 = torch.float64
BF16, FP16 = torch.bfloat16, torch.float16
B, NH, HD = 2, 2, 64
H = NH * HD
SCALE = 1.0 / math.sqrt(HD)
SALT = 5
SWITCH = "PDNLP_FA_BWD_SPLIT"


def ext():
    from pdnlp_amd.ops import ext as _ext
    e = _ext()
    assert e is not None, "HIP extension must be built on the GPU box"
    return e


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, list):
        return "-".join(map(str, v))
    return None


@contextlib.contextmanager
def _split():
    """The two-kernel backward for the calls inside (read per call)."""
    assert SWITCH not in os.environ
    os.environ[SWITCH] = "1"
    try:
        yield
    finally:
        del os.environ[SWITCH]


def _seed():
    return torch.tensor([99], dtype=torch.int64, device=DEV)


def _rel(a, ref):
    return ((a.to(F64) - ref).abs().max().item()
            / max(ref.std().item(), 1.0))


def _composition(qkv, mask, keep, dout, p, dt):
    """scores, mask add, softmax, keep/(1-p), @ V and the autograd backward
    of one batch [N, L, 3H] in dtype ``dt``; keep [N, NH, L, L]. Returns
    dqkv."""
    q = qkv.to(dt).detach().requires_grad_()
    N, L = q.shape[0], q.shape[1]
    qh, kh, vh = (t.reshape(N, L, NH, HD).transpose(1, 2)
                  for t in q.split(H, dim=-1))
    s = torch.matmul(qh, kh.transpose(-1, -2)) * SCALE
    if mask is not None:
        s = s + mask.to(dt)
    pr = torch.softmax(s, dim=-1) * keep.to(dt) / (1.0 - p)
    o = torch.matmul(pr, vh).transpose(1, 2).reshape(N, L, H)
    o.backward(dout.to(dt))
    return q.grad


def _gate(name, got, same, ref):
    """The two gates of the module docstring; returns the kernel's error."""
    assert torch.isfinite(got).all(), name
    k_err, t_err = _rel(got, ref), _rel(same, ref)
    print(f"{name}: kernel {k_err:.3e}  torch-same-dtype {t_err:.3e}")
    torch.testing.assert_close(got.to(F64), ref, rtol=5e-2, atol=5e-2)
    assert k_err <= 2 * t_err, (name, k_err, t_err)
    return k_err


def _report_thirds(name, fused, split):
    """Largest fused-vs-split difference per q/k/v third of dqkv; dK and dV
    keep the split kernel's orientation and add order, so they are expected
    (not asserted) to be bit-equal."""
    for i, third in enumerate("qkv"):
        a = fused[..., i * H:(i + 1) * H]
        b = split[..., i * H:(i + 1) * H]
        print(f"{name} d{third}: max|fused - split| "
              f"{(a.float() - b.float()).abs().max().item():.3e}  "
              f"bit-equal {torch.equal(a, b)}")


# ------------------------------------------------------------ 1. padded
def _probe_padded(e, qkv, mask, p, seed, salt):
    """[B, NH, S, S]: the (dropped, rescaled) probabilities the kernel
    applies, read out with V = identity on one 64-key chunk at a time."""
    S = qkv.shape[1]
    out = torch.zeros(B, NH, S, S, device=DEV)
    eye = torch.eye(64, device=DEV, dtype=qkv.dtype)
    for c in range(S // 64):
        probe = qkv.clone()
        probe[..., 2 * H:] = 0
        for h in range(NH):
            probe[:, c * 64:(c + 1) * 64,
                  2 * H + h * HD:2 * H + (h + 1) * HD] = eye
        o, _ = e.flash_attn_qkv_fwd(probe, mask, NH, SCALE, p, seed, salt)
        out[..., c * 64:(c + 1) * 64] = o.float().reshape(
            B, S, NH, HD).transpose(1, 2)
    return out


@functools.lru_cache(maxsize=None)
def _padded_case(S, dtype, with_mask, p):
    """Inputs, both backward paths and the references of one case; computed
    once and left unchanged."""
    e = ext()
    torch.manual_seed(20)
    qkv = torch.randn(B, S, 3 * H, device=DEV, dtype=dtype)
    dout = torch.randn(B, S, H, device=DEV, dtype=dtype)
    if with_mask:
        live = torch.ones(B, 1, 1, S, device=DEV, dtype=torch.bool)
        live[1, :, :, S - S // 4:] = False
        mask = ((~live).to(dtype) * -10000.0).contiguous()
    else:
        mask = torch.Tensor().to(DEV)
    seed = _seed() if p else torch.Tensor()
    keep = torch.ones(B, NH, S, S, device=DEV, dtype=torch.bool)
    if p:
        pd = _probe_padded(e, qkv, mask, p, seed, SALT)
        p0 = _probe_padded(e, qkv, mask, 0.0, torch.Tensor(), 0)
        keep = (pd != 0) | (p0 == 0)
    o, lse = e.flash_attn_qkv_fwd(qkv, mask, NH, SCALE, p, seed, SALT)

    def bwd():
        return e.flash_attn_qkv_bwd(dout, qkv, o, lse, mask, NH, SCALE, p,
                                    seed, SALT)
    fused = bwd()
    with _split():
        split = bwd()
    m = mask if with_mask else None
    return dict(bwd=bwd, fused=fused, split=split,
                ref64=_composition(qkv, m, keep, dout, p, F64),
                ref_t=_composition(qkv, m, keep, dout, p, dtype))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=_ids)
@pytest.mark.parametrize("S", [64, 128])
def test_fused_bwd_padded_against_fp64(S, dtype, with_mask, p):
    c = _padded_case(S, dtype, with_mask, p)
    name = f"S={S} {dtype} mask={with_mask} p={p}"
    _gate(f"{name} fused", c["fused"], c["ref_t"], c["ref64"])
    _gate(f"{name} split", c["split"], c["ref_t"], c["ref64"])
    _report_thirds(name, c["fused"], c["split"])


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [64, 128])
def test_fused_bwd_determinism_and_switch(S, p):
    c = _padded_case(S, BF16, True, p)
    assert torch.equal(c["bwd"](), c["fused"])
    assert torch.equal(c["bwd"](), c["fused"])
    with _split():
        again = c["bwd"]()
    assert torch.equal(again, c["split"])
    assert SWITCH not in os.environ


# ------------------------------------------------------------ 2. packed
def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def _probe_varlen(e, qkv, cu, cu_t, mx, p, seed, salt):
    """Per sequence [NH, L, L]: the probabilities the packed forward applies,
    read out as in _probe_padded."""
    spans = [(s0, s1) for s0, s1 in zip(cu[:-1], cu[1:]) if s1 > s0]
    outs = [torch.zeros(NH, s1 - s0, s1 - s0, device=DEV) for s0, s1 in spans]
    eye = torch.eye(64, device=DEV, dtype=qkv.dtype)
    for c in range((mx + 63) // 64):
        probe = qkv.clone()
        probe[:, 2 * H:] = 0
        for s0, s1 in spans:
            lo, hi = s0 + c * 64, min(s1, s0 + c * 64 + 64)
            for h in range(NH):
                if hi > lo:
                    probe[lo:hi, 2 * H + h * HD:2 * H + (h + 1) * HD] = \
                        eye[:hi - lo]
        o, _ = e.flash_attn_varlen_fwd(probe, cu_t, mx, NH, SCALE, p, seed,
                                       salt)
        for out, (s0, s1) in zip(outs, spans):
            L = s1 - s0
            n = min(L - c * 64, 64)
            if n > 0:
                out[:, :, c * 64:c * 64 + n] = o[s0:s1].float().reshape(
                    L, NH, HD).transpose(0, 1)[:, :, :n]
    return spans, outs


VARLEN_LENS = [[5, 64, 1, 33, 128, 70], [0, 20, 0, 128]]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=_ids)
@pytest.mark.parametrize("lens", VARLEN_LENS, ids=_ids)
def test_fused_bwd_varlen(lens, dtype, p):
    e = ext()
    torch.manual_seed(21)
    cu, mx = _cu(lens), 128
    total = cu[-1]
    T = (total + 63) // 64 * 64
    qkv = torch.randn(T, 3 * H, device=DEV, dtype=dtype)
    dout = torch.randn(T, H, device=DEV, dtype=dtype)
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    seed = _seed() if p else torch.Tensor()
    o, lse = e.flash_attn_varlen_fwd(qkv, cu_t, mx, NH, SCALE, p, seed, SALT)

    def bwd(c=cu_t):
        return e.flash_attn_varlen_bwd(dout, qkv, o, lse, c, mx, NH, SCALE, p,
                                       seed, SALT)
    fused = bwd()
    with _split():
        split = bwd()

    spans, pd = _probe_varlen(e, qkv, cu, cu_t, mx, p, seed, SALT)
    _, p0 = _probe_varlen(e, qkv, cu, cu_t, mx, 0.0, torch.Tensor(), 0)
    ref64 = torch.zeros(T, 3 * H, device=DEV, dtype=F64)
    ref_t = torch.zeros(T, 3 * H, device=DEV, dtype=dtype)
    for (s0, s1), a, a0 in zip(spans, pd, p0):
        keep = ((a != 0) | (a0 == 0))[None] if p else \
            torch.ones_like(a0, dtype=torch.bool)[None]
        for ref, dt in ((ref64, F64), (ref_t, dtype)):
            ref[s0:s1] = _composition(qkv[None, s0:s1], None, keep,
                                      dout[None, s0:s1], p, dt)[0]

    inside = torch.zeros(T, dtype=torch.bool, device=DEV)
    for s0, s1 in spans:
        inside[s0:s1] = True
    name = f"lens={lens} {dtype} p={p}"
    for path, got in (("fused", fused), ("split", split)):
        # every row outside a sequence is exactly 0
        assert (got[~inside] == 0).all(), path
        _gate(f"{name} {path}", got[inside], ref_t[inside], ref64[inside])
    _report_thirds(name, fused, split)
    assert torch.equal(bwd(), fused)

    # empty sequences change nothing: the same stream without them
    if 0 in lens:
        cu2 = torch.tensor(_cu([n for n in lens if n]), dtype=torch.int32,
                           device=DEV)
        assert torch.equal(bwd(cu2), fused)


# ---------------------------------------------------------- 3. boundary
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_longer_sequences_keep_the_streamed_path(p):
    """max_seqlen = 192 is past the fused kernel: the two-kernel path runs
    with and without the switch, so the bits are equal. This shows the
    dispatch condition, not the kernel."""
    e = ext()
    torch.manual_seed(22)
    seed = _seed() if p else torch.Tensor()
    none = torch.Tensor().to(DEV)

    qkv = torch.randn(B, 192, 3 * H, device=DEV, dtype=BF16)
    dout = torch.randn(B, 192, H, device=DEV, dtype=BF16)
    o, lse = e.flash_attn_qkv_fwd(qkv, none, NH, SCALE, p, seed, SALT)

    def padded():
        return e.flash_attn_qkv_bwd(dout, qkv, o, lse, none, NH, SCALE, p,
                                    seed, SALT)

    cu = _cu([150, 192, 30, 12])
    cu_t = torch.tensor(cu, dtype=torch.int32, device=DEV)
    qkv_v = torch.randn(cu[-1], 3 * H, device=DEV, dtype=BF16)
    dout_v = torch.randn(cu[-1], H, device=DEV, dtype=BF16)
    o_v, lse_v = e.flash_attn_varlen_fwd(qkv_v, cu_t, 192, NH, SCALE, p, seed,
                                         SALT)

    def packed():
        return e.flash_attn_varlen_bwd(dout_v, qkv_v, o_v, lse_v, cu_t, 192,
                                       NH, SCALE, p, seed, SALT)

    for fn in (padded, packed):
        default = fn()
        assert torch.isfinite(default).all()
        with _split():
            assert torch.equal(fn(), default)
