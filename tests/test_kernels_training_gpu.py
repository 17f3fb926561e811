"""GPU numerics tests of the kernels as training runs them: attention and
bias+dropout+residual+LN with dropout on, forward and backward, LayerNorm
statistics on rows that are not zero-mean, and the small kernels at odd
sizes and hard values. Every reference is plain torch in float64, computed
from the dtype-rounded inputs the kernel receives."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def ext():
    from pdnlp_amd.ops import ext as _ext
    e = _ext()
    assert e is not None, "HIP extension must be built on the GPU box"
    return e


DEV = "cuda:0"
F64 = torch.float64
EPS = 1e-12
FP32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16
# (rtol, atol) of the LayerNorm / bdrl tests of test_kernels_gpu.py; fp16
# takes the bf16 row
LN_TOL = {FP32: (1e-5, 1e-5), BF16: (2e-2, 2e-2), FP16: (2e-2, 2e-2)}
# (rtol, atol) of test_bias_gelu and, for 16 bit, of test_masked_softmax
ELT_TOL = {FP32: (1e-5, 1e-6), BF16: (2e-2, 2e-2), FP16: (2e-2, 2e-2)}
SM_TOL = {FP32: (1e-5, 1e-6), BF16: (1e-2, 1e-2), FP16: (1e-2, 1e-2)}
# largest spacing of the format relative to the value (one ulp at the bottom
# of a binade); round-to-nearest is off by at most half of it
ULP = {FP32: 2.0 ** -23, BF16: 2.0 ** -7, FP16: 2.0 ** -10}
# spacing of the subnormals, below which the relative one does not hold
TINY = {FP32: 2.0 ** -149, BF16: 2.0 ** -133, FP16: 2.0 ** -24}


def _ids(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


def _close(got, ref, rtol, atol, what=""):
    """assert_close in float64; ``atol`` may be a tensor that broadcasts."""
    got, ref = got.to(F64), ref.to(F64)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    excess = (got - ref).abs() - (rtol * ref.abs() + atol)
    assert (excess <= 0).all(), (
        f"{what}: max excess {excess.max().item():.3e} over rtol={rtol}, "
        f"max|err|={(got - ref).abs().max().item():.3e}")


def _ln64(x, w, b):
    return F.layer_norm(x.to(F64), (x.shape[-1],), w.to(F64), b.to(F64), EPS)


def _stats64(x):
    x = x.to(F64)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + EPS)


# ------------------------------------------- A. padded attention + dropout
A_B, A_NH, A_HD, A_P, A_SALT = 2, 2, 64, 0.1, 5
A_H = A_NH * A_HD
A_SCALE = 1.0 / math.sqrt(A_HD)

# max|x - ref64| / max(std(ref64), 1) as test_flash_attn_dropout_same_mask
# prints it on an MI355X, kernel / plain torch ops of the same dtype (the
# bound is twice the latter, measured anew in every run), with the additive
# mask; without it the kernel's figures are within 15% of these:
#   S=128 bf16  o 3.06e-03 / 5.14e-03   dqkv 5.62e-03 / 8.97e-03
#   S=128 fp16  o 3.84e-04 / 1.12e-03   dqkv 6.17e-04 / 1.77e-03
#   S=192 bf16  o 2.58e-03 / 6.74e-03   dqkv 3.71e-03 / 1.15e-02
#   S=192 fp16  o 3.51e-04 / 1.64e-03   dqkv 6.52e-04 / 1.93e-03
# Drop rates measured 0.1010 .. 0.1024 for p = 0.1 (5 sigma is 0.004 .. 0.006).


def _heads(t, dt):
    return t.to(dt).reshape(A_B, -1, A_NH, A_HD).transpose(1, 2)


def _attn_composition(qkv, mask, keep, dout, dt):
    """scores, mask add, softmax, keep/(1-p), @ V and the autograd backward,
    all in dtype ``dt``. Returns (o, dqkv)."""
    q = qkv.to(dt).detach().requires_grad_()
    qh, kh, vh = (_heads(t, dt) for t in q.split(A_H, dim=-1))
    s = torch.matmul(qh, kh.transpose(-1, -2)) * A_SCALE
    if mask is not None:
        s = s + mask.to(dt)
    pr = torch.softmax(s, dim=-1) * keep.to(dt) / (1.0 - A_P)
    o = torch.matmul(pr, vh).transpose(1, 2).reshape(A_B, -1, A_H)
    o.backward(dout.to(dt))
    return o.detach(), q.grad


def _probe_probs(e, qkv, mask, p, seed, salt):
    """[B, nh, S, S]: the (dropped, rescaled) probabilities the kernel
    applies, read out with V = identity on one 64-key chunk at a time."""
    S = qkv.shape[1]
    out = torch.zeros(A_B, A_NH, S, S, device=DEV)
    eye = torch.eye(64, device=DEV, dtype=qkv.dtype)
    for c in range(S // 64):
        probe = qkv.clone()
        probe[..., 2 * A_H:] = 0
        for h in range(A_NH):
            probe[:, c * 64:(c + 1) * 64,
                  2 * A_H + h * A_HD:2 * A_H + (h + 1) * A_HD] = eye
        o, _ = e.flash_attn_qkv_fwd(probe, mask, A_NH, A_SCALE, p, seed, salt)
        out[..., c * 64:(c + 1) * 64] = o.float().reshape(
            A_B, S, A_NH, A_HD).transpose(1, 2)
    return out


@functools.lru_cache(maxsize=None)
def _attn_case(S, dtype, with_mask):
    """Kernel outputs, the kernel's own keep mask and the references for one
    case; computed once and shared."""
    e = ext()
    torch.manual_seed(20)
    qkv = torch.randn(A_B, S, 3 * A_H, device=DEV, dtype=dtype)
    dout = torch.randn(A_B, S, A_H, device=DEV, dtype=dtype)
    live = torch.ones(A_B, 1, 1, S, device=DEV, dtype=torch.bool)
    if with_mask:
        live[1, :, :, S - S // 4:] = False
        mask = ((~live).to(dtype) * -10000.0).contiguous()
    else:
        mask = torch.Tensor().to(DEV)
    seed = torch.tensor([99], dtype=torch.int64, device=DEV)
    pd = _probe_probs(e, qkv, mask, A_P, seed, A_SALT)
    p0 = _probe_probs(e, qkv, mask, 0.0, torch.Tensor(), 0)
    keep = (pd != 0) | (p0 == 0)
    live = live.expand(A_B, A_NH, S, S)

    o, lse = e.flash_attn_qkv_fwd(qkv, mask, A_NH, A_SCALE, A_P, seed, A_SALT)
    dqkv = e.flash_attn_qkv_bwd(dout, qkv, o, lse, mask, A_NH, A_SCALE, A_P,
                                seed, A_SALT)
    m = mask if with_mask else None
    o64, dqkv64 = _attn_composition(qkv, m, keep, dout, F64)
    o_t, dqkv_t = _attn_composition(qkv, m, keep, dout, dtype)
    return dict(p0=p0, keep=keep, live=live, o=o, dqkv=dqkv, o64=o64,
                dqkv64=dqkv64, o_t=o_t, dqkv_t=dqkv_t)


_attn_params = pytest.mark.parametrize(
    "S,dtype,with_mask",
    [(S, dt, wm) for S in (128, 192) for dt in (BF16, FP16)
     for wm in (True, False)], ids=_ids)


@_attn_params
def test_flash_attn_dropout_mask_statistics(S, dtype, with_mask):
    c = _attn_case(S, dtype, with_mask)
    keep, live = c["keep"], c["live"]
    # the recovery of the mask needs every unmasked probability to be nonzero
    assert (c["p0"][live] != 0).all()
    n = int(live.sum().item())
    rate = 1.0 - keep[live].float().mean().item()
    sigma = math.sqrt(A_P * (1 - A_P) / n)
    print(f"drop rate {rate:.5f} over {n} entries (5 sigma = {5 * sigma:.5f})")
    assert abs(rate - A_P) < 5 * sigma
    # two (batch, head) pairs draw independent masks: a counter that ignored
    # the head or the batch would make them equal
    agree_p = A_P ** 2 + (1 - A_P) ** 2
    for (b0, h0), (b1, h1) in (((0, 0), (0, 1)), ((0, 0), (1, 0)),
                               ((0, 1), (1, 0))):
        both = live[b0, h0] & live[b1, h1]
        nb = int(both.sum().item())
        agree = (keep[b0, h0] == keep[b1, h1])[both].float().mean().item()
        sg = math.sqrt(agree_p * (1 - agree_p) / nb)
        print(f"masks of (b{b0},h{h0}) and (b{b1},h{h1}) agree on "
              f"{agree:.5f} of {nb} (expected {agree_p:.4f})")
        assert abs(agree - agree_p) < 5 * sg


def _rel(a, ref):
    return ((a.to(F64) - ref).abs().max().item()
            / max(ref.std().item(), 1.0))


@_attn_params
def test_flash_attn_dropout_same_mask(S, dtype, with_mask):
    """Forward and backward against fp64 under the kernel's own mask: at
    the tolerances of the no-dropout tests, and within twice the error of
    the same composition in plain torch ops of the kernel's dtype (the
    factor 2 is for summation order)."""
    c = _attn_case(S, dtype, with_mask)
    assert torch.isfinite(c["o"]).all() and torch.isfinite(c["dqkv"]).all()
    for name, got, same, ref, tol in (
            ("o", c["o"], c["o_t"], c["o64"], 3e-2),
            ("dqkv", c["dqkv"], c["dqkv_t"], c["dqkv64"], 5e-2)):
        k_err, t_err = _rel(got, ref), _rel(same, ref)
        print(f"S={S} {dtype} mask={with_mask} {name}: kernel {k_err:.3e}  "
              f"torch-same-dtype {t_err:.3e}")
        torch.testing.assert_close(got.to(F64), ref, rtol=tol, atol=tol)
        assert k_err <= 2 * t_err, (name, k_err, t_err)


# ----------------------------- B. bias+dropout+residual+LN backward, p > 0
@pytest.mark.parametrize("H", [256, 768])
@pytest.mark.parametrize("dtype", [FP32, BF16, FP16], ids=_ids)
def test_bdrl_dropout_fwd_bwd(dtype, H):
    e = ext()
    torch.manual_seed(21)
    # R = 37: the last block holds one of its four rows, and the column
    # reduce runs 19 chunks of two rows, the last with one
    R, p = 37, 0.1
    rtol, atol = LN_TOL[dtype]
    ulp = ULP[dtype]
    y = torch.randn(R, H, device=DEV, dtype=dtype)
    bias = torch.randn(H, device=DEV, dtype=dtype)
    res = torch.randn(R, H, device=DEV, dtype=dtype)
    lnw = torch.randn(H, device=DEV, dtype=dtype)
    lnb = torch.randn(H, device=DEV, dtype=dtype)
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    out, xsum, mask, mean, rstd = e.bias_dropout_residual_ln_fwd(
        y, bias, res, lnw, lnb, p, EPS, seed, 7)
    assert mask.shape == (R, H) and ((mask == 0) | (mask == 1)).all()
    m64 = mask.to(F64)
    assert 0.05 < 1.0 - m64.mean().item() < 0.15

    # forward: xsum = dropout(y + bias) + res under the returned mask. One
    # spacing of the dtype for the rounding of the result, 2^-21 for the
    # four fp32 operations before it, both relative to the two addends
    h64 = m64 * (y.to(F64) + bias.to(F64)) / (1 - p)
    x64 = h64 + res.to(F64)
    _close(xsum, x64, 0.0, TINY[dtype]
           + (ulp + 2.0 ** -21) * (h64.abs() + res.to(F64).abs()), "xsum")
    mean64, rstd64 = _stats64(xsum)
    amax = xsum.to(F64).abs().amax(-1)
    assert ((mean.to(F64) - mean64).abs() <= 2.0 ** -22 * amax).all()
    rstd_err = ((rstd.to(F64) - rstd64).abs() / rstd64).max().item()
    print(f"bdrl p={p} {dtype} H={H}: rstd rel err {rstd_err:.3e}")
    assert rstd_err <= 1e-5
    _close(out, _ln64(xsum, lnw, lnb), rtol, atol, "out")

    # backward against fp64 autograd of LN(mask * (y + bias) / (1-p) + res)
    dout = torch.randn(R, H, device=DEV, dtype=dtype)
    dy, dbias, dres, dlnw, dlnb = e.bias_dropout_residual_ln_bwd(
        dout, xsum, mask, lnw, mean, rstd, p)
    leaves = [t.to(F64).detach().requires_grad_()
              for t in (y, bias, res, lnw, lnb)]
    yr, br, rr, lw, lb = leaves
    F.layer_norm(m64 * (yr + br) / (1 - p) + rr, (H,), lw, lb,
                 EPS).backward(dout.to(F64))
    _close(dy, yr.grad, rtol, atol * 10, "dy")
    _close(dres, rr.grad, rtol, atol * 10, "dres")
    _close(dbias, br.grad, 5e-2, atol * 100, "dbias")
    _close(dlnw, lw.grad, rtol, atol * 50, "dlnw")
    _close(dlnb, lb.grad, rtol, atol * 50, "dlnb")

    # structure of the dropout backward
    assert (dy[mask == 0] == 0).all()
    # dy and dres are two roundings of g / (1-p) and g, half a spacing each.
    # 1/(1-p) is the fp32 value the kernel multiplies by.
    inv_keep = (1.0 / (1.0 - torch.tensor(p, dtype=FP32))).to(F64).item()
    kept = mask == 1
    want = dres.to(F64)[kept] * inv_keep
    one_ulp = (ulp * want.abs()).clamp(min=TINY[dtype])
    assert ((dy.to(F64)[kept] - want).abs() <= one_ulp).all()
    # dbias is the column sum of the returned dy: the rounding of the result
    # and R fp32 additions
    col = dy.to(F64).sum(0)
    _close(dbias, col, ulp, 2.0 ** -24 * R * dy.to(F64).abs().sum(0), "dbias")
    nodb = e.bias_dropout_residual_ln_bwd_nodb(dout, xsum, mask, lnw, mean,
                                               rstd, p)
    for name, a, b in zip(("dy", "dres", "dlnw", "dlnb"), nodb,
                          (dy, dres, dlnw, dlnb)):
        assert torch.equal(a, b), name


# ---------------- C. LayerNorm statistics on rows that are not zero-mean
# rstd relative error against fp64 on the offset rows, range over the three
# forwards, H and dtypes (MI355X), with the unshifted sumsq/H - mean^2 of
# the commit before and with the variance shifted by the row's first element:
#   rows (30, 1)    1.5e-05 .. 8.8e-05   ->   4.3e-08 .. 3.2e-07
#   rows (100, 1)   3.7e-04 .. 9.5e-04   ->   3.0e-08 .. 2.6e-07
#   rows (-50, 2)   1.9e-05 .. 6.9e-05   ->   4.8e-08 .. 2.9e-07
# mean was within 1e-07 relative before and after. The constant-0.3 rows
# gave rstd = NaN before at fp16 H=1024 (all three forwards) and at fp32
# H=100 (ln, emb), and rstd of 7e3 .. 9e3 instead of 1e6 at fp32 H=768/1024.
LN_ROWS = 8
LN_FORWARDS = [("ln", 100), ("ln", 768), ("ln", 1024),
               ("bdrl", 768), ("bdrl", 1024),
               ("emb", 100), ("emb", 768), ("emb", 1024)]


def _ln_forward(kind, x, w, b):
    """(y, mean, rstd) of rows ``x`` through one of the three forwards."""
    e = ext()
    R, H = x.shape
    if kind == "ln":
        return e.layernorm_fwd(x, w, b, EPS)
    if kind == "bdrl":
        out, xsum, _, mean, rstd = e.bias_dropout_residual_ln_fwd(
            x, torch.zeros_like(w), torch.zeros_like(x), w, b, 0.0, EPS,
            torch.Tensor(), 0)
        assert torch.equal(xsum, x)
        return out, mean, rstd
    # the rows are the word table; position and type tables are zero
    ids = torch.arange(R, device=DEV).flip(0).reshape(2, R // 2).contiguous()
    pids = torch.arange(R // 2, device=DEV).repeat(2, 1).contiguous()
    tids = (pids % 2).contiguous()
    pos = torch.zeros(R // 2, H, device=DEV, dtype=x.dtype)
    typ = torch.zeros(2, H, device=DEV, dtype=x.dtype)
    y, mean, rstd = e.embedding_ln_fwd(ids, tids, pids, x, pos, typ, w, b, EPS)
    back = torch.arange(R, device=DEV).flip(0)
    return y.reshape(R, H)[back], mean[back], rstd[back]


def _ln_wb(H, dtype):
    g = torch.Generator(device=DEV).manual_seed(22)
    return (torch.randn(H, device=DEV, dtype=dtype, generator=g),
            torch.randn(H, device=DEV, dtype=dtype, generator=g))


@pytest.mark.parametrize("mu,sd", [(30.0, 1.0), (100.0, 1.0), (-50.0, 2.0)])
@pytest.mark.parametrize("dtype", [FP32, BF16, FP16], ids=_ids)
@pytest.mark.parametrize("kind,H", LN_FORWARDS)
def test_layernorm_stats_offset_rows(kind, H, dtype, mu, sd):
    torch.manual_seed(23)
    x = (mu + sd * torch.randn(LN_ROWS, H, device=DEV)).to(dtype)
    w, b = _ln_wb(H, dtype)
    y, mean, rstd = _ln_forward(kind, x, w, b)
    mean64, rstd64 = _stats64(x)
    rstd_err = ((rstd.to(F64) - rstd64).abs() / rstd64).max().item()
    mean_err = ((mean.to(F64) - mean64).abs() / mean64.abs()).max().item()
    print(f"{kind} H={H} {dtype} rows ({mu}, {sd}): rstd rel err "
          f"{rstd_err:.3e}  mean rel err {mean_err:.3e}")
    assert rstd_err <= 1e-5
    assert mean_err <= 2.0 ** -22
    _close(y, _ln64(x, w, b), *LN_TOL[dtype], "y")


@pytest.mark.parametrize("const", [0.3, 1.0, 0.0])
@pytest.mark.parametrize("dtype", [FP32, BF16, FP16], ids=_ids)
@pytest.mark.parametrize("kind,H", LN_FORWARDS)
def test_layernorm_stats_flat_rows(kind, H, dtype, const):
    """The variance of a constant row is 0, so rstd is not pinned; a NaN or
    a normalised value beyond 1 is what must not happen."""
    x = torch.full((LN_ROWS, H), const, device=DEV).to(dtype)
    w, b = _ln_wb(H, dtype)
    y, mean, rstd = _ln_forward(kind, x, w, b)
    print(f"{kind} H={H} {dtype} const {const}: rstd {rstd[0].item():.4e} "
          f"mean {mean[0].item():.8f} max|y-b| "
          f"{(y.to(F64) - b.to(F64)).abs().max().item():.3e}")
    assert torch.isfinite(y).all()
    assert torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    assert (rstd > 0).all()
    assert ((y.to(F64) - b.to(F64)).abs() <= w.to(F64).abs()).all()


# ------------------------- D. odd sizes and hard values, the small kernels
def _hard_values(shape, dtype, seed):
    torch.manual_seed(seed)
    x = (torch.randn(*shape, device=DEV) * 2).to(dtype)
    x[0, 0], x[0, 1], x[0, 2], x[-1, -1] = 6.0, -6.0, 0.0, -6.0
    return x


# 60 and 51 elements: neither a multiple of the 8 a thread takes at a time
ODD_SHAPES = [(5, 12), (3, 17)]


def _shape_id(s):
    return f"{s[0]}x{s[1]}"


@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("dtype", [FP32, BF16, FP16], ids=_ids)
def test_bias_gelu_odd_sizes(dtype, shape):
    e = ext()
    rtol, atol = ELT_TOL[dtype]
    x = _hard_values(shape, dtype, 24)
    b = torch.randn(shape[1], device=DEV).to(dtype)
    b[:3] = 0          # the pre-activation is exactly 6, -6 and 0 there
    b[-1] = 0
    y = e.bias_gelu_fwd(x, b)
    xr = x.to(F64).detach().requires_grad_()
    br = b.to(F64).detach().requires_grad_()
    ref = F.gelu(xr + br)
    _close(y, ref.detach(), rtol, atol, "y")
    dy = torch.randn(*shape, device=DEV).to(dtype)
    dx, db = e.bias_gelu_bwd(dy, x, b)
    ref.backward(dy.to(F64))
    _close(dx, xr.grad, rtol, atol, "dx")
    _close(db, br.grad, rtol, atol * 100, "db")


@pytest.mark.parametrize("shape", ODD_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=_ids)
@pytest.mark.parametrize("op", ["gelu_bwd", "tanh_bwd"])
def test_act_bwd_odd_sizes(op, dtype, shape):
    e = ext()
    rtol, atol = ELT_TOL[dtype]
    pre = _hard_values(shape, dtype, 25)
    dy = torch.randn(*shape, device=DEV).to(dtype)
    dx = getattr(e, op)(dy, pre)
    pr = pre.to(F64).detach().requires_grad_()
    (F.gelu(pr) if op == "gelu_bwd" else torch.tanh(pr)).backward(dy.to(F64))
    _close(dx, pr.grad, rtol, atol, "dx")


@pytest.mark.parametrize("S", [1, 100, 1024])
@pytest.mark.parametrize("dtype", [FP32, BF16, FP16], ids=_ids)
def test_masked_softmax_odd_sizes(dtype, S):
    e = ext()
    torch.manual_seed(26)
    B, NH = 2, 2
    rtol, atol = SM_TOL[dtype]
    scores = (torch.randn(B, NH, S, S, device=DEV) * 4).to(dtype)
    mask = torch.zeros(B, 1, 1, S, device=DEV, dtype=dtype)
    mask[0] = -10000.0     # batch 0: every key masked; batch 1: none
    scale = 1.0 / math.sqrt(64)
    p = e.masked_softmax_fwd(scores, mask, scale)
    assert torch.isfinite(p).all()
    ref = torch.softmax(scores.to(F64) * scale + mask.to(F64), dim=-1)
    # the kernel adds the mask in fp32, as the model's softmax does: a score
    # near -10000 is rounded to half of fp32's spacing there, 2^-11, and a
    # probability moves by at most twice that, relatively
    rt = torch.tensor([rtol + 2.0 ** -10, rtol], device=DEV, dtype=F64)
    excess = (p.to(F64) - ref).abs() - (rt.view(B, 1, 1, 1) * ref + atol)
    assert (excess <= 0).all(), excess.max().item()
    # rows sum to 1: half a spacing per entry, relative to the entry, and 22
    # fp32 additions (16 per lane, 6 butterfly steps) behind the normaliser
    assert ((p.to(F64).sum(-1) - 1).abs() <= ULP[dtype] + 2.0 ** -19).all()

    dy = torch.randn(B, NH, S, S, device=DEV).to(dtype)
    dx = e.masked_softmax_bwd(dy, p)
    p64, dy64 = p.to(F64), dy.to(F64)
    dref = (dy64 - (dy64 * p64).sum(-1, keepdim=True)) * p64
    _close(dx, dref, rtol, atol, "dx")


@pytest.mark.parametrize("B,C", [(1, 6), (5, 70)])
def test_cross_entropy_hard_logits(B, C):
    e = ext()
    torch.manual_seed(27)
    logits = torch.randn(B, C, device=DEV) * 3
    labels = torch.randint(0, C, (B,), device=DEV)
    logits[0, 1], logits[0, 2], labels[0] = 80.0, -80.0, 2   # loss near 160
    if B > 1:
        logits[1] = 7.5                       # a row of equal values
        logits[2, 3], labels[2] = 80.0, 3     # loss near 0
    cases = [(logits, labels)]
    if B == 1:
        cases.append((torch.full((1, C), -3.25, device=DEV), labels))
    for lg, lb in cases:
        loss, logprobs = e.cross_entropy_fwd(lg, lb)
        assert torch.isfinite(loss) and torch.isfinite(logprobs).all()
        lr = lg.to(F64).detach().requires_grad_()
        lp64 = torch.log_softmax(lr, dim=-1)
        ref = F.nll_loss(lp64, lb)
        # log-sum-exp is formed at the magnitude of the largest logit: one
        # fp32 spacing at 80 is 2^-17
        _close(logprobs, lp64.detach(), 1e-5, 2.0 ** -17, "logprobs")
        _close(loss, ref.detach(), 1e-5, 2.0 ** -17, "loss")
        dloss = torch.tensor(1.7, device=DEV)
        dl = e.cross_entropy_bwd(dloss, logprobs, lb)
        (ref * 1.7).backward()
        assert torch.isfinite(dl).all()
        _close(dl, lr.grad, 1e-5, 2.0 ** -17 * 1.7 / B, "dlogits")


@pytest.mark.parametrize("dtype", [FP32, BF16], ids=_ids)
def test_embedding_ln_padded_packed_ids(dtype):
    """Mostly id 0 (a padded batch), positions that restart inside a row (a
    packed batch) and R = 33 rows, which is two 16-row chunks and one row."""
    e = ext()
    torch.manual_seed(28)
    B, S, H, V = 3, 11, 128, 16
    rtol, atol = LN_TOL[dtype]
    ids = torch.randint(1, V, (B, S), device=DEV)
    ids[torch.rand(B, S, device=DEV) < 0.8] = 0
    pids = torch.tensor(list(range(5)) + list(range(6)),
                        device=DEV).repeat(B, 1).contiguous()
    tids = (torch.arange(B * S, device=DEV) % 2).reshape(B, S).contiguous()
    word = torch.randn(V, H, device=DEV, dtype=dtype)
    pos = torch.randn(8, H, device=DEV, dtype=dtype)
    typ = torch.randn(2, H, device=DEV, dtype=dtype)
    lnw = torch.randn(H, device=DEV, dtype=dtype)
    lnb = torch.randn(H, device=DEV, dtype=dtype)
    y, mean, rstd = e.embedding_ln_fwd(ids, tids, pids, word, pos, typ,
                                       lnw, lnb, EPS)
    wr, pr, tr, lw, lb = (t.to(F64).detach().requires_grad_()
                          for t in (word, pos, typ, lnw, lnb))
    emb = F.embedding(ids, wr) + F.embedding(pids, pr) + F.embedding(tids, tr)
    ref = F.layer_norm(emb, (H,), lw, lb, EPS)
    _close(y, ref.detach(), rtol, atol, "y")

    dy = torch.randn(B, S, H, device=DEV, dtype=dtype)
    grads = e.embedding_ln_bwd(dy, ids, tids, pids, word, pos, typ, lnw,
                               mean, rstd)
    ref.backward(dy.to(F64))

    def count(idx, n):
        return torch.bincount(idx.flatten(), minlength=n).clamp(min=1).to(F64)

    R = B * S
    # fp32: atomics reorder the sum and add no error, so atol grows with the
    # number of rows summed only; bf16: the multipliers of test_embedding_ln
    dup = [count(ids, V)[:, None], count(pids, 8)[:, None],
           count(tids, 2)[:, None], float(R), float(R)]
    mult = [20, 20, 50, 50, 50]
    names = ["dword", "dpos", "dtype", "dlnw", "dlnb"]
    for name, got, want, d, k in zip(names, grads, (wr, pr, tr, lw, lb),
                                     dup, mult):
        _close(got, want.grad, rtol, atol * (d if dtype == FP32 else k), name)
