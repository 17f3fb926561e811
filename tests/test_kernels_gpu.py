"""GPU numerics tests: every HIP kernel vs a plain PyTorch fp32 reference
(the torch-path composition in functional.py). fp32 kernel runs get tight
tolerances; bf16 runs get bf16-roundoff tolerances."""

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


# ---------------------------------------------------------------- layernorm
@pytest.mark.parametrize("dtype,rtol,atol", [
    (torch.float32, 1e-5, 1e-5), (torch.bfloat16, 2e-2, 2e-2)])
@pytest.mark.parametrize("H", [64, 768, 1024])
def test_layernorm_fwd_bwd(dtype, rtol, atol, H):
    e = ext()
    torch.manual_seed(0)
    R = 512
    x = torch.randn(R, H, device=DEV, dtype=dtype)
    w = torch.randn(H, device=DEV, dtype=dtype)
    b = torch.randn(H, device=DEV, dtype=dtype)
    y, mean, rstd = e.layernorm_fwd(x, w, b, 1e-12)
    ref = F.layer_norm(x.float(), (H,), w.float(), b.float(), 1e-12)
    torch.testing.assert_close(y.float(), ref, rtol=rtol, atol=atol)

    dy = torch.randn_like(x)
    dx, dw, db = e.layernorm_bwd(dy, x, w, mean, rstd)
    xr = x.float().detach().requires_grad_()
    wr = w.float().detach().requires_grad_()
    br = b.float().detach().requires_grad_()
    F.layer_norm(xr, (H,), wr, br, 1e-12).backward(dy.float())
    torch.testing.assert_close(dx.float(), xr.grad, rtol=rtol, atol=atol * 10)
    torch.testing.assert_close(dw.float(), wr.grad, rtol=rtol, atol=atol * 50)
    torch.testing.assert_close(db.float(), br.grad, rtol=rtol, atol=atol * 50)


# ------------------------------------------------------------- embedding+LN
@pytest.mark.parametrize("dtype,rtol,atol", [
    (torch.float32, 1e-5, 1e-5), (torch.bfloat16, 2e-2, 2e-2)])
def test_embedding_ln(dtype, rtol, atol):
    e = ext()
    torch.manual_seed(1)
    B, S, H, V = 4, 32, 768, 1000
    ids = torch.randint(0, V, (B, S), device=DEV)
    tids = torch.randint(0, 2, (B, S), device=DEV)
    pids = torch.arange(S, device=DEV).repeat(B, 1).contiguous()
    word = torch.randn(V, H, device=DEV, dtype=dtype)
    pos = torch.randn(S, H, device=DEV, dtype=dtype)
    typ = torch.randn(2, H, device=DEV, dtype=dtype)
    lnw = torch.randn(H, device=DEV, dtype=dtype)
    lnb = torch.randn(H, device=DEV, dtype=dtype)
    y, mean, rstd = e.embedding_ln_fwd(ids, tids, pids, word, pos, typ,
                                       lnw, lnb, 1e-12)
    emb = (F.embedding(ids, word.float()) + F.embedding(pids, pos.float())
           + F.embedding(tids, typ.float()))
    ref = F.layer_norm(emb, (H,), lnw.float(), lnb.float(), 1e-12)
    torch.testing.assert_close(y.float(), ref, rtol=rtol, atol=atol)

    dy = torch.randn(B, S, H, device=DEV, dtype=dtype)
    dword, dpos, dtyp, dlnw, dlnb = e.embedding_ln_bwd(
        dy, ids, tids, pids, word, pos, typ, lnw, mean, rstd)
    wr = word.float().detach().requires_grad_()
    pr = pos.float().detach().requires_grad_()
    tr = typ.float().detach().requires_grad_()
    lw = lnw.float().detach().requires_grad_()
    lb = lnb.float().detach().requires_grad_()
    emb = F.embedding(ids, wr) + F.embedding(pids, pr) + F.embedding(tids, tr)
    F.layer_norm(emb, (H,), lw, lb, 1e-12).backward(dy.float())
    torch.testing.assert_close(dword.float(), wr.grad, rtol=rtol, atol=atol * 20)
    torch.testing.assert_close(dpos.float(), pr.grad, rtol=rtol, atol=atol * 20)
    torch.testing.assert_close(dtyp.float(), tr.grad, rtol=rtol, atol=atol * 50)
    torch.testing.assert_close(dlnw.float(), lw.grad, rtol=rtol, atol=atol * 50)
    torch.testing.assert_close(dlnb.float(), lb.grad, rtol=rtol, atol=atol * 50)


# ------------------------------------------------------------ masked softmax
@pytest.mark.parametrize("dtype,rtol,atol", [
    (torch.float32, 1e-5, 1e-6), (torch.bfloat16, 1e-2, 1e-2)])
@pytest.mark.parametrize("S", [128, 512])
def test_masked_softmax(dtype, rtol, atol, S):
    e = ext()
    torch.manual_seed(2)
    B, NH = 4, 12
    scores = torch.randn(B, NH, S, S, device=DEV, dtype=dtype) * 4
    mask = torch.zeros(B, 1, 1, S, device=DEV, dtype=dtype)
    mask[:, :, :, S // 2:] = -10000.0
    scale = 1.0 / math.sqrt(64)
    p = e.masked_softmax_fwd(scores, mask, scale)
    ref = F.softmax(scores.float() * scale + mask.float(), dim=-1)
    torch.testing.assert_close(p.float(), ref, rtol=rtol, atol=atol)
    assert torch.allclose(p.float().sum(-1),
                          torch.ones(B, NH, S, S // S, device=DEV).squeeze(-1),
                          atol=1e-2)

    dy = torch.randn_like(scores)
    dx = e.masked_softmax_bwd(dy, p)
    sref = (scores.float() * scale + mask.float()).detach().requires_grad_()
    F.softmax(sref, dim=-1).backward(dy.float())
    torch.testing.assert_close(dx.float(), sref.grad, rtol=rtol, atol=atol)


# ------------------------------------------------------------------ gelu ops
@pytest.mark.parametrize("dtype,rtol,atol", [
    (torch.float32, 1e-5, 1e-6), (torch.bfloat16, 2e-2, 2e-2)])
def test_bias_gelu(dtype, rtol, atol):
    e = ext()
    torch.manual_seed(3)
    R, N = 512, 3072
    x = torch.randn(R, N, device=DEV, dtype=dtype)
    b = torch.randn(N, device=DEV, dtype=dtype)
    y = e.bias_gelu_fwd(x, b)
    ref = F.gelu(x.float() + b.float())
    torch.testing.assert_close(y.float(), ref, rtol=rtol, atol=atol)

    dy = torch.randn_like(x)
    dx, db = e.bias_gelu_bwd(dy, x, b)
    xr = x.float().detach().requires_grad_()
    br = b.float().detach().requires_grad_()
    F.gelu(xr + br).backward(dy.float())
    torch.testing.assert_close(dx.float(), xr.grad, rtol=rtol, atol=atol)
    torch.testing.assert_close(db.float(), br.grad, rtol=rtol, atol=atol * 100)


# ------------------------------------------- bias+dropout+residual+layernorm
@pytest.mark.parametrize("dtype,rtol,atol", [
    (torch.float32, 1e-5, 1e-5), (torch.bfloat16, 2e-2, 2e-2)])
def test_bdrl_no_dropout(dtype, rtol, atol):
    e = ext()
    torch.manual_seed(4)
    R, H = 512, 768
    y = torch.randn(R, H, device=DEV, dtype=dtype)
    bias = torch.randn(H, device=DEV, dtype=dtype)
    res = torch.randn(R, H, device=DEV, dtype=dtype)
    lnw = torch.randn(H, device=DEV, dtype=dtype)
    lnb = torch.randn(H, device=DEV, dtype=dtype)
    out, xsum, mask, mean, rstd = e.bias_dropout_residual_ln_fwd(
        y, bias, res, lnw, lnb, 0.0, 1e-12, torch.Tensor(), 0)
    ref = F.layer_norm(y.float() + bias.float() + res.float(), (H,),
                       lnw.float(), lnb.float(), 1e-12)
    torch.testing.assert_close(out.float(), ref, rtol=rtol, atol=atol)

    dout = torch.randn_like(y)
    dy, dbias, dres, dlnw, dlnb = e.bias_dropout_residual_ln_bwd(
        dout, xsum, mask, lnw, mean, rstd, 0.0)
    yr = y.float().detach().requires_grad_()
    br = bias.float().detach().requires_grad_()
    rr = res.float().detach().requires_grad_()
    lw = lnw.float().detach().requires_grad_()
    lb = lnb.float().detach().requires_grad_()
    F.layer_norm(yr + br + rr, (H,), lw, lb, 1e-12).backward(dout.float())
    torch.testing.assert_close(dy.float(), yr.grad, rtol=rtol, atol=atol * 10)
    torch.testing.assert_close(dres.float(), rr.grad, rtol=rtol, atol=atol * 10)
    torch.testing.assert_close(dbias.float(), br.grad, rtol=5e-2, atol=atol * 100)
    torch.testing.assert_close(dlnw.float(), lw.grad, rtol=rtol, atol=atol * 50)
    torch.testing.assert_close(dlnb.float(), lb.grad, rtol=rtol, atol=atol * 50)


def test_bdrl_dropout_statistics():
    e = ext()
    torch.manual_seed(5)
    R, H, p = 2048, 768, 0.1
    y = torch.randn(R, H, device=DEV, dtype=torch.float32)
    z = torch.zeros(H, device=DEV)
    res = torch.zeros(R, H, device=DEV)
    lnw = torch.ones(H, device=DEV)
    lnb = torch.zeros(H, device=DEV)
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    out, xsum, mask, mean, rstd = e.bias_dropout_residual_ln_fwd(
        y, z, res, lnw, lnb, p, 1e-12, seed, 7)
    keep_rate = mask.float().mean().item()
    assert abs(keep_rate - (1 - p)) < 5e-3, keep_rate
    # kept elements are scaled by 1/(1-p) before the residual add
    kept = mask.view(R, H).bool()
    torch.testing.assert_close(xsum[kept], y[kept] / (1 - p),
                               rtol=1e-5, atol=1e-5)
    assert (xsum[~kept] == 0).all()
    # determinism in (device seed, salt)
    out2, xsum2, mask2, _, _ = e.bias_dropout_residual_ln_fwd(
        y, z, res, lnw, lnb, p, 1e-12, seed, 7)
    assert torch.equal(mask, mask2)
    # updating the DEVICE seed changes the mask (hipGraph replay contract)
    seed.fill_(99)
    _, _, mask3, _, _ = e.bias_dropout_residual_ln_fwd(
        y, z, res, lnw, lnb, p, 1e-12, seed, 7)
    assert not torch.equal(mask, mask3)


# ---------------------------------------------------------------------- gemm
@pytest.mark.parametrize("M,N,K", [(256, 768, 768), (4096, 3072, 768),
                                   (4096, 768, 3072), (32, 768, 768),
                                   (100, 128, 64)])
def test_gemm_nt_bf16(M, N, K):
    e = ext()
    torch.manual_seed(6)
    A = (torch.randn(M, K, device=DEV) / math.sqrt(K)).bfloat16()
    W = torch.randn(N, K, device=DEV).bfloat16()
    bias = torch.randn(N, device=DEV).bfloat16()
    C, _ = e.gemm_nt_fwd(A, W, bias, "none")
    ref = A.float() @ W.float().t() + bias.float()
    err = (C.float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err < 2e-2 * max(scale, 1.0), (err, scale)


def test_gemm_identity_and_transpose_detection():
    """Asymmetric-B identity test (guide: symmetric inputs miss transposes)."""
    e = ext()
    K = 64
    A = torch.eye(128, K, device=DEV).bfloat16()
    W = torch.zeros(128, K, device=DEV)
    for i in range(128):
        for j in range(0, K, 7):
            W[i, j] = i * 0.01 + j  # asymmetric
    W = W.bfloat16()
    C, _ = e.gemm_nt_fwd(A, W, torch.Tensor().to(DEV), "none")
    ref = A.float() @ W.float().t()
    torch.testing.assert_close(C.float(), ref, rtol=1e-3, atol=1e-3)


def test_gemm_gelu_epilogue():
    e = ext()
    torch.manual_seed(7)
    M, N, K = 512, 3072, 768
    A = (torch.randn(M, K, device=DEV) / math.sqrt(K)).bfloat16()
    W = torch.randn(N, K, device=DEV).bfloat16()
    bias = torch.randn(N, device=DEV).bfloat16()
    C, pre = e.gemm_nt_fwd(A, W, bias, "gelu")
    pre_ref = A.float() @ W.float().t() + bias.float()
    ref = F.gelu(pre_ref)
    assert (pre.float() - pre_ref).abs().max().item() < 0.05
    assert (C.float() - ref).abs().max().item() < 0.05


# --------------------------------------------------------------------- adamw
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_multi_tensor_adamw(dtype):
    import pdnlp_amd.ops.adamw as A
    torch.manual_seed(8)
    shapes = [(768,), (768, 768), (3072,), (21128, 768), (5,)]
    params = [torch.randn(*s, device=DEV, dtype=dtype) for s in shapes]
    grads = [torch.randn(*s, device=DEV, dtype=dtype) for s in shapes]
    ms = [torch.rand(*s, device=DEV) * 0.1 for s in shapes]
    vs = [torch.rand(*s, device=DEV) * 0.01 for s in shapes]
    use_master = dtype != torch.float32
    masters = [p.float().clone() if use_master else None for p in params]

    ref_p = [p.clone() for p in params]
    ref_m = [m.clone() for m in ms]
    ref_v = [v.clone() for v in vs]
    ref_mw = [mw.clone() if mw is not None else None for mw in masters]

    e = ext()
    e.multi_tensor_adamw(params, grads, ms, vs,
                         masters if use_master else [],
                         1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001, 1.0,
                         torch.Tensor())
    # python reference (the fallback in ops.adamw)
    import os
    os.environ["PDNLP_FORCE_TORCH"] = "1"
    try:
        A.multi_tensor_adamw(ref_p, grads, ref_m, ref_v, ref_mw,
                             1e-3, 0.9, 0.999, 1e-8, 0.01,
                             step=1, grad_scale_inv=1.0)
    finally:
        del os.environ["PDNLP_FORCE_TORCH"]
    # step=1 with betas -> bc1=0.1, bc2=0.001 matches the raw bc args above
    for p, rp in zip(params, ref_p):
        tol = 1e-6 if dtype == torch.float32 else 1e-2
        torch.testing.assert_close(p.float(), rp.float(), rtol=tol, atol=tol)
    for m, rm in zip(ms, ref_m):
        torch.testing.assert_close(m, rm, rtol=1e-5, atol=1e-6)


def test_multi_tensor_unscale():
    e = ext()
    g1 = torch.full((1000,), 8.0, device=DEV)
    g2 = torch.full((37,), 4.0, device=DEV)
    found = torch.zeros(1, device=DEV)
    e.multi_tensor_unscale([g1, g2], found, 0.25)
    assert found.item() == 0
    torch.testing.assert_close(g1, torch.full((1000,), 2.0, device=DEV))
    torch.testing.assert_close(g2, torch.full((37,), 1.0, device=DEV))
    g1[500] = float("inf")
    e.multi_tensor_unscale([g1], found, 1.0)
    assert found.item() == 1


# ------------------------------------------------------------- cross entropy
def test_cross_entropy():
    e = ext()
    torch.manual_seed(9)
    B, C = 32, 6
    logits = torch.randn(B, C, device=DEV)
    labels = torch.randint(0, C, (B,), device=DEV)
    loss, logprobs = e.cross_entropy_fwd(logits, labels)
    ref = F.cross_entropy(logits, labels)
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
    dloss = torch.tensor(1.7, device=DEV)
    dl = e.cross_entropy_bwd(dloss, logprobs, labels)
    lr = logits.detach().requires_grad_()
    (F.cross_entropy(lr, labels) * 1.7).backward()
    torch.testing.assert_close(dl, lr.grad, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------- flash attention
def _attn_ref(qkv, mask, nh, p=0.0):
    """fp32 reference of attention_packed on the packed qkv tensor."""
    B, S, H3 = qkv.shape
    H = H3 // 3
    hd = H // nh
    q, k, v = qkv.float().split(H, dim=-1)
    q = q.view(B, S, nh, hd).transpose(1, 2)
    k = k.view(B, S, nh, hd).transpose(1, 2)
    v = v.view(B, S, nh, hd).transpose(1, 2)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
    if mask is not None:
        s = s + mask.float()
    p_ = F.softmax(s, dim=-1)
    return torch.matmul(p_, v).transpose(1, 2).reshape(B, S, H)


@pytest.mark.parametrize("S,nh", [(128, 12), (512, 4), (64, 2), (192, 2)])
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_flash_attn_fwd(S, nh, with_mask, dtype):
    e = ext()
    torch.manual_seed(0)
    B, hd = 3, 64
    H = nh * hd
    qkv = torch.randn(B, S, 3 * H, device=DEV, dtype=dtype)
    if with_mask:
        keep = torch.ones(B, S, device=DEV)
        keep[:, S // 2:] = 0  # mask out the tail keys
        keep[0] = 1
        mask = ((1.0 - keep[:, None, None, :]) * -10000.0).to(dtype)
    else:
        mask = torch.Tensor().to(DEV)
    o, lse = e.flash_attn_qkv_fwd(qkv, mask, nh, 1.0 / math.sqrt(hd), 0.0,
                                  torch.Tensor(), 0)
    ref = _attn_ref(qkv, mask if with_mask else None, nh)
    torch.testing.assert_close(o.float(), ref, rtol=3e-2, atol=3e-2)
    # lse finite and plausible
    assert torch.isfinite(lse).all()


@pytest.mark.parametrize("S,nh", [(128, 12), (512, 4), (192, 2)])
def test_flash_attn_bwd(S, nh):
    e = ext()
    torch.manual_seed(1)
    B, hd = 2, 64
    H = nh * hd
    qkv = torch.randn(B, S, 3 * H, device=DEV, dtype=torch.bfloat16)
    keep = torch.ones(B, S, device=DEV)
    keep[1, S // 4:] = 0
    mask = ((1.0 - keep[:, None, None, :]) * -10000.0).to(torch.bfloat16)
    scale = 1.0 / math.sqrt(hd)
    o, lse = e.flash_attn_qkv_fwd(qkv, mask, nh, scale, 0.0, torch.Tensor(), 0)
    dout = torch.randn(B, S, H, device=DEV, dtype=torch.bfloat16)
    dqkv = e.flash_attn_qkv_bwd(dout, qkv, o, lse, mask, nh, scale, 0.0,
                                torch.Tensor(), 0)
    qr = qkv.float().detach().requires_grad_()
    _attn_ref(qr, mask, nh).backward(dout.float())
    torch.testing.assert_close(dqkv.float(), qr.grad, rtol=5e-2, atol=5e-2)


def test_flash_attn_dropout_determinism_and_rate():
    e = ext()
    torch.manual_seed(2)
    B, S, nh, hd = 2, 128, 4, 64
    H = nh * hd
    qkv = torch.randn(B, S, 3 * H, device=DEV, dtype=torch.bfloat16)
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    scale = 1.0 / math.sqrt(hd)
    o1, lse1 = e.flash_attn_qkv_fwd(qkv, torch.Tensor(), nh, scale, 0.1, seed, 7)
    o2, _ = e.flash_attn_qkv_fwd(qkv, torch.Tensor(), nh, scale, 0.1, seed, 7)
    torch.testing.assert_close(o1, o2)  # bit-identical on same (seed, salt)
    o3, _ = e.flash_attn_qkv_fwd(qkv, torch.Tensor(), nh, scale, 0.1, seed, 8)
    assert not torch.equal(o1, o3)      # new salt -> new masks
    # expectation: E[dropout(P)] = P, so mean output stays close to p=0 output
    o0, _ = e.flash_attn_qkv_fwd(qkv, torch.Tensor(), nh, scale, 0.0,
                                 torch.Tensor(), 0)
    assert (o1.float() - o0.float()).abs().mean() < 0.2


def test_flash_attn_dropout_bwd_matches_masked_ref():
    """Backward under dropout vs an fp32 reference that applies the SAME
    mask, extracted by probing the kernel with uniform V."""
    e = ext()
    torch.manual_seed(3)
    B, S, nh, hd = 1, 64, 1, 64
    H = nh * hd
    p = 0.3
    scale = 1.0 / math.sqrt(hd)
    seed = torch.tensor([99], dtype=torch.int64, device=DEV)
    qkv = torch.randn(B, S, 3 * H, device=DEV, dtype=torch.bfloat16)
    # probe: with V=identity-ish columns we can't extract the mask directly;
    # instead verify analytically: compare kernel grads against reference
    # grads computed with the kernel's own forward P-dropout realization.
    # Reference: rebuild P in fp32, re-derive the keep mask from the kernel's
    # hash by comparing a probe forward with p>0 against p=0 probabilities.
    # Probe uses V = e_j basis so O = Pd @ V = Pd — read the dropped P rows.
    qkv_probe = qkv.clone()
    qkv_probe[..., 2 * H:] = 0
    eye = torch.eye(S, device=DEV)
    # V [S, hd]: only works when S == hd; here S = 64 = hd
    qkv_probe[..., 2 * H:] = eye.to(torch.bfloat16).repeat(B, 1, 1)
    od, _ = e.flash_attn_qkv_fwd(qkv_probe, torch.Tensor(), nh, scale, p,
                                 seed, 5)
    o0, _ = e.flash_attn_qkv_fwd(qkv_probe, torch.Tensor(), nh, scale, 0.0,
                                 torch.Tensor(), 0)
    pd = od.float()   # dropped, scaled P
    p0 = o0.float()   # undropped P
    keep = (pd.abs() > 1e-12) | (p0.abs() < 1e-12)
    # rate sanity: ~p of entries dropped
    drop_rate = 1.0 - keep.float().mean().item()
    assert abs(drop_rate - p) < 0.05
    assert (p0 != 0).all()   # else a dropped entry could not be told apart

    # forward and backward on the real V against the fp32 reference under
    # that mask (B = nh = 1: the [S, S] probe output is the mask of the
    # only head)
    o, lse = e.flash_attn_qkv_fwd(qkv, torch.Tensor(), nh, scale, p, seed, 5)
    dout = torch.randn(B, S, H, device=DEV, dtype=torch.bfloat16)
    dqkv = e.flash_attn_qkv_bwd(dout, qkv, o, lse, torch.Tensor(), nh, scale,
                                p, seed, 5)
    qr = qkv.float().detach().requires_grad_()
    q, k, v = qr.split(H, dim=-1)
    pr = F.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1)
    ref = torch.matmul(pr * keep.float() / (1.0 - p), v)
    torch.testing.assert_close(o.float(), ref.detach(), rtol=3e-2, atol=3e-2)
    ref.backward(dout.float())
    torch.testing.assert_close(dqkv.float(), qr.grad, rtol=5e-2, atol=5e-2)


def test_col_sum():
    e = ext()
    torch.manual_seed(5)
    dy = torch.randn(2048, 3072, device=DEV, dtype=torch.bfloat16)
    cs = e.col_sum(dy)
    torch.testing.assert_close(cs.float(), dy.float().sum(0),
                               rtol=2e-2, atol=2e-1)


@pytest.mark.parametrize("M,N,K", [(4096, 2304, 768), (4096, 768, 3072),
                                   (512, 768, 768)])
def test_gemm_tn(M, N, K):
    e = ext()
    torch.manual_seed(7)
    A = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
    B = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    C = e.gemm_tn(A, B)
    ref = A.float().t() @ B.float()
    torch.testing.assert_close(C.float(), ref, rtol=3e-2, atol=3e-1)


def test_adamw_device_side_overflow_skip():
    """found_inf flag set on device -> the fused AdamW must be a no-op."""
    e = ext()
    torch.manual_seed(9)
    p = torch.randn(1000, device=DEV, dtype=torch.bfloat16)
    p0 = p.clone()
    g = torch.randn_like(p)
    m = torch.zeros(1000, device=DEV, dtype=torch.float32)
    v = torch.zeros_like(m)
    flag = torch.ones(1, device=DEV, dtype=torch.float32)
    e.multi_tensor_adamw([p], [g], [m], [v], [], 1e-2, 0.9, 0.999, 1e-8,
                         0.0, 0.1, 0.001, 1.0, flag)
    torch.testing.assert_close(p, p0)   # skipped
    assert m.abs().max().item() == 0.0
    flag.zero_()
    e.multi_tensor_adamw([p], [g], [m], [v], [], 1e-2, 0.9, 0.999, 1e-8,
                         0.0, 0.1, 0.001, 1.0, flag)
    assert not torch.equal(p, p0)       # applied


@pytest.mark.parametrize("M,N,K", [(4096, 2304, 768), (4096, 768, 3072),
                                   (4096, 3072, 768), (4096, 768, 768),
                                   (512, 768, 768), (100, 128, 64)])
def test_gemm_nn(M, N, K):
    """dX NN kernel: C = A @ B vs fp32 torch."""
    e = ext()
    torch.manual_seed(8)
    A = (torch.randn(M, N, device=DEV) / math.sqrt(N)).bfloat16()
    B = torch.randn(N, K, device=DEV, dtype=torch.bfloat16)
    C = e.gemm_nn(A, B)
    ref = A.float() @ B.float()
    err = (C.float() - ref).abs().max().item()
    scale = ref.abs().std().item()
    assert err < 6e-2 * max(scale, 1.0), (err, scale)


def test_gemm_nn_transpose_detection():
    """Asymmetric-B identity: catches scrambled tr-fragment addressing."""
    e = ext()
    N = 64
    A = torch.eye(128, N, device=DEV).bfloat16()
    B = torch.zeros(N, 128, device=DEV)
    for i in range(N):
        for j in range(0, 128, 7):
            B[i, j] = i * 0.01 + j
    B = B.bfloat16()
    C = e.gemm_nn(A, B)
    ref = A.float() @ B.float()
    torch.testing.assert_close(C.float(), ref, rtol=1e-3, atol=1e-3)


def test_gemm_nn_tiles_agree():
    """Every (tile, wave) template instantiation computes the same product."""
    import os
    e = ext()
    torch.manual_seed(9)
    A = (torch.randn(4096, 768, device=DEV) / 28.0).bfloat16()
    B = torch.randn(768, 3072, device=DEV, dtype=torch.bfloat16)
    base = e.gemm_nn(A, B)
    for tile in ("64x64", "64x128", "128x128"):
        for w4 in (False, True):
            os.environ["PDNLP_NN_TILE"] = tile
            if w4:
                os.environ["PDNLP_NN_W4"] = "1"
            try:
                got = e.gemm_nn(A, B)
            finally:
                os.environ.pop("PDNLP_NN_TILE", None)
                os.environ.pop("PDNLP_NN_W4", None)
            torch.testing.assert_close(got.float(), base.float(),
                                       rtol=1e-3, atol=1e-2), (tile, w4)


def test_gemm_nt_tiles_agree(monkeypatch):
    """Every (tile, waves) instantiation of the forward GEMM computes the same
    C and pre-activation as the auto-picked one. M=200 leaves a row tail,
    N=192 a column tail for the 128-wide tiles, K=192 is three K-tiles, so
    both LDS buffers are reused."""
    e = ext()
    torch.manual_seed(12)
    M, N, K = 200, 192, 192
    A = (torch.randn(M, K, device=DEV) / math.sqrt(K)).bfloat16()
    W = torch.randn(N, K, device=DEV).bfloat16()
    bias = torch.randn(N, device=DEV).bfloat16()
    monkeypatch.delenv("PDNLP_GEMM_TILE", raising=False)
    monkeypatch.delenv("PDNLP_GEMM_W4", raising=False)
    C0, pre0 = e.gemm_nt_fwd(A, W, bias, "gelu")
    pre_ref = A.float() @ W.float().t() + bias.float()
    assert (pre0.float() - pre_ref).abs().max().item() < 0.05
    assert (C0.float() - F.gelu(pre_ref)).abs().max().item() < 0.05
    # 128x64 exists at 4 waves only and takes them without PDNLP_GEMM_W4
    pairs = [("64x64", 8), ("64x64", 4), ("64x128", 8), ("64x128", 4),
             ("128x64", 4), ("128x128", 8), ("128x128", 4)]
    for tile, waves in pairs:
        monkeypatch.setenv("PDNLP_GEMM_TILE", tile)
        if waves == 4 and tile != "128x64":
            monkeypatch.setenv("PDNLP_GEMM_W4", "1")
        else:
            monkeypatch.delenv("PDNLP_GEMM_W4", raising=False)
        C, pre = e.gemm_nt_fwd(A, W, bias, "gelu")
        for name, got, want in (("C", C, C0), ("pre", pre, pre0)):
            torch.testing.assert_close(
                got.float(), want.float(), rtol=1e-3, atol=1e-2,
                msg=lambda m: f"{tile} w{waves} {name}: {m}")


def test_gemm_tile_override_rejected(monkeypatch):
    """A tile override that has no kernel is refused on the host, before
    anything is launched; without the override the same call works."""
    e = ext()
    torch.manual_seed(13)
    A = (torch.randn(128, 128, device=DEV) / math.sqrt(128)).bfloat16()
    B = torch.randn(128, 128, device=DEV, dtype=torch.bfloat16)
    D = torch.randn(128, 128, device=DEV, dtype=torch.bfloat16)
    nobias = torch.Tensor().to(DEV)
    # outputs are ~N(0,1) rounded to bf16 (2^-9 relative): the file's bf16
    # roundoff tolerance
    tol = dict(rtol=2e-2, atol=2e-2)

    monkeypatch.setenv("PDNLP_GEMM_TILE", "256x256")
    with pytest.raises(RuntimeError):
        e.gemm_nt_fwd(A, B, nobias, "none")
    monkeypatch.delenv("PDNLP_GEMM_TILE")
    C, _ = e.gemm_nt_fwd(A, B, nobias, "none")
    torch.testing.assert_close(C.float(), A.float() @ B.float().t(),
                               rtol=2e-2, atol=2e-2)

    for tile in ("256x128", "128x64"):
        monkeypatch.setenv("PDNLP_NN_TILE", tile)
        with pytest.raises(RuntimeError):
            e.gemm_nn(A, B)
    monkeypatch.setenv("PDNLP_NN_TILE", "256x128")
    with pytest.raises(RuntimeError):
        e.gemm_nn_add(A, B, D)
    monkeypatch.delenv("PDNLP_NN_TILE")
    ref = A.float() @ B.float()
    torch.testing.assert_close(e.gemm_nn(A, B).float(), ref,
                               rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(e.gemm_nn_add(A, B, D).float(),
                               ref + D.float(), rtol=2e-2, atol=2e-2)


def test_gemm_tn_w4_w8_agree():
    import os
    e = ext()
    torch.manual_seed(10)
    A = torch.randn(4096, 768, device=DEV, dtype=torch.bfloat16)
    B = torch.randn(4096, 768, device=DEV, dtype=torch.bfloat16)
    w8 = e.gemm_tn(A, B)
    os.environ["PDNLP_TN_W4"] = "1"
    try:
        w4 = e.gemm_tn(A, B)
    finally:
        os.environ.pop("PDNLP_TN_W4", None)
    torch.testing.assert_close(w8.float(), w4.float(), rtol=1e-3, atol=1e-2)


def test_linear_backward_firstparty_matches_blas(monkeypatch):
    """ops.linear backward with PDNLP_DGEMM=hip (gemm_nn/gemm_tn) must match
    the rocBLAS path — the dispatch seam for VERDICT r1 item 2."""
    from pdnlp_amd.ops import functional as Fops

    torch.manual_seed(11)
    x = (torch.randn(512, 768, device=DEV) / 28.0).bfloat16()
    w = torch.randn(768, 768, device=DEV, dtype=torch.bfloat16)
    b = torch.randn(768, device=DEV, dtype=torch.bfloat16)
    grads = {}
    for mode in ("blas", "hip"):
        monkeypatch.setenv("PDNLP_DGEMM", mode)
        xi = x.clone().requires_grad_(True)
        wi = w.clone().requires_grad_(True)
        bi = b.clone().requires_grad_(True)
        y = Fops.linear(xi, wi, bi, act="gelu")
        y.float().square().mean().backward()
        grads[mode] = (xi.grad.clone(), wi.grad.clone(), bi.grad.clone())
    for g_hip, g_blas in zip(grads["hip"], grads["blas"]):
        torch.testing.assert_close(g_hip.float(), g_blas.float(),
                                   rtol=5e-2, atol=5e-4)


def test_gemm_tn_v2_matches_v1(monkeypatch):
    """split-M 128x128 partials path vs the single-pass 64x64 kernel."""
    e = ext()
    torch.manual_seed(12)
    for (M, N, K) in [(4096, 768, 768), (4096, 2304, 768), (512, 768, 3072)]:
        A = (torch.randn(M, N, device=DEV) / math.sqrt(M)).bfloat16()
        B = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
        v2 = e.gemm_tn(A, B)          # default path
        monkeypatch.setenv("PDNLP_TN_V1", "1")
        v1 = e.gemm_tn(A, B)
        monkeypatch.delenv("PDNLP_TN_V1")
        ref = A.float().t() @ B.float()
        for got, tag in ((v2, "v2"), (v1, "v1")):
            err = (got.float() - ref).abs().max().item()
            assert err < 6e-2 * max(ref.abs().std().item(), 1.0), (tag, err)
        # split-M changes the summation order: allow a bf16 ULP
        torch.testing.assert_close(v2.float(), v1.float(),
                                   rtol=1e-2, atol=3e-2)


def test_gemm_tn_v2_split_sweep(monkeypatch):
    """Every split factor computes the same dW."""
    e = ext()
    torch.manual_seed(13)
    A = (torch.randn(4096, 768, device=DEV) / 64.0).bfloat16()
    B = torch.randn(4096, 768, device=DEV, dtype=torch.bfloat16)
    base = e.gemm_tn(A, B)
    for sm in ("1", "2", "4", "8", "16"):
        monkeypatch.setenv("PDNLP_TN_SM", sm)
        got = e.gemm_tn(A, B)
        monkeypatch.delenv("PDNLP_TN_SM")
        torch.testing.assert_close(got.float(), base.float(),
                                   rtol=1e-2, atol=3e-2), sm


def test_skinny_linear_vs_torch():
    """K9 wave-level classifier head (N=6) fwd+bwd vs fp32 torch."""
    e = ext()
    torch.manual_seed(14)
    x = (torch.randn(32, 768, device=DEV) / 28.0).bfloat16().requires_grad_(True)
    w = torch.randn(6, 768, device=DEV, dtype=torch.bfloat16).requires_grad_(True)
    b = torch.randn(6, device=DEV, dtype=torch.bfloat16).requires_grad_(True)
    from pdnlp_amd.ops.functional import _SkinnyLinearFn
    y = _SkinnyLinearFn.apply(x, w, b)
    ref = torch.nn.functional.linear(x.float().detach(), w.float().detach(),
                                     b.float().detach())
    torch.testing.assert_close(y.float(), ref, rtol=2e-2, atol=2e-2)
    y.float().square().mean().backward()
    xr = x.float().detach().requires_grad_(True)
    wr = w.float().detach().requires_grad_(True)
    br = b.float().detach().requires_grad_(True)
    torch.nn.functional.linear(xr, wr, br).square().mean().backward()
    torch.testing.assert_close(x.grad.float(), xr.grad, rtol=5e-2, atol=1e-3)
    torch.testing.assert_close(w.grad.float(), wr.grad, rtol=5e-2, atol=1e-3)
    torch.testing.assert_close(b.grad.float(), br.grad, rtol=5e-2, atol=1e-3)


def test_standalone_dropout_kernel():
    """K16: keep-rate, scaling, mask-consistent backward, device-seed
    replay contract."""
    from pdnlp_amd.ops import functional as Fops
    x = torch.ones(4096, 768, device=DEV, dtype=torch.bfloat16,
                   requires_grad=True)
    y = Fops.dropout(x, 0.1, training=True)
    keep = (y != 0).float().mean().item()
    assert abs(keep - 0.9) < 0.01, keep
    live = y[y != 0].float()
    torch.testing.assert_close(live, torch.full_like(live, 1.0 / 0.9),
                               rtol=1e-2, atol=1e-2)
    g = torch.randn_like(y)
    y.backward(g)
    mask = (y != 0)
    torch.testing.assert_close(x.grad.float()[mask], (g.float() / 0.9)[mask],
                               rtol=1e-2, atol=1e-2)
    assert torch.all(x.grad[~mask] == 0)
    # reseed changes the mask (hipGraph replay contract)
    from pdnlp_amd.ops import reseed_dropout
    y1 = Fops.dropout(x.detach(), 0.1, training=True)
    reseed_dropout(4242)
    y2 = Fops.dropout(x.detach(), 0.1, training=True)
    assert not torch.equal(y1, y2)


def test_fused_sgd_hip_matches_cpu():
    """K15 multi-tensor SGD vs the torch-loop reference."""
    from pdnlp_amd.ops.adamw import FusedSGD
    torch.manual_seed(15)
    shapes = [(768, 768), (768,), (3072, 768)]
    cpu_params = [torch.randn(*s).float() for s in shapes]
    gpu_params = [p.clone().bfloat16().to(DEV).requires_grad_(False)
                  for p in cpu_params]
    cpu_params = [p.clone().requires_grad_(False) for p in cpu_params]
    grads = [torch.randn(*s) * 0.1 for s in shapes]
    for p, g in zip(cpu_params, grads):
        p.grad = g.clone()
    for p, g in zip(gpu_params, grads):
        p.grad = g.bfloat16().to(DEV)
    opt_c = FusedSGD(cpu_params, lr=1e-2, momentum=0.9, weight_decay=0.01)
    opt_g = FusedSGD(gpu_params, lr=1e-2, momentum=0.9, weight_decay=0.01)
    for _ in range(3):
        opt_c.step()
        opt_g.step()
    for pc, pg in zip(cpu_params, gpu_params):
        torch.testing.assert_close(pg.float().cpu(), pc, rtol=2e-2, atol=2e-2)


def test_gemm_shape_fuzz():
    """Randomized shapes through all three GEMM kernels vs fp32 torch —
    guards the tile-pick rules against out-of-bounds staging regressions
    (a 64x128 NN tile once read past the K extent at K=64)."""
    import random
    rng = random.Random(99)
    e = ext()
    for _ in range(12):
        M = rng.choice([16, 64, 100, 256, 1024, 4096])
        N = rng.choice([64, 128, 192, 768, 2304])
        K = rng.choice([64, 128, 192, 768, 3072])
        A = (torch.randn(M, K, device=DEV) / math.sqrt(K)).bfloat16()
        W = torch.randn(N, K, device=DEV, dtype=torch.bfloat16)
        C, _ = e.gemm_nt_fwd(A, W, torch.Tensor().to(DEV), "none")
        ref = A.float() @ W.float().t()
        assert (C.float() - ref).abs().max().item() < 6e-2 * max(
            ref.abs().std().item(), 1.0), ("nt", M, N, K)
        # NN: [M,N] @ [N,K2]
        B2 = torch.randn(K, N, device=DEV, dtype=torch.bfloat16)
        Cn = e.gemm_nn(A, B2)
        refn = A.float() @ B2.float()
        assert (Cn.float() - refn).abs().max().item() < 6e-2 * max(
            refn.abs().std().item(), 1.0), ("nn", M, K, N)
        # TN needs M % 64
        if M % 64 == 0:
            Ct = e.gemm_tn(A, A)
            reft = A.float().t() @ A.float()
            assert (Ct.float() - reft).abs().max().item() < 6e-2 * max(
                reft.abs().std().item(), 1.0), ("tn", M, K)


def test_gemm_nn_add_fused():
    """C = A@B + D epilogue vs separate matmul+add."""
    e = ext()
    torch.manual_seed(17)
    A = (torch.randn(512, 768, device=DEV) / 28.0).bfloat16()
    B = torch.randn(768, 768, device=DEV, dtype=torch.bfloat16)
    D = torch.randn(512, 768, device=DEV, dtype=torch.bfloat16)
    C = e.gemm_nn_add(A, B, D)
    ref = A.float() @ B.float() + D.float()
    assert (C.float() - ref).abs().max().item() < 6e-2 * max(
        ref.abs().std().item(), 1.0)


def test_linear_fork_matches_unforked(monkeypatch):
    """linear_fork + fused residual-grad add == plain linear + autograd
    fan-in: full fwd/bwd parity on the layer-input fork pattern."""
    from pdnlp_amd.ops import functional as Fops

    torch.manual_seed(18)
    x0 = (torch.randn(512, 768, device=DEV) / 28.0).bfloat16()
    w = torch.randn(768, 768, device=DEV, dtype=torch.bfloat16)
    b = torch.randn(768, device=DEV, dtype=torch.bfloat16)
    g1 = torch.randn(512, 768, device=DEV, dtype=torch.bfloat16)
    g2 = torch.randn(512, 768, device=DEV, dtype=torch.bfloat16)

    xa = x0.clone().requires_grad_(True)
    wa = w.clone().requires_grad_(True)
    y, xr = Fops.linear_fork(xa, wa, b)
    torch.autograd.backward([y, xr], [g1, g2])

    xb = x0.clone().requires_grad_(True)
    wb = w.clone().requires_grad_(True)
    y2 = Fops.linear(xb, wb, b)
    torch.autograd.backward([y2, xb], [g1, g2])

    torch.testing.assert_close(y.float(), y2.float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(xa.grad.float(), xb.grad.float(),
                               rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(wa.grad.float(), wb.grad.float(),
                               rtol=3e-2, atol=3e-1)
