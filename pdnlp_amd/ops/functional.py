"""Functional op API with HIP/torch dispatch.

Each public function runs the hand-written CDNA4 kernel when its input lives
on a ROCm GPU and the in-tree extension is built, and a plain differentiable
torch composition otherwise (the numerics reference the GPU kernels are
tested against). Kernel inventory mirrors SURVEY.md §2.3 K1-K16.
"""

from __future__ import annotations

import contextlib
import math
import os
import threading
from typing import Optional

import torch
import torch.nn.functional as F

from . import hip_enabled, ext
from .tile_plan import AttnTilePlan, plan_from_reference, plan_views


# --------------------------------------------------------------------------
# Forward-only (serving) kernel selection
# --------------------------------------------------------------------------

_infer_state = threading.local()


@contextlib.contextmanager
def inference_kernels(enabled: bool = True):
    """Inside this context, with autograd off, tile-packed attention and the
    fused bias+residual+LN epilogue run their forward-only instantiations
    (``flash_attn_tilepack_infer``, ``bias_dropout_residual_ln_infer``):
    same output bits, but nothing is stored that only a backward reads
    (lse, xsum, mean, rstd) and the attention output needs no fill launch.
    The flag is thread-local and never set implicitly; outside the context,
    or with autograd on, every op runs as before."""
    prev = getattr(_infer_state, "on", False)
    _infer_state.on = bool(enabled)
    try:
        yield
    finally:
        _infer_state.on = prev


def _infer_active() -> bool:
    return getattr(_infer_state, "on", False) \
        and not torch.is_grad_enabled()


# --------------------------------------------------------------------------
# LayerNorm (K1 partner; fp32 stats, bf16/fp16/fp32 in/out)
# --------------------------------------------------------------------------

class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.contiguous()
        y, mean, rstd = ext().layernorm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        dx, dw, db = ext().layernorm_bwd(dy.contiguous(), x, weight, mean, rstd)
        return dx, dw, db, None


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              eps: float = 1e-12) -> torch.Tensor:
    if hip_enabled(x):
        return _LayerNormFn.apply(x, weight, bias, eps)
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


# --------------------------------------------------------------------------
# Embedding gather + add + LayerNorm (K1): word+pos+type embed fused with LN
# --------------------------------------------------------------------------

class _EmbeddingLNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input_ids, token_type_ids, position_ids,
                word_w, pos_w, type_w, ln_w, ln_b, eps):
        y, mean, rstd = ext().embedding_ln_fwd(
            input_ids, token_type_ids, position_ids,
            word_w, pos_w, type_w, ln_w, ln_b, eps)
        ctx.save_for_backward(input_ids, token_type_ids, position_ids,
                              word_w, pos_w, type_w, ln_w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        (ids, type_ids, pos_ids, word_w, pos_w, type_w, ln_w,
         mean, rstd) = ctx.saved_tensors
        dword, dpos, dtype_, dlnw, dlnb = ext().embedding_ln_bwd(
            dy.contiguous(), ids, type_ids, pos_ids,
            word_w, pos_w, type_w, ln_w, mean, rstd)
        return (None, None, None, dword, dpos, dtype_, dlnw, dlnb, None)


def embedding_layernorm(input_ids, token_type_ids, position_ids,
                        word_w, pos_w, type_w, ln_w, ln_b,
                        eps: float = 1e-12) -> torch.Tensor:
    if hip_enabled(word_w):
        return _EmbeddingLNFn.apply(
            input_ids.contiguous(), token_type_ids.contiguous(),
            position_ids.contiguous(), word_w, pos_w, type_w, ln_w, ln_b, eps)
    emb = (F.embedding(input_ids, word_w)
           + F.embedding(position_ids, pos_w)
           + F.embedding(token_type_ids, type_w))
    return F.layer_norm(emb, (emb.shape[-1],), ln_w, ln_b, eps)


# --------------------------------------------------------------------------
# Linear (K2/K6/K7/K8 GEMMs). HIP MFMA GEMM for the hot shapes; the
# backward dGEMMs follow one policy (_dx / _dw_db below).
# --------------------------------------------------------------------------

class _DwStream:
    """Optional side stream for the dW GEMMs (PDNLP_DW_STREAM=1).

    dW = dY^T·X does not feed the backward chain (only dX does), so it can
    overlap the next layer's backward. Lifetime/order handling:
    - the side stream waits the producing stream before each dW;
    - dY/X are record_stream'd so the allocator cannot recycle them under
      the in-flight GEMM;
    - consumers (optimizer step, DDP bucket reduction) call ``join()``
      which makes the current stream wait the side stream ONCE.
    Default OFF — and measured SLOWER on the flagship shape (4109 -> 3373
    samples/s): the dGEMM grids already fill all 256 CUs, so the "overlap"
    just time-slices CUs while the per-layer stream switches and waits add
    real cost. Kept as an env-gated experiment with the measurement
    recorded (DESIGN.md negative results).
    """

    def __init__(self):
        self.stream = None

    def enabled(self) -> bool:
        return (os.environ.get("PDNLP_DW_STREAM", "0") == "1"
                and torch.cuda.is_available())

    def get(self):
        if self.stream is None:
            self.stream = torch.cuda.Stream()
        return self.stream

    def join(self):
        if self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)


dw_stream = _DwStream()


def dw_stream_join() -> None:
    """Make the current stream wait all side-stream dW GEMMs (call before
    consuming gradients when PDNLP_DW_STREAM=1)."""
    dw_stream.join()


def _dgemm_mode() -> str:
    """Backward dGEMM policy (PDNLP_DGEMM env):

    "auto" (default): first-party MFMA kernels everywhere they measured at
    or above hipBLASLt, vendor GEMM only on the shapes where the library's
    deep-pipelined assembly schedules still win (ffn-down-style dX with
    K>=3072, and M>=8192 dX — profiles/r02_dgemm_vs_hipblaslt.txt,
    r02_nn256_sweep.txt). dW is first-party on every measured shape.
    "hip": force first-party for ALL dGEMMs (pure-rocprof-hand-written).
    "blas": force torch.matmul (rocBLAS/hipBLASLt) for A/B sweeps."""
    return os.environ.get("PDNLP_DGEMM", "auto")


def _nn_blas_faster(m: int, k: int) -> bool:
    """Measured winners table for the dX NN shape (m rows, k out-cols)."""
    if k >= 3072:
        return True        # 562-795 TF hip vs 736-1081 blas
    if m >= 8192 and k >= 1024:
        return True        # 964 vs 1064 at (8192, 1024-col)
    return False


def _tn_shape_ok(dy2, x2) -> bool:
    return (dy2.dtype in (torch.bfloat16, torch.float16)
            and dy2.shape[0] % 64 == 0 and dy2.shape[1] % 64 == 0
            and x2.shape[1] % 64 == 0)


def _bias_grad(dy2):
    if dy2.shape[-1] % 4 == 0 and dy2.shape[0] >= 256 \
            and dy2.dtype != torch.float32:
        return ext().col_sum(dy2)
    return dy2.sum(0)


# The backward-GEMM policy of every HIP linear lives in _dx and _dw_db. The
# forward gate (_gemm_shape_ok) already guarantees what the NN kernel needs
# (bf16/fp16, in- and out-features multiples of 64), so _dx checks no shape.

def _dx(dy2, w, dpass=None):
    """dX = dy2 @ w (+ dpass, the gradient of a forked pass-through input):
    first-party MFMA NN unless the policy (_dgemm_mode / _nn_blas_faster)
    hands the shape to rocBLAS."""
    mode = _dgemm_mode()
    hip = (mode == "hip"
           or (mode == "auto"
               and not _nn_blas_faster(dy2.shape[0], w.shape[1])))
    if dpass is None:
        return ext().gemm_nn(dy2, w) if hip else dy2 @ w
    if not hip:
        # vendor-GEMM shapes: addmm fuses the residual-grad add too
        return torch.addmm(dpass.reshape(-1, dpass.shape[-1]), dy2, w)
    if dpass.is_contiguous():
        # the add rides in the dX GEMM's epilogue
        return ext().gemm_nn_add(dy2, w, dpass.view(-1, dpass.shape[-1]))
    return ext().gemm_nn(dy2, w) + dpass.reshape(-1, dpass.shape[-1])


def _dw_db(dy2, x2, need_db, side_stream=False):
    """(dW, db) = (dy2^T @ x2, column sums of dy2 or None). On the
    first-party grid a needed db comes out of the dW GEMM itself
    (gemm_tn_colsum); elsewhere from _bias_grad. ``side_stream`` lets
    PDNLP_DW_STREAM=1 move dW off the backward critical path."""
    db = None
    if side_stream and dw_stream.enabled():
        s = dw_stream.get()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dw = dy2.t() @ x2
        dy2.record_stream(s)
        x2.record_stream(s)
        dw.record_stream(torch.cuda.current_stream())
    elif _dgemm_mode() in ("hip", "auto") and _tn_shape_ok(dy2, x2):
        if need_db:
            dw, db = ext().gemm_tn_colsum(dy2, x2)  # dW + db in one pass
        else:
            dw = ext().gemm_tn(dy2, x2)             # first-party MFMA TN
    else:
        dw = dy2.t() @ x2                           # rocBLAS TN
    if need_db and db is None:
        db = _bias_grad(dy2)
    return dw, db


def _linear_fwd(ctx, x, w, b, act):
    x2 = x.contiguous().view(-1, x.shape[-1])
    y, pre = ext().gemm_nt_fwd(x2, w, b if b is not None else torch.Tensor(),
                               act)
    ctx.save_for_backward(x2, w, pre if act != "none" else torch.Tensor())
    ctx.act = act
    ctx.in_shape = x.shape
    return y.view(*x.shape[:-1], w.shape[0])


def _linear_bwd(ctx, dy, need_db, dpass=None, side_stream=False):
    """Activation backward, then the two dGEMMs: (dx, dw, db)."""
    x2, w, pre = ctx.saved_tensors
    dy2 = dy.contiguous().view(-1, dy.shape[-1])
    if ctx.act == "gelu":
        dy2 = ext().gelu_bwd(dy2, pre)
    elif ctx.act == "tanh":
        dy2 = ext().tanh_bwd(dy2, pre)
    dx = _dx(dy2, w, dpass)
    dw, db = _dw_db(dy2, x2, need_db, side_stream)
    return dx.view(ctx.in_shape), dw, db


class _LinearHipFn(torch.autograd.Function):
    """y = x @ w^T + b with the forward GEMM on the hand-written MFMA kernel
    (optionally fused activation); backward dGEMMs on first-party MFMA
    kernels (gemm_nn/gemm_tn) with a rocBLAS fallback for off-grid shapes
    or PDNLP_DGEMM=blas."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        ctx.has_bias = b is not None
        return _linear_fwd(ctx, x, w, b, act)

    @staticmethod
    def backward(ctx, dy):
        # the only linear whose dW may go to the PDNLP_DW_STREAM side stream
        return (*_linear_bwd(ctx, dy, ctx.has_bias, side_stream=True), None)


class _LinearDeferredBiasHipFn(torch.autograd.Function):
    """y = x @ w^T whose bias ``b`` is applied DOWNSTREAM (in the fused
    bias+dropout+residual+LN epilogue). ``b`` is an input for gradient
    purposes only: forward does not add it, backward returns its gradient
    — the column sum of dy, which is also d(loss)/d(b) because the epilogue
    adds ``b`` straight onto this output — from the dW GEMM that reads dy
    anyway (``gemm_tn_colsum``) instead of a separate pass in the epilogue's
    backward."""

    @staticmethod
    def forward(ctx, x, w, b):
        return _linear_fwd(ctx, x, w, None, "none")

    @staticmethod
    def backward(ctx, dy):
        return _linear_bwd(ctx, dy, ctx.needs_input_grad[2])


class _LinearForkHipFn(torch.autograd.Function):
    """linear() that ALSO returns its input as a second output.

    When the same activation feeds a projection AND a residual stream (the
    BERT layer input into qkv-linear + post-attention LN residual), routing
    the residual through this fork gives the input ONE consumer — the
    residual gradient then arrives here as ``dpass`` and is added inside
    the dX GEMM's epilogue (``gemm_nn_add``) instead of by a separate
    autograd fan-in add kernel (24 launches / 129 µs per step in r2
    profiles)."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        ctx.has_bias = b is not None
        return _linear_fwd(ctx, x, w, b, act), x

    @staticmethod
    def backward(ctx, dy, dpass):
        return (*_linear_bwd(ctx, dy, ctx.has_bias, dpass=dpass), None)


def linear_fork(x: torch.Tensor, w: torch.Tensor,
                b: Optional[torch.Tensor] = None, act: str = "none"):
    """Returns ``(linear(x, w, b, act), x)`` — use the second output as the
    residual stream so the fan-in add fuses into the dX GEMM (HIP); on CPU
    this is exactly ``(linear(...), x)`` with autograd doing the add."""
    if hip_enabled(x) and _gemm_shape_ok(x, w):
        return _LinearForkHipFn.apply(x, w, b, act)
    return linear(x, w, b, act), x


class _SkinnyLinearFn(torch.autograd.Function):
    """Wave-level dot-product kernel for skinny heads (N <= 16):
    the 6-way classifier wastes an MFMA fragment (16x16 vs N=6)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.contiguous().view(-1, x.shape[-1])
        y = ext().skinny_linear_fwd(x2, w,
                                    b if b is not None else torch.Tensor())
        ctx.save_for_backward(x2, w)
        ctx.has_bias = b is not None
        ctx.in_shape = x.shape
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, dy.shape[-1])
        dx, dw, db = ext().skinny_linear_bwd(dy2, x2, w, ctx.has_bias)
        return (dx.view(ctx.in_shape), dw,
                db if ctx.has_bias else None)


def linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None,
           act: str = "none") -> torch.Tensor:
    """act in {"none", "gelu", "tanh"} — fused into the GEMM epilogue on HIP.

    PDNLP_FWD=blas routes plain (no-activation) projections through
    F.linear/hipBLASLt for A/B sweeps; activations always stay on the
    fused first-party kernel (unfusing them costs a full HBM round trip)."""
    if os.environ.get("PDNLP_FWD") == "blas" and act == "none":
        return F.linear(x, w, b)
    if hip_enabled(x) and _gemm_shape_ok(x, w):
        return _LinearHipFn.apply(x, w, b, act)
    if hip_enabled(x) and act == "none" \
            and w.shape[0] in (1, 2, 4, 6, 8, 16) \
            and x.dtype in (torch.bfloat16, torch.float16):
        return _SkinnyLinearFn.apply(x, w, b)
    y = F.linear(x, w, b)
    if act == "gelu":
        y = F.gelu(y)
    elif act == "tanh":
        y = torch.tanh(y)
    return y


def _gemm_shape_ok(x, w) -> bool:
    if x.dtype not in (torch.bfloat16, torch.float16):
        return False
    m = x.numel() // x.shape[-1]
    n, k = w.shape
    return (k % 64 == 0) and (n % 64 == 0) and (m % 16 == 0)


# --------------------------------------------------------------------------
# Bias + GELU (K7 epilogue when unfused)
# --------------------------------------------------------------------------

class _BiasGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, b):
        y = ext().bias_gelu_fwd(x.contiguous(), b)
        ctx.save_for_backward(x, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, b = ctx.saved_tensors
        dx, db = ext().bias_gelu_bwd(dy.contiguous(), x, b)
        return dx, db


def bias_gelu(x: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if hip_enabled(x):
        return _BiasGeluFn.apply(x, b)
    return F.gelu(x + b)


# --------------------------------------------------------------------------
# Masked softmax (K4): y = softmax(scores * scale + additive_mask)
# --------------------------------------------------------------------------

class _MaskedSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, mask, scale):
        probs = ext().masked_softmax_fwd(scores.contiguous(),
                                         mask.contiguous() if mask is not None
                                         else torch.Tensor(), scale)
        ctx.save_for_backward(probs)
        return probs

    @staticmethod
    def backward(ctx, dy):
        (probs,) = ctx.saved_tensors
        return ext().masked_softmax_bwd(dy.contiguous(), probs), None, None


def masked_softmax(scores: torch.Tensor, mask: Optional[torch.Tensor],
                   scale: float = 1.0) -> torch.Tensor:
    """scores: [B, H, S, S]; mask: additive [B, 1, 1, S] (0 keep / -inf drop)."""
    if hip_enabled(scores):
        return _MaskedSoftmaxFn.apply(scores, mask, scale)
    s = scores * scale
    if mask is not None:
        s = s + mask
    return F.softmax(s, dim=-1)


# --------------------------------------------------------------------------
# Attention (K3-K5). Default: batched GEMMs + fused masked softmax.
# Flash path (fused MFMA online-softmax kernel) used when available.
# --------------------------------------------------------------------------

def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              mask: Optional[torch.Tensor], dropout_p: float = 0.0,
              training: bool = False) -> torch.Tensor:
    """q,k,v: [B, H, S, D]; mask: additive [B, 1, 1, S]. Returns [B, H, S, D].

    Unfused composition (batched GEMMs + fused masked softmax) — the fallback
    behind :func:`attention_packed` and the CPU numerics reference.
    """
    scale = 1.0 / math.sqrt(q.shape[-1])
    scores = torch.matmul(q, k.transpose(-1, -2))
    probs = masked_softmax(scores, mask, scale)
    if dropout_p > 0.0 and training:
        probs = F.dropout(probs, p=dropout_p, training=True)
    return torch.matmul(probs, v)


class _FlashAttnQKVFn(torch.autograd.Function):
    """Fused flash attention over the packed QKV projection [B, S, 3H] —
    K3+K4+K5 (+ attention dropout K16) in one MFMA kernel; returns the
    [B, S, H] context ready for the output projection. Dropout masks are
    recomputed in backward from the device seed + salt (valid as long as
    ``reseed_dropout`` is only called between steps, which is the step
    contract everywhere in this framework)."""

    @staticmethod
    def forward(ctx, qkv, mask, nh, scale, p_drop):
        if p_drop > 0.0:
            seed_buf, salt = _dropout_seed.get(qkv.device)
        else:
            seed_buf, salt = torch.Tensor(), 0
        mask_t = mask if mask is not None else torch.Tensor()
        o, lse = ext().flash_attn_qkv_fwd(qkv, mask_t, nh, scale, p_drop,
                                          seed_buf, salt)
        ctx.save_for_backward(qkv, o, lse,
                              mask if mask is not None else torch.Tensor(),
                              seed_buf if p_drop > 0.0 else torch.Tensor())
        ctx.nh, ctx.scale, ctx.p, ctx.salt = nh, scale, p_drop, salt
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, mask, seed_buf = ctx.saved_tensors
        dqkv = ext().flash_attn_qkv_bwd(do.contiguous(), qkv, o, lse, mask,
                                        ctx.nh, ctx.scale, ctx.p, seed_buf,
                                        ctx.salt)
        return dqkv, None, None, None, None


def attention_packed(qkv: torch.Tensor, mask: Optional[torch.Tensor],
                     num_heads: int, dropout_p: float = 0.0,
                     training: bool = False) -> torch.Tensor:
    """Attention on the packed QKV projection output.

    qkv: [B, S, 3H] (q | k | v along the last dim, H = num_heads*64);
    mask: additive [B, 1, 1, S] in qkv's dtype. Returns context [B, S, H].
    On a ROCm GPU with head_dim 64, S%64==0 and bf16/fp16 this runs the
    fused MFMA flash kernel; otherwise it falls back to the split
    batched-GEMM composition."""
    B, S, H3 = qkv.shape
    H = H3 // 3
    hd = H // num_heads
    p_eff = float(dropout_p if training else 0.0)
    if hip_enabled(qkv) and hd == 64 and S % 64 == 0 \
            and qkv.dtype in (torch.bfloat16, torch.float16):
        scale = 1.0 / math.sqrt(hd)
        return _FlashAttnQKVFn.apply(
            qkv.contiguous(),
            mask.contiguous() if mask is not None else None,
            num_heads, scale, p_eff)
    q, k, v = qkv.split(H, dim=-1)
    q = q.view(B, S, num_heads, hd).transpose(1, 2)
    k = k.view(B, S, num_heads, hd).transpose(1, 2)
    v = v.view(B, S, num_heads, hd).transpose(1, 2)
    ctx = attention(q, k, v, mask, p_eff, training)
    return ctx.transpose(1, 2).reshape(B, S, H)


class _FlashAttnVarlenFn(torch.autograd.Function):
    """Flash attention over a packed token stream [T, 3H] whose sequence
    boundaries are ``cu_seqlens`` — the padding-free counterpart of
    _FlashAttnQKVFn (same kernels, VARLEN instantiations). Rows outside
    every sequence come back exactly zero in the output and in dqkv."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, nh, scale, p_drop):
        if p_drop > 0.0:
            seed_buf, salt = _dropout_seed.get(qkv.device)
        else:
            seed_buf, salt = torch.Tensor(), 0
        o, lse = ext().flash_attn_varlen_fwd(qkv, cu_seqlens, max_seqlen, nh,
                                             scale, p_drop, seed_buf, salt)
        ctx.save_for_backward(qkv, o, lse, cu_seqlens,
                              seed_buf if p_drop > 0.0 else torch.Tensor())
        ctx.max_seqlen = max_seqlen
        ctx.nh, ctx.scale, ctx.p, ctx.salt = nh, scale, p_drop, salt
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, cu_seqlens, seed_buf = ctx.saved_tensors
        dqkv = ext().flash_attn_varlen_bwd(
            do.contiguous(), qkv, o, lse, cu_seqlens, ctx.max_seqlen, ctx.nh,
            ctx.scale, ctx.p, seed_buf, ctx.salt)
        return dqkv, None, None, None, None, None


class _FlashAttnTilePackFn(torch.autograd.Function):
    """_FlashAttnVarlenFn over a tile plan (``varlen_attention_plan``): the
    tile-packed kernel instantiations, in which one 64-row tile holds
    several whole consecutive short sequences. Same layouts, same dropout
    masks and the same zero rows as the per-sequence kernels."""

    @staticmethod
    def forward(ctx, qkv, plan_buf, max_seqlen, nh, scale, p_drop):
        if p_drop > 0.0:
            seed_buf, salt = _dropout_seed.get(qkv.device)
        else:
            seed_buf, salt = torch.Tensor(), 0
        o, lse = ext().flash_attn_tilepack_fwd(qkv, plan_buf, max_seqlen, nh,
                                               scale, p_drop, seed_buf, salt)
        ctx.save_for_backward(qkv, o, lse, plan_buf,
                              seed_buf if p_drop > 0.0 else torch.Tensor())
        ctx.max_seqlen = max_seqlen
        ctx.nh, ctx.scale, ctx.p, ctx.salt = nh, scale, p_drop, salt
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, plan_buf, seed_buf = ctx.saved_tensors
        dqkv = ext().flash_attn_tilepack_bwd(
            do.contiguous(), qkv, o, lse, plan_buf, ctx.max_seqlen, ctx.nh,
            ctx.scale, ctx.p, seed_buf, ctx.salt)
        return dqkv, None, None, None, None, None


def varlen_attention_plan(cu_seqlens: torch.Tensor,
                          total_rows: int) -> AttnTilePlan:
    """Tile plan of tile-packed attention for a packed batch of
    ``total_rows`` rows (see ops/tile_plan.py). A pure function of the
    contents of ``cu_seqlens``; on the HIP path one small launch with no
    host sync, so a captured graph stays valid for any boundaries. Build it
    once per model forward and hand it to every ``attention_varlen``."""
    total_rows = int(total_rows)
    if hip_enabled(cu_seqlens) and total_rows % 64 == 0:
        return plan_views(
            ext().flash_attn_tilepack_plan(cu_seqlens.contiguous(),
                                           total_rows), total_rows)
    return plan_from_reference(cu_seqlens, total_rows)


def attention_varlen(qkv: torch.Tensor, cu_seqlens: torch.Tensor,
                     max_seqlen: int, num_heads: int, dropout_p: float = 0.0,
                     training: bool = False,
                     plan: Optional[AttnTilePlan] = None) -> torch.Tensor:
    """Attention on a packed (padding-free) QKV projection output.

    qkv: [T, 3H]; sequence b occupies rows cu_seqlens[b]..cu_seqlens[b+1]
    (int32 [B+1]); T >= cu_seqlens[B]. ``max_seqlen`` is the longest
    sequence as a host int. Returns the context [T, H]; rows outside every
    sequence are exactly zero, forward and backward. On a ROCm GPU with
    head_dim 64, T%64==0 and bf16/fp16 this runs the fused MFMA flash
    kernel; otherwise a per-sequence loop over :func:`attention` (which
    reads cu_seqlens on the host). With a ``plan`` of
    :func:`varlen_attention_plan` the fused path runs the tile-packed
    kernels; the per-sequence loop ignores it."""
    T, H3 = qkv.shape
    H = H3 // 3
    hd = H // num_heads
    p_eff = float(dropout_p if training else 0.0)
    if hip_enabled(qkv) and hd == 64 and T % 64 == 0 \
            and qkv.dtype in (torch.bfloat16, torch.float16):
        if plan is not None:
            if p_eff == 0.0 and _infer_active():
                return ext().flash_attn_tilepack_infer(
                    qkv.contiguous(), plan.buf, int(max_seqlen), num_heads,
                    1.0 / math.sqrt(hd))
            return _FlashAttnTilePackFn.apply(
                qkv.contiguous(), plan.buf, int(max_seqlen), num_heads,
                1.0 / math.sqrt(hd), p_eff)
        return _FlashAttnVarlenFn.apply(
            qkv.contiguous(), cu_seqlens.contiguous(), int(max_seqlen),
            num_heads, 1.0 / math.sqrt(hd), p_eff)
    bounds = cu_seqlens.tolist()
    outs = []
    for s0, s1 in zip(bounds[:-1], bounds[1:]):
        q, k, v = (t.view(1, s1 - s0, num_heads, hd).transpose(1, 2)
                   for t in qkv[s0:s1].split(H, dim=-1))
        c = attention(q, k, v, None, p_eff, training)
        outs.append(c.transpose(1, 2).reshape(s1 - s0, H))
    outs.append(qkv.new_zeros(T - bounds[-1], H))
    return torch.cat(outs, dim=0)


class _ClsAttnFn(torch.autograd.Function):
    """Attention of every sequence's first token over its own sequence, on
    the packed QKV projection [T, 3H] (cls_attention.hip): one output row
    per sequence, [rows_out, H]. Built like _FlashAttnVarlenFn: dropout
    masks are recomputed in backward from the device seed + salt, and the
    masks are those ``flash_attn_varlen_fwd`` gives these rows. dqkv comes
    back in the packed layout: k and v columns of every sequence row, q
    columns of the first rows, everything else exactly zero."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, rows_out, max_seqlen, nh, scale,
                p_drop):
        if p_drop > 0.0:
            seed_buf, salt = _dropout_seed.get(qkv.device)
        else:
            seed_buf, salt = torch.Tensor(), 0
        o, lse = ext().cls_attn_fwd(qkv, cu_seqlens, rows_out, max_seqlen,
                                    nh, scale, p_drop, seed_buf, salt)
        ctx.save_for_backward(qkv, o, lse, cu_seqlens,
                              seed_buf if p_drop > 0.0 else torch.Tensor())
        ctx.max_seqlen = max_seqlen
        ctx.nh, ctx.scale, ctx.p, ctx.salt = nh, scale, p_drop, salt
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, cu_seqlens, seed_buf = ctx.saved_tensors
        dqkv = ext().cls_attn_bwd(
            do.contiguous(), qkv, o, lse, cu_seqlens, ctx.max_seqlen, ctx.nh,
            ctx.scale, ctx.p, seed_buf, ctx.salt)
        return dqkv, None, None, None, None, None, None


def cls_attention(qkv: torch.Tensor, cu_seqlens: torch.Tensor, rows_out: int,
                  max_seqlen: int, num_heads: int, dropout_p: float = 0.0,
                  training: bool = False) -> torch.Tensor:
    """First-token attention on a packed QKV projection output.

    qkv: [T, 3H] and cu_seqlens int32 [B+1] as in :func:`attention_varlen`.
    Returns [rows_out, H] with ``rows_out >= B``: row i < B is the attention
    output of sequence i's first token over the keys of its own sequence;
    rows of empty sequences and rows >= B are exactly zero. This is
    ``attention_varlen(...)[cu_seqlens[:-1]]`` without the other T - B query
    rows. Runs the one-wave-per-(sequence, head) HIP kernel wherever
    :func:`attention_varlen` runs its fused kernel, and a torch composition
    (which reads cu_seqlens on the host) otherwise."""
    T, H3 = qkv.shape
    H = H3 // 3
    hd = H // num_heads
    rows_out = int(rows_out)
    p_eff = float(dropout_p if training else 0.0)
    if hip_enabled(qkv) and hd == 64 and T % 64 == 0 \
            and qkv.dtype in (torch.bfloat16, torch.float16):
        scale = 1.0 / math.sqrt(hd)
        if p_eff == 0.0 and _infer_active():
            return ext().cls_attn_infer(
                qkv.contiguous(), cu_seqlens.contiguous(), rows_out,
                int(max_seqlen), num_heads, scale)
        return _ClsAttnFn.apply(
            qkv.contiguous(), cu_seqlens.contiguous(), rows_out,
            int(max_seqlen), num_heads, scale, p_eff)
    bounds = cu_seqlens.tolist()
    if rows_out < len(bounds) - 1:
        raise ValueError("cls_attention: rows_out must be at least the "
                         "number of sequences")
    outs = []
    for s0, s1 in zip(bounds[:-1], bounds[1:]):
        if s1 <= s0:
            outs.append(qkv.new_zeros(1, H))
            continue
        q, k, v = (t.view(1, -1, num_heads, hd).transpose(1, 2)
                   for t in qkv[s0:s1].split(H, dim=-1))
        c = attention(q[:, :, :1], k, v, None, p_eff, training)
        outs.append(c.transpose(1, 2).reshape(1, H))
    outs.append(qkv.new_zeros(rows_out - (len(bounds) - 1), H))
    return torch.cat(outs, dim=0)


# --------------------------------------------------------------------------
# Bias + dropout + residual + LayerNorm (K6/K8 epilogue)
# --------------------------------------------------------------------------

class _DropoutSeedState:
    """Device-resident dropout seed (hipGraph-safe: the kernel reads the
    seed from device memory, so ``reseed()`` between graph replays changes
    the masks while the captured kernel args stay fixed). The per-call-site
    salt keeps masks distinct within a step."""

    def __init__(self):
        self.buf = None
        self.salt = 0

    def get(self, device):
        if self.buf is None or self.buf.device != device:
            self.buf = torch.randint(0, 2**62, (1,), dtype=torch.int64,
                                     device=device)
        self.salt += 1
        return self.buf, self.salt

    def reseed(self, seed=None):
        if self.buf is not None:
            if seed is None:
                seed = int(torch.randint(0, 2**62, (1,)).item())
            self.buf.fill_(seed)


_dropout_seed = _DropoutSeedState()


def reseed_dropout(seed=None) -> None:
    """Refresh the device dropout seed — call once per step when replaying
    hipGraph-captured training steps."""
    _dropout_seed.reseed(seed)


class _BiasDropResLNFn(torch.autograd.Function):
    """``need_dbias=False``: the bias has no gradient path here — the
    backward skips the bias column sum (one of the three input streams of
    its second pass) and the producing projection returns that gradient
    instead (_LinearDeferredBiasHipFn)."""

    @staticmethod
    def forward(ctx, y, bias, residual, ln_w, ln_b, p, training, eps,
                need_dbias):
        p_eff = float(p if training else 0.0)
        if p_eff > 0.0:
            seed_buf, salt = _dropout_seed.get(y.device)
        else:
            seed_buf, salt = torch.Tensor(), 0
        out, xsum, mask, mean, rstd = ext().bias_dropout_residual_ln_fwd(
            y.contiguous(), bias, residual.contiguous(), ln_w, ln_b,
            p_eff, eps, seed_buf, salt)
        ctx.save_for_backward(xsum, mask, ln_w, mean, rstd)
        ctx.p = p_eff
        ctx.need_dbias = need_dbias
        return out

    @staticmethod
    def backward(ctx, dout):
        args = (dout.contiguous(), *ctx.saved_tensors, ctx.p)
        if ctx.need_dbias:
            dy, dbias, dres, dlnw, dlnb = \
                ext().bias_dropout_residual_ln_bwd(*args)
        else:
            dbias = None
            dy, dres, dlnw, dlnb = \
                ext().bias_dropout_residual_ln_bwd_nodb(*args)
        return dy, dbias, dres, dlnw, dlnb, None, None, None, None


def bias_dropout_residual_layernorm(
        y: torch.Tensor, bias: torch.Tensor, residual: torch.Tensor,
        ln_w: torch.Tensor, ln_b: torch.Tensor, p: float = 0.1,
        training: bool = False, eps: float = 1e-12) -> torch.Tensor:
    """out = LN(dropout(y + bias) + residual) — the fused epilogue after the
    attention-output and FFN-down projections."""
    if hip_enabled(y) and y.shape[-1] % 256 == 0 and y.shape[-1] <= 1024:
        if not (p > 0.0 and training) and _infer_active():
            return ext().bias_dropout_residual_ln_infer(
                y.contiguous(), bias, residual.contiguous(), ln_w, ln_b, eps)
        return _BiasDropResLNFn.apply(y, bias, residual, ln_w, ln_b, p,
                                      training, eps, True)
    h = y + bias
    if p > 0.0 and training:
        h = F.dropout(h, p=p, training=True)
    h = h + residual
    return F.layer_norm(h, (h.shape[-1],), ln_w, ln_b, eps)


def linear_bias_dropout_residual_layernorm(
        x: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
        residual: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor,
        p: float = 0.1, training: bool = False,
        eps: float = 1e-12) -> torch.Tensor:
    """out = LN(dropout(x @ w^T + b) + residual): a projection whose bias is
    applied in the fused epilogue (attention-output and FFN-down).

    On HIP, with the first-party dW GEMM in use, the bias gradient is taken
    inside that GEMM (``gemm_tn_colsum``) and the epilogue's backward no
    longer sums dy for it. Everywhere else this is exactly
    ``bias_dropout_residual_layernorm(linear(x, w, None), b, ...)``."""
    H = w.shape[0]
    rows = x.numel() // x.shape[-1]
    if hip_enabled(x) and H % 256 == 0 and H <= 1024 \
            and os.environ.get("PDNLP_FWD") != "blas" \
            and _dgemm_mode() in ("hip", "auto") \
            and not dw_stream.enabled() \
            and _gemm_shape_ok(x, w) and rows % 64 == 0:
        proj = _LinearDeferredBiasHipFn.apply(x, w, b)
        if not (p > 0.0 and training) and _infer_active():
            return ext().bias_dropout_residual_ln_infer(
                proj.contiguous(), b, residual.contiguous(), ln_w, ln_b, eps)
        return _BiasDropResLNFn.apply(
            proj, b.detach(), residual, ln_w, ln_b, p, training, eps, False)
    return bias_dropout_residual_layernorm(
        linear(x, w, None), b, residual, ln_w, ln_b, p, training, eps)


# --------------------------------------------------------------------------
# Dropout (K16) — standalone counter-hash kernel on HIP (device seed +
# per-call salt, hipGraph-replay safe like the fused variants); torch RNG
# on CPU.
# --------------------------------------------------------------------------

class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        seed_buf, salt = _dropout_seed.get(x.device)
        y, mask = ext().dropout_fwd(x.contiguous(), p, seed_buf, salt)
        ctx.save_for_backward(mask)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return ext().dropout_bwd(dy.contiguous(), mask, ctx.p), None


def dropout(x: torch.Tensor, p: float, training: bool) -> torch.Tensor:
    if p > 0.0 and training and hip_enabled(x):
        return _DropoutFn.apply(x, float(p))
    return F.dropout(x, p=p, training=training)


# --------------------------------------------------------------------------
# CrossEntropy (K10): fused log-softmax + NLL on [B, num_labels]
# --------------------------------------------------------------------------

class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        loss, logprobs = ext().cross_entropy_fwd(logits.contiguous(),
                                                 labels.contiguous())
        ctx.save_for_backward(logprobs, labels)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logprobs, labels = ctx.saved_tensors
        return ext().cross_entropy_bwd(dloss, logprobs, labels), None


class _CrossEntropyIgnoreFn(torch.autograd.Function):
    """Mean over the rows whose label is not ``ignore_index``. The count of
    those rows stays on the device (``nvalid``): no host sync, so the op can
    be captured in a graph and replayed for any mix of valid/ignored rows."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        labels = labels.contiguous()
        loss, logprobs, nvalid = ext().cross_entropy_ignore_fwd(
            logits.contiguous(), labels, ignore_index)
        ctx.save_for_backward(logprobs, labels, nvalid)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logprobs, labels, nvalid = ctx.saved_tensors
        return ext().cross_entropy_ignore_bwd(
            dloss, logprobs, labels, nvalid, ctx.ignore_index), None, None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor,
                  ignore_index: Optional[int] = None) -> torch.Tensor:
    """``ignore_index=None``: mean over all rows. Otherwise the semantics of
    ``F.cross_entropy(..., ignore_index=...)``: mean over the rows whose
    label differs from it (at least one such row is a precondition), zero
    gradient for the others."""
    if ignore_index is None:
        if hip_enabled(logits):
            return _CrossEntropyFn.apply(logits.float(), labels)
        return F.cross_entropy(logits.float(), labels)
    if hip_enabled(logits):
        return _CrossEntropyIgnoreFn.apply(logits.float(), labels,
                                           int(ignore_index))
    return F.cross_entropy(logits.float(), labels,
                           ignore_index=int(ignore_index))
