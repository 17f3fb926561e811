"""The one-pass fused epilogue kernels (``bdrl_fwd1_kernel``,
``bdrl_bwd1_kernel`` + ``bdrl_fold_kernel``) against the loop kernels they
replace, which ``PDNLP_BDRL_2PASS`` keeps.

Per-row outputs (out, xsum, mask, mean, rstd, dy, dres) must keep their bits.
The column sums (dlnw, dlnb, dbias) are the same fp32 sums in another order
and are held to a bound derived from the formats: with ``t_r`` the terms in
fp64 from the tensors the kernel reads and ``S`` their sum over rows,

    |got - S| <= spacing_T(S) + (R + 8) * 2^-24 * sum_r |t_r|

one final rounding to ``T``, plus the ``R - 1`` fp32 additions in any order
and three roundings per term. Both paths must meet it.

Rows: the backward runs eight waves per workgroup and at most one workgroup
per CU. R = 1 is a single row; 33 = 4 * 8 + 1 leaves the last workgroup one
live wave (37, one live wave of the forward's four, leaves it five); 130 is
17 workgroups, the last with two live waves; at 4133 on a 256-CU device the
partial-row cap holds, every wave walks several rows, and 37 of the 2048
waves walk three rows where the others walk two.

The forward runs four waves per workgroup and one row per wave up to eight
workgroups per CU, so its waves walk rows only past R = 32 * CUs (8192 rows on
256 CUs), more than any R above. ``test_forward_walks_rows`` therefore takes
R from the device: 32 * CUs + 37 gives 37 waves a second row (the prefetch,
the register rotation and the second row's hash, mask and statistics
indices), 64 * CUs + 37 a third. H = 512 (NV = 2) is in the list because the
fp16 dropout backward of the loop kernels rounds dy differently in its
two-iteration main loop and in its remainder: 256 and 768 end in the
remainder, 1024 runs the main loop twice, 512 once and nothing else."""

import os

import pytest
import torch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

EPS = 1e-12
SALT = 7
HS = [256, 512, 768, 1024]
RS = [1, 33, 37, 130, 4133]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
PS = [0.0, 0.1]
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
_ids = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
ROW_NAMES = ("out", "xsum", "mask", "mean", "rstd", "dy", "dres")


def ext():
    from pdnlp_amd.ops import ext as _ext
    e = _ext()
    assert e is not None, "HIP extension must be built on the GPU box"
    return e


def _two_pass(fn, *args):
    """the same call on the loop kernels"""
    os.environ["PDNLP_BDRL_2PASS"] = "1"
    try:
        return fn(*args)
    finally:
        del os.environ["PDNLP_BDRL_2PASS"]


def _inputs(R, H, dtype, seed=0, integer_dout=False):
    g = torch.Generator(device=DEV).manual_seed(1000 * R + H + seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).to(dtype)
    d = dict(y=rnd(R, H), bias=rnd(H), res=rnd(R, H), lnw=rnd(H), lnb=rnd(H),
             dout=rnd(R, H))
    if integer_dout:
        d["dout"] = torch.randint(-1, 3, (R, H), device=DEV,
                                  generator=g).to(dtype)
    return d


def _seed_buf(p, value=1234):
    if p > 0:
        return torch.tensor([value], dtype=torch.int64, device=DEV)
    return torch.Tensor()


def _run(e, d, p, seed_buf):
    """forward and both backward variants, as one dict of named tensors"""
    out, xsum, mask, mean, rstd = e.bias_dropout_residual_ln_fwd(
        d["y"], d["bias"], d["res"], d["lnw"], d["lnb"], p, EPS, seed_buf,
        SALT if p > 0 else 0)
    args = (d["dout"], xsum, mask, d["lnw"], mean, rstd, p)
    dy, dbias, dres, dlnw, dlnb = e.bias_dropout_residual_ln_bwd(*args)
    dy2, dres2, dlnw2, dlnb2 = e.bias_dropout_residual_ln_bwd_nodb(*args)
    return dict(out=out, xsum=xsum, mask=mask, mean=mean, rstd=rstd, dy=dy,
                dres=dres, dbias=dbias, dlnw=dlnw, dlnb=dlnb, dy_nodb=dy2,
                dres_nodb=dres2, dlnw_nodb=dlnw2, dlnb_nodb=dlnb2)


def _spacing(S, dtype):
    """distance between neighbours of ``dtype`` at |S| (fp64 tensor)"""
    fi = torch.finfo(dtype)
    _, ex = torch.frexp(S.abs().clamp_min(fi.tiny))  # |S| = m * 2^ex, m < 1
    return torch.ldexp(torch.ones_like(S), ex - 1 - MANT[dtype])


def _check_sums(r, d, R, dtype, tag):
    f64 = torch.float64
    xh = (r["xsum"].to(f64) - r["mean"].to(f64)[:, None]) \
        * r["rstd"].to(f64)[:, None]
    terms = {"dlnw": d["dout"].to(f64) * xh, "dlnb": d["dout"].to(f64),
             "dbias": r["dy"].to(f64)}
    for name, t in terms.items():
        S = t.sum(0)
        bound = _spacing(S, dtype) + (R + 8) * 2.0 ** -24 * t.abs().sum(0)
        for key in (name, name + "_nodb"):
            if key not in r:
                continue
            err = (r[key].to(f64) - S).abs()
            worst = (err / bound).max().item()
            assert worst <= 1.0, f"{tag} {key}: error / bound = {worst:.3f}"


def _check_case(H, R, dtype, p):
    e = ext()
    d = _inputs(R, H, dtype)
    seed = _seed_buf(p)
    assert "PDNLP_BDRL_2PASS" not in os.environ
    new = _run(e, d, p, seed)
    old = _two_pass(_run, e, d, p, seed)

    # per-row outputs keep their bits, in both backward variants
    if p > 0:
        assert new["mask"].shape == (R, H)
    for name in ROW_NAMES:
        assert torch.equal(new[name], old[name]), name
    for r in (new, old):
        assert torch.equal(r["dy"], r["dy_nodb"])
        assert torch.equal(r["dres"], r["dres_nodb"])
        assert torch.equal(r["dlnw"], r["dlnw_nodb"])
        assert torch.equal(r["dlnb"], r["dlnb_nodb"])

    # column sums inside the derived bound, on both paths
    _check_sums(new, d, R, dtype, "one-pass")
    _check_sums(old, d, R, dtype, "loop kernels")

    # no dependence on arrival order
    again = _run(e, d, p, seed)
    for name in ("dlnw", "dlnb", "dbias", "dlnw_nodb", "dlnb_nodb"):
        assert torch.equal(new[name], again[name]), name


@pytest.mark.parametrize("p", PS, ids=["p0", "p0.1"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("H", HS)
def test_onepass_against_loop_kernels(H, R, dtype, p):
    _check_case(H, R, dtype, p)


@pytest.mark.parametrize("p", PS, ids=["p0", "p0.1"])
@pytest.mark.parametrize("rows_per_cu", [32, 64], ids=["2rows", "3rows"])
@pytest.mark.parametrize("H", [256, 768])
def test_forward_walks_rows(H, rows_per_cu, p):
    """R past 32 * CUs (64 * CUs): 37 waves of the forward walk a second (a
    third) row; the backward's waves walk four to nine."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _check_case(H, rows_per_cu * cus + 37, torch.bfloat16, p)


@pytest.mark.parametrize("p", PS, ids=["p0", "p0.1"])
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("H", HS)
def test_every_row_counted_once(H, R, p):
    """Integer dout in {-1, 0, 1, 2}, fp32: the column sums of dout stay
    below 2^24, so every order is exact and a skipped or doubled row shows."""
    e = ext()
    d = _inputs(R, H, torch.float32, seed=1, integer_dout=True)
    r = _run(e, d, p, _seed_buf(p))
    want = d["dout"].to(torch.float64).sum(0).to(torch.float32)
    assert torch.equal(r["dlnb"], want)
    assert torch.equal(r["dlnb_nodb"], want)


def test_graph_replay_follows_seed():
    """forward + backward captured once, replayed under two seeds: the seed
    is read from device memory, nothing persists between replays"""
    e = ext()
    R, H, p = 130, 768, 0.1
    d = _inputs(R, H, torch.bfloat16, seed=2)
    seed = _seed_buf(p, 5)
    for _ in range(2):
        _run(e, d, p, seed)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _run(e, d, p, seed)
    masks = []
    for value in (77, 78):
        seed.fill_(value)
        graph.replay()
        want = _run(e, d, p, seed)
        for name, t in want.items():
            assert torch.equal(got[name], t), (value, name)
        masks.append(got["mask"].clone())
    assert not torch.equal(masks[0], masks[1])
