import sys, time, torch
sys.path.insert(0, ".")
from pdnlp_amd.ops import ext
e = ext()
dev = "cuda:0"
torch.manual_seed(0)
for (B, nh, S) in [(16, 16, 512), (32, 12, 128)]:
    H = nh * 64
    qkv = (torch.randn(B, S, 3*H, device=dev) / 28).bfloat16()
    mask = torch.zeros(B, 1, 1, S, device=dev, dtype=torch.bfloat16).reshape(B, S).contiguous()
    o, lse = e.flash_attn_qkv_fwd(qkv, mask, nh, 0.125, 0.0, torch.Tensor(), 0)
    do = torch.randn_like(o)
    def t_fwd():
        return e.flash_attn_qkv_fwd(qkv, mask, nh, 0.125, 0.0, torch.Tensor(), 0)
    def t_bwd():
        return e.flash_attn_qkv_bwd(do, qkv, o, lse, mask, nh, 0.125, 0.0, torch.Tensor(), 0)
    for name, fn in (("fwd", t_fwd), ("bwd", t_bwd)):
        for _ in range(5): fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(30): fn()
        torch.cuda.synchronize()
        us = (time.perf_counter()-t0)/30*1e6
        print(f"B{B} nh{nh} S{S} {name}: {us:.0f} us")
