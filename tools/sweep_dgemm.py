#!/usr/bin/env python
"""Tile/wave sweep for the first-party dGEMM kernels on the BERT backward
shapes. Writes the winning config per shape to stdout — feeds the
pick_tile_nn / SM tables.

    python tools/sweep_dgemm.py
"""
import os
import sys
import time

import torch

sys.path.insert(0, ".")
from pdnlp_amd.ops import ext  # noqa: E402

NN_SHAPES = [(4096, 2304, 768), (4096, 768, 768), (4096, 3072, 768),
             (4096, 768, 3072), (8192, 3072, 1024), (8192, 1024, 4096)]
TN_SHAPES = [(4096, 2304, 768), (4096, 768, 768), (4096, 3072, 768),
             (4096, 768, 3072), (8192, 3072, 1024), (8192, 1024, 4096)]


def timeit(fn, iters=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    e = ext()
    dev = "cuda:0"
    torch.manual_seed(0)
    print("== NN (dX) tile sweep ==")
    for (M, N, K) in NN_SHAPES:
        A = (torch.randn(M, N, device=dev) / N ** 0.5).bfloat16()
        B = torch.randn(N, K, device=dev, dtype=torch.bfloat16)
        fl = 2.0 * M * N * K
        row = []
        for tile in ("64x64", "64x128", "128x128"):
            for w4 in (False, True):
                os.environ["PDNLP_NN_TILE"] = tile
                if w4:
                    os.environ["PDNLP_NN_W4"] = "1"
                t = timeit(lambda: e.gemm_nn(A, B))
                os.environ.pop("PDNLP_NN_TILE", None)
                os.environ.pop("PDNLP_NN_W4", None)
                row.append((fl / t / 1e12, f"{tile}w{'4' if w4 else '8'}"))
        blas = fl / timeit(lambda: A @ B) / 1e12
        ok = torch.allclose(e.gemm_nn(A, B).float(), (A.float() @ B.float()),
                            rtol=6e-2, atol=6e-1)
        row.sort(reverse=True)
        tops = " ".join(f"{n}:{v:.0f}" for v, n in row[:3])
        print(f"NN {M}x{N}x{K}: best {tops} (ok={ok}) | blas {blas:.0f}")
    print("== TN (dW) split sweep ==")
    for (M, N, K) in TN_SHAPES:
        A = (torch.randn(M, N, device=dev) / M ** 0.5).bfloat16()
        B = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        fl = 2.0 * M * N * K
        row = []
        for sm in (1, 2, 4, 8, 16):
            if M % (64 * sm):
                continue
            os.environ["PDNLP_TN_SM"] = str(sm)
            t = timeit(lambda: e.gemm_tn(A, B))
            os.environ.pop("PDNLP_TN_SM", None)
            row.append((fl / t / 1e12, f"sm{sm}"))
        os.environ["PDNLP_TN_V1"] = "1"
        v1 = fl / timeit(lambda: e.gemm_tn(A, B)) / 1e12
        os.environ.pop("PDNLP_TN_V1", None)
        auto = fl / timeit(lambda: e.gemm_tn(A, B)) / 1e12
        # auto runs the raw-barrier schedule; PDNLP_TN_SYNC reverts it
        os.environ["PDNLP_TN_SYNC"] = "1"
        sync = fl / timeit(lambda: e.gemm_tn(A, B)) / 1e12
        ok = torch.allclose(e.gemm_tn(A, B).float(),
                            (A.float().t() @ B.float()), rtol=6e-2, atol=6e-1)
        os.environ.pop("PDNLP_TN_SYNC", None)
        blas = fl / timeit(lambda: A.t() @ B) / 1e12
        row.sort(reverse=True)
        tops = " ".join(f"{n}:{v:.0f}" for v, n in row)
        print(f"TN {M}x{N}x{K}: {tops} | auto {auto:.0f} sync {sync:.0f} "
              f"(ok={ok}) v1 {v1:.0f} blas {blas:.0f}")


if __name__ == "__main__":
    main()
