// Hand-written CDNA4 NN GEMM: C[M,K] = A[M,N] @ B[N,K] — the dX
// input-gradient GEMMs of the BERT backward (dX = dY·W).
//
// These have the SAME output geometry as the forward NT GEMMs (M=4096 rows,
// 768..3072 columns at BERT-base) where our MFMA kernel beats hipBLASLt on
// the chip-filling small-N shapes — the difference is only that the B
// operand (W, stored [N,K] row-major by torch Linear) is consumed with the
// contraction along its ROWS, i.e. transposed fragments.
//
// MI355X-native structure:
//  - A (dY) staged exactly like gemm.hip's A: [BM rows][64 contraction]
//    XOR-swizzled 128-byte-row LDS image via global_load_lds, fragments as
//    plain 16-B ds_reads.
//  - B (W) staged per 64-column group into the gfx950 tr-read image
//    (gemm_common.h) and consumed with ds_read_b64_tr_b16 hardware
//    transpose-reads (guide T10) — no per-lane b16 gathers.
//  - BK=64 contraction chunks, double-buffered, one vmcnt(0)+barrier per
//    chunk; 4- or 8-wave wave grids; fp32 accumulation; XCD-aware block
//    remap (guide T1); tile shape picked by the same grid-fill rules swept
//    for the forward GEMM (PDNLP_NN_TILE=MxN overrides for sweeps).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdlib>

#include "gemm_common.h"

namespace {

constexpr int BK = 64;   // contraction chunk

// A (dY) uses the row-major image (stage_tile/read_frag), B (W) the tr-read
// image (stage_tr/frag_tr*) of gemm_common.h.
template <typename T, typename V8, int BM, int BN, int NW, bool ADDD>
__global__ __launch_bounds__(NW * WAVE)
void gemm_nn_kernel(const T* __restrict__ A, const T* __restrict__ B,
                    T* __restrict__ C, long M, long N, long K,
                    int tiles_n, int nwg, const T* __restrict__ D) {
  constexpr int WM = NW == 8 ? 2 : ((BM >= 128 || BN < 128) ? 2 : 1);
  constexpr int WN = NW / WM;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int RM = TM / 16, RN = TN / 16;
  constexpr int NGB = BN / 64;         // 64-col B groups

  const int wg = xcd_remap(blockIdx.x, nwg);
  const long tile_m = wg / tiles_n, tile_n = wg % tiles_n;
  const long m0 = tile_m * BM, k0 = tile_n * BN;

  __shared__ __attribute__((aligned(16))) char lds_a[2][BM * 128];
  __shared__ __attribute__((aligned(16))) char lds_b[2][NGB * 8192];

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wr = (wid / WN) * TM, wc = (wid % WN) * TN;

  f32x4 acc[RM][RN] = {};

  auto stage_b = [&](long n_base, char* lds) {
#pragma unroll
    for (int g = 0; g < NGB; ++g)
      stage_tr<T, NW>(B, K, n_base, N, k0 + g * 64, lds + g * 8192);
  };

  stage_tile<T, BM, NW>(A, N, m0, M, 0, lds_a[0]);
  stage_b(0, lds_b[0]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int ntiles = (int)(N / BK);
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) {
      stage_tile<T, BM, NW>(A, N, m0, M, (long)(t + 1) * BK, lds_a[cur ^ 1]);
      stage_b((long)(t + 1) * BK, lds_b[cur ^ 1]);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a_frag[RM], b_frag[RN];
#pragma unroll
      for (int i = 0; i < RM; ++i)
        a_frag[i] = read_frag<V8>(lds_a[cur], wr + i * 16, ks);
#pragma unroll
      for (int j = 0; j + 1 < RN; j += 2) {
        const int c0 = wc + j * 16, c1 = wc + (j + 1) * 16;
        frag_tr2<V8>(
            frag_tr_base(lds_b[cur] + (c0 >> 6) * 8192, c0 & 63, ks * 32),
            frag_tr_base(lds_b[cur] + (c1 >> 6) * 8192, c1 & 63, ks * 32),
            &b_frag[j]);
      }
      if constexpr (RN & 1) {
        const int c0 = wc + (RN - 1) * 16;
        b_frag[RN - 1] = frag_tr1<V8>(
            frag_tr_base(lds_b[cur] + (c0 >> 6) * 8192, c0 & 63, ks * 32));
      }
#pragma unroll
      for (int i = 0; i < RM; ++i) {
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          acc[i][j] = mfma16<V8>(a_frag[i], b_frag[j], acc[i][j]);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }

  const int crow_off = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int i = 0; i < RM; ++i) {
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const long k = k0 + wc + j * 16 + ccol;
      if (k >= K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long m = m0 + wr + i * 16 + crow_off + r;
        if (m >= M) continue;
        float v = acc[i][j][r];
        // fused residual-grad add (C = A@B + D): replaces the autograd
        // fan-in add kernel for the layer-input fork (dX_qkv + dres)
        if (ADDD) v += to_f32<T>(D[m * K + k]);
        C[m * K + k] = from_f32<T>(v);
      }
    }
  }
}

struct TileChoice { int bm, bn; };

static TileChoice pick_tile_nn(long M, long K) {
  // BN=128 tiles stage B in two 64-column groups: the LAST tile would read
  // past the K extent unless K % 128 == 0 (B's contraction ROWS are
  // clamped, its columns are not) — a 64-wide tile is always in-bounds
  // because the host requires K % 64 == 0
  if (const char* env = std::getenv("PDNLP_NN_TILE")) {
    // the grid is sized from this tile, so only a tile that has a kernel
    // and stays in bounds may pass
    int bm = 0, bn = 0;
    const bool parsed = std::sscanf(env, "%dx%d", &bm, &bn) == 2;
    TORCH_CHECK(parsed && ((bm == 64 && (bn == 64 || bn == 128)) ||
                           (bm == 128 && bn == 128)),
                "PDNLP_NN_TILE=", env,
                ": accepted tiles are 64x64, 64x128, 128x128");
    TORCH_CHECK(bn == 64 || K % 128 == 0, "PDNLP_NN_TILE=", env,
                ": a 128-wide tile needs K % 128 == 0, K is ", K);
    return {bm, bn};
  }
  auto wgs = [&](int bm, int bn) {
    return ((M + bm - 1) / bm) * ((K + bn - 1) / bn);
  };
  if (K % 128 != 0) return {64, 64};
  // swept on MI355X (gpurun_out/sweep_dgemm.log): skinny outputs want the
  // chip-filling 64x64 grid; K>768 wants 128x128 intensity once >=384 WGs
  // (64x128 lost 30-40% on the M=8192 shapes)
  if (K <= 768) {
    if (wgs(64, 64) >= 512) return {64, 64};
    return {64, 128};
  }
  if (wgs(128, 128) >= 384) return {128, 128};
  return {64, 128};
}

template <typename T>
using NnKernel = void (*)(const T*, const T*, T*, long, long, long, int, int,
                          const T*);

// pick_tile_nn returns only the three tiles listed here. 8 waves are the
// default; PDNLP_NN_W4 selects 4 for the plain 64-row tiles and has no
// effect on 128x128 or on the fused-add kernels, which exist at 8 waves
// only.
template <typename T, typename V8>
NnKernel<T> nn_kernel(TileChoice tc, int nw, bool addd) {
  const bool w8 = nw == 8;
  if (tc.bm == 64 && tc.bn == 64)
    return addd ? gemm_nn_kernel<T, V8, 64, 64, 8, true>
           : w8 ? gemm_nn_kernel<T, V8, 64, 64, 8, false>
                : gemm_nn_kernel<T, V8, 64, 64, 4, false>;
  if (tc.bm == 64 && tc.bn == 128)
    return addd ? gemm_nn_kernel<T, V8, 64, 128, 8, true>
           : w8 ? gemm_nn_kernel<T, V8, 64, 128, 8, false>
                : gemm_nn_kernel<T, V8, 64, 128, 4, false>;
  return addd ? gemm_nn_kernel<T, V8, 128, 128, 8, true>
              : gemm_nn_kernel<T, V8, 128, 128, 8, false>;
}

// C = A @ B, plus D when `dptr` is given (the fused residual-grad add)
template <typename T, typename V8>
void launch_nn(const torch::Tensor& A, const torch::Tensor& B,
               torch::Tensor& C, hipStream_t stream,
               const T* dptr = nullptr) {
  const long M = A.size(0), N = A.size(1), K = B.size(1);
  const TileChoice tc = pick_tile_nn(M, K);
  const int tiles_m = (int)((M + tc.bm - 1) / tc.bm);
  const int tiles_n = (int)((K + tc.bn - 1) / tc.bn);
  const int nwg = tiles_m * tiles_n;
  const bool addd = dptr != nullptr;
  const bool w4 = !addd && tc.bm == 64 &&
                  std::getenv("PDNLP_NN_W4") != nullptr;
  const int nw = w4 ? 4 : 8;
  auto kernel = nn_kernel<T, V8>(tc, nw, addd);
  hipLaunchKernelGGL(kernel, dim3(nwg), dim3(nw * WAVE), 0, stream,
                     (const T*)A.data_ptr(), (const T*)B.data_ptr(),
                     (T*)C.data_ptr(), M, N, K, tiles_n, nwg, dptr);
}

}  // namespace

// C = A @ B for row-major A [M, N], B [N, K]; fp32 accumulation, C in A's
// dtype. Requires N % 64 == 0 and K % 64 == 0 (M tail handled by clamping).
torch::Tensor gemm_nn(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() && B.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(1) == B.size(0));
  const long M = A.size(0), N = A.size(1), K = B.size(1);
  TORCH_CHECK(N % 64 == 0, "gemm_nn: N (contraction) must be a multiple of 64");
  TORCH_CHECK(K % 64 == 0, "gemm_nn: K must be a multiple of 64");
  auto C = torch::empty({M, K}, A.options());
  auto stream = at::hip::getCurrentHIPStream();
  if (A.scalar_type() == torch::kBFloat16) {
    launch_nn<__hip_bfloat16, bf16x8>(A, B, C, stream);
  } else if (A.scalar_type() == torch::kHalf) {
    launch_nn<__half, f16x8>(A, B, C, stream);
  } else {
    TORCH_CHECK(false, "gemm_nn: bf16/fp16 only");
  }
  return C;
}

// C = A @ B + D (fused residual-grad add; same constraints as gemm_nn,
// D contiguous [M, K] in A's dtype)
torch::Tensor gemm_nn_add(torch::Tensor A, torch::Tensor B, torch::Tensor D) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() && B.is_contiguous()
              && D.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(1) == B.size(0));
  const long M = A.size(0), N = A.size(1), K = B.size(1);
  TORCH_CHECK(D.numel() == M * K && D.scalar_type() == A.scalar_type());
  TORCH_CHECK(N % 64 == 0 && K % 64 == 0,
              "gemm_nn_add: N and K must be multiples of 64");
  auto C = torch::empty({M, K}, A.options());
  auto stream = at::hip::getCurrentHIPStream();
  if (A.scalar_type() == torch::kBFloat16) {
    launch_nn<__hip_bfloat16, bf16x8>(A, B, C, stream,
                                      (const __hip_bfloat16*)D.data_ptr());
  } else if (A.scalar_type() == torch::kHalf) {
    launch_nn<__half, f16x8>(A, B, C, stream, (const __half*)D.data_ptr());
  } else {
    TORCH_CHECK(false, "gemm_nn_add: bf16/fp16 only");
  }
  return C;
}
