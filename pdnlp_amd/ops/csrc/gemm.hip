// Hand-written CDNA4 MFMA GEMM: C[M,N] = A[M,K] @ W[N,K]^T (+bias) (+act)
// — the forward GEMMs of the BERT hot path with
// the bias/GELU/tanh epilogue fused into the C-write.
//
// Structure (the "step-3" ladder structure of the CDNA4 guide, §5):
//  - templated BM x BN output tile, BK=64, 8 waves (512 threads) by default
//    and 4 waves (256 threads) for 128x64 or under PDNLP_GEMM_W4; wave grid
//    WMxWN, each wave an (BM/WM)x(BN/WN) sub-tile of
//    v_mfma_f32_16x16x32_bf16 fragments (f16 variant for fp16), fp32
//    accumulation in AGPRs.
//  - global->LDS staging via __builtin_amdgcn_global_load_lds width 16
//    (2 LDS buffers, stage tile t+1 while computing tile t, one
//    vmcnt(0)+barrier per tile).
//  - LDS bank-conflict fix: XOR swizzle byte ^= ((row&7)<<4) applied on the
//    *global source address* (glds writes lane-linear; guide §5.4 rule 21)
//    and on the ds_read fragment address — ≤2-way instead of 8-way.
//  - XCD-aware block swizzle (T1): contiguous tile chunks per XCD for L2
//    affinity (bijective variant).
//  - Tile shape picked per GEMM shape at launch: 128x128 when the grid
//    fills the 256 CUs, 64x128 / 128x64 for skinny-N/M shapes where the
//    128x128 grid would underfill the chip (e.g. the attention-output and
//    FFN-down projections at N=768: 192 WGs -> 384 WGs).
//    Override for sweeps: env PDNLP_GEMM_TILE=MxN (e.g. 64x128), one of
//    the instantiated tiles listed at pick_tile.
//
// A-fragment: lane l holds A[l&15][(l>>4)*8 + i], i=0..7 -> one ds_read_b128.
// B-fragment: lane l holds W[n0 + (l&15)][k0 + (l>>4)*8 + i] — the same
// pattern because W is stored [N,K] row-major (torch Linear layout) and
// C = A @ W^T. C/D: col = lane&15, row = (lane>>4)*4 + reg.
//
// The backward dGEMMs (dX = dY@W, dW = dY^T@X) are the first-party kernels
// of gemm_nn.hip and gemm_tn.hip; functional.py picks per shape between
// them and the vendor GEMM (PDNLP_DGEMM).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdlib>

#include "gemm_common.h"

namespace {

constexpr int BK = 64;

__device__ __forceinline__ float gelu_f2(float x) {
  return 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
}

enum Act { ACT_NONE = 0, ACT_GELU = 1, ACT_TANH = 2 };

template <typename T, typename V8, bool HAS_BIAS, int ACT, int BM, int BN,
          int NW>
__global__ __launch_bounds__(NW * WAVE)
void gemm_nt_kernel(const T* __restrict__ A, const T* __restrict__ W,
                    const T* __restrict__ bias, T* __restrict__ C,
                    T* __restrict__ pre, long M, long N, long K,
                    int tiles_n, int nwg) {
  // the pre-activation is saved exactly when there is an activation
  constexpr bool SAVE_PRE = ACT != ACT_NONE;
  // wave grid: 2x2 (4 waves) for square-ish tiles, 1x4 / 4x1 for skinny
  // ones; 2x4 at 8 waves (more waves hide the end-of-tile vmcnt stall)
  constexpr int WM = NW == 8 ? 2 : ((BM >= 128 || BN < 128) ? 2 : 1);
  constexpr int WN = NW / WM;
  constexpr int TM = BM / WM, TN = BN / WN;     // per-wave sub-tile
  constexpr int RM = TM / 16, RN = TN / 16;     // fragment repeats

  // XCD-aware bijective remap of the tile id (guide T1)
  const int wg = xcd_remap(blockIdx.x, nwg);
  const long tile_m = wg / tiles_n, tile_n = wg % tiles_n;
  const long m0 = tile_m * BM, n0 = tile_n * BN;

  __shared__ __attribute__((aligned(16))) char lds_a[2][BM * 128];
  __shared__ __attribute__((aligned(16))) char lds_b[2][BN * 128];

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wr = (wid / WN) * TM, wc = (wid % WN) * TN;

  f32x4 acc[RM][RN] = {};

  stage_tile<T, BM, NW>(A, K, m0, M, 0, lds_a[0]);
  stage_tile<T, BN, NW>(W, K, n0, N, 0, lds_b[0]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int ntiles = (int)(K / BK);
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) {
      stage_tile<T, BM, NW>(A, K, m0, M, (long)(t + 1) * BK, lds_a[cur ^ 1]);
      stage_tile<T, BN, NW>(W, K, n0, N, (long)(t + 1) * BK, lds_b[cur ^ 1]);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a_frag[RM], b_frag[RN];
#pragma unroll
      for (int i = 0; i < RM; ++i)
        a_frag[i] = read_frag<V8>(lds_a[cur], wr + i * 16, ks);
#pragma unroll
      for (int j = 0; j < RN; ++j)
        b_frag[j] = read_frag<V8>(lds_b[cur], wc + j * 16, ks);
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

  // epilogue: bias + activation fused into the C write
  const int crow_off = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int i = 0; i < RM; ++i) {
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const long n = n0 + wc + j * 16 + ccol;
      if (n >= N) continue;
      const float bv = HAS_BIAS ? to_f32<T>(bias[n]) : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long m = m0 + wr + i * 16 + crow_off + r;
        if (m >= M) continue;
        float v = acc[i][j][r] + bv;
        if (SAVE_PRE) pre[m * N + n] = from_f32<T>(v);
        if (ACT == ACT_GELU) v = gelu_f2(v);
        if (ACT == ACT_TANH) v = tanhf(v);
        C[m * N + n] = from_f32<T>(v);
      }
    }
  }
}

struct TileChoice { int bm, bn, nw; };

// The instantiated (tile, waves) pairs: 64x64, 64x128 and 128x128 at 8 or 4
// waves, 128x64 at 4 waves only. 8 waves are the default (swept +8-15% over
// 4), PDNLP_GEMM_W4 reverts to 4; 128x64 takes 4 waves whatever it says.
static TileChoice with_waves(int bm, int bn) {
  const bool w4 = std::getenv("PDNLP_GEMM_W4") != nullptr;
  return {bm, bn, (w4 || (bm == 128 && bn == 64)) ? 4 : 8};
}

// pick the tile so the grid fills 256 CUs (>= ~2 WGs per CU preferred),
// falling back to the highest-intensity 128x128 when everything fills.
static TileChoice pick_tile(long M, long N) {
  if (const char* env = std::getenv("PDNLP_GEMM_TILE")) {
    // the grid is sized from this tile, so only a tile that has a kernel
    // may pass
    int bm = 0, bn = 0;
    const bool parsed = std::sscanf(env, "%dx%d", &bm, &bn) == 2;
    TORCH_CHECK(parsed && (bm == 64 || bm == 128) && (bn == 64 || bn == 128),
                "PDNLP_GEMM_TILE=", env,
                ": accepted tiles are 64x64, 64x128, 128x64, 128x128");
    return with_waves(bm, bn);
  }
  auto wgs = [&](int bm, int bn) {
    return ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  };
  // swept on MI355X (profiles/r01 microbench + r02 sweep_fwd.log):
  // 128x128 only wins once the grid is deep (>=1024 WGs, or M>=8192 where
  // it beat 64x128 by 20-40% on every bert-large shape); small-K BERT
  // shapes prefer smaller tiles with more workgroups; N<=768 prefers
  // 64x64 (attnout 411 vs 261 TF).
  if (M >= 8192 && wgs(128, 128) >= 384) return with_waves(128, 128);
  if (wgs(128, 128) >= 1024) return with_waves(128, 128);
  if (N <= 768) {
    if (wgs(64, 64) >= 512) return with_waves(64, 64);
    return with_waves(64, 128);
  }
  if (wgs(64, 128) >= 512) return with_waves(64, 128);
  return with_waves(128, 128);
}

template <typename T>
using NtKernel = void (*)(const T*, const T*, const T*, T*, T*, long, long,
                          long, int, int);

template <typename T, typename V8, int BM, int BN, int NW>
NtKernel<T> nt_epilogue(bool has_bias, int act) {
  if (act == ACT_GELU)
    return has_bias ? gemm_nt_kernel<T, V8, true, ACT_GELU, BM, BN, NW>
                    : gemm_nt_kernel<T, V8, false, ACT_GELU, BM, BN, NW>;
  if (act == ACT_TANH)
    return has_bias ? gemm_nt_kernel<T, V8, true, ACT_TANH, BM, BN, NW>
                    : gemm_nt_kernel<T, V8, false, ACT_TANH, BM, BN, NW>;
  return has_bias ? gemm_nt_kernel<T, V8, true, ACT_NONE, BM, BN, NW>
                  : gemm_nt_kernel<T, V8, false, ACT_NONE, BM, BN, NW>;
}

// pick_tile returns only pairs listed here
template <typename T, typename V8>
NtKernel<T> nt_kernel(TileChoice tc, bool has_bias, int act) {
  const bool w8 = tc.nw == 8;
  if (tc.bm == 64 && tc.bn == 64)
    return w8 ? nt_epilogue<T, V8, 64, 64, 8>(has_bias, act)
              : nt_epilogue<T, V8, 64, 64, 4>(has_bias, act);
  if (tc.bm == 64 && tc.bn == 128)
    return w8 ? nt_epilogue<T, V8, 64, 128, 8>(has_bias, act)
              : nt_epilogue<T, V8, 64, 128, 4>(has_bias, act);
  if (tc.bm == 128 && tc.bn == 64)
    return nt_epilogue<T, V8, 128, 64, 4>(has_bias, act);
  return w8 ? nt_epilogue<T, V8, 128, 128, 8>(has_bias, act)
            : nt_epilogue<T, V8, 128, 128, 4>(has_bias, act);
}

template <typename T, typename V8>
void launch_gemm(const torch::Tensor& A, const torch::Tensor& W,
                 const torch::Tensor& bias, torch::Tensor& C,
                 torch::Tensor& pre, int act, bool has_bias,
                 hipStream_t stream) {
  const long M = A.size(0), K = A.size(1), N = W.size(0);
  const TileChoice tc = pick_tile(M, N);
  const int tiles_m = (int)((M + tc.bm - 1) / tc.bm);
  const int tiles_n = (int)((N + tc.bn - 1) / tc.bn);
  const int nwg = tiles_m * tiles_n;
  const T* bptr = has_bias ? (const T*)bias.data_ptr() : nullptr;
  T* pptr = act != ACT_NONE ? (T*)pre.data_ptr() : nullptr;
  auto kernel = nt_kernel<T, V8>(tc, has_bias, act);
  hipLaunchKernelGGL(kernel, dim3(nwg), dim3(tc.nw * WAVE), 0, stream,
                     (const T*)A.data_ptr(), (const T*)W.data_ptr(), bptr,
                     (T*)C.data_ptr(), pptr, M, N, K, tiles_n, nwg);
}

}  // namespace

// {C, pre}: C = act(A @ W^T + bias); pre is the pre-activation, saved for
// the backward when there is an activation (else empty)
std::vector<torch::Tensor> gemm_nt_fwd(torch::Tensor A, torch::Tensor W,
                                       torch::Tensor bias, std::string act) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() && W.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && W.dim() == 2 && A.size(1) == W.size(1));
  TORCH_CHECK(A.size(1) % BK == 0, "K must be a multiple of 64");
  const long M = A.size(0), N = W.size(0);
  const bool has_bias = bias.defined() && bias.numel() > 0;
  const int actv = act == "gelu" ? ACT_GELU : act == "tanh" ? ACT_TANH
                                                            : ACT_NONE;
  auto C = torch::empty({M, N}, A.options());
  auto pre = actv != ACT_NONE ? torch::empty({M, N}, A.options())
                              : torch::empty({0}, A.options());
  auto stream = at::hip::getCurrentHIPStream();
  if (A.scalar_type() == torch::kBFloat16) {
    launch_gemm<__hip_bfloat16, bf16x8>(A, W, bias, C, pre, actv, has_bias,
                                        stream);
  } else if (A.scalar_type() == torch::kHalf) {
    launch_gemm<__half, f16x8>(A, W, bias, C, pre, actv, has_bias, stream);
  } else {
    TORCH_CHECK(false, "gemm_nt_fwd: bf16/fp16 only");
  }
  return {C, pre};
}
