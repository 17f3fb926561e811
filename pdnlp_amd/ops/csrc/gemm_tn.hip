// Hand-written CDNA4 TN GEMM: C[N,K] = A[M,N]^T @ B[M,K] — the dW
// weight-gradient GEMMs of the BERT backward (dW = dY^T X).
// hipBLASLt tops out at ~300-450 TF on these shapes (small output, long
// contraction; verified with PyTorch TunableOp exhaustive search), because
// the M=4096 contraction has to stream through a small C tile.
//
// MI355X-native design:
//  - 64x64 output tile, contraction chunked by 64, 4 waves (2x2) each
//    owning a 32x32 sub-tile -> 432-576 workgroups on the BERT shapes
//    (fills the 256 CUs without split-K).
//  - Both operands are consumed TRANSPOSED (rows of dY^T / X^T): both are
//    staged into the tr-read LDS image and read with gfx950's
//    ds_read_b64_tr_b16 hardware transpose-read (layout and lane math in
//    gemm_common.h) instead of per-lane b16 gathers.
//  - fp32 accumulation, bf16/fp16 C write, double-buffered staging.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdlib>

#include "gemm_common.h"

namespace {

constexpr int NTHREADS = 256;
constexpr int BT = 64;   // output tile is BT x BT
constexpr int BC = 64;   // contraction chunk

// 4-wave 64x64 kernel (PDNLP_TN_W4): 2x2 waves, a 32x32 sub-tile each
template <typename T, typename V8>
__global__ __launch_bounds__(NTHREADS)
void gemm_tn_kernel(const T* __restrict__ A, const T* __restrict__ B,
                    T* __restrict__ C, long M, long N, long K,
                    int tiles_k, int nwg) {
  // XCD-aware bijective remap (guide T1)
  const int wg = xcd_remap(blockIdx.x, nwg);
  const long n0 = (wg / tiles_k) * BT, k0 = (wg % tiles_k) * BT;

  __shared__ __attribute__((aligned(16))) char lds_a[2][BC * BT * 2];
  __shared__ __attribute__((aligned(16))) char lds_b[2][BC * BT * 2];

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wr = (wid >> 1) * 32, wc = (wid & 1) * 32;  // 32x32 per wave

  f32x4 acc[2][2] = {};

  stage_tr<T, 4>(A, N, 0, M, n0, lds_a[0]);
  stage_tr<T, 4>(B, K, 0, M, k0, lds_b[0]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int nchunks = (int)(M / BC);
  int cur = 0;
  for (int t = 0; t < nchunks; ++t) {
    if (t + 1 < nchunks) {
      stage_tr<T, 4>(A, N, (long)(t + 1) * BC, M, n0, lds_a[cur ^ 1]);
      stage_tr<T, 4>(B, K, (long)(t + 1) * BC, M, k0, lds_b[cur ^ 1]);
    }
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      V8 a_frag[2], b_frag[2];
      frag_tr4<V8>(frag_tr_base(lds_a[cur], wr, ms * 32),
                   frag_tr_base(lds_a[cur], wr + 16, ms * 32),
                   frag_tr_base(lds_b[cur], wc, ms * 32),
                   frag_tr_base(lds_b[cur], wc + 16, ms * 32),
                   a_frag, b_frag);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
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
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long k = k0 + wc + j * 16 + ccol;
      if (k >= K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long n = n0 + wr + i * 16 + crow_off + r;
        if (n >= N) continue;
        C[n * K + k] = from_f32<T>(acc[i][j][r]);
      }
    }
  }
}

// 8-wave variant (512 threads): wave grid 2(n) x 4(k), each wave a 32x16
// sub-tile — more waves hide the end-of-chunk vmcnt stall (same lever that
// bought 8-15% on the forward NT GEMM).
template <typename T, typename V8>
__global__ __launch_bounds__(512)
void gemm_tn_w8_kernel(const T* __restrict__ A, const T* __restrict__ B,
                       T* __restrict__ C, long M, long N, long K,
                       int tiles_k, int nwg) {
  const int wg = xcd_remap(blockIdx.x, nwg);
  const long n0 = (wg / tiles_k) * BT, k0 = (wg % tiles_k) * BT;

  __shared__ __attribute__((aligned(16))) char lds_a[2][BC * BT * 2];
  __shared__ __attribute__((aligned(16))) char lds_b[2][BC * BT * 2];

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wr = (wid >> 2) * 32, wc = (wid & 3) * 16;  // 32x16 per wave

  f32x4 acc[2] = {};

  stage_tr<T, 8>(A, N, 0, M, n0, lds_a[0]);
  stage_tr<T, 8>(B, K, 0, M, k0, lds_b[0]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int nchunks = (int)(M / BC);
  int cur = 0;
  for (int t = 0; t < nchunks; ++t) {
    if (t + 1 < nchunks) {
      stage_tr<T, 8>(A, N, (long)(t + 1) * BC, M, n0, lds_a[cur ^ 1]);
      stage_tr<T, 8>(B, K, (long)(t + 1) * BC, M, k0, lds_b[cur ^ 1]);
    }
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      V8 a_frag[2];
      frag_tr2<V8>(frag_tr_base(lds_a[cur], wr, ms * 32),
                   frag_tr_base(lds_a[cur], wr + 16, ms * 32), a_frag);
      V8 b_frag = frag_tr1<V8>(frag_tr_base(lds_b[cur], wc, ms * 32));
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        acc[i] = mfma16<V8>(a_frag[i], b_frag, acc[i]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }

  const int crow_off = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long k = k0 + wc + ccol;
    if (k >= K) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long n = n0 + wr + i * 16 + crow_off + r;
      if (n >= N) continue;
      C[n * K + k] = from_f32<T>(acc[i][r]);
    }
  }
}

// ---- v2: 128x128 tiles + split-M + fp32 partials --------------------------
// The 64x64 kernel is HBM-bound: every output element re-reads
// (64+64)/(64*64) contraction bytes. 128x128 tiles cut that re-read 2x per
// dimension, and splitting the M contraction across SM workgroups restores
// the grid depth the bigger tile loses (dW outputs are small: 72-288
// tiles). Each split writes its fp32 partial slice [s][N][K] without
// atomics; a vectorized reduce+cast kernel folds the S slices (few us at
// the 8 TB/s roofline). Measured (gpurun_out/bench_dgemm*.log): the 64x64
// single-pass kernel reached 117-381 TF on the BERT dW shapes vs
// hipBLASLt's 169-445; this structure targets ~500 TF on all of them.
//
// COLSUM: the workgroups of the k0 == 0 tile column also produce the column
// sums of A over their M span (db = sum_m dY[m, n], the bias gradient of the
// projection whose dW this GEMM computes). sum_m A[m, n] is A^T times a
// column of ones, i.e. one more MFMA on an a_frag that is already in
// registers, against an all-ones B fragment: every column of that 16x16
// result holds the row sums, so the lanes with (lane & 15) == 0 own
// colsum[n0 + wr + i*16 + (lane>>4)*4 + r]. The four waves that share a wr
// hold identical a_frag[0..3]; wave (wid & 3) == q takes a_frag[q], so each
// wave issues 9 MFMAs per ms step instead of 8. The fp32 slices land behind
// the dW partials, P[sm*N*K + split*N + n], without atomics. The dW
// accumulators are untouched, so C is bit-identical to the plain kernel's.
template <typename T, typename V8, bool RAWBAR, bool COLSUM>
__global__ __launch_bounds__(512)
void gemm_tn_sk_kernel(const T* __restrict__ A, const T* __restrict__ B,
                       float* __restrict__ P, long M, long N, long K,
                       int tiles_k, int ntiles, int sm, int nwg) {
  constexpr int BTN = 128, BTK = 128;
  constexpr int GLDS = 4;  // stage_tr wave-instructions per buffer
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int split = wg / ntiles;
  const int tile = wg % ntiles;
  const long n0 = (tile / tiles_k) * BTN, k0 = (tile % tiles_k) * BTK;
  const long mspan = M / sm;              // host guarantees M % (64*sm) == 0
  const long mbase = split * mspan;

  __shared__ __attribute__((aligned(16))) char lds_a[2][2 * 8192];
  __shared__ __attribute__((aligned(16))) char lds_b[2][2 * 8192];

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wr = (wid >> 2) * 64, wc = (wid & 3) * 32;  // 64x32 per wave

  f32x4 acc[4][2] = {};
  // wave-uniform: only the k0 == 0 tile of each n-tile row sums A
  const bool do_cs = COLSUM && k0 == 0;
  const int cs_q = wid & 3;
  f32x4 cs_acc = {};
  V8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = 1.0f;

  auto stage = [&](long m_chunk, int buf) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      stage_tr<T, 8>(A, N, m_chunk, M, n0 + g * 64, lds_a[buf] + g * 8192);
      stage_tr<T, 8>(B, K, m_chunk, M, k0 + g * 64, lds_b[buf] + g * 8192);
    }
  };

  stage(mbase, 0);
  if constexpr (!RAWBAR) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  const int nchunks = (int)(mspan / BC);
  int cur = 0;
  const int a_grp = wr >> 6;              // wave-uniform group of the a frags
  for (int t = 0; t < nchunks; ++t) {
    if (t + 1 < nchunks) stage(mbase + (long)(t + 1) * BC, cur ^ 1);
    if constexpr (RAWBAR) {
      // counted wait keeps buffer t+1's GLDS loads in flight across the
      // barriers and tile t's MFMAs (see gemm_nn.hip note)
      if (t + 1 < nchunks)
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"i"(GLDS)
                     : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      V8 a_frag[4], b_frag[2];
#pragma unroll
      for (int i = 0; i < 4; i += 2)
        frag_tr2<V8>(
            frag_tr_base(lds_a[cur] + a_grp * 8192, (wr & 63) + i * 16,
                         ms * 32),
            frag_tr_base(lds_a[cur] + a_grp * 8192, (wr & 63) + (i + 1) * 16,
                         ms * 32),
            &a_frag[i]);
      {
        const int c0 = wc, c1 = wc + 16;
        frag_tr2<V8>(
            frag_tr_base(lds_b[cur] + (c0 >> 6) * 8192, c0 & 63, ms * 32),
            frag_tr_base(lds_b[cur] + (c1 >> 6) * 8192, c1 & 63, ms * 32),
            b_frag);
      }
      if constexpr (COLSUM) {
        if (do_cs) {
          // Issued BEFORE the dW MFMAs: behind them, the next ms step's
          // LDS reads (which overwrite the fragment registers) would have
          // to wait until this MFMA leaves the queue, i.e. for all 8 dW
          // MFMAs to drain (measured: +12% kernel time).
          // Wave-uniform pick through 32-bit selects: indexing a_frag by
          // cs_q would put the fragments in scratch.
          typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
          u32x4 sel;
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const unsigned int f0 = reinterpret_cast<u32x4&>(a_frag[0])[d];
            const unsigned int f1 = reinterpret_cast<u32x4&>(a_frag[1])[d];
            const unsigned int f2 = reinterpret_cast<u32x4&>(a_frag[2])[d];
            const unsigned int f3 = reinterpret_cast<u32x4&>(a_frag[3])[d];
            const unsigned int lo = (cs_q & 1) ? f1 : f0;
            const unsigned int hi = (cs_q & 1) ? f3 : f2;
            sel[d] = (cs_q & 2) ? hi : lo;
          }
          const V8 av = reinterpret_cast<V8&>(sel);
          cs_acc = mfma16<V8>(av, ones, cs_acc);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = mfma16<V8>(a_frag[i], b_frag[j], acc[i][j]);
        }
      }
    }
    if constexpr (RAWBAR) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    cur ^= 1;
  }

  float* Pout = P + (long)split * N * K;
  const int crow_off = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long k = k0 + wc + j * 16 + ccol;
      if (k >= K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long n = n0 + wr + i * 16 + crow_off + r;
        if (n >= N) continue;
        Pout[n * K + k] = acc[i][j][r];
      }
    }
  }
  if constexpr (COLSUM) {
    if (do_cs && ccol == 0) {
      float* PS = P + (long)sm * N * K + (long)split * N;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long n = n0 + wr + cs_q * 16 + crow_off + r;
        if (n < N) PS[n] = cs_acc[r];
      }
    }
  }
}

// fold the SM split partials and cast: C[n,k] = T(sum_s P[s,n,k])
template <typename T>
__device__ __forceinline__ void fold_partials4(const float* __restrict__ P,
                                               T* __restrict__ C, long i4,
                                               long NK, int sm) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 acc = *reinterpret_cast<const f4*>(P + i4);
  for (int s = 1; s < sm; ++s) {
    f4 v = *reinterpret_cast<const f4*>(P + (long)s * NK + i4);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += v[q];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) C[i4 + q] = from_f32<T>(acc[q]);
}

template <typename T>
__global__ __launch_bounds__(256)
void reduce_partials_kernel(const float* __restrict__ P, T* __restrict__ C,
                            long NK, int sm) {
  const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= NK) return;
  fold_partials4<T>(P, C, i4, NK, sm);
}

// same fold, plus (in the blocks past the dW ones) the column-sum slices
// P[sm*NK + s*N + n] of the COLSUM kernel into CS[n] — one launch for both
template <typename T>
__global__ __launch_bounds__(256)
void reduce_partials_colsum_kernel(const float* __restrict__ P,
                                   T* __restrict__ C, T* __restrict__ CS,
                                   long NK, long N, int sm, int rblocks) {
  if ((int)blockIdx.x < rblocks) {
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= NK) return;
    fold_partials4<T>(P, C, i4, NK, sm);
  } else {
    const long i4 = ((long)(blockIdx.x - rblocks) * 256 + threadIdx.x) * 4;
    if (i4 >= N) return;
    fold_partials4<T>(P + (long)sm * NK, CS, i4, N, sm);
  }
}

// split-M depth of the v2 path for an [M] contraction and tiles2 128x128
// output tiles (shared by gemm_tn and gemm_tn_colsum so C stays identical)
int tn_v2_split(long M, int tiles2) {
  int sm = 1;
  if (const char* env = getenv("PDNLP_TN_SM")) sm = atoi(env);
  else if (tiles2 < 512)
    // swept (gpurun_out/sweep_dgemm.log): sm4 wins for small outputs
    // (<=108 tiles), sm2 everywhere else under 512 tiles — deeper splits
    // pay more in fp32-partial traffic than they buy in grid fill
    sm = tiles2 <= 108 ? 4 : 2;
  if (sm < 1) sm = 1;
  while (sm > 1 && M % (64L * sm) != 0) sm /= 2;
  return sm;
}

// v2 (default): 128x128 tiles + split-M + fp32 partials when on-grid
bool tn_v2_ok(long N, long K) {
  return getenv("PDNLP_TN_V1") == nullptr && N % 128 == 0 && K % 128 == 0;
}

// v2 launches: gemm_tn_sk_kernel into the partials P, then the fold into C
// (and CS when `colsum`). `sync` picks the vmcnt(0)+__syncthreads schedule
// over the raw-barrier counted-vmcnt one.
template <typename T, typename V8>
void launch_tn_v2(const torch::Tensor& A, const torch::Tensor& B,
                  torch::Tensor& P, torch::Tensor& C, torch::Tensor& CS,
                  long M, long N, long K, int tiles2, int sm, bool colsum,
                  bool sync, hipStream_t stream) {
  const int nwg2 = tiles2 * sm;
  const long NK = N * K;
  const int rblocks = (int)((NK / 4 + 255) / 256);
  auto kernel =
      colsum ? (sync ? gemm_tn_sk_kernel<T, V8, false, true>
                     : gemm_tn_sk_kernel<T, V8, true, true>)
             : (sync ? gemm_tn_sk_kernel<T, V8, false, false>
                     : gemm_tn_sk_kernel<T, V8, true, false>);
  hipLaunchKernelGGL(kernel, dim3(nwg2), dim3(512), 0, stream,
                     (const T*)A.data_ptr(), (const T*)B.data_ptr(),
                     (float*)P.data_ptr(), M, N, K, (int)(K / 128), tiles2,
                     sm, nwg2);
  if (colsum) {
    const int cblocks = (int)((N / 4 + 255) / 256);
    hipLaunchKernelGGL((reduce_partials_colsum_kernel<T>),
                       dim3(rblocks + cblocks), dim3(256), 0, stream,
                       (const float*)P.data_ptr(), (T*)C.data_ptr(),
                       (T*)CS.data_ptr(), NK, N, sm, rblocks);
  } else {
    hipLaunchKernelGGL((reduce_partials_kernel<T>), dim3(rblocks), dim3(256),
                       0, stream, (const float*)P.data_ptr(),
                       (T*)C.data_ptr(), NK, sm);
  }
}

// single-pass 64x64 launches (off the 128 grid, or PDNLP_TN_V1)
template <typename T, typename V8>
void launch_tn_64(const torch::Tensor& A, const torch::Tensor& B,
                  torch::Tensor& C, long M, long N, long K,
                  hipStream_t stream) {
  const int tiles_k = (int)((K + BT - 1) / BT);
  const int nwg = (int)((N + BT - 1) / BT) * tiles_k;
  const bool w8 = getenv("PDNLP_TN_W4") == nullptr;  // 8 waves default
  auto kernel = w8 ? gemm_tn_w8_kernel<T, V8> : gemm_tn_kernel<T, V8>;
  hipLaunchKernelGGL(kernel, dim3(nwg), dim3(w8 ? 512 : NTHREADS), 0, stream,
                     (const T*)A.data_ptr(), (const T*)B.data_ptr(),
                     (T*)C.data_ptr(), M, N, K, tiles_k, nwg);
}

}  // namespace

torch::Tensor col_sum(torch::Tensor x);

namespace {

// {C, CS}: C = A^T @ B; with `colsum`, CS[n] = sum_m A[m, n] (else undefined).
// Both entry points run this, so C cannot differ between them.
std::pair<torch::Tensor, torch::Tensor> tn_impl(const torch::Tensor& A,
                                                const torch::Tensor& B,
                                                bool colsum) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() && B.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(0) == B.size(0));
  const long M = A.size(0), N = A.size(1), K = B.size(1);
  TORCH_CHECK(M % BC == 0, "gemm_tn: M must be a multiple of 64");
  // the 64-col stage_tr groups read [col0, col0+64) with only the
  // contraction rows clamped — partial-width column tiles would read OOB
  TORCH_CHECK(N % 64 == 0 && K % 64 == 0,
              "gemm_tn: N and K must be multiples of 64");
  const bool bf16 = A.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || A.scalar_type() == torch::kHalf,
              "gemm_tn: bf16/fp16 only");
  TORCH_CHECK(A.scalar_type() == B.scalar_type(),
              "gemm_tn: A and B dtypes differ");
  auto C = torch::empty({N, K}, A.options());
  torch::Tensor CS;
  auto stream = at::hip::getCurrentHIPStream();
  if (!tn_v2_ok(N, K)) {
    if (bf16) launch_tn_64<__hip_bfloat16, bf16x8>(A, B, C, M, N, K, stream);
    else launch_tn_64<__half, f16x8>(A, B, C, M, N, K, stream);
    if (colsum) CS = col_sum(A);
    return {C, CS};
  }
  const int tiles2 = (int)((N / 128) * (K / 128));
  const int sm = tn_v2_split(M, tiles2);
  // dW partials [sm][N][K], then (colsum) the column-sum slices [sm][N]
  auto P = torch::empty({(long)sm * (N * K + (colsum ? N : 0))},
                        A.options().dtype(torch::kFloat32));
  if (colsum) CS = torch::empty({N}, A.options());
  // raw-barrier counted-vmcnt schedule is the default (step-level +2.5-3%
  // measured on two boxes), PDNLP_TN_SYNC reverts — except that plain fp16
  // has only ever run the synchronous one (open inconsistency)
  const bool sync = getenv("PDNLP_TN_SYNC") != nullptr || (!colsum && !bf16);
  if (bf16)
    launch_tn_v2<__hip_bfloat16, bf16x8>(A, B, P, C, CS, M, N, K, tiles2, sm,
                                         colsum, sync, stream);
  else
    launch_tn_v2<__half, f16x8>(A, B, P, C, CS, M, N, K, tiles2, sm, colsum,
                                sync, stream);
  return {C, CS};
}

}  // namespace

// C = A^T @ B for row-major A [M, N], B [M, K]; returns C [N, K] in A's
// dtype (fp32 accumulation). Requires M, N and K to be multiples of 64.
torch::Tensor gemm_tn(torch::Tensor A, torch::Tensor B) {
  return tn_impl(A, B, false).first;
}

// {C, colsum} with C = gemm_tn(A, B) (bit-identical) and colsum[n] =
// sum_m A[m, n] in A's dtype — the dW/db pair of a biased projection from
// one pass over dY. On the v2 grid the sums ride along in the GEMM (see
// COLSUM above); the 64x64 path takes them from col_sum.
std::vector<torch::Tensor> gemm_tn_colsum(torch::Tensor A, torch::Tensor B) {
  auto r = tn_impl(A, B, true);
  return {r.first, r.second};
}
