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
//  - Both operands are consumed TRANSPOSED (rows of dY^T / X^T). Instead of
//    per-lane b16 gathers this uses gfx950's ds_read_b64_tr_b16 hardware
//    transpose-read (guide T10): each 4-lane cluster reads 4 rows of a 4x4
//    bf16 block (8-B aligned) and receives the block column-major.
//  - The LDS image for a [32 m][16 col] subtile is the tr-read layout
//    addr(m, c) = c + (m&3)*16 + (m>>3)*64 + ((m>>2)&1)*256 (elements),
//    built directly by global_load_lds: dest element run l*8..l*8+7 decodes
//    to (m_rel = ((l>>3)&3)*8 + (l>>5)*4 + ((l>>1)&3), c0 = (l&1)*8), i.e.
//    each lane fetches 16 contiguous bytes of one global row — coalesced.
//  - fp32 accumulation, bf16/fp16 C write, double-buffered staging.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdlib>

#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));

constexpr int NTHREADS = 256;
constexpr int BT = 64;   // output tile is BT x BT
constexpr int BC = 64;   // contraction chunk

// stage a [BC m][BT cols] tile of `src` (row stride ld) into the tr-read
// image. 8 subtiles of 512 elements; one glds wave-instruction fills one
// subtile; NW waves x (8/NW) calls cover the tile. Rows clamped to max_m.
template <typename T, int NW>
__device__ __forceinline__ void stage_tr(const T* __restrict__ src, long ld,
                                         long m0, long max_m, long col0,
                                         char* lds) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  // lane -> (m_rel within 32, c half) inside one subtile
  const int m_rel = ((lane >> 3) & 3) * 8 + (lane >> 5) * 4 + ((lane >> 1) & 3);
  const int c0 = (lane & 1) * 8;
  constexpr int SPW = 8 / NW;
#pragma unroll
  for (int s = 0; s < SPW; ++s) {
    const int sub = wid * SPW + s;        // subtile 0..7
    const int s_m = sub >> 2;             // m half (0: m 0..31, 1: 32..63)
    const int s_c = sub & 3;              // 16-col group
    long gm = m0 + s_m * 32 + m_rel;
    gm = gm < max_m ? gm : max_m - 1;
    const char* gp = (const char*)(src + gm * ld + col0 + s_c * 16 + c0);
    char* lp = lds + sub * 1024;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)gp,
        (__attribute__((address_space(3))) unsigned int*)lp, 16, 0, 0);
  }
}

// per-lane base address of the transposed fragment at (ent0, m_sub):
// lane l will receive data[ent0 + (l&15)][m_sub + (l>>4)*8 + i], i = 0..7.
__device__ __forceinline__ unsigned int frag_tr_base(const char* lds, int ent0,
                                                     int m_sub) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int sub = (m_sub >> 5) * 4 + (ent0 >> 4);
  // lane-LINEAR 8-B addresses over each quarter's 128-B [4m][16c] block —
  // the hardware transposes within the block (guide T10: "no internal lane
  // offset"); wrong per-lane math here silently feeds scrambled operands.
  return (unsigned int)(unsigned long)lds + sub * 1024 + (lane & 15) * 8 +
         (lane >> 4) * 128;
}

// 4 transposed fragments (2 A + 2 B) in ONE asm block: 8x
// ds_read_b64_tr_b16 then s_waitcnt lgkmcnt(0) INSIDE the block — the
// compiler cannot count asm ds ops, so the wait must come before the
// outputs escape the block.
template <typename V8>
__device__ __forceinline__ void frag_tr4(unsigned int a0, unsigned int a1,
                                         unsigned int b0, unsigned int b1,
                                         V8* af, V8* bf) {
  uint2v r0, r1, r2, r3, r4, r5, r6, r7;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\t"
      "ds_read_b64_tr_b16 %1, %8 offset:512\n\t"
      "ds_read_b64_tr_b16 %2, %9\n\t"
      "ds_read_b64_tr_b16 %3, %9 offset:512\n\t"
      "ds_read_b64_tr_b16 %4, %10\n\t"
      "ds_read_b64_tr_b16 %5, %10 offset:512\n\t"
      "ds_read_b64_tr_b16 %6, %11\n\t"
      "ds_read_b64_tr_b16 %7, %11 offset:512\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5),
        "=&v"(r6), "=&v"(r7)
      : "v"(a0), "v"(a1), "v"(b0), "v"(b1)
      : "memory");
  reinterpret_cast<uint2v*>(&af[0])[0] = r0;
  reinterpret_cast<uint2v*>(&af[0])[1] = r1;
  reinterpret_cast<uint2v*>(&af[1])[0] = r2;
  reinterpret_cast<uint2v*>(&af[1])[1] = r3;
  reinterpret_cast<uint2v*>(&bf[0])[0] = r4;
  reinterpret_cast<uint2v*>(&bf[0])[1] = r5;
  reinterpret_cast<uint2v*>(&bf[1])[0] = r6;
  reinterpret_cast<uint2v*>(&bf[1])[1] = r7;
}

template <typename V8>
__device__ __forceinline__ void frag_tr2(unsigned int a0, unsigned int a1,
                                         V8* f) {
  uint2v r0, r1, r2, r3;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %4 offset:512\n\t"
      "ds_read_b64_tr_b16 %2, %5\n\t"
      "ds_read_b64_tr_b16 %3, %5 offset:512\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
      : "v"(a0), "v"(a1)
      : "memory");
  reinterpret_cast<uint2v*>(&f[0])[0] = r0;
  reinterpret_cast<uint2v*>(&f[0])[1] = r1;
  reinterpret_cast<uint2v*>(&f[1])[0] = r2;
  reinterpret_cast<uint2v*>(&f[1])[1] = r3;
}

template <typename V8>
__device__ __forceinline__ V8 frag_tr1(unsigned int a0) {
  uint2v r0, r1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %2 offset:512\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1)
      : "v"(a0)
      : "memory");
  V8 f;
  reinterpret_cast<uint2v*>(&f)[0] = r0;
  reinterpret_cast<uint2v*>(&f)[1] = r1;
  return f;
}

template <typename T, typename V8, bool PREFETCH>
__global__ __launch_bounds__(NTHREADS)
void gemm_tn_kernel(const T* __restrict__ A, const T* __restrict__ B,
                    T* __restrict__ C, long M, long N, long K,
                    int tiles_k, int nwg) {
  // XCD-aware bijective remap (guide T1)
  int wg = blockIdx.x;
  {
    const int nxcd = 8;
    const int q = nwg / nxcd, r = nwg % nxcd;
    const int xcd = wg % nxcd, idx = wg / nxcd;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
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
    if (PREFETCH && t + 1 < nchunks) {
      stage_tr<T, 4>(A, N, (long)(t + 1) * BC, M, n0, lds_a[cur ^ 1]);
      stage_tr<T, 4>(B, K, (long)(t + 1) * BC, M, k0, lds_b[cur ^ 1]);
    }
    if (!PREFETCH && t > 0) {
      stage_tr<T, 4>(A, N, (long)t * BC, M, n0, lds_a[0]);
      stage_tr<T, 4>(B, K, (long)t * BC, M, k0, lds_b[0]);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
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
          if constexpr (std::is_same<V8, bf16x8>::value) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
          } else {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (PREFETCH) cur ^= 1;
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
  int wg = blockIdx.x;
  {
    const int nxcd = 8;
    const int q = nwg / nxcd, r = nwg % nxcd;
    const int xcd = wg % nxcd, idx = wg / nxcd;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
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
        if constexpr (std::is_same<V8, bf16x8>::value) {
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[i], b_frag, acc[i], 0, 0, 0);
        } else {
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
              a_frag[i], b_frag, acc[i], 0, 0, 0);
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
template <typename T, typename V8, bool RAWBAR = false,
          bool NOSYNC = false,  // TIMING PROBE ONLY: numerics invalid
          bool COLSUM = false>
__global__ __launch_bounds__(512)
void gemm_tn_sk_kernel(const T* __restrict__ A, const T* __restrict__ B,
                       float* __restrict__ P, long M, long N, long K,
                       int tiles_k, int ntiles, int sm, int nwg) {
  constexpr int BTN = 128, BTK = 128;
  constexpr int GLDS = 4;  // stage_tr wave-instructions per buffer
  int wg = blockIdx.x;
  {
    const int nxcd = 8;
    const int q = nwg / nxcd, r = nwg % nxcd;
    const int xcd = wg % nxcd, idx = wg / nxcd;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
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
      if constexpr (!NOSYNC) __builtin_amdgcn_s_barrier();
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
          if constexpr (std::is_same<V8, bf16x8>::value)
            cs_acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, ones, cs_acc,
                                                             0, 0, 0);
          else
            cs_acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, ones, cs_acc,
                                                            0, 0, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (std::is_same<V8, bf16x8>::value) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
          } else {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                a_frag[i], b_frag[j], acc[i][j], 0, 0, 0);
          }
        }
      }
    }
    if constexpr (RAWBAR) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if constexpr (!NOSYNC) __builtin_amdgcn_s_barrier();
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

bool tn_v2_ok(const torch::Tensor& A, long N, long K) {
  return getenv("PDNLP_TN_V1") == nullptr
      && getenv("PDNLP_TN_SERIAL") == nullptr
      && N % 128 == 0 && K % 128 == 0
      && (A.scalar_type() == torch::kBFloat16
          || A.scalar_type() == torch::kHalf);
}

template <typename T, typename V8>
void launch_tn_colsum(const torch::Tensor& A, const torch::Tensor& B,
                      torch::Tensor& P, torch::Tensor& C, torch::Tensor& CS,
                      long M, long N, long K, int tiles2, int sm,
                      hipStream_t stream) {
  const int nwg2 = tiles2 * sm;
  const long NK = N * K;
  const int rblocks = (int)((NK / 4 + 255) / 256);
  const int cblocks = (int)((N / 4 + 255) / 256);
  if (getenv("PDNLP_TN_SYNC") == nullptr)
    hipLaunchKernelGGL((gemm_tn_sk_kernel<T, V8, true, false, true>),
                       dim3(nwg2), dim3(512), 0, stream,
                       (const T*)A.data_ptr(), (const T*)B.data_ptr(),
                       (float*)P.data_ptr(), M, N, K, (int)(K / 128), tiles2,
                       sm, nwg2);
  else
    hipLaunchKernelGGL((gemm_tn_sk_kernel<T, V8, false, false, true>),
                       dim3(nwg2), dim3(512), 0, stream,
                       (const T*)A.data_ptr(), (const T*)B.data_ptr(),
                       (float*)P.data_ptr(), M, N, K, (int)(K / 128), tiles2,
                       sm, nwg2);
  hipLaunchKernelGGL((reduce_partials_colsum_kernel<T>),
                     dim3(rblocks + cblocks), dim3(256), 0, stream,
                     (const float*)P.data_ptr(), (T*)C.data_ptr(),
                     (T*)CS.data_ptr(), NK, N, sm, rblocks);
}

}  // namespace

// C = A^T @ B for row-major A [M, N], B [M, K]; returns C [N, K] in A's
// dtype (fp32 accumulation). Requires M % 64 == 0, N % 16 == 0, K % 16 == 0.
torch::Tensor gemm_tn(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() && B.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(0) == B.size(0));
  const long M = A.size(0), N = A.size(1), K = B.size(1);
  TORCH_CHECK(M % BC == 0, "gemm_tn: M must be a multiple of 64");
  // the 64-col stage_tr groups read [col0, col0+64) with only the
  // contraction rows clamped — partial-width column tiles would read OOB
  TORCH_CHECK(N % 64 == 0 && K % 64 == 0,
              "gemm_tn: N and K must be multiples of 64");
  auto C = torch::empty({N, K}, A.options());
  auto stream = at::hip::getCurrentHIPStream();
  const bool serial = getenv("PDNLP_TN_SERIAL") != nullptr;
  const bool w8 = getenv("PDNLP_TN_W4") == nullptr;  // 8 waves default
  // v2 (default): 128x128 tiles + split-M + fp32 partials when on-grid
  const bool v2_ok = getenv("PDNLP_TN_V1") == nullptr && !serial
      && N % 128 == 0 && K % 128 == 0
      && (A.scalar_type() == torch::kBFloat16
          || A.scalar_type() == torch::kHalf);
  if (v2_ok) {
    const int tiles2 = (int)((N / 128) * (K / 128));
    const int sm = tn_v2_split(M, tiles2);
    const int nwg2 = tiles2 * sm;
    auto P = torch::empty({sm, N, K},
                          A.options().dtype(torch::kFloat32));
    const long NK = N * K;
    const int rblocks = (int)((NK / 4 + 255) / 256);
    // raw-barrier counted-vmcnt schedule is DEFAULT (step-level +2.5-3%
    // measured on two boxes: gpurun_out/b_rb*.log); PDNLP_TN_SYNC reverts
    const bool rb = getenv("PDNLP_TN_SYNC") == nullptr;
    // TIMING PROBE (numerics INVALID — races by construction): bounds what
    // a perfect barrier-free pipeline could buy on this structure
    const bool probe = getenv("PDNLP_TN_PROBE") != nullptr;
    if (A.scalar_type() == torch::kBFloat16) {
      if (probe)
        hipLaunchKernelGGL(
            (gemm_tn_sk_kernel<__hip_bfloat16, bf16x8, true, true>),
            dim3(nwg2), dim3(512), 0, stream,
            (const __hip_bfloat16*)A.data_ptr(),
            (const __hip_bfloat16*)B.data_ptr(), (float*)P.data_ptr(),
            M, N, K, (int)(K / 128), tiles2, sm, nwg2);
      else if (rb)
        hipLaunchKernelGGL((gemm_tn_sk_kernel<__hip_bfloat16, bf16x8, true>),
                           dim3(nwg2), dim3(512), 0, stream,
                           (const __hip_bfloat16*)A.data_ptr(),
                           (const __hip_bfloat16*)B.data_ptr(),
                           (float*)P.data_ptr(), M, N, K,
                           (int)(K / 128), tiles2, sm, nwg2);
      else
        hipLaunchKernelGGL((gemm_tn_sk_kernel<__hip_bfloat16, bf16x8>),
                           dim3(nwg2), dim3(512), 0, stream,
                           (const __hip_bfloat16*)A.data_ptr(),
                           (const __hip_bfloat16*)B.data_ptr(),
                           (float*)P.data_ptr(), M, N, K,
                           (int)(K / 128), tiles2, sm, nwg2);
      hipLaunchKernelGGL((reduce_partials_kernel<__hip_bfloat16>),
                         dim3(rblocks), dim3(256), 0, stream,
                         (const float*)P.data_ptr(),
                         (__hip_bfloat16*)C.data_ptr(), NK, sm);
    } else {
      hipLaunchKernelGGL((gemm_tn_sk_kernel<__half, f16x8>),
                         dim3(nwg2), dim3(512), 0, stream,
                         (const __half*)A.data_ptr(),
                         (const __half*)B.data_ptr(),
                         (float*)P.data_ptr(), M, N, K,
                         (int)(K / 128), tiles2, sm, nwg2);
      hipLaunchKernelGGL((reduce_partials_kernel<__half>),
                         dim3(rblocks), dim3(256), 0, stream,
                         (const float*)P.data_ptr(),
                         (__half*)C.data_ptr(), NK, sm);
    }
    return C;
  }
  const int tiles_n = (int)((N + BT - 1) / BT);
  const int tiles_k = (int)((K + BT - 1) / BT);
  const int nwg = tiles_n * tiles_k;
  if (A.scalar_type() == torch::kBFloat16) {
    if (serial)
      hipLaunchKernelGGL((gemm_tn_kernel<__hip_bfloat16, bf16x8, false>),
                         dim3(nwg), dim3(NTHREADS), 0, stream,
                         (const __hip_bfloat16*)A.data_ptr(),
                         (const __hip_bfloat16*)B.data_ptr(),
                         (__hip_bfloat16*)C.data_ptr(), M, N, K, tiles_k, nwg);
    else if (w8)
      hipLaunchKernelGGL((gemm_tn_w8_kernel<__hip_bfloat16, bf16x8>),
                         dim3(nwg), dim3(512), 0, stream,
                         (const __hip_bfloat16*)A.data_ptr(),
                         (const __hip_bfloat16*)B.data_ptr(),
                         (__hip_bfloat16*)C.data_ptr(), M, N, K, tiles_k, nwg);
    else
      hipLaunchKernelGGL((gemm_tn_kernel<__hip_bfloat16, bf16x8, true>),
                         dim3(nwg), dim3(NTHREADS), 0, stream,
                         (const __hip_bfloat16*)A.data_ptr(),
                         (const __hip_bfloat16*)B.data_ptr(),
                         (__hip_bfloat16*)C.data_ptr(), M, N, K, tiles_k, nwg);
  } else if (A.scalar_type() == torch::kHalf) {
    if (w8)
      hipLaunchKernelGGL((gemm_tn_w8_kernel<__half, f16x8>), dim3(nwg),
                         dim3(512), 0, stream,
                         (const __half*)A.data_ptr(),
                         (const __half*)B.data_ptr(),
                         (__half*)C.data_ptr(), M, N, K, tiles_k, nwg);
    else
      hipLaunchKernelGGL((gemm_tn_kernel<__half, f16x8, true>), dim3(nwg),
                         dim3(NTHREADS), 0, stream,
                         (const __half*)A.data_ptr(), (const __half*)B.data_ptr(),
                         (__half*)C.data_ptr(), M, N, K, tiles_k, nwg);
  } else {
    TORCH_CHECK(false, "gemm_tn: bf16/fp16 only");
  }
  return C;
}

torch::Tensor col_sum(torch::Tensor x);

// {C, colsum} with C = gemm_tn(A, B) (bit-identical) and colsum[n] =
// sum_m A[m, n] in A's dtype — the dW/db pair of a biased projection from
// one pass over dY. On the v2 grid the sums ride along in the GEMM (see
// COLSUM above); every other path computes C as gemm_tn does and takes the
// sums from col_sum.
std::vector<torch::Tensor> gemm_tn_colsum(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() && B.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(0) == B.size(0));
  const long M = A.size(0), N = A.size(1), K = B.size(1);
  if (!tn_v2_ok(A, N, K) || getenv("PDNLP_TN_PROBE") != nullptr)
    return {gemm_tn(A, B), col_sum(A)};
  TORCH_CHECK(M % BC == 0, "gemm_tn: M must be a multiple of 64");
  TORCH_CHECK(A.scalar_type() == B.scalar_type(),
              "gemm_tn_colsum: A and B dtypes differ");
  auto C = torch::empty({N, K}, A.options());
  auto CS = torch::empty({N}, A.options());
  const int tiles2 = (int)((N / 128) * (K / 128));
  const int sm = tn_v2_split(M, tiles2);
  // dW partials [sm][N][K], then the column-sum slices [sm][N]
  auto P = torch::empty({(long)sm * (N * K + N)},
                        A.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  if (A.scalar_type() == torch::kBFloat16)
    launch_tn_colsum<__hip_bfloat16, bf16x8>(A, B, P, C, CS, M, N, K, tiles2,
                                             sm, stream);
  else
    launch_tn_colsum<__half, f16x8>(A, B, P, C, CS, M, N, K, tiles2, sm,
                                    stream);
  return {C, CS};
}
