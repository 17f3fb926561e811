// Hand-written CDNA4 MFMA GEMM: C[M,N] = A[M,K] @ W[N,K]^T (+bias) (+act)
// — the forward GEMMs of the BERT hot path with
// the bias/GELU/tanh epilogue fused into the C-write.
//
// Structure (the "step-3" ladder structure of the CDNA4 guide, §5):
//  - templated BM x BN output tile, BK=64, 4 waves (256 threads); wave grid
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
//    Override for sweeps: env PDNLP_GEMM_TILE=MxN (e.g. 64x128).
//
// A-fragment: lane l holds A[l&15][(l>>4)*8 + i], i=0..7 -> one ds_read_b128.
// B-fragment: lane l holds W[n0 + (l&15)][k0 + (l>>4)*8 + i] — the same
// pattern because W is stored [N,K] row-major (torch Linear layout) and
// C = A @ W^T. C/D: col = lane&15, row = (lane>>4)*4 + reg.
//
// Backward dGEMMs (dX = dY@W, dW = dY^T@X) are plain non-fused GEMMs and go
// through rocBLAS (torch.matmul) from functional.py.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdlib>

#include "gemm_common.h"

namespace {

constexpr int BK = 64;
constexpr int NTHREADS = 256;

__device__ __forceinline__ float gelu_f2(float x) {
  return 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
}

enum Act { ACT_NONE = 0, ACT_GELU = 1, ACT_TANH = 2 };

template <typename T, typename V8, bool HAS_BIAS, int ACT, bool SAVE_PRE,
          int BM, int BN, int NW, bool RAWBAR = false>
__global__ __launch_bounds__(NW * WAVE)
void gemm_nt_kernel(const T* __restrict__ A, const T* __restrict__ W,
                    const T* __restrict__ bias, T* __restrict__ C,
                    T* __restrict__ pre, long M, long N, long K,
                    int tiles_n, int nwg) {
  // glds wave-instructions per buffer (counted-vmcnt schedule)
  constexpr int GLDS = BM / (8 * NW) + BN / (8 * NW);
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
  if constexpr (!RAWBAR) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  const int ntiles = (int)(K / BK);
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) {
      stage_tile<T, BM, NW>(A, K, m0, M, (long)(t + 1) * BK, lds_a[cur ^ 1]);
      stage_tile<T, BN, NW>(W, K, n0, N, (long)(t + 1) * BK, lds_b[cur ^ 1]);
    }
    if constexpr (RAWBAR) {
      // counted wait keeps tile t+1's loads in flight across the barriers
      // and tile t's MFMAs (gemm_tn.hip note; pays at <=2 blocks/CU)
      if (t + 1 < ntiles)
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"i"(GLDS)
                     : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
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
    if constexpr (RAWBAR) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
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


// 3-deep pipelined variant (8 waves, dynamic LDS): stage tile t+2 while
// computing tile t, wait only vmcnt(NGLDS) (= t+2's in-flight loads) before
// a RAW s_barrier — __syncthreads() would drain the glds queue to zero
// (the ~70% wave-park the PMC profile shows on the 2-barrier loop).
template <typename T, typename V8, bool HAS_BIAS, int ACT, bool SAVE_PRE,
          int BM, int BN>
__global__ __launch_bounds__(512)
void gemm_nt_pipe_kernel(const T* __restrict__ A, const T* __restrict__ W,
                         const T* __restrict__ bias, T* __restrict__ C,
                         T* __restrict__ pre, long M, long N, long K,
                         int tiles_n, int nwg) {
  constexpr int NW = 8;
  constexpr int WM = 2, WN = 4;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int RM = TM / 16, RN = TN / 16;
  constexpr int NGLDS = BM / (8 * NW) + BN / (8 * NW);  // glds per wave/tile

  const int wg = xcd_remap(blockIdx.x, nwg);
  const long tile_m = wg / tiles_n, tile_n = wg % tiles_n;
  const long m0 = tile_m * BM, n0 = tile_n * BN;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto lds_a = [&](int i) -> char* { return smem + i * (BM + BN) * 128; };
  auto lds_b = [&](int i) -> char* {
    return smem + i * (BM + BN) * 128 + BM * 128;
  };

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wr = (wid / WN) * TM, wc = (wid % WN) * TN;

  f32x4 acc[RM][RN] = {};

  const int ntiles = (int)(K / BK);
  stage_tile<T, BM, NW>(A, K, m0, M, 0, lds_a(0));
  stage_tile<T, BN, NW>(W, K, n0, N, 0, lds_b(0));
  if (1 < ntiles) {
    stage_tile<T, BM, NW>(A, K, m0, M, BK, lds_a(1));
    stage_tile<T, BN, NW>(W, K, n0, N, BK, lds_b(1));
  }
  if constexpr (NGLDS == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t % 3;
    const bool staged = t + 2 < ntiles;
    if (staged) {
      stage_tile<T, BM, NW>(A, K, m0, M, (long)(t + 2) * BK,
                            lds_a((t + 2) % 3));
      stage_tile<T, BN, NW>(W, K, n0, N, (long)(t + 2) * BK,
                            lds_b((t + 2) % 3));
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a_frag[RM], b_frag[RN];
#pragma unroll
      for (int i = 0; i < RM; ++i)
        a_frag[i] = read_frag<V8>(lds_a(cur), wr + i * 16, ks);
#pragma unroll
      for (int j = 0; j < RN; ++j)
        b_frag[j] = read_frag<V8>(lds_b(cur), wc + j * 16, ks);
#pragma unroll
      for (int i = 0; i < RM; ++i) {
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          acc[i][j] = mfma16<V8>(a_frag[i], b_frag[j], acc[i][j]);
        }
      }
    }
    if (staged) {
      if constexpr (NGLDS == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
  }

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


// Register-staged BK=128 variant (8 waves, ONE 64-KB LDS buffer): the next
// K-tile is loaded global->registers while the current tile computes from
// LDS (T14 issue-early/write-late), then written LDS after a barrier. Twice
// the MFMA work per barrier pair vs the BK=64 loop — the structure Tensile's
// winning MT128x128x128 configs use on these small-K shapes.
template <typename T, typename V8, bool HAS_BIAS, int ACT, bool SAVE_PRE>
__global__ __launch_bounds__(512)
void gemm_nt_rs_kernel(const T* __restrict__ A, const T* __restrict__ W,
                       const T* __restrict__ bias, T* __restrict__ C,
                       T* __restrict__ pre, long M, long N, long K,
                       int tiles_n, int nwg) {
  constexpr int BM = 128, BN = 128, BKR = 128;
  constexpr int WM = 2, WN = 4;
  constexpr int TM = BM / WM, TN = BN / WN;   // 64 x 32
  constexpr int RM = TM / 16, RN = TN / 16;   // 4 x 2

  const int wg = xcd_remap(blockIdx.x, nwg);
  const long tile_m = wg / tiles_n, tile_n = wg % tiles_n;
  const long m0 = tile_m * BM, n0 = tile_n * BN;

  __shared__ __attribute__((aligned(16))) char lds_a[BM * 256];
  __shared__ __attribute__((aligned(16))) char lds_b[BN * 256];

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wr = (wid / WN) * TM, wc = (wid % WN) * TN;

  // staging geometry: wave wid owns rows [wid*16, wid*16+16) of each tile;
  // pass p covers 4 rows (16 lanes x 16 B per row = one 256-B row quarter...
  // actually 64 lanes = 4 rows x 16 lanes x 16 B); 4 passes per tile.
  const int st_row = (lane >> 4);          // 0..3 within a pass
  const int st_byte = (lane & 15) * 16;    // 16-B piece of the 256-B row
  typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
  uint4v rega[4], regb[4];

  auto load_tile_regs = [&](long k0) {
#pragma unroll
    for (int pss = 0; pss < 4; ++pss) {
      const int r = wid * 16 + pss * 4 + st_row;
      long gra = m0 + r < M ? m0 + r : M - 1;
      long grb = n0 + r < N ? n0 + r : N - 1;
      rega[pss] = *reinterpret_cast<const uint4v*>(
          (const char*)(A + gra * K + k0) + st_byte);
      regb[pss] = *reinterpret_cast<const uint4v*>(
          (const char*)(W + grb * K + k0) + st_byte);
    }
  };
  auto write_tile_lds = [&]() {
#pragma unroll
    for (int pss = 0; pss < 4; ++pss) {
      const int r = wid * 16 + pss * 4 + st_row;
      const int byte = st_byte ^ ((r & 7) << 4);
      *reinterpret_cast<uint4v*>(lds_a + r * 256 + byte) = rega[pss];
      *reinterpret_cast<uint4v*>(lds_b + r * 256 + byte) = regb[pss];
    }
  };
  auto read_frag256 = [&](const char* lds, int frag_row0, int ks) {
    const int row = frag_row0 + (lane & 15);
    const int colbyte = (ks * 64 + (lane >> 4) * 16) ^ ((row & 7) << 4);
    return *reinterpret_cast<const V8*>(lds + row * 256 + colbyte);
  };

  f32x4 acc[RM][RN] = {};

  load_tile_regs(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  write_tile_lds();
  __syncthreads();

  const int ntiles = (int)(K / BKR);
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) load_tile_regs((long)(t + 1) * BKR);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      V8 a_frag[RM], b_frag[RN];
#pragma unroll
      for (int i = 0; i < RM; ++i)
        a_frag[i] = read_frag256(lds_a, wr + i * 16, ks);
#pragma unroll
      for (int j = 0; j < RN; ++j)
        b_frag[j] = read_frag256(lds_b, wc + j * 16, ks);
#pragma unroll
      for (int i = 0; i < RM; ++i) {
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          acc[i][j] = mfma16<V8>(a_frag[i], b_frag[j], acc[i][j]);
        }
      }
    }
    if (t + 1 < ntiles) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();            // everyone done READING the buffer
      write_tile_lds();
      __syncthreads();            // buffer refilled
    }
  }

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

// 3-buffer glds span for the 64x64 8-wave tile (the fwd/attnout workhorse;
// PMC shows its waves ~80% parked on waits): one tile stays IN FLIGHT
// across each raw barrier (counted vmcnt(4)), 48 KB LDS. Guide: +83% vs
// serial at 1 block/CU but regime-gated null at high occupancy — this
// measures which regime the 64x64w8 shape actually sits in.
template <typename T, typename V8, bool HAS_BIAS, int ACT, bool SAVE_PRE>
__global__ __launch_bounds__(512)
void gemm_nt_3b_kernel(const T* __restrict__ A, const T* __restrict__ W,
                       const T* __restrict__ bias, T* __restrict__ C,
                       T* __restrict__ pre, long M, long N, long K,
                       int tiles_n, int nwg) {
  constexpr int BM = 64, BN = 64, NW = 8;
  constexpr int WM = 2, WN = 4;
  constexpr int TM = BM / WM, TN = BN / WN;   // 32 x 16
  constexpr int RM = TM / 16, RN = TN / 16;   // 2 x 1

  const int wg = xcd_remap(blockIdx.x, nwg);
  const long tile_m = wg / tiles_n, tile_n = wg % tiles_n;
  const long m0 = tile_m * BM, n0 = tile_n * BN;

  __shared__ __attribute__((aligned(16))) char lds[3][2][BM * 128];

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wr = (wid / WN) * TM, wc = (wid % WN) * TN;

  f32x4 acc[RM][RN] = {};

  const int ntiles = (int)(K / BK);
  stage_tile<T, BM, NW>(A, K, m0, M, 0, lds[0][0]);
  stage_tile<T, BN, NW>(W, K, n0, N, 0, lds[0][1]);
  if (1 < ntiles) {
    stage_tile<T, BM, NW>(A, K, m0, M, BK, lds[1][0]);
    stage_tile<T, BN, NW>(W, K, n0, N, BK, lds[1][1]);
  }

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t % 3;
    if (t + 2 < ntiles) {
      stage_tile<T, BM, NW>(A, K, m0, M, (long)(t + 2) * BK,
                            lds[(t + 2) % 3][0]);
      stage_tile<T, BN, NW>(W, K, n0, N, (long)(t + 2) * BK,
                            lds[(t + 2) % 3][1]);
    }
    // wait buffer t's 2 glds; leave the younger buffers' loads in flight
    if (t + 2 < ntiles)
      asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    else if (t + 1 < ntiles)
      asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a_frag[RM], b_frag[RN];
#pragma unroll
      for (int i = 0; i < RM; ++i)
        a_frag[i] = read_frag<V8>(lds[cur][0], wr + i * 16, ks);
#pragma unroll
      for (int j = 0; j < RN; ++j)
        b_frag[j] = read_frag<V8>(lds[cur][1], wc + j * 16, ks);
#pragma unroll
      for (int i = 0; i < RM; ++i) {
#pragma unroll
        for (int j = 0; j < RN; ++j) {
          acc[i][j] = mfma16<V8>(a_frag[i], b_frag[j], acc[i][j]);
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

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

struct TileChoice { int bm, bn; };

// pick the tile so the grid fills 256 CUs (>= ~2 WGs per CU preferred),
// falling back to the highest-intensity 128x128 when everything fills.
static TileChoice pick_tile(long M, long N) {
  if (const char* env = std::getenv("PDNLP_GEMM_TILE")) {
    int bm, bn;
    if (std::sscanf(env, "%dx%d", &bm, &bn) == 2) return {bm, bn};
  }
  auto wgs = [&](int bm, int bn) {
    return ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  };
  // swept on MI355X (profiles/r01 microbench + r02 sweep_fwd.log):
  // 128x128 only wins once the grid is deep (>=1024 WGs, or M>=8192 where
  // it beat 64x128 by 20-40% on every bert-large shape); small-K BERT
  // shapes prefer smaller tiles with more workgroups; N<=768 prefers
  // 64x64 (attnout 411 vs 261 TF).
  if (M >= 8192 && wgs(128, 128) >= 384) return {128, 128};
  if (wgs(128, 128) >= 1024) return {128, 128};
  if (N <= 768) {
    if (wgs(64, 64) >= 512) return {64, 64};
    return {64, 128};
  }
  if (wgs(64, 128) >= 512) return {64, 128};
  return {128, 128};
}

template <typename T, typename V8>
void launch_gemm(const torch::Tensor& A, const torch::Tensor& W,
                 const torch::Tensor& bias, torch::Tensor& C,
                 torch::Tensor& pre, int act, bool has_bias, bool save_pre,
                 hipStream_t stream) {
  const long M = A.size(0), K = A.size(1), N = W.size(0);
  const TileChoice tc = pick_tile(M, N);
  const int tiles_m = (int)((M + tc.bm - 1) / tc.bm);
  const int tiles_n = (int)((N + tc.bn - 1) / tc.bn);
  const int nwg = tiles_m * tiles_n;
  const T* bptr = has_bias ? (const T*)bias.data_ptr() : nullptr;
  T* pptr = save_pre ? (T*)pre.data_ptr() : nullptr;

  // 8 waves default (swept +8-15% over 4): PDNLP_GEMM_W4 reverts
  const bool w8 = std::getenv("PDNLP_GEMM_W4") == nullptr;
  // pipelined variant needs >= 3 K-tiles in flight: its prologue waits
  // vmcnt(NGLDS) assuming tile 1 was staged — at ntiles < 3 that wait is a
  // no-op over unstaged LDS, so shallow-K shapes take the 2-buffer kernel
  const bool pipe = std::getenv("PDNLP_GEMM_PIPE") != nullptr && K / BK >= 3;
  const bool b3 = std::getenv("PDNLP_GEMM_3B") != nullptr && K / BK >= 3;
  // raw-barrier 128x128 measured SLOWER at the step level on bert-large
  // (448 vs 454 samples/s) despite the 2-blocks/CU regime — unlike the TN
  // kernel, the forward epilogue writes give the tail waves useful work
  // during the drain; env opt-in only
  const bool rb128 = std::getenv("PDNLP_GEMM_RB") != nullptr;
  const bool rs = std::getenv("PDNLP_GEMM_RS") != nullptr && K % 128 == 0;
#define LAUNCH_RS(HB, ACTV, SP)                                                \
  hipLaunchKernelGGL((gemm_nt_rs_kernel<T, V8, HB, ACTV, SP>), dim3(nwg),      \
                     dim3(512), 0, stream, (const T*)A.data_ptr(),             \
                     (const T*)W.data_ptr(), bptr, (T*)C.data_ptr(), pptr,     \
                     M, N, K, tiles_n, nwg)
#define LAUNCH_P(HB, ACTV, SP, BMV, BNV)                                       \
  do {                                                                         \
    constexpr int shmem = 3 * (BMV + BNV) * 128;                               \
    static bool attr_set_##BMV##_##BNV = false;                                \
    if (!attr_set_##BMV##_##BNV) {                                             \
      hipFuncSetAttribute(                                                     \
          (const void*)&gemm_nt_pipe_kernel<T, V8, HB, ACTV, SP, BMV, BNV>,    \
          hipFuncAttributeMaxDynamicSharedMemorySize, shmem);                  \
      attr_set_##BMV##_##BNV = true;                                           \
    }                                                                          \
    hipLaunchKernelGGL((gemm_nt_pipe_kernel<T, V8, HB, ACTV, SP, BMV, BNV>),   \
                       dim3(nwg), dim3(512), shmem, stream,                    \
                       (const T*)A.data_ptr(), (const T*)W.data_ptr(), bptr,   \
                       (T*)C.data_ptr(), pptr, M, N, K, tiles_n, nwg);         \
  } while (0)
#define LAUNCH_T(HB, ACTV, SP, BMV, BNV, NWV)                                  \
  hipLaunchKernelGGL((gemm_nt_kernel<T, V8, HB, ACTV, SP, BMV, BNV, NWV>),     \
                     dim3(nwg), dim3(NWV * WAVE), 0, stream,                   \
                     (const T*)A.data_ptr(), (const T*)W.data_ptr(), bptr,     \
                     (T*)C.data_ptr(), pptr, M, N, K, tiles_n, nwg)
#define LAUNCH(HB, ACTV, SP)                                                   \
  do {                                                                         \
    if (tc.bm == 64 && tc.bn == 128) {                                         \
      if (pipe) LAUNCH_P(HB, ACTV, SP, 64, 128);                               \
      else if (w8) LAUNCH_T(HB, ACTV, SP, 64, 128, 8);                         \
      else LAUNCH_T(HB, ACTV, SP, 64, 128, 4);                                 \
    } else if (tc.bm == 128 && tc.bn == 64) LAUNCH_T(HB, ACTV, SP, 128, 64, 4);\
    else if (tc.bm == 64 && tc.bn == 64) {                                     \
      if (b3)                                                                  \
        hipLaunchKernelGGL((gemm_nt_3b_kernel<T, V8, HB, ACTV, SP>),           \
                           dim3(nwg), dim3(512), 0, stream,                    \
                           (const T*)A.data_ptr(), (const T*)W.data_ptr(),     \
                           bptr, (T*)C.data_ptr(), pptr, M, N, K, tiles_n,     \
                           nwg);                                               \
      else if (w8) LAUNCH_T(HB, ACTV, SP, 64, 64, 8);                          \
      else LAUNCH_T(HB, ACTV, SP, 64, 64, 4);                                  \
    }                                                                          \
    else if (rs) LAUNCH_RS(HB, ACTV, SP);                                      \
    else if (pipe) LAUNCH_P(HB, ACTV, SP, 128, 128);                           \
    else if (w8 && rb128)                                                      \
      hipLaunchKernelGGL((gemm_nt_kernel<T, V8, HB, ACTV, SP, 128, 128, 8,     \
                                         true>),                               \
                         dim3(nwg), dim3(8 * WAVE), 0, stream,                 \
                         (const T*)A.data_ptr(), (const T*)W.data_ptr(), bptr, \
                         (T*)C.data_ptr(), pptr, M, N, K, tiles_n, nwg);       \
    else if (w8) LAUNCH_T(HB, ACTV, SP, 128, 128, 8);                          \
    else LAUNCH_T(HB, ACTV, SP, 128, 128, 4);                                  \
  } while (0)

  if (act == ACT_NONE) {
    if (has_bias) LAUNCH(true, ACT_NONE, false);
    else LAUNCH(false, ACT_NONE, false);
  } else if (act == ACT_GELU) {
    if (has_bias) LAUNCH(true, ACT_GELU, true);
    else LAUNCH(false, ACT_GELU, true);
  } else {
    if (has_bias) LAUNCH(true, ACT_TANH, true);
    else LAUNCH(false, ACT_TANH, true);
  }
#undef LAUNCH
#undef LAUNCH_T
}

}  // namespace

std::vector<torch::Tensor> gemm_nt_fwd(torch::Tensor A, torch::Tensor W,
                                       torch::Tensor bias, std::string act) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() && W.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && W.dim() == 2 && A.size(1) == W.size(1));
  TORCH_CHECK(A.size(1) % BK == 0, "K must be a multiple of 64");
  const long M = A.size(0), N = W.size(0);
  const bool has_bias = bias.defined() && bias.numel() > 0;
  const int actv = act == "gelu" ? ACT_GELU : act == "tanh" ? ACT_TANH
                                                            : ACT_NONE;
  const bool save_pre = actv != ACT_NONE;
  auto C = torch::empty({M, N}, A.options());
  auto pre = save_pre ? torch::empty({M, N}, A.options())
                      : torch::empty({0}, A.options());
  auto stream = at::hip::getCurrentHIPStream();
  if (A.scalar_type() == torch::kBFloat16) {
    launch_gemm<__hip_bfloat16, bf16x8>(A, W, bias, C, pre, actv, has_bias,
                                        save_pre, stream);
  } else if (A.scalar_type() == torch::kHalf) {
    launch_gemm<__half, f16x8>(A, W, bias, C, pre, actv, has_bias, save_pre,
                               stream);
  } else {
    TORCH_CHECK(false, "gemm_nt_fwd: bf16/fp16 only");
  }
  return {C, pre};
}
