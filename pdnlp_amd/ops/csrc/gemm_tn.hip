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
#include <mutex>
#include <unordered_map>

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
//
// FOLD: no second launch. Each workgroup stores its fp32 slab, publishes it
// and takes a ticket on its tile's counter; the workgroup that draws the
// tile's last ticket folds the sm slabs in slice order (the add order of
// fold_partials4, so C and CS are bit-identical to the two-launch path's)
// and writes the C tile. See "in-launch fold" below the main loop.
template <typename T, typename V8, bool RAWBAR, bool COLSUM, bool FOLD>
__global__ __launch_bounds__(512)
void gemm_tn_sk_kernel(const T* __restrict__ A, const T* __restrict__ B,
                       float* __restrict__ P, T* __restrict__ C,
                       T* __restrict__ CS, unsigned int* __restrict__ cnt,
                       long M, long N, long K, int tiles_k, int ntiles,
                       int sm, int nwg) {
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

  const int crow_off = (lane >> 4) * 4;
  const int ccol = lane & 15;
  if constexpr (COLSUM) {
    if (do_cs && ccol == 0) {
      float* PS = P + (long)sm * N * K + (long)split * N;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long n = n0 + wr + cs_q * 16 + crow_off + r;
        if (n >= N) continue;
        if constexpr (FOLD)  // handed to the folding workgroup: sc1 store
          __hip_atomic_store(PS + n, cs_acc[r], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        else
          PS[n] = cs_acc[r];
      }
    }
  }
  if constexpr (!FOLD) {
    float* Pout = P + (long)split * N * K;
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
  } else {
    // ---- in-launch fold ----------------------------------------------------
    // Slabs are private workspace in fragment order: slab (split, tile) is
    // [wave][i][j][lane] f32x4, so one wave-instruction stores 1 KiB
    // contiguous in 16-byte lanes (the host only takes this path on the full
    // 128 grid, so no bounds here).
    //
    // Hand-off without fences: every slab byte is stored write-through
    // (sc1, 16 B per lane) and drained by its wave before one lane takes
    // the tile's ticket, and every slab load of the folding workgroup is an
    // sc1 load, which no CU's L1 serves. Plain stores behind an agent-scope
    // release cost the launch more than the fold launch they replace: the
    // release writes the XCD's L2 back once per workgroup.
    constexpr long SLAB = (long)BTN * BTK;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int foff = (wid * 8 * WAVE + lane) * 16;  // bytes into a slab
    auto slab_rsrc = [&](int s) {  // wave-uniform descriptor of one slab
      return __builtin_amdgcn_make_buffer_rsrc(
          P + ((long)s * ntiles + tile) * SLAB, 0, (int)(SLAB * 4),
          0x00020000);
    };
    {
      const auto rs = slab_rsrc(split);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          __builtin_amdgcn_raw_buffer_store_b128(
              reinterpret_cast<const u32x4&>(acc[i][j]), rs,
              foff + (i * 2 + j) * WAVE * 16, 0, /*sc1*/ 16);
      }
    }
    // publish: every wave drains its stores, then one lane takes the
    // ticket. The counter wraps to 0 with the last ticket (atomic inc with
    // bound sm - 1), so it is back at 0 for the next launch whatever that
    // launch's sm is, with no reset and no epoch.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the staging LDS is idle from here on: its first word carries the
    // ticket to the other waves (no further __shared__ object)
    unsigned int* lds_ticket = reinterpret_cast<unsigned int*>(&lds_b[0][0]);
    if (threadIdx.x == 0)
      *lds_ticket = __builtin_amdgcn_atomic_inc32(
          cnt + tile, (unsigned int)(sm - 1), __ATOMIC_RELAXED, "agent");
    __syncthreads();
    if (*lds_ticket != (unsigned int)(sm - 1)) return;  // not last: done

    // last arriver: all sm slabs of the tile are in memory. Its own slab is
    // still in registers and takes its place in the slice order from there
    // (the same bits, 64 KB less to read); the branch is wave-uniform and
    // around all eight loads of a slab, not one per load.
    auto get_slab = [&](int s, f32x4 (&v)[8]) {
      if (s == split) {
#pragma unroll
        for (int f = 0; f < 8; ++f) v[f] = acc[f >> 1][f & 1];
      } else {
        const auto rs = slab_rsrc(s);
#pragma unroll
        for (int f = 0; f < 8; ++f) {
          const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(
              rs, foff + f * WAVE * 16, 0, /*sc1*/ 16);
          v[f] = reinterpret_cast<const f32x4&>(x);
        }
      }
    };
    f32x4 sum[8];
    get_slab(0, sum);
    for (int s = 1; s < sm; ++s) {
      f32x4 v[8];
      get_slab(s, v);
#pragma unroll
      for (int f = 0; f < 8; ++f) {
#pragma unroll
        for (int q = 0; q < 4; ++q) sum[f][q] += v[f][q];
      }
    }
    // through the staging LDS as a [128][128] tile of T, then full rows out
    T* lds_c = reinterpret_cast<T*>(&lds_a[0][0]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          lds_c[(wr + i * 16 + crow_off + r) * BTK + wc + j * 16 + ccol] =
              from_f32<T>(sum[i * 2 + j][r]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int q = it * 512 + threadIdx.x;  // 16-byte piece of the tile
      const int row = q >> 4, c8 = (q & 15) * 8;
      *reinterpret_cast<u32x4*>(C + (n0 + row) * K + k0 + c8) =
          *reinterpret_cast<const u32x4*>(lds_c + row * BTK + c8);
    }
    if constexpr (COLSUM) {
      if (do_cs && threadIdx.x < BTN) {
        const float* PS = P + (long)sm * N * K + n0 + threadIdx.x;
        float a = __hip_atomic_load(PS, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
        for (int s = 1; s < sm; ++s)
          a += __hip_atomic_load(PS + (long)s * N, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
        CS[n0 + threadIdx.x] = from_f32<T>(a);
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

// ---- per-tile ticket counters of the in-launch fold -------------------------
// One persistent zeroed buffer per device, TN_CNT_SLOTS regions of
// TN_CNT_TILES counters; every stream that launches the fold gets a region of
// its own, so launches that can overlap never share a counter, and launches
// on one stream are ordered. A counter returns to 0 with its tile's last
// ticket (see the kernel), so nothing is reset per call, the same counters
// serve any sm in turn, and a replayed graph finds them as a first launch
// does. The buffer is made on the first eager call; a capture that comes
// before it, a 17th stream or more tiles than a region holds get nullptr and
// take the two-launch path. A launch that dies midway leaves counters
// unbalanced, as it leaves everything else on its device.
constexpr int TN_CNT_TILES = 4096;
constexpr int TN_CNT_SLOTS = 16;

struct TnCounters {
  torch::Tensor buf;
  std::unordered_map<hipStream_t, int> slot;
};

unsigned int* tn_fold_counters(const torch::Tensor& like, hipStream_t stream,
                               int tiles2) {
  if (tiles2 > TN_CNT_TILES) return nullptr;
  static std::mutex mu;
  static auto* pool = new std::unordered_map<int, TnCounters>();  // leaked
  std::lock_guard<std::mutex> lock(mu);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_CHECK(hipStreamIsCapturing(stream, &cap));
  const int dev = like.get_device();
  auto it = pool->find(dev);
  if (it == pool->end()) {
    if (cap != hipStreamCaptureStatusNone) return nullptr;
    TnCounters c;
    c.buf = torch::zeros({(long)TN_CNT_SLOTS * TN_CNT_TILES},
                         like.options().dtype(torch::kInt32));
    // the fill runs on this stream; other streams' regions must see it too
    HIP_CHECK(hipStreamSynchronize(stream));
    it = pool->emplace(dev, std::move(c)).first;
  }
  auto& c = it->second;
  auto st = c.slot.find(stream);
  if (st == c.slot.end()) {
    if ((int)c.slot.size() >= TN_CNT_SLOTS) return nullptr;
    st = c.slot.emplace(stream, (int)c.slot.size()).first;
  }
  return reinterpret_cast<unsigned int*>(c.buf.data_ptr<int>()) +
         (long)st->second * TN_CNT_TILES;
}

// v2 launches: gemm_tn_sk_kernel, which folds its own partials into C (and
// CS when `colsum`) when it gets ticket counters `cnt`, else writes them to
// P for the fold launch behind it. `sync` picks the vmcnt(0)+__syncthreads
// schedule over the raw-barrier counted-vmcnt one.
template <typename T, typename V8>
void launch_tn_v2(const torch::Tensor& A, const torch::Tensor& B,
                  torch::Tensor& P, torch::Tensor& C, torch::Tensor& CS,
                  long M, long N, long K, int tiles2, int sm, bool colsum,
                  bool sync, unsigned int* cnt, hipStream_t stream) {
  const int nwg2 = tiles2 * sm;
  const long NK = N * K;
  const int rblocks = (int)((NK / 4 + 255) / 256);
  DISPATCH_BOOL(cnt != nullptr, FOLD, [&] {
    auto kernel =
        colsum ? (sync ? gemm_tn_sk_kernel<T, V8, false, true, FOLD>
                       : gemm_tn_sk_kernel<T, V8, true, true, FOLD>)
               : (sync ? gemm_tn_sk_kernel<T, V8, false, false, FOLD>
                       : gemm_tn_sk_kernel<T, V8, true, false, FOLD>);
    hipLaunchKernelGGL(kernel, dim3(nwg2), dim3(512), 0, stream,
                       (const T*)A.data_ptr(), (const T*)B.data_ptr(),
                       (float*)P.data_ptr(), (T*)C.data_ptr(),
                       colsum ? (T*)CS.data_ptr() : nullptr, cnt, M, N, K,
                       (int)(K / 128), tiles2, sm, nwg2);
  });
  if (cnt != nullptr) return;
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
  // the fold runs inside the GEMM launch; PDNLP_TN_FOLD2 keeps the separate
  // fold launch (the A/B baseline and the reference of the bit-identity test)
  unsigned int* cnt = getenv("PDNLP_TN_FOLD2") != nullptr
                          ? nullptr
                          : tn_fold_counters(A, stream, tiles2);
  if (bf16)
    launch_tn_v2<__hip_bfloat16, bf16x8>(A, B, P, C, CS, M, N, K, tiles2, sm,
                                         colsum, sync, cnt, stream);
  else
    launch_tn_v2<__half, f16x8>(A, B, P, C, CS, M, N, K, tiles2, sm, colsum,
                                sync, cnt, stream);
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
