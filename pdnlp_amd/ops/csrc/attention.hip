// Fused flash-style attention for CDNA4/gfx950 — SURVEY.md K3+K4+K5 in one
// kernel (reference: the cuBLAS batched QK^T / softmax / PV inside HF BERT,
// multi-gpu-distributed-cls.py:132-136), plus its full backward.
//
// MI355X-first design decisions:
//  - Operates DIRECTLY on the packed QKV projection output [B, S, 3H]
//    (rows of 3H elements; head h's q/k/v at columns h*64 / H+h*64 / 2H+h*64)
//    and writes a [B, S, H] context tensor — no split/transpose/contiguous
//    copies on either side of the kernel, and backward emits dqkv in the
//    same packed layout for the fused-QKV GEMM backward.
//  - Online softmax (flash-style): S×S scores never hit HBM; handles
//    S=128 (BERT-base) through S=512 (BERT-large) with the same code.
//  - MFMA v_mfma_f32_16x16x32_bf16/f16 everywhere; fp32 accumulation.
//    Block = 4 waves × 16 rows = 64-row tile; KV streamed in 64-key tiles,
//    double-buffered through LDS via global_load_lds.
//  - Attention-probability dropout is fused: mask is a counter-based hash of
//    (device-resident seed + salt, element index), recomputed bit-exactly in
//    backward — nothing saved but (o, lse). hipGraph-safe (seed read from
//    device memory; host reseeds between replays).
//  - Backward: two atomics-free passes. dQ pass owns 64-row blocks; dK/dV
//    pass owns 64-key blocks and computes S^T = K@Q^T so every GEMM is the
//    native MFMA A@B^T form. Transposed B-operands (V^T, K^T, Q^T, dO^T)
//    come from ds_read_b64_tr_b16 hardware transpose reads. Sequences of
//    at most 128 rows take ONE launch instead: fa_bwd_fused_kernel holds a
//    whole head in LDS and computes every P and dS entry once.
//
// VARLEN instantiations run the same three kernels over a padding-free
// token stream [T, 3H]: sequence b is rows cu_seqlens[b]..cu_seqlens[b+1],
// the grid is (ceil(max_seqlen/64), B*nh), a block reads its sequence bounds
// once in the prologue (never inside the KV loop) and leaves at once when
// its 64-row tile lies past the sequence end. Tail keys are masked and tail
// rows are never stored, so the zero-filled outputs stay exactly zero
// outside the sequences.
//
// TP (tile-packed) instantiations are VARLEN kernels whose blocks come from
// a device-built tile plan: one 64-row tile may hold several whole
// consecutive short sequences, and scores between them are masked inside
// the tile (see TP_COUNT below and fa_tile_plan_kernel). Opt-in; the other
// instantiations do not change.
//
// LDS image convention: every tile is a gfx950 "tr-image" (see tr_addr
// below) that serves both normal and hardware-transposed fragment reads
// from the same staging.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdlib>
#include <optional>

#include "attn_common.h"  // drop_idx, varlen_len
#include "gemm_common.h"  // vector typedefs, mfma16

namespace {

constexpr int NTHREADS = 256;  // 4 waves

template <typename T>
__device__ __forceinline__ unsigned short f32_bits16(float v) {
  T t = from_f32<T>(v);
  return *reinterpret_cast<unsigned short*>(&t);
}

// All attention tiles live in the gfx950 "tr-image" layout: a [64 m][64 c]
// tile is 8 subtiles of [32 m][16 c], element (m, c) at byte
//   2*((c&15) + (m&3)*16 + ((m>>3)&3)*64 + ((m>>2)&1)*256
//      + ((m>>5)*4 + (c>>4))*512).
// ONE image then serves BOTH fragment orientations:
//  - entity-along-m fragments (row-major consumption) read 16 contiguous
//    bytes per lane (read_n);
//  - entity-along-c fragments (transposed consumption: V^T, K^T, Q^T, dO^T)
//    use ds_read_b64_tr_b16 hardware transpose reads over the 128-B
//    [4 m][16 c] blocks (read_tr4) — no per-lane b16 gathers.

__device__ __forceinline__ int tr_addr(int m, int c) {
  return 2 * ((c & 15) + (m & 3) * 16 + ((m >> 3) & 3) * 64 +
              ((m >> 2) & 1) * 256 + ((m >> 5) * 4 + (c >> 4)) * 512);
}

// stage a [64 m][64 c] tile (row stride ld elements, rows clamped to
// max_row) into the tr-image via global_load_lds: dest element run
// l*8..l*8+7 decodes to (m_rel, c half); each lane fetches 16 contiguous
// bytes of one source row — coalesced.
template <typename T>
__device__ __forceinline__ void stage64(const T* __restrict__ src, long ld,
                                        long row0, long max_row, char* lds) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int m_rel = ((lane >> 3) & 3) * 8 + (lane >> 5) * 4 + ((lane >> 1) & 3);
  const int c0 = (lane & 1) * 8;
#pragma unroll
  for (int sidx = 0; sidx < 2; ++sidx) {
    const int sub = wid * 2 + sidx;       // subtile 0..7
    const int s_m = sub >> 2;
    const int s_c = sub & 3;
    long gr = row0 + s_m * 32 + m_rel;
    gr = gr < max_row ? gr : max_row - 1;
    const char* gp = (const char*)(src + gr * ld + s_c * 16 + c0);
    char* lp = lds + sub * 1024;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)gp,
        (__attribute__((address_space(3))) unsigned int*)lp, 16, 0, 0);
  }
}

// entity-along-m fragment: lane l holds tile[row0 + (l&15)][ks*32 +
// (l>>4)*8 + i], i = 0..7 — one 16-B read per lane (c-run stays inside one
// 16-c subtile).
template <typename V8>
__device__ __forceinline__ V8 read_n(const char* lds, int row0, int ks) {
  const int lane = threadIdx.x & (WAVE - 1);
  return *reinterpret_cast<const V8*>(
      lds + tr_addr(row0 + (lane & 15), ks * 32 + (lane >> 4) * 8));
}

// per-lane base for a hardware-transpose fragment at (ent0 on c, m_sub):
// lane-LINEAR 8-B addresses over each quarter's 128-B block.
__device__ __forceinline__ unsigned int tr_base(const char* lds, int ent0,
                                                int m_sub) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int sub = (m_sub >> 5) * 4 + (ent0 >> 4);
  return (unsigned int)(unsigned long)lds + sub * 1024 + (lane & 15) * 8 +
         (lane >> 4) * 128;
}

// four transposed fragments in ONE asm block (8x ds_read_b64_tr_b16 +
// s_waitcnt INSIDE — the compiler cannot count asm ds ops, and the outputs
// must be earlyclobber so they never alias the address inputs).
template <typename V8>
__device__ __forceinline__ void read_tr4(unsigned int b0, unsigned int b1,
                                         unsigned int b2, unsigned int b3,
                                         V8* f) {
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
      : "v"(b0), "v"(b1), "v"(b2), "v"(b3)
      : "memory");
  reinterpret_cast<uint2v*>(&f[0])[0] = r0;
  reinterpret_cast<uint2v*>(&f[0])[1] = r1;
  reinterpret_cast<uint2v*>(&f[1])[0] = r2;
  reinterpret_cast<uint2v*>(&f[1])[1] = r3;
  reinterpret_cast<uint2v*>(&f[2])[0] = r4;
  reinterpret_cast<uint2v*>(&f[2])[1] = r5;
  reinterpret_cast<uint2v*>(&f[3])[0] = r6;
  reinterpret_cast<uint2v*>(&f[3])[1] = r7;
}

// 16-lane (quarter-wave) butterfly reductions — score rows live across the
// 16 lanes that share lane>>4.
__device__ __forceinline__ float qmax(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = fmaxf(x, __shfl_xor(x, off, WAVE));
  return x;
}
__device__ __forceinline__ float qsum(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

// drop_idx (dropout counter) and varlen_len (clamped sequence length):
// attn_common.h, shared with cls_attention.hip

// Tile-packed (TP) instantiations: the VARLEN kernels over a tile plan (see
// fa_tile_plan_kernel) instead of over (sequence, tile) pairs. The plan is
// one int32 buffer that rides in the cu_seqlens argument: the item count at
// [TP_COUNT], gridDim.x items {first packed row, row count, tile, 0} from
// TP_ITEMS on, then {start, end} of every packed row's sequence. A block
// takes (row0, len, tile) from item blockIdx.x; an item of at most 64 rows
// is a group of whole consecutive sequences that share one tile, and a score
// is live only where the key lies inside the query row's own sequence.
constexpr int TP_COUNT = 0;
constexpr int TP_ITEMS = 4;

// TP prologue: {start, end} - row0 of the 64 rows of tile `tile` into LDS
// (ordinary loads, before the KV loop). Rows past the item's end hold
// clamped copies and are never stored: they get the item's own span, which
// keeps their scores finite as in the VARLEN kernels.
__device__ __forceinline__ void tp_stage_bounds(const int* plan, long row0,
                                                int len, long tile,
                                                int* bnd_lds) {
  if (threadIdx.x < 64) {
    const long g = tile * 64 + threadIdx.x;
    int lo = 0, hi = len;
    if (g < len) {
      const int* bp = plan + TP_ITEMS + 4 * (long)gridDim.x + 2 * (row0 + g);
      lo = bp[0] - (int)row0;
      hi = bp[1] - (int)row0;
      lo = lo > 0 ? lo : 0;
      hi = hi < len ? hi : len;
    }
    bnd_lds[2 * threadIdx.x] = lo;
    bnd_lds[2 * threadIdx.x + 1] = hi;
  }
}

// INFER forward: the output is not zero-filled by the host, so the rows
// outside every sequence (plan bounds start == end) are zeroed here, with no
// launch of their own. The grid is (M, nh) with M >= T/64 (both arms of
// flash_attn_tilepack_max_items are; host-checked): block (x, h) with
// x < T/64 zeroes head h's 64 columns of the free rows of stripe x, four
// lanes of 16 columns per row. No item stores a free row (items cover
// sequence rows only, clamped as the bounds are), so nothing races, and all
// of it is ordinary loads and stores before any barrier or LDS load.
template <typename T>
__device__ __forceinline__ void tp_zero_free_rows(const int* plan,
                                                  T* __restrict__ o, int T_rows,
                                                  int nh, long h) {
  const long g = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  if (g >= T_rows) return;
  const int2 be = *reinterpret_cast<const int2*>(
      plan + TP_ITEMS + 4 * (long)gridDim.x + 2 * g);
  if (be.x != be.y) return;
  uint4* dst = reinterpret_cast<uint4*>(o + g * ((long)nh * 64) + h * 64 +
                                        (threadIdx.x & 3) * 16);
  dst[0] = make_uint4(0u, 0u, 0u, 0u);
  dst[1] = make_uint4(0u, 0u, 0u, 0u);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

// INFER (serving; TP without dropout or mask only): no lse store, and the
// output arrives uninitialised instead of zero-filled, so the kernel writes
// the zero rows itself (see tp_zero_free_rows).
template <typename T, typename V8, bool HAS_MASK, bool DROP, bool PRELOAD,
          bool VARLEN, bool TP, bool INFER = false>
__global__ __launch_bounds__(NTHREADS)
void fa_fwd_kernel(const T* __restrict__ qkv, const T* __restrict__ mask,
                   T* __restrict__ o, float* __restrict__ lse,
                   const unsigned long long* __restrict__ seed_base,
                   unsigned long long salt, float scale, float p,
                   int nh, int S, const int* __restrict__ cu_seqlens) {
  scale *= 1.4426950408889634f;  // exp2 domain (log2 e)
  static_assert(!INFER || (TP && VARLEN && !DROP && !HAS_MASK),
                "INFER is a tile-packed, dropout-free, mask-free form");
  const int bh = blockIdx.y;
  const long b = TP ? 0 : bh / nh, h = TP ? bh : bh % nh;
  // before the item count is looked at: a block past it still owns a stripe
  if constexpr (INFER) tp_zero_free_rows<T>(cu_seqlens, o, S, nh, h);
  // TP: cu_seqlens carries the tile plan, blockIdx.x an item of it
  if (TP && (int)blockIdx.x >= cu_seqlens[TP_COUNT]) return;  // block-uniform
  const int* item =
      TP ? cu_seqlens + TP_ITEMS + 4 * (long)blockIdx.x : nullptr;
  const long rb = TP ? (long)item[2] : (long)blockIdx.x;
  const long H = (long)nh * 64, ld = 3 * H;
  // the block's sequence is rows [row0, row0 + len); VARLEN: S carries T
  const long row0 = TP ? (long)item[0] : VARLEN ? (long)cu_seqlens[b] : b * S;
  const int len = TP ? item[1]
                     : VARLEN ? varlen_len(cu_seqlens, b, row0, S) : S;
  if (VARLEN && rb * 64 >= len) return;  // block-uniform, before any barrier
  const long stat0 = VARLEN ? h * S + row0 : (long)bh * S;  // lse row base
  const T* qbase = qkv + row0 * ld + h * 64;
  const T* kbase = qbase + H;
  const T* vbase = qbase + 2 * H;
  T* obase = o + row0 * H + h * 64;

  __shared__ __attribute__((aligned(16))) char q_lds[64 * 128];
  __shared__ __attribute__((aligned(16))) char k_lds[2][64 * 128];
  __shared__ __attribute__((aligned(16))) char v_lds[2][64 * 128];
  __shared__ __attribute__((aligned(16))) char p_lds[64 * 128];
  // in-loop ORDINARY global loads force hipcc to wait vmcnt(0) while glds
  // are in flight (guide: mixing load kinds drains the pipeline) — the
  // mask row is hoisted to LDS in the prologue instead (host caps S<=1024)
  __shared__ T mask_lds[HAS_MASK ? 1024 : 1];

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wr = wid * 16;
  const unsigned long long seed = DROP ? (*seed_base + salt) : 0ull;
  const unsigned int seed32 = (unsigned int)(seed ^ (seed >> 32));
  const float inv_keep = DROP ? 1.f / (1.f - p) : 1.f;

  stage64<T>(qbase, ld, rb * 64, len, q_lds);
  stage64<T>(kbase, ld, 0, len, k_lds[0]);
  stage64<T>(vbase, ld, 0, len, v_lds[0]);
  if (PRELOAD && len > 64) {
    // S <= 128: the whole K/V fits the double buffers — stage everything
    // up front and run the KV loop with NO mid-loop barriers/waits
    stage64<T>(kbase, ld, 64, len, k_lds[1]);
    stage64<T>(vbase, ld, 64, len, v_lds[1]);
  }
  if (HAS_MASK)
    for (int i = threadIdx.x; i < S; i += NTHREADS)
      mask_lds[i] = mask[b * S + i];
  int* bnd_lds = nullptr;
  if constexpr (TP) {
    __shared__ int bnd_s[128];
    bnd_lds = bnd_s;
    tp_stage_bounds(cu_seqlens, row0, len, rb, bnd_lds);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float m[4], l[4];
  f32x4 acc_o[4] = {};
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
  // TP: live keys of this lane's four query rows, [klo, khi) relative to row0
  int klo[4] = {}, khi[4] = {};
  if constexpr (TP) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      klo[r] = bnd_lds[2 * (wr + (lane >> 4) * 4 + r)];
      khi[r] = bnd_lds[2 * (wr + (lane >> 4) * 4 + r) + 1];
    }
  }

  const int nt = VARLEN ? (len + 63) / 64 : S / 64;
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    if (!PRELOAD && t + 1 < nt) {
      stage64<T>(kbase, ld, (long)(t + 1) * 64, len, k_lds[cur ^ 1]);
      stage64<T>(vbase, ld, (long)(t + 1) * 64, len, v_lds[cur ^ 1]);
    }
    f32x4 acc_s[4] = {};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a = read_n<V8>(q_lds, wr, ks);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc_s[j] =
            mfma16<V8>(a, read_n<V8>(k_lds[cur], j * 16, ks), acc_s[j]);
    }
    float mv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      mv[j] = HAS_MASK
                  ? to_f32<T>(mask_lds[t * 64 + j * 16 + (lane & 15)]) *
                        1.4426950408889634f
                  : 0.f;
    float s[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j][r] = acc_s[j][r] * scale + mv[j];
        // keys past the sequence end (the staged rows there are clamped
        // copies): score -inf, so P is exactly 0. Tile t always holds at
        // least one real key, which keeps the running max finite.
        // TP: also keys of the tile's other sequences. A real row of a
        // group has itself as a key in the group's only tile, a row of a
        // long sequence has a key in every tile as above, and rows past
        // the item's end see its whole span: the running max stays finite.
        if (TP ? (t * 64 + j * 16 + (lane & 15) < klo[r] ||
                  t * 64 + j * 16 + (lane & 15) >= khi[r])
               : (VARLEN && t * 64 + j * 16 + (lane & 15) >= len))
          s[j][r] = -INFINITY;
        x = fmaxf(x, s[j][r]);
      }
      const float mn = fmaxf(m[r], qmax(x));
      const float alpha = exp2f(m[r] - mn);  // first tile: exp2(-inf) = 0
      m[r] = mn;
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j][r] = exp2f(s[j][r] - mn);
        sum += s[j][r];
      }
      l[r] = l[r] * alpha + qsum(sum);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd) acc_o[jd][r] *= alpha;
    }
    // dropout + P tile into LDS (own wave's 16 rows only)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int prow = wr + (lane >> 4) * 4 + r;
      const unsigned int grow =
          VARLEN ? (unsigned int)(stat0 + rb * 64 + prow)
                 : (unsigned int)bh * S + rb * 64 + prow;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kcol = j * 16 + (lane & 15);
        float pv = s[j][r];
        if (DROP) {
          // TP: key index inside the row's own sequence, so the masks are
          // those of the per-sequence kernels
          const unsigned int rr = hash_rng32(
              seed32, drop_idx<VARLEN>(
                          grow, t * 64 + kcol - (TP ? klo[r] : 0), S));
          pv = (rr * 2.3283064365386963e-10f) >= p ? pv * inv_keep : 0.f;
        }
        *reinterpret_cast<unsigned short*>(
            p_lds + tr_addr(prow, kcol)) =
            f32_bits16<T>(pv);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a = read_n<V8>(p_lds, wr, ks);
      V8 bv[4];
      read_tr4<V8>(tr_base(v_lds[cur], 0, ks * 32),
                   tr_base(v_lds[cur], 16, ks * 32),
                   tr_base(v_lds[cur], 32, ks * 32),
                   tr_base(v_lds[cur], 48, ks * 32), bv);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd)
        acc_o[jd] = mfma16<V8>(a, bv[jd], acc_o[jd]);
    }
    if (!PRELOAD) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    cur ^= 1;
  }

  const int ccol = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int prow = wr + (lane >> 4) * 4 + r;
    const long grow = rb * 64 + prow;
    const float invl = l[r] > 0.f ? 1.f / l[r] : 0.f;
    if (VARLEN && grow >= len) continue;  // tail rows are never stored
#pragma unroll
    for (int jd = 0; jd < 4; ++jd)
      obase[grow * H + jd * 16 + ccol] = from_f32<T>(acc_o[jd][r] * invl);
    if (!INFER && ccol == 0)
      lse[stat0 + grow] = m[r] + log2f(fmaxf(l[r], 1e-30f));
  }
}

// ---------------------------------------------------------------------------
// backward dQ: grid over 64-row blocks; recompute P from lse, stream K/V
// ---------------------------------------------------------------------------

template <typename T, typename V8, bool HAS_MASK, bool DROP, bool PRELOAD,
          bool VARLEN, bool TP>
__global__ __launch_bounds__(NTHREADS)
void fa_bwd_dq_kernel(const T* __restrict__ dout, const T* __restrict__ qkv,
                      const T* __restrict__ o, const float* __restrict__ lse,
                      float* __restrict__ dvec,
                      const T* __restrict__ mask, T* __restrict__ dqkv,
                      const unsigned long long* __restrict__ seed_base,
                      unsigned long long salt, float scale, float p,
                      int nh, int S, const int* __restrict__ cu_seqlens) {
  const float scale2 = scale * 1.4426950408889634f;  // exp2 domain
  const int bh = blockIdx.y;
  const long b = TP ? 0 : bh / nh, h = TP ? bh : bh % nh;
  // TP: cu_seqlens carries the tile plan, blockIdx.x an item of it
  if (TP && (int)blockIdx.x >= cu_seqlens[TP_COUNT]) return;  // block-uniform
  const int* item =
      TP ? cu_seqlens + TP_ITEMS + 4 * (long)blockIdx.x : nullptr;
  const long rb = TP ? (long)item[2] : (long)blockIdx.x;
  const long H = (long)nh * 64, ld = 3 * H;
  // sequence rows [row0, row0 + len), as in fa_fwd_kernel
  const long row0 = TP ? (long)item[0] : VARLEN ? (long)cu_seqlens[b] : b * S;
  const int len = TP ? item[1]
                     : VARLEN ? varlen_len(cu_seqlens, b, row0, S) : S;
  if (VARLEN && rb * 64 >= len) return;  // block-uniform, before any barrier
  const long stat0 = VARLEN ? h * S + row0 : (long)bh * S;  // lse/dvec base
  const T* qbase = qkv + row0 * ld + h * 64;
  const T* kbase = qbase + H;
  const T* vbase = qbase + 2 * H;
  const T* dobase = dout + row0 * H + h * 64;
  const T* obase = o + row0 * H + h * 64;
  T* dqbase = dqkv + row0 * ld + h * 64;

  __shared__ __attribute__((aligned(16))) char q_lds[64 * 128];
  __shared__ __attribute__((aligned(16))) char do_lds[64 * 128];
  __shared__ __attribute__((aligned(16))) char k_lds[2][64 * 128];
  __shared__ __attribute__((aligned(16))) char v_lds[2][64 * 128];
  __shared__ __attribute__((aligned(16))) char ds_lds[64 * 128];
  __shared__ float dv_s[4][16];
  __shared__ T mask_lds[HAS_MASK ? 1024 : 1];  // see fa_fwd note

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wr = wid * 16;
  const unsigned long long seed = DROP ? (*seed_base + salt) : 0ull;
  const unsigned int seed32 = (unsigned int)(seed ^ (seed >> 32));
  const float inv_keep = DROP ? 1.f / (1.f - p) : 1.f;

  stage64<T>(qbase, ld, rb * 64, len, q_lds);
  stage64<T>(dobase, H, rb * 64, len, do_lds);
  // the dS buffer is free until the KV loop: stage O through it to compute
  // Dvec = rowsum(dO * O) here (replaces the separate fa_bwd_pre kernel)
  stage64<T>(obase, H, rb * 64, len, ds_lds);
  stage64<T>(kbase, ld, 0, len, k_lds[0]);
  stage64<T>(vbase, ld, 0, len, v_lds[0]);
  if (PRELOAD && len > 64) {
    stage64<T>(kbase, ld, 64, len, k_lds[1]);
    stage64<T>(vbase, ld, 64, len, v_lds[1]);
  }
  if (HAS_MASK)
    for (int i = threadIdx.x; i < S; i += NTHREADS)
      mask_lds[i] = mask[b * S + i];
  int* bnd_lds = nullptr;
  if constexpr (TP) {
    __shared__ int bnd_s[128];
    bnd_lds = bnd_s;
    tp_stage_bounds(cu_seqlens, row0, len, rb, bnd_lds);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // TP: live keys of this lane's four query rows, as in fa_fwd_kernel
  int klo[4] = {}, khi[4] = {};
  if constexpr (TP) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      klo[r] = bnd_lds[2 * (wr + (lane >> 4) * 4 + r)];
      khi[r] = bnd_lds[2 * (wr + (lane >> 4) * 4 + r) + 1];
    }
  }
  {
    // lane l&15 accumulates row wr+(l&15) over its quarter's 8 columns
    float acc = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 dv = read_n<V8>(do_lds, wr, ks);
      V8 ov = read_n<V8>(ds_lds, wr, ks);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float a, bvv;
        if constexpr (std::is_same<V8, bf16x8>::value) {
          a = (float)((__bf16*)&dv)[i];
          bvv = (float)((__bf16*)&ov)[i];
        } else {
          a = (float)((_Float16*)&dv)[i];
          bvv = (float)((_Float16*)&ov)[i];
        }
        acc += a * bvv;
      }
    }
    acc += __shfl_xor(acc, 16, WAVE);
    acc += __shfl_xor(acc, 32, WAVE);
    if ((lane >> 4) == 0) dv_s[wid][lane & 15] = acc;
  }
  // waits for dv_s AND guards ds_lds reuse by the KV loop
  __syncthreads();
  float lse_r[4], dvec_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int prow = wr + (lane >> 4) * 4 + r;
    const long grow = rb * 64 + prow;
    // tail rows have no lse (forward never stored one): not read
    lse_r[r] = (!VARLEN || grow < len) ? lse[stat0 + grow] : 0.f;
    dvec_r[r] = dv_s[prow >> 4][prow & 15];
  }
  // one lane per row publishes Dvec for the dK/dV pass (same stream)
  if ((lane >> 4) == 0 && (!VARLEN || rb * 64 + wr + (lane & 15) < len))
    dvec[stat0 + rb * 64 + wr + (lane & 15)] = dv_s[wid][lane & 15];

  f32x4 acc_dq[4] = {};
  const int nt = VARLEN ? (len + 63) / 64 : S / 64;
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    if (!PRELOAD && t + 1 < nt) {
      stage64<T>(kbase, ld, (long)(t + 1) * 64, len, k_lds[cur ^ 1]);
      stage64<T>(vbase, ld, (long)(t + 1) * 64, len, v_lds[cur ^ 1]);
    }
    f32x4 acc_s[4] = {}, acc_dp[4] = {};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 aq = read_n<V8>(q_lds, wr, ks);
      V8 ad = read_n<V8>(do_lds, wr, ks);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc_s[j] =
            mfma16<V8>(aq, read_n<V8>(k_lds[cur], j * 16, ks), acc_s[j]);
        acc_dp[j] =
            mfma16<V8>(ad, read_n<V8>(v_lds[cur], j * 16, ks), acc_dp[j]);
      }
    }
    float mv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      mv[j] = HAS_MASK
                  ? to_f32<T>(mask_lds[t * 64 + j * 16 + (lane & 15)]) *
                        1.4426950408889634f
                  : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int prow = wr + (lane >> 4) * 4 + r;
      const unsigned int grow =
          VARLEN ? (unsigned int)(stat0 + rb * 64 + prow)
                 : (unsigned int)bh * S + rb * 64 + prow;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kcol = j * 16 + (lane & 15);
        const float pv = exp2f(acc_s[j][r] * scale2 + mv[j] - lse_r[r]);
        float dp = acc_dp[j][r];
        if (DROP) {
          const unsigned int rr = hash_rng32(
              seed32, drop_idx<VARLEN>(
                          grow, t * 64 + kcol - (TP ? klo[r] : 0), S));
          dp = (rr * 2.3283064365386963e-10f) >= p ? dp * inv_keep : 0.f;
        }
        float dsv = pv * (dp - dvec_r[r]) * scale;
        // tail keys and tail query rows: dS is 0 by index (pv there comes
        // from clamped copies, not from data). TP: keys of another
        // sequence too, where exp2(s - lse) may have overflowed.
        if (TP ? (t * 64 + kcol < klo[r] || t * 64 + kcol >= khi[r] ||
                  rb * 64 + prow >= len)
               : (VARLEN && (t * 64 + kcol >= len || rb * 64 + prow >= len)))
          dsv = 0.f;
        *reinterpret_cast<unsigned short*>(
            ds_lds + tr_addr(prow, kcol)) =
            f32_bits16<T>(dsv);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a = read_n<V8>(ds_lds, wr, ks);
      V8 bk[4];
      read_tr4<V8>(tr_base(k_lds[cur], 0, ks * 32),
                   tr_base(k_lds[cur], 16, ks * 32),
                   tr_base(k_lds[cur], 32, ks * 32),
                   tr_base(k_lds[cur], 48, ks * 32), bk);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd)
        acc_dq[jd] = mfma16<V8>(a, bk[jd], acc_dq[jd]);
    }
    if (!PRELOAD) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    cur ^= 1;
  }

  const int ccol = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long grow = rb * 64 + wr + (lane >> 4) * 4 + r;
    if (VARLEN && grow >= len) continue;  // tail rows are never stored
#pragma unroll
    for (int jd = 0; jd < 4; ++jd)
      dqbase[grow * ld + jd * 16 + ccol] = from_f32<T>(acc_dq[jd][r]);
  }
}

// ---------------------------------------------------------------------------
// backward dK/dV: grid over 64-key blocks; S^T = K@Q^T so all GEMMs are A@B^T
// ---------------------------------------------------------------------------

template <typename T, typename V8, bool HAS_MASK, bool DROP, bool PRELOAD,
          bool VARLEN, bool TP>
__global__ __launch_bounds__(NTHREADS)
void fa_bwd_dkv_kernel(const T* __restrict__ dout, const T* __restrict__ qkv,
                       const T* __restrict__ /*o: consumed by the dQ pass*/,
                       const float* __restrict__ lse,
                       float* __restrict__ dvec,
                       const T* __restrict__ mask, T* __restrict__ dqkv,
                       const unsigned long long* __restrict__ seed_base,
                       unsigned long long salt, float scale, float p,
                       int nh, int S, const int* __restrict__ cu_seqlens) {
  const float scale2 = scale * 1.4426950408889634f;  // exp2 domain
  const int bh = blockIdx.y;
  const long b = TP ? 0 : bh / nh, h = TP ? bh : bh % nh;
  // TP: cu_seqlens carries the tile plan, blockIdx.x an item of it
  if (TP && (int)blockIdx.x >= cu_seqlens[TP_COUNT]) return;  // block-uniform
  const int* item =
      TP ? cu_seqlens + TP_ITEMS + 4 * (long)blockIdx.x : nullptr;
  const long kb = TP ? (long)item[2] : (long)blockIdx.x;
  const long H = (long)nh * 64, ld = 3 * H;
  // sequence rows [row0, row0 + len), as in fa_fwd_kernel
  const long row0 = TP ? (long)item[0] : VARLEN ? (long)cu_seqlens[b] : b * S;
  const int len = TP ? item[1]
                     : VARLEN ? varlen_len(cu_seqlens, b, row0, S) : S;
  if (VARLEN && kb * 64 >= len) return;  // block-uniform, before any barrier
  const long stat0 = VARLEN ? h * S + row0 : (long)bh * S;  // lse/dvec base
  const T* qbase = qkv + row0 * ld + h * 64;
  const T* kbase = qbase + H;
  const T* vbase = qbase + 2 * H;
  const T* dobase = dout + row0 * H + h * 64;
  T* dkbase = dqkv + row0 * ld + H + h * 64;
  T* dvbase = dqkv + row0 * ld + 2 * H + h * 64;

  __shared__ __attribute__((aligned(16))) char k_lds[64 * 128];
  __shared__ __attribute__((aligned(16))) char v_lds[64 * 128];
  __shared__ __attribute__((aligned(16))) char q_lds[2][64 * 128];
  __shared__ __attribute__((aligned(16))) char do_lds[2][64 * 128];
  __shared__ __attribute__((aligned(16))) char pds_lds[64 * 128];
  // lse/dvec are read per query-row inside the KV loop; as ordinary global
  // loads they force vmcnt(0) drains of the in-flight glds (guide) — hoist
  // the whole rows to LDS in the prologue (host caps S<=1024)
  __shared__ float lse_lds[1024];
  __shared__ float dvec_lds[1024];

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int kr = wid * 16;
  const unsigned long long seed = DROP ? (*seed_base + salt) : 0ull;
  const unsigned int seed32 = (unsigned int)(seed ^ (seed >> 32));
  const float inv_keep = DROP ? 1.f / (1.f - p) : 1.f;

  stage64<T>(kbase, ld, kb * 64, len, k_lds);
  stage64<T>(vbase, ld, kb * 64, len, v_lds);
  stage64<T>(qbase, ld, 0, len, q_lds[0]);
  stage64<T>(dobase, H, 0, len, do_lds[0]);
  if (PRELOAD && len > 64) {
    stage64<T>(qbase, ld, 64, len, q_lds[1]);
    stage64<T>(dobase, H, 64, len, do_lds[1]);
  }
  for (int i = threadIdx.x; i < len; i += NTHREADS) {
    lse_lds[i] = lse[stat0 + i];
    dvec_lds[i] = dvec[stat0 + i];
  }
  int* bnd_lds = nullptr;
  if constexpr (TP) {
    __shared__ int bnd_s[128];
    bnd_lds = bnd_s;
    tp_stage_bounds(cu_seqlens, row0, len, kb, bnd_lds);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // TP: the bounds of the four OWNED key rows; a query row is live for a
  // key when it lies inside the key's sequence, [klo, khi) relative to row0
  int klo[4] = {}, khi[4] = {};
  if constexpr (TP) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      klo[r] = bnd_lds[2 * (kr + (lane >> 4) * 4 + r)];
      khi[r] = bnd_lds[2 * (kr + (lane >> 4) * 4 + r) + 1];
    }
  }

  float mv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long gkey = kb * 64 + kr + (lane >> 4) * 4 + r;
    mv[r] = HAS_MASK
                ? to_f32<T>(mask[b * S + gkey]) * 1.4426950408889634f
                : 0.f;
  }

  f32x4 acc_dk[4] = {}, acc_dv[4] = {};
  const int nt = VARLEN ? (len + 63) / 64 : S / 64;
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    if (!PRELOAD && t + 1 < nt) {
      stage64<T>(qbase, ld, (long)(t + 1) * 64, len, q_lds[cur ^ 1]);
      stage64<T>(dobase, H, (long)(t + 1) * 64, len, do_lds[cur ^ 1]);
    }
    // S^T = K @ Q^T and dP^T = V @ dO^T on this 64-query tile
    f32x4 acc_st[4] = {}, acc_dpt[4] = {};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 ak = read_n<V8>(k_lds, kr, ks);
      V8 av = read_n<V8>(v_lds, kr, ks);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc_st[j] = mfma16<V8>(
            ak, read_n<V8>(q_lds[cur], j * 16, ks), acc_st[j]);
        acc_dpt[j] = mfma16<V8>(
            av, read_n<V8>(do_lds[cur], j * 16, ks), acc_dpt[j]);
      }
    }
    float pt[4][4];
    bool live[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long qrow = (long)t * 64 + j * 16 + (lane & 15);
      const float lse_j = lse_lds[qrow];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long gkey = kb * 64 + kr + (lane >> 4) * 4 + r;
        pt[j][r] = exp2f(acc_st[j][r] * scale2 + mv[r] - lse_j);
        // tail query rows have no lse/dvec (lse_lds holds nothing there):
        // their P^T is 0 by index, never by arithmetic on that slot
        // TP: query rows of another sequence too (their lse is not this
        // key's: the exp2 above may have overflowed)
        if (TP ? (qrow < klo[r] || qrow >= khi[r]) : (VARLEN && qrow >= len))
          pt[j][r] = 0.f;
        live[j][r] = true;
        if (DROP) {
          const unsigned int grow =
              VARLEN ? (unsigned int)(stat0 + qrow)
                     : (unsigned int)bh * S + (unsigned int)qrow;
          const unsigned int rr = hash_rng32(
              seed32,
              drop_idx<VARLEN>(
                  grow, (unsigned int)(gkey - (TP ? klo[r] : 0)), S));
          live[j][r] = (rr * 2.3283064365386963e-10f) >= p;
        }
      }
    }
    // Pd^T tile -> LDS; dV += Pd^T @ dO
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int prow = kr + (lane >> 4) * 4 + r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int qcol = j * 16 + (lane & 15);
        const float pv = live[j][r] ? pt[j][r] * inv_keep : 0.f;
        *reinterpret_cast<unsigned short*>(
            pds_lds + tr_addr(prow, qcol)) =
            f32_bits16<T>(pv);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a = read_n<V8>(pds_lds, kr, ks);
      V8 bd[4];
      read_tr4<V8>(tr_base(do_lds[cur], 0, ks * 32),
                   tr_base(do_lds[cur], 16, ks * 32),
                   tr_base(do_lds[cur], 32, ks * 32),
                   tr_base(do_lds[cur], 48, ks * 32), bd);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd)
        acc_dv[jd] = mfma16<V8>(a, bd[jd], acc_dv[jd]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // dS^T tile -> LDS (same buffer); dK += dS^T @ Q
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int prow = kr + (lane >> 4) * 4 + r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long qrow = (long)t * 64 + j * 16 + (lane & 15);
        const float dvec_j = dvec_lds[qrow];
        const float dpt = live[j][r] ? acc_dpt[j][r] * inv_keep : 0.f;
        float dsv = pt[j][r] * (dpt - dvec_j) * scale;
        // dvec_j is not data there (TP: not this key's sequence)
        if (TP ? (qrow < klo[r] || qrow >= khi[r]) : (VARLEN && qrow >= len))
          dsv = 0.f;
        const int qcol = j * 16 + (lane & 15);
        *reinterpret_cast<unsigned short*>(
            pds_lds + tr_addr(prow, qcol)) =
            f32_bits16<T>(dsv);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      V8 a = read_n<V8>(pds_lds, kr, ks);
      V8 bq[4];
      read_tr4<V8>(tr_base(q_lds[cur], 0, ks * 32),
                   tr_base(q_lds[cur], 16, ks * 32),
                   tr_base(q_lds[cur], 32, ks * 32),
                   tr_base(q_lds[cur], 48, ks * 32), bq);
#pragma unroll
      for (int jd = 0; jd < 4; ++jd)
        acc_dk[jd] = mfma16<V8>(a, bq[jd], acc_dk[jd]);
    }
    if (!PRELOAD) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    cur ^= 1;
  }

  const int ccol = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long gkey = kb * 64 + kr + (lane >> 4) * 4 + r;
    if (VARLEN && gkey >= len) continue;  // tail keys are never stored
#pragma unroll
    for (int jd = 0; jd < 4; ++jd) {
      dkbase[gkey * ld + jd * 16 + ccol] = from_f32<T>(acc_dk[jd][r]);
      dvbase[gkey * ld + jd * 16 + ccol] = from_f32<T>(acc_dv[jd][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// backward, fused: sequences of at most 128 rows. One workgroup per (batch,
// head) holds Q, K, V and dO of the whole head in LDS and computes every P
// and dS entry once: S^T = K@Q^T per (key tile, query tile) pair as the dK/dV
// kernel does, dV and dK from the wave's own 16 key rows of the P^T / dS^T
// image, and dQ from the same dS^T image read transposed for the wave's own
// 16 query rows. Dvec stays in LDS; nothing goes through global memory
// between the parts. dK and dV accumulate in the dK/dV kernel's order, dQ
// over the key tiles in the dQ kernel's order.
// ---------------------------------------------------------------------------

// dynamic-LDS carve (bytes, every offset a multiple of 16; no static LDS in
// the kernel, so the dynamic base stays aligned): two tiles each of Q, K, V
// and dO, one P^T / dS^T image, then the lse, Dvec and mask rows
constexpr int FB_TILE = 64 * 128;
constexpr int FB_Q = 0;
constexpr int FB_K = 2 * FB_TILE;
constexpr int FB_V = 4 * FB_TILE;
constexpr int FB_DO = 6 * FB_TILE;
constexpr int FB_PDS = 8 * FB_TILE;
constexpr int FB_LSE = 9 * FB_TILE;
constexpr int FB_DVEC = FB_LSE + 128 * 4;
constexpr int FB_MASK = FB_DVEC + 128 * 4;
constexpr int FB_LDS_BYTES = FB_MASK + 128 * 2;  // 75008: two per CU

// two transposed fragments, as read_tr4
template <typename V8>
__device__ __forceinline__ void read_tr2(unsigned int b0, unsigned int b1,
                                         V8* f) {
  uint2v r0, r1, r2, r3;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %4\n\t"
      "ds_read_b64_tr_b16 %1, %4 offset:512\n\t"
      "ds_read_b64_tr_b16 %2, %5\n\t"
      "ds_read_b64_tr_b16 %3, %5 offset:512\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
      : "v"(b0), "v"(b1)
      : "memory");
  reinterpret_cast<uint2v*>(&f[0])[0] = r0;
  reinterpret_cast<uint2v*>(&f[0])[1] = r1;
  reinterpret_cast<uint2v*>(&f[1])[0] = r2;
  reinterpret_cast<uint2v*>(&f[1])[1] = r3;
}

// two waves per SIMD (the second __launch_bounds__ argument): the register
// budget that lets the two workgroups the LDS admits share a CU
template <typename T, typename V8, bool HAS_MASK, bool DROP, bool VARLEN>
__global__ __launch_bounds__(NTHREADS, 2)
void fa_bwd_fused_kernel(const T* __restrict__ dout, const T* __restrict__ qkv,
                         const T* __restrict__ o, const float* __restrict__ lse,
                         const T* __restrict__ mask, T* __restrict__ dqkv,
                         const unsigned long long* __restrict__ seed_base,
                         unsigned long long salt, float scale, float p,
                         int nh, int S, const int* __restrict__ cu_seqlens) {
  extern __shared__ __attribute__((aligned(16))) char fb_lds[];
  const float scale2 = scale * 1.4426950408889634f;  // exp2 domain
  const int bh = blockIdx.x;
  const long b = bh / nh, h = bh % nh;
  const long H = (long)nh * 64, ld = 3 * H;
  // sequence rows [row0, row0 + len), as in fa_fwd_kernel; the host sends
  // max_seqlen <= 128 here, and a longer sequence of a bad cu_seqlens is cut
  // to the 128 rows the LDS holds
  const long row0 = VARLEN ? (long)cu_seqlens[b] : b * S;
  int len = VARLEN ? varlen_len(cu_seqlens, b, row0, S) : S;
  len = len < 128 ? len : 128;
  if (VARLEN && len <= 0) return;  // block-uniform, before any barrier
  const int nt = (len + 63) / 64;  // 1 or 2
  const long stat0 = VARLEN ? h * S + row0 : (long)bh * S;  // lse row base
  const T* qbase = qkv + row0 * ld + h * 64;
  const T* kbase = qbase + H;
  const T* vbase = qbase + 2 * H;
  const T* dobase = dout + row0 * H + h * 64;
  const T* obase = o + row0 * H + h * 64;
  T* dqbase = dqkv + row0 * ld + h * 64;
  T* dkbase = dqbase + H;
  T* dvbase = dqbase + 2 * H;

  char* q_lds = fb_lds + FB_Q;
  char* k_lds = fb_lds + FB_K;
  char* v_lds = fb_lds + FB_V;
  char* do_lds = fb_lds + FB_DO;
  char* pds_lds = fb_lds + FB_PDS;
  float* lse_lds = reinterpret_cast<float*>(fb_lds + FB_LSE);
  float* dvec_lds = reinterpret_cast<float*>(fb_lds + FB_DVEC);
  T* mask_lds = reinterpret_cast<T*>(fb_lds + FB_MASK);

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid >> 6;
  const int wr = wid * 16;  // the wave's key rows (dK/dV) and query rows (dQ)
  const unsigned long long seed = DROP ? (*seed_base + salt) : 0ull;
  const unsigned int seed32 = (unsigned int)(seed ^ (seed >> 32));
  const float inv_keep = DROP ? 1.f / (1.f - p) : 1.f;

  // prologue: every global load of the kernel. The ordinary loads go out
  // first (lse, mask, and O in the fragment layout read_n gives dO in: lane
  // l holds O[wr + (l&15)][ks*32 + (l>>4)*8 + i], rows clamped as staging
  // clamps them), then the tiles by global_load_lds: one round trip.
  float lse_v = 0.f;
  if (tid < len) lse_v = lse[stat0 + tid];  // tail rows have no lse: not read
  T mask_v = from_f32<T>(0.f);
  if (HAS_MASK && tid < S) mask_v = mask[b * S + tid];
  V8 ov[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t < nt) {
      long r = t * 64 + wr + (lane & 15);
      r = r < len ? r : len - 1;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        ov[t][ks] = *reinterpret_cast<const V8*>(obase + r * H + ks * 32 +
                                                 (lane >> 4) * 8);
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t < nt) {
      stage64<T>(dobase, H, t * 64, len, do_lds + t * FB_TILE);
      stage64<T>(qbase, ld, t * 64, len, q_lds + t * FB_TILE);
      stage64<T>(kbase, ld, t * 64, len, k_lds + t * FB_TILE);
      stage64<T>(vbase, ld, t * 64, len, v_lds + t * FB_TILE);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (tid < 128) {
    lse_lds[tid] = lse_v;
    if (HAS_MASK) mask_lds[tid] = mask_v;
  }
  __syncthreads();

  // Dvec = rowsum(dO * O): the dQ kernel's expression and add order; lane
  // l&15 accumulates row wr+(l&15) over its quarter's 8 columns
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t < nt) {
      float acc = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        V8 dv = read_n<V8>(do_lds + t * FB_TILE, wr, ks);
        V8 o8 = ov[t][ks];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float a, bvv;
          if constexpr (std::is_same<V8, bf16x8>::value) {
            a = (float)((__bf16*)&dv)[i];
            bvv = (float)((__bf16*)&o8)[i];
          } else {
            a = (float)((_Float16*)&dv)[i];
            bvv = (float)((_Float16*)&o8)[i];
          }
          acc += a * bvv;
        }
      }
      acc += __shfl_xor(acc, 16, WAVE);
      acc += __shfl_xor(acc, 32, WAVE);
      if ((lane >> 4) == 0) dvec_lds[t * 64 + wr + (lane & 15)] = acc;
    }
  }
  __syncthreads();

  f32x4 acc_dq[2][4] = {};
  for (int kb = 0; kb < nt; ++kb) {
    const char* kt_lds = k_lds + kb * FB_TILE;
    const char* vt_lds = v_lds + kb * FB_TILE;
    float mv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      mv[r] = HAS_MASK
                  ? to_f32<T>(mask_lds[kb * 64 + wr + (lane >> 4) * 4 + r]) *
                        1.4426950408889634f
                  : 0.f;
    f32x4 acc_dk[4] = {}, acc_dv[4] = {};
    for (int t = 0; t < nt; ++t) {
      {
        const char* qt_lds = q_lds + t * FB_TILE;
        const char* dot_lds = do_lds + t * FB_TILE;
        // S^T = K @ Q^T and dP^T = V @ dO^T on this (key, query) tile pair
        f32x4 acc_st[4] = {}, acc_dpt[4] = {};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          V8 ak = read_n<V8>(kt_lds, wr, ks);
          V8 av = read_n<V8>(vt_lds, wr, ks);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc_st[j] =
                mfma16<V8>(ak, read_n<V8>(qt_lds, j * 16, ks), acc_st[j]);
            acc_dpt[j] =
                mfma16<V8>(av, read_n<V8>(dot_lds, j * 16, ks), acc_dpt[j]);
          }
        }
        float pt[4][4];
        bool live[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int qrow = t * 64 + j * 16 + (lane & 15);
          const float lse_j = lse_lds[qrow];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int gkey = kb * 64 + wr + (lane >> 4) * 4 + r;
            pt[j][r] = exp2f(acc_st[j][r] * scale2 + mv[r] - lse_j);
            // tail query rows have no lse: their P^T is 0 by index, never
            // by arithmetic on that slot
            if (VARLEN && qrow >= len) pt[j][r] = 0.f;
            live[j][r] = true;
            if (DROP) {
              const unsigned int grow =
                  VARLEN ? (unsigned int)(stat0 + qrow)
                         : (unsigned int)bh * S + (unsigned int)qrow;
              const unsigned int rr = hash_rng32(
                  seed32, drop_idx<VARLEN>(grow, (unsigned int)gkey, S));
              live[j][r] = (rr * 2.3283064365386963e-10f) >= p;
            }
          }
        }
        // the image is free once every wave has read the previous pair's
        // dS^T for its dQ
        __syncthreads();
        // Pd^T tile -> LDS; dV += Pd^T @ dO
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int prow = wr + (lane >> 4) * 4 + r;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int qcol = j * 16 + (lane & 15);
            const float pv = live[j][r] ? pt[j][r] * inv_keep : 0.f;
            *reinterpret_cast<unsigned short*>(
                pds_lds + tr_addr(prow, qcol)) =
                f32_bits16<T>(pv);
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          V8 a = read_n<V8>(pds_lds, wr, ks);
          V8 bd[4];
          read_tr4<V8>(tr_base(dot_lds, 0, ks * 32),
                       tr_base(dot_lds, 16, ks * 32),
                       tr_base(dot_lds, 32, ks * 32),
                       tr_base(dot_lds, 48, ks * 32), bd);
#pragma unroll
          for (int jd = 0; jd < 4; ++jd)
            acc_dv[jd] = mfma16<V8>(a, bd[jd], acc_dv[jd]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // dS^T tile -> LDS (same buffer); dK += dS^T @ Q
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int prow = wr + (lane >> 4) * 4 + r;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int qrow = t * 64 + j * 16 + (lane & 15);
            const float dvec_j = dvec_lds[qrow];
            const float dpt = live[j][r] ? acc_dpt[j][r] * inv_keep : 0.f;
            float dsv = pt[j][r] * (dpt - dvec_j) * scale;
            // tail query rows and, for dQ, tail keys: dS is 0 by index (the
            // values there come from clamped copies, not from data)
            if (VARLEN && (qrow >= len || kb * 64 + prow >= len)) dsv = 0.f;
            const int qcol = j * 16 + (lane & 15);
            *reinterpret_cast<unsigned short*>(
                pds_lds + tr_addr(prow, qcol)) =
                f32_bits16<T>(dsv);
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          V8 a = read_n<V8>(pds_lds, wr, ks);
          V8 bq[4];
          read_tr4<V8>(tr_base(qt_lds, 0, ks * 32),
                       tr_base(qt_lds, 16, ks * 32),
                       tr_base(qt_lds, 32, ks * 32),
                       tr_base(qt_lds, 48, ks * 32), bq);
#pragma unroll
          for (int jd = 0; jd < 4; ++jd)
            acc_dk[jd] = mfma16<V8>(a, bq[jd], acc_dk[jd]);
        }
        // every wave's 16 key rows of dS^T are in the image
        __syncthreads();
        // dQ += dS @ K: the image holds dS^T [key][query], so the wave's 16
        // query rows are an entity-along-c fragment (hardware transpose)
        V8 ads[2];
        read_tr2<V8>(tr_base(pds_lds, wr, 0), tr_base(pds_lds, wr, 32), ads);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          V8 bk[4];
          read_tr4<V8>(tr_base(kt_lds, 0, ks * 32),
                       tr_base(kt_lds, 16, ks * 32),
                       tr_base(kt_lds, 32, ks * 32),
                       tr_base(kt_lds, 48, ks * 32), bk);
          // t is block-uniform: static indices keep acc_dq in registers
          if (t == 0) {
#pragma unroll
            for (int jd = 0; jd < 4; ++jd)
              acc_dq[0][jd] = mfma16<V8>(ads[ks], bk[jd], acc_dq[0][jd]);
          } else {
#pragma unroll
            for (int jd = 0; jd < 4; ++jd)
              acc_dq[1][jd] = mfma16<V8>(ads[ks], bk[jd], acc_dq[1][jd]);
          }
        }
      }
    }
    const int ccol = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long gkey = kb * 64 + wr + (lane >> 4) * 4 + r;
      if (VARLEN && gkey >= len) continue;  // tail keys are never stored
#pragma unroll
      for (int jd = 0; jd < 4; ++jd) {
        dkbase[gkey * ld + jd * 16 + ccol] = from_f32<T>(acc_dk[jd][r]);
        dvbase[gkey * ld + jd * 16 + ccol] = from_f32<T>(acc_dv[jd][r]);
      }
    }
  }

  const int ccol = lane & 15;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long grow = t * 64 + wr + (lane >> 4) * 4 + r;
        if (VARLEN && grow >= len) continue;  // tail rows are never stored
#pragma unroll
        for (int jd = 0; jd < 4; ++jd)
          dqbase[grow * ld + jd * 16 + ccol] = from_f32<T>(acc_dq[t][jd][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// tile plan of the TP instantiations: one workgroup, once per model forward
// ---------------------------------------------------------------------------

constexpr int TP_MAX_SEQS = 4096;  // cu_seqlens is staged in LDS

// Walks the sequences in order. A sequence of more than 64 rows gives one
// item per 64-row tile of itself (the live blocks of the VARLEN grid);
// consecutive sequences of at most 64 rows are collected greedily into a
// group, which closes when the next one would take it past 64 rows or is
// long, and is one item of contiguous rows [g0, g0 + n). Empty sequences
// give nothing. Lengths are clamped as varlen_len clamps them. Thread 0
// does the greedy pass over LDS; the per-row bounds are filled in parallel
// by a binary search (cu_seqlens ascending is the callers' precondition).
__global__ __launch_bounds__(NTHREADS)
void fa_tile_plan_kernel(const int* __restrict__ cu_seqlens, int B, int T,
                         int max_items, int* __restrict__ plan) {
  __shared__ int cu[TP_MAX_SEQS + 1];
  int* items = plan + TP_ITEMS;
  int* bnd = items + 4 * (long)max_items;
  for (int i = threadIdx.x; i <= B; i += NTHREADS) {
    const int c = cu_seqlens[i];
    cu[i] = c < 0 ? 0 : c > T ? T : c;
  }
  for (int i = threadIdx.x; i < 4 * max_items; i += NTHREADS) items[i] = 0;
  if (threadIdx.x < TP_ITEMS) plan[threadIdx.x] = 0;
  __syncthreads();

  for (int r = threadIdx.x; r < T; r += NTHREADS) {
    int lo = 0, hi = B + 1;  // first index whose cu is past row r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cu[mid] > r) hi = mid; else lo = mid + 1;
    }
    int s = 0, e = 0;  // rows outside every sequence: start == end
    if (lo >= 1 && lo <= B) {
      s = cu[lo - 1];
      e = cu[lo] - s > 1024 ? s + 1024 : cu[lo];
      if (r >= e) s = e = 0;
    }
    *reinterpret_cast<int2*>(bnd + 2 * (long)r) = make_int2(s, e);
  }

  if (threadIdx.x == 0) {
    int n_items = 0, g0 = 0, gn = 0;
    auto emit = [&](int r0, int n, int tile) {
      if (n_items < max_items)  // holds by the host bound; guards bad input
        *reinterpret_cast<int4*>(items + 4 * n_items) =
            make_int4(r0, n, tile, 0);
      ++n_items;
    };
    for (int b = 0; b < B; ++b) {
      const int s0 = cu[b];
      int n = cu[b + 1] - s0;
      n = n > 1024 ? 1024 : n;
      if (n <= 0) continue;
      if (n > 64) {
        if (gn) emit(g0, gn, 0);
        gn = 0;
        for (int t = 0; t * 64 < n; ++t) emit(s0, n, t);
      } else {
        if (gn && (g0 + gn != s0 || gn + n > 64)) {
          emit(g0, gn, 0);
          gn = 0;
        }
        if (!gn) g0 = s0;
        gn += n;
      }
    }
    if (gn) emit(g0, gn, 0);
    plan[TP_COUNT] = n_items < max_items ? n_items : max_items;
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

static void check_fa_args(const torch::Tensor& qkv, const torch::Tensor& mask,
                          long nh) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 3,
              "flash_attn: qkv must be contiguous [B, S, 3H]");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 ||
                  qkv.scalar_type() == torch::kHalf,
              "flash_attn: bf16/fp16 only");
  const long S = qkv.size(1);
  TORCH_CHECK(qkv.size(2) == 3 * nh * 64,
              "flash_attn: head_dim must be 64 and qkv last dim 3*nh*64");
  TORCH_CHECK(S % 64 == 0, "flash_attn: S must be a multiple of 64");
  TORCH_CHECK(S <= 1024, "flash_attn: S > 1024 unsupported (LDS-resident "
              "mask/lse/dvec rows are sized for 1024)");
  if (mask.defined() && mask.numel() > 0) {
    TORCH_CHECK(mask.is_contiguous() && mask.numel() == qkv.size(0) * S &&
                    mask.scalar_type() == qkv.scalar_type(),
                "flash_attn: mask must be contiguous [B,1,1,S] of qkv dtype");
  }
}

// Launch helpers shared by the padded and the packed (VARLEN) entry points.
// S is the padded sequence length, or the packed row count T under VARLEN;
// seq_max the longest sequence (picks PRELOAD and the grid); cu_seqlens is
// nullptr for padded batches. VARLEN instantiates HAS_MASK = false only.
struct FaLaunch {
  dim3 grid;
  hipStream_t stream;
  const unsigned long long* seed;  // nullptr without dropout
  bool has_mask, drop, preload;
};

static FaLaunch fa_launch_setup(const torch::Tensor& mask, long seq_max,
                                long batch_heads, double p,
                                const torch::Tensor& seed_buf) {
  FaLaunch L;
  L.grid = dim3((seq_max + 63) / 64, batch_heads);
  L.stream = at::hip::getCurrentHIPStream();
  L.has_mask = mask.defined() && mask.numel() > 0;
  L.drop = p > 0.0;
  L.preload = seq_max <= 128;
  TORCH_CHECK(!L.drop || (seed_buf.defined() && seed_buf.is_cuda() &&
                          seed_buf.scalar_type() == torch::kLong),
              "flash_attn: dropout needs a cuda int64 seed buffer");
  L.seed = L.drop ? (const unsigned long long*)seed_buf.data_ptr() : nullptr;
  return L;
}

// runs the lambda with scalar_t, V8, HAS_MASK, DROP and PRELOAD bound
#define FA_DISPATCH(DTYPE, L, VARLEN, ...)                                     \
  DISPATCH_FLOAT_TYPES(DTYPE, "flash_attn", [&] {                              \
    if constexpr (!std::is_same<scalar_t, float>::value) {                     \
      using V8 = std::conditional_t<                                           \
          std::is_same<scalar_t, __hip_bfloat16>::value, bf16x8, f16x8>;       \
      DISPATCH_BOOL(L.has_mask, HM_, [&] {                                     \
        constexpr bool HAS_MASK = !VARLEN && HM_;                              \
        DISPATCH_BOOL(L.drop, DROP, [&] {                                      \
          DISPATCH_BOOL(L.preload, PRELOAD, [&] { __VA_ARGS__(); });           \
        });                                                                    \
      });                                                                      \
    } else {                                                                   \
      TORCH_CHECK(false, "flash_attn: fp32 not supported");                    \
    }                                                                          \
  })

// TP (tile-packed): cu_seqlens carries the tile plan and the grid is
// (tp_items, nh), one block per plan slot and head
template <bool VARLEN, bool TP = false>
static void fa_fwd_launch(const torch::Tensor& qkv, const torch::Tensor& mask,
                          torch::Tensor& o, torch::Tensor& lse,
                          const int* cu_seqlens, long seq_max, long batch,
                          long S, long nh, double scale, double p,
                          const torch::Tensor& seed_buf, long salt,
                          long tp_items = 0) {
  FaLaunch L = fa_launch_setup(mask, seq_max, batch * nh, p, seed_buf);
  if (TP) L.grid = dim3(tp_items, nh);
  FA_DISPATCH(qkv.scalar_type(), L, VARLEN, [&] {
    hipLaunchKernelGGL(
        (fa_fwd_kernel<scalar_t, V8, HAS_MASK, DROP, PRELOAD, VARLEN, TP>), L.grid,
        dim3(NTHREADS), 0, L.stream, (const scalar_t*)qkv.data_ptr(),
        HAS_MASK ? (const scalar_t*)mask.data_ptr() : nullptr,
        (scalar_t*)o.data_ptr(), (float*)lse.data_ptr(), L.seed,
        (unsigned long long)salt, (float)scale, (float)p, (int)nh, (int)S,
        cu_seqlens);
  });
}

// Sequences of at most 128 rows (not tile-packed) take fa_bwd_fused_kernel.
// PDNLP_FA_BWD_SPLIT (read per call) keeps the two-kernel backward for them:
// the A/B baseline and the reference of tests/test_attn_bwd_fused_gpu.py.
template <bool TP>
static bool fa_bwd_fused(long seq_max) {
  return !TP && seq_max <= 128 && getenv("PDNLP_FA_BWD_SPLIT") == nullptr;
}

// the fused kernel's LDS is past the 64 KB a launch gets by default: raise
// the instantiation's limit, once per device
template <auto Kernel>
static void fa_raise_dynamic_lds(int bytes) {
  constexpr int MAX_DEV = 64;
  static bool raised[MAX_DEV] = {};
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev >= 0 && dev < MAX_DEV && raised[dev]) return;
  HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                bytes));
  if (dev >= 0 && dev < MAX_DEV) raised[dev] = true;
}

// Split path: Dvec = rowsum(dO*O) is computed inside the dQ pass (it already
// stages dO; O goes through the dS buffer) and consumed by dK/dV through
// `dvec`. Fused path (`fused`, from fa_bwd_fused): one launch, `dvec` unused
// and undefined.
template <bool VARLEN, bool TP = false>
static void fa_bwd_launch(const torch::Tensor& dout, const torch::Tensor& qkv,
                          const torch::Tensor& o, const torch::Tensor& lse,
                          const torch::Tensor& mask, torch::Tensor& dvec,
                          bool fused,
                          torch::Tensor& dqkv, const int* cu_seqlens,
                          long seq_max, long batch, long S, long nh,
                          double scale, double p,
                          const torch::Tensor& seed_buf, long salt,
                          long tp_items = 0) {
  FaLaunch L = fa_launch_setup(mask, seq_max, batch * nh, p, seed_buf);
  if (TP) L.grid = dim3(tp_items, nh);
  FA_DISPATCH(qkv.scalar_type(), L, VARLEN, [&] {
    if constexpr (!TP && PRELOAD) {
      if (fused) {
        constexpr auto kernel =
            fa_bwd_fused_kernel<scalar_t, V8, HAS_MASK, DROP, VARLEN>;
        fa_raise_dynamic_lds<kernel>(FB_LDS_BYTES);
        hipLaunchKernelGGL(
            kernel, dim3(batch * nh), dim3(NTHREADS), FB_LDS_BYTES, L.stream,
            (const scalar_t*)dout.data_ptr(), (const scalar_t*)qkv.data_ptr(),
            (const scalar_t*)o.data_ptr(), (const float*)lse.data_ptr(),
            HAS_MASK ? (const scalar_t*)mask.data_ptr() : nullptr,
            (scalar_t*)dqkv.data_ptr(), L.seed, (unsigned long long)salt,
            (float)scale, (float)p, (int)nh, (int)S, cu_seqlens);
        return;
      }
    }
    TORCH_CHECK(!fused && dvec.defined(),
                "flash_attn: the two-kernel backward needs dvec");
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(
          kernel, L.grid, dim3(NTHREADS), 0, L.stream,
          (const scalar_t*)dout.data_ptr(), (const scalar_t*)qkv.data_ptr(),
          (const scalar_t*)o.data_ptr(), (const float*)lse.data_ptr(),
          (float*)dvec.data_ptr(),
          HAS_MASK ? (const scalar_t*)mask.data_ptr() : nullptr,
          (scalar_t*)dqkv.data_ptr(), L.seed, (unsigned long long)salt,
          (float)scale, (float)p, (int)nh, (int)S, cu_seqlens);
    };
    launch(fa_bwd_dq_kernel<scalar_t, V8, HAS_MASK, DROP, PRELOAD, VARLEN, TP>);
    launch(fa_bwd_dkv_kernel<scalar_t, V8, HAS_MASK, DROP, PRELOAD, VARLEN, TP>);
  });
}

std::vector<torch::Tensor> flash_attn_qkv_fwd(torch::Tensor qkv,
                                              torch::Tensor mask, long nh,
                                              double scale, double p,
                                              torch::Tensor seed_buf,
                                              long salt) {
  check_fa_args(qkv, mask, nh);
  const long B = qkv.size(0), S = qkv.size(1), H = (long)nh * 64;
  auto o = torch::empty({B, S, H}, qkv.options());
  auto lse = torch::empty({B * nh, S}, qkv.options().dtype(torch::kFloat));
  fa_fwd_launch<false>(qkv, mask, o, lse, nullptr, S, B, S, nh, scale, p,
                       seed_buf, salt);
  return {o, lse};
}

torch::Tensor flash_attn_qkv_bwd(torch::Tensor dout, torch::Tensor qkv,
                                 torch::Tensor o, torch::Tensor lse,
                                 torch::Tensor mask, long nh, double scale,
                                 double p, torch::Tensor seed_buf, long salt) {
  check_fa_args(qkv, mask, nh);
  const long B = qkv.size(0), S = qkv.size(1);
  auto dqkv = torch::empty_like(qkv);
  const bool fused = fa_bwd_fused<false>(S);
  torch::Tensor dvec;  // global Dvec row: the two-kernel path only
  if (!fused)
    dvec = torch::empty({B * nh, S}, qkv.options().dtype(torch::kFloat));
  fa_bwd_launch<false>(dout, qkv, o, lse, mask, dvec, fused, dqkv, nullptr, S,
                       B, S, nh, scale, p, seed_buf, salt);
  return dqkv;
}

// ---------------------------------------------------------------------------
// variable-length (padding-free) entry points: qkv [T, 3H] packed stream,
// cu_seqlens int32 [B+1] on the device, max_seqlen known on the host (no
// sync). Preconditions the host cannot check without a sync and the data
// collate guarantees: cu_seqlens ascending from 0, every length in
// [1, max_seqlen], cu_seqlens[B] <= T.
// ---------------------------------------------------------------------------

static void check_fa_varlen_args(const torch::Tensor& qkv,
                                 const torch::Tensor& cu_seqlens,
                                 long max_seqlen, long nh) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 2,
              "flash_attn_varlen: qkv must be contiguous [T, 3H]");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 ||
                  qkv.scalar_type() == torch::kHalf,
              "flash_attn_varlen: bf16/fp16 only");
  TORCH_CHECK(qkv.size(1) == 3 * nh * 64,
              "flash_attn_varlen: head_dim must be 64 and qkv last dim "
              "3*nh*64");
  TORCH_CHECK(qkv.size(0) > 0 && qkv.size(0) % 64 == 0,
              "flash_attn_varlen: T must be a positive multiple of 64");
  TORCH_CHECK(nh * qkv.size(0) <= (1L << 22),
              "flash_attn_varlen: nh*T > 2^22 unsupported (32-bit dropout "
              "counter)");
  TORCH_CHECK(cu_seqlens.is_cuda() && cu_seqlens.is_contiguous() &&
                  cu_seqlens.dim() == 1 && cu_seqlens.numel() >= 2 &&
                  cu_seqlens.scalar_type() == torch::kInt,
              "flash_attn_varlen: cu_seqlens must be a contiguous cuda int32 "
              "[B+1]");
  TORCH_CHECK(max_seqlen >= 1 && max_seqlen <= 1024,
              "flash_attn_varlen: max_seqlen must be in [1, 1024] "
              "(LDS-resident lse/dvec rows are sized for 1024)");
}

std::vector<torch::Tensor> flash_attn_varlen_fwd(torch::Tensor qkv,
                                                 torch::Tensor cu_seqlens,
                                                 long max_seqlen, long nh,
                                                 double scale, double p,
                                                 torch::Tensor seed_buf,
                                                 long salt) {
  check_fa_varlen_args(qkv, cu_seqlens, max_seqlen, nh);
  const long S = qkv.size(0), B = cu_seqlens.numel() - 1, H = (long)nh * 64;
  // zero-filled: rows outside every sequence are never stored and the
  // downstream dW GEMMs contract over all T rows
  auto o = torch::zeros({S, H}, qkv.options());
  auto lse = torch::empty({nh, S}, qkv.options().dtype(torch::kFloat));
  fa_fwd_launch<true>(qkv, torch::Tensor(), o, lse,
                      (const int*)cu_seqlens.data_ptr(), max_seqlen, B, S, nh,
                      scale, p, seed_buf, salt);
  return {o, lse};
}

torch::Tensor flash_attn_varlen_bwd(torch::Tensor dout, torch::Tensor qkv,
                                    torch::Tensor o, torch::Tensor lse,
                                    torch::Tensor cu_seqlens, long max_seqlen,
                                    long nh, double scale, double p,
                                    torch::Tensor seed_buf, long salt) {
  check_fa_varlen_args(qkv, cu_seqlens, max_seqlen, nh);
  const long S = qkv.size(0), B = cu_seqlens.numel() - 1, H = (long)nh * 64;
  TORCH_CHECK(dout.is_cuda() && dout.is_contiguous() &&
                  dout.scalar_type() == qkv.scalar_type() &&
                  dout.dim() == 2 && dout.size(0) == S && dout.size(1) == H,
              "flash_attn_varlen: dout must be contiguous [T, H] of qkv "
              "dtype");
  TORCH_CHECK(o.is_contiguous() && o.sizes() == dout.sizes() &&
                  lse.is_contiguous() && lse.numel() == nh * S,
              "flash_attn_varlen: o [T, H] / lse [nh, T] from the forward");
  auto dqkv = torch::zeros_like(qkv);  // see flash_attn_varlen_fwd
  const bool fused = fa_bwd_fused<false>(max_seqlen);
  torch::Tensor dvec;  // global Dvec row: the two-kernel path only
  if (!fused) dvec = torch::empty({nh, S}, qkv.options().dtype(torch::kFloat));
  fa_bwd_launch<true>(dout, qkv, o, lse, torch::Tensor(), dvec, fused, dqkv,
                      (const int*)cu_seqlens.data_ptr(), max_seqlen, B, S, nh,
                      scale, p, seed_buf, salt);
  return dqkv;
}

// ---------------------------------------------------------------------------
// tile-packed entry points: the VARLEN kernels over a tile plan, in which a
// 64-row tile holds several whole consecutive short sequences
// ---------------------------------------------------------------------------

// Upper bound on the plan's item count from (T, B) alone; it sizes the item
// list and the attention grid, so no launch depends on the boundaries.
// Let R <= T be the rows inside sequences.
//  (a) A long sequence of L > 64 rows gives ceil(L/64) <= floor(L/64) + 1
//      items, a group is one item and holds at least one sequence, so
//      items <= floor(R/64) + (long sequences + groups) <= T/64 + B.
//  (b) A group closes only when the next short sequence would take it past
//      64 rows, so two groups in a row hold at least 65 rows together and a
//      run of k groups between long sequences holds >= 65*floor(k/2) rows:
//      k <= 2*rows/65 + 1. A long sequence has L >= 65, so its ceil(L/64)
//      <= (L + 63)/64 <= (L + 63*L/65)/64 = 2*L/65 items. With n long
//      sequences of R_l rows in all there are at most n + 1 runs and
//      n <= R_l/65, so items <= 2*R/65 + n + 1 <= 3*R/65 + 1 <= 3*T/65 + 1.
long flash_attn_tilepack_max_items(long T, long B) {
  const long a = T / 64 + B, b = 3 * T / 65 + 1;
  return std::max(1L, std::min(a, b));
}

torch::Tensor flash_attn_tilepack_plan(torch::Tensor cu_seqlens, long T) {
  TORCH_CHECK(cu_seqlens.is_cuda() && cu_seqlens.is_contiguous() &&
                  cu_seqlens.dim() == 1 && cu_seqlens.numel() >= 2 &&
                  cu_seqlens.scalar_type() == torch::kInt,
              "flash_attn_tilepack: cu_seqlens must be a contiguous cuda "
              "int32 [B+1]");
  TORCH_CHECK(T > 0 && T % 64 == 0 && T <= (1L << 22),
              "flash_attn_tilepack: total_rows must be a positive multiple "
              "of 64, at most 2^22");
  const long B = cu_seqlens.numel() - 1;
  TORCH_CHECK(B <= TP_MAX_SEQS, "flash_attn_tilepack: more than ",
              TP_MAX_SEQS, " sequences unsupported (cu_seqlens is staged in "
              "LDS)");
  const long M = flash_attn_tilepack_max_items(T, B);
  auto plan = torch::empty({TP_ITEMS + 4 * M + 2 * T}, cu_seqlens.options());
  hipLaunchKernelGGL(fa_tile_plan_kernel, dim3(1), dim3(NTHREADS), 0,
                     at::hip::getCurrentHIPStream(),
                     (const int*)cu_seqlens.data_ptr(), (int)B, (int)T, (int)M,
                     (int*)plan.data_ptr());
  return plan;
}

// item slots of a plan buffer made for T rows; rejects any other buffer
static long check_fa_tilepack_plan(const torch::Tensor& plan, long T) {
  TORCH_CHECK(plan.is_cuda() && plan.is_contiguous() && plan.dim() == 1 &&
                  plan.scalar_type() == torch::kInt,
              "flash_attn_tilepack: plan must be the contiguous cuda int32 "
              "buffer of flash_attn_tilepack_plan");
  const long rest = plan.numel() - TP_ITEMS - 2 * T;
  TORCH_CHECK(rest >= 4 && rest % 4 == 0 &&
                  rest / 4 <= flash_attn_tilepack_max_items(T, TP_MAX_SEQS),
              "flash_attn_tilepack: plan was not built for total_rows = ", T);
  return rest / 4;
}

std::vector<torch::Tensor> flash_attn_tilepack_fwd(torch::Tensor qkv,
                                                   torch::Tensor plan,
                                                   long max_seqlen, long nh,
                                                   double scale, double p,
                                                   torch::Tensor seed_buf,
                                                   long salt) {
  check_fa_varlen_args(qkv, plan, max_seqlen, nh);
  const long S = qkv.size(0), H = (long)nh * 64;
  const long M = check_fa_tilepack_plan(plan, S);
  auto o = torch::zeros({S, H}, qkv.options());  // see flash_attn_varlen_fwd
  auto lse = torch::empty({nh, S}, qkv.options().dtype(torch::kFloat));
  fa_fwd_launch<true, true>(qkv, torch::Tensor(), o, lse,
                            (const int*)plan.data_ptr(), max_seqlen, 1, S, nh,
                            scale, p, seed_buf, salt, M);
  return {o, lse};
}

torch::Tensor flash_attn_tilepack_bwd(torch::Tensor dout, torch::Tensor qkv,
                                      torch::Tensor o, torch::Tensor lse,
                                      torch::Tensor plan, long max_seqlen,
                                      long nh, double scale, double p,
                                      torch::Tensor seed_buf, long salt) {
  check_fa_varlen_args(qkv, plan, max_seqlen, nh);
  const long S = qkv.size(0), H = (long)nh * 64;
  const long M = check_fa_tilepack_plan(plan, S);
  TORCH_CHECK(dout.is_cuda() && dout.is_contiguous() &&
                  dout.scalar_type() == qkv.scalar_type() &&
                  dout.dim() == 2 && dout.size(0) == S && dout.size(1) == H,
              "flash_attn_tilepack: dout must be contiguous [T, H] of qkv "
              "dtype");
  TORCH_CHECK(o.is_contiguous() && o.sizes() == dout.sizes() &&
                  lse.is_contiguous() && lse.numel() == nh * S,
              "flash_attn_tilepack: o [T, H] / lse [nh, T] from the forward");
  auto dqkv = torch::zeros_like(qkv);  // see flash_attn_varlen_fwd
  auto dvec = torch::empty({nh, S}, qkv.options().dtype(torch::kFloat));
  fa_bwd_launch<true, true>(dout, qkv, o, lse, torch::Tensor(), dvec, false,
                            dqkv, (const int*)plan.data_ptr(), max_seqlen, 1,
                            S, nh, scale, p, seed_buf, salt, M);
  return dqkv;
}

// the four INFER instantiations: PRELOAD x {bf16, fp16}
template <typename T, typename V8>
static void fa_infer_launch(const torch::Tensor& qkv, const torch::Tensor& plan,
                            torch::Tensor& o, dim3 grid, long max_seqlen,
                            long nh, double scale) {
  DISPATCH_BOOL(max_seqlen <= 128, PRELOAD, [&] {
    hipLaunchKernelGGL(
        (fa_fwd_kernel<T, V8, false, false, PRELOAD, true, true, true>), grid,
        dim3(NTHREADS), 0, at::hip::getCurrentHIPStream(),
        (const T*)qkv.data_ptr(), (const T*)nullptr, (T*)o.data_ptr(),
        (float*)nullptr, (const unsigned long long*)nullptr, 0ull,
        (float)scale, 0.f, (int)nh, (int)qkv.size(0),
        (const int*)plan.data_ptr());
  });
}

// Serving form of flash_attn_tilepack_fwd at p = 0: the INFER instantiations.
// No lse, no fill launch: o is torch::empty (or the caller's out) and comes
// back with the bits of flash_attn_tilepack_fwd's o, zero rows included.
torch::Tensor flash_attn_tilepack_infer(torch::Tensor qkv, torch::Tensor plan,
                                        long max_seqlen, long nh, double scale,
                                        std::optional<torch::Tensor> out) {
  check_fa_varlen_args(qkv, plan, max_seqlen, nh);
  const long S = qkv.size(0), H = (long)nh * 64;
  const long M = check_fa_tilepack_plan(plan, S);
  // the zero rows of stripe x are written by blocks (x, *)
  TORCH_CHECK(M >= S / 64, "flash_attn_tilepack_infer: the plan has fewer "
              "item slots than total_rows / 64");
  torch::Tensor o;
  if (out.has_value() && out->defined()) {
    o = *out;
    TORCH_CHECK(o.is_cuda() && o.device() == qkv.device() &&
                    o.is_contiguous() &&
                    o.scalar_type() == qkv.scalar_type() && o.dim() == 2 &&
                    o.size(0) == S && o.size(1) == H,
                "flash_attn_tilepack_infer: out must be contiguous [T, H] of "
                "qkv's dtype and device");
  } else {
    o = torch::empty({S, H}, qkv.options());
  }
  const dim3 grid(M, nh);
  // bf16 or fp16: check_fa_varlen_args
  if (qkv.scalar_type() == torch::kBFloat16)
    fa_infer_launch<__hip_bfloat16, bf16x8>(qkv, plan, o, grid, max_seqlen,
                                            nh, scale);
  else
    fa_infer_launch<__half, f16x8>(qkv, plan, o, grid, max_seqlen, nh, scale);
  return o;
}
