// Device helpers shared by the MFMA GEMM kernels (gemm.hip: forward NT,
// gemm_nn.hip: dX, gemm_tn.hip: dW): fragment vector types, the XCD block
// remap, the MFMA dtype switch and the two LDS images with their staging
// and fragment reads.
#pragma once

#include <type_traits>

#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));

// XCD-aware bijective remap of the workgroup id (guide T1): hardware deals
// consecutive block ids round-robin over the 8 XCDs; this gives each XCD a
// contiguous chunk of tile ids instead (L2 affinity), for any nwg.
__device__ __forceinline__ int xcd_remap(int wg, int nwg) {
  const int nxcd = 8;
  const int q = nwg / nxcd, r = nwg % nxcd;
  const int xcd = wg % nxcd, idx = wg / nxcd;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// acc += a * b on one 16x16x32 MFMA, bf16 or fp16 by fragment type
template <typename V8>
__device__ __forceinline__ f32x4 mfma16(V8 a, V8 b, f32x4 c) {
  if constexpr (std::is_same<V8, bf16x8>::value)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// ---- row-major image: [ROWS][64 contraction], XOR-swizzled 128-B rows ------
// stage a ROWS x 64 tile (row stride `ld` elements) into LDS via
// global_load_lds. Linear LDS image [ROWS][128 bytes]; the XOR swizzle is
// pre-applied on the source byte offset. Each wave-instruction moves 8 rows
// (8 lanes of 16 B per row); NW waves x (ROWS/(8*NW)) calls cover ROWS rows.
template <typename T, int ROWS, int NW>
__device__ __forceinline__ void stage_tile(const T* __restrict__ src, long ld,
                                           long row0, long max_row, long k0,
                                           char* lds) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int sub_row = lane >> 3;           // 0..7
  const int piece = lane & 7;              // 16B piece within the 128B row
  const int kbyte = (piece * 16) ^ (sub_row << 4);  // source pre-swizzle
  constexpr int CPW = ROWS / (8 * NW);     // 8-row chunks per wave
#pragma unroll
  for (int c = 0; c < CPW; ++c) {
    const int r = (wid * CPW + c) * 8 + sub_row;
    long gr = row0 + r;
    gr = gr < max_row ? gr : max_row - 1;        // clamp tail (stores guard)
    const char* gp = (const char*)(src + gr * ld + k0) + kbyte;
    // LDS dest operand is WAVE-UNIFORM (start of this call's 8-row chunk);
    // hardware writes lane l at dest + l*16 = row (l>>3), piece (l&7).
    char* lp = lds + (long)(wid * CPW + c) * 8 * 128;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)gp,
        (__attribute__((address_space(3))) unsigned int*)lp, 16, 0, 0);
  }
}

// read one 16x(8k) fragment from the swizzled LDS image
template <typename V8>
__device__ __forceinline__ V8 read_frag(const char* lds, int frag_row0,
                                        int ks) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int row = frag_row0 + (lane & 15);
  const int colbyte = (ks * 64 + (lane >> 4) * 16) ^ ((row & 7) << 4);
  return *reinterpret_cast<const V8*>(lds + row * 128 + colbyte);
}

// ---- tr-read image: [64 m][64 cols] for transposed consumption -------------
// Operands consumed TRANSPOSED use gfx950's ds_read_b64_tr_b16 hardware
// transpose-read (guide T10) instead of per-lane b16 gathers: each 4-lane
// cluster reads 4 rows of a 4x4 bf16 block (8-B aligned) and receives the
// block column-major. The LDS image for a [32 m][16 col] subtile is
//   addr(m, c) = c + (m&3)*16 + (m>>3)*64 + ((m>>2)&1)*256 (elements),
// built directly by global_load_lds: dest element run l*8..l*8+7 decodes to
// (m_rel = ((l>>3)&3)*8 + (l>>5)*4 + ((l>>1)&3), c0 = (l&1)*8), i.e. each
// lane fetches 16 contiguous bytes of one global row — coalesced.
//
// stage a [64 m][64 cols] tile of `src` (row stride ld) into the 8-KB
// tr-read image. 8 subtiles of 512 elements; one glds wave-instruction fills
// one subtile; NW waves x (8/NW) calls cover the tile. Rows clamped to
// max_m; columns are NOT clamped (callers keep col0 + 64 in bounds).
template <typename T, int NW>
__device__ __forceinline__ void stage_tr(const T* __restrict__ src, long ld,
                                         long m0, long max_m, long col0,
                                         char* lds) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  // lane -> (m_rel within 32, c half) inside one subtile
  const int m_rel = ((lane >> 3) & 3) * 8 + (lane >> 5) * 4 + ((lane >> 1) & 3);
  const int c0 = (lane & 1) * 8;
  constexpr int SPW = 8 / NW;             // subtiles per wave
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
// outputs escape the block. Outputs are EARLYCLOBBER or LLVM aliases them
// with still-needed address inputs.
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

// two transposed fragments, same single-asm-block rule
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

// one transposed fragment
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
