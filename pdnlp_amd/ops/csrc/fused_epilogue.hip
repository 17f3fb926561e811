// Fused bias + dropout + residual + LayerNorm forward/backward
// (SURVEY.md K6/K8 epilogues + K16 dropout).
//
//   out = LN(dropout(y + bias) + residual)
//
// One wavefront per row, four rows per 256-thread block, all global access
// vectorized as short4 (8 B) — hipcc does not auto-vectorize scalar bf16
// loads (guide §6 rule 2: scalar 2B loads halve effective HBM bandwidth).
// Dropout mask from a counter-based hash RNG (deterministic in
// (seed, element index), saved packed as u8x4 for backward — SURVEY.md K16).
// The pre-LN sum is saved (bf16) so backward avoids recomputing the dropout
// path. Five vendor-kernel passes in the reference (bias add, dropout,
// residual add, LN stats, LN affine) collapse to one HBM round trip.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

// seed is read from DEVICE memory (seed_base) + a per-call-site salt so the
// dropout mask changes across hipGraph replays (the host updates *seed_base
// between replays; a kernel-arg seed would be frozen into the graph).
// INFER (serving, DROP = false): only out is produced. xsum, mask, mean and
// rstd are neither allocated nor stored; the second pass forms xsum again
// from its inputs (the same two rounded adds) instead of reading it back.
template <typename T, bool DROP, bool INFER = false>
__global__ __launch_bounds__(256)
void bdrl_fwd_kernel(const T* __restrict__ y, const T* __restrict__ bias,
                     const T* __restrict__ res, const T* __restrict__ lnw,
                     const T* __restrict__ lnb, T* __restrict__ out,
                     T* __restrict__ xsum,
                     unsigned char* __restrict__ mask_out,
                     float* __restrict__ mean_out,
                     float* __restrict__ rstd_out, int H, float p, float eps,
                     const unsigned long long* __restrict__ seed_base,
                     unsigned long long salt, long R) {
  static_assert(!INFER || !DROP, "INFER is a dropout-free form");
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const unsigned long long seed = (DROP ? *seed_base : 0ull) + salt;
  const int lane = threadIdx.x & (WAVE - 1);
  const T* yr = y + row * H;
  const T* rr = res + row * H;
  T* xr = INFER ? nullptr : xsum + row * H;
  T* outr = out + row * H;
  const float inv_keep = 1.f / (1.f - p);

  // one-pass statistics of xsum - shift (see shifted_stats in common.h);
  // every lane derives the row's first xsum element the way the loop does
  float shift = to_f32<T>(yr[0]) + to_f32<T>(bias[0]);
  if (DROP) {
    const unsigned int r = hash_rng(seed, row * (unsigned long long)H);
    shift = (r * 2.3283064365386963e-10f) >= p ? shift * inv_keep : 0.f;
  }
  shift = to_f32<T>(from_f32<T>(shift + to_f32<T>(rr[0])));

  float sum = 0.f, sumsq = 0.f;
  for (int c = lane * 4; c < H; c += WAVE * 4) {
    const v4_t<T> yv = ld4(yr + c), bv = ld4(bias + c), rv = ld4(rr + c);
    v4_t<T> xv;
    uchar4 mv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float h = elem<T>(yv, j) + elem<T>(bv, j);
      if (DROP) {
        const unsigned int r =
            hash_rng(seed, row * (unsigned long long)H + c + j);
        const bool live = (r * 2.3283064365386963e-10f) >= p;
        reinterpret_cast<unsigned char*>(&mv)[j] = live;
        h = live ? h * inv_keep : 0.f;
      }
      h += elem<T>(rv, j);
      set_elem<T>(xv, j, h);
      // stats from the rounded value so they match the saved xsum exactly
      const float hs = elem<T>(xv, j) - shift;
      sum += hs;
      sumsq += hs * hs;
    }
    if (!INFER) st4(xr + c, xv);
    if (DROP) *reinterpret_cast<uchar4*>(mask_out + row * H + c) = mv;
  }
  float md, mean, rstd;  // md = mean - shift
  shifted_stats(wave_sum(sum), wave_sum(sumsq), shift, H, eps, md, mean, rstd);
  if (!INFER && lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
  for (int c = lane * 4; c < H; c += WAVE * 4) {
    const v4_t<T> wv = ld4(lnw + c), bv = ld4(lnb + c);
    v4_t<T> xv;
    if constexpr (INFER) {
      const v4_t<T> yv = ld4(yr + c), pv = ld4(bias + c), rv = ld4(rr + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float h = elem<T>(yv, j) + elem<T>(pv, j);
        h += elem<T>(rv, j);
        set_elem<T>(xv, j, h);
      }
    } else {
      xv = ld4(xr + c);
    }
    v4_t<T> ov;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xh = (elem<T>(xv, j) - shift - md) * rstd;
      set_elem<T>(ov, j, xh * elem<T>(wv, j) + elem<T>(bv, j));
    }
    st4(outr + c, ov);
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(256)
void bdrl_bwd_dx_kernel(const T* __restrict__ dout, const T* __restrict__ xsum,
                        const unsigned char* __restrict__ mask,
                        const T* __restrict__ lnw,
                        const float* __restrict__ mean,
                        const float* __restrict__ rstd, T* __restrict__ dy,
                        T* __restrict__ dres, int H, float p, long R) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const T* dor = dout + row * H;
  const T* xr = xsum + row * H;
  T* dyr = dy + row * H;
  T* drr = dres + row * H;
  const float mu = mean[row], rs = rstd[row];
  const float inv_keep = 1.f / (1.f - p);

  float s1 = 0.f, s2 = 0.f;
  for (int c = lane * 4; c < H; c += WAVE * 4) {
    const v4_t<T> dv = ld4(dor + c), xv = ld4(xr + c), wv = ld4(lnw + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dw = elem<T>(dv, j) * elem<T>(wv, j);
      const float xh = (elem<T>(xv, j) - mu) * rs;
      s1 += dw;
      s2 += dw * xh;
    }
  }
  s1 = wave_sum(s1) / H;
  s2 = wave_sum(s2) / H;
  for (int c = lane * 4; c < H; c += WAVE * 4) {
    const v4_t<T> dv = ld4(dor + c), xv = ld4(xr + c), wv = ld4(lnw + c);
    uchar4 mv;
    if (DROP) mv = *reinterpret_cast<const uchar4*>(mask + row * H + c);
    v4_t<T> dyv, drv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dw = elem<T>(dv, j) * elem<T>(wv, j);
      const float xh = (elem<T>(xv, j) - mu) * rs;
      const float dxs = rs * (dw - s1 - xh * s2);
      set_elem<T>(drv, j, dxs);
      float g = dxs;
      if (DROP)
        g = reinterpret_cast<unsigned char*>(&mv)[j] ? g * inv_keep : 0.f;
      set_elem<T>(dyv, j, g);
    }
    st4(drr + c, drv);
    st4(dyr + c, dyv);
  }
}

// LN-weight/LN-bias/projection-bias column sums in a second pass.
// v2 layout: block = 16 row-strips x 16 column-quads over a 64-column
// group — short4 (8-B) vectorized loads (the r1 one-col-per-thread scalar
// version ran ~5x off the read roofline: 2-B loads halve bandwidth and
// H threads per chunk under-fill the chip), strips folded through LDS,
// deterministic partials [chunk][3][H] for reduce_cols_cast. grid =
// (H/64, chunks) so both axes stay parallel.
// DBIAS=false drops the projection-bias sum (the dy stream and the third
// partial row): partials are [chunk][2][H]. Used when the projection's own
// dW GEMM produces that column sum (gemm_tn_colsum).
template <typename T, bool DBIAS = true>
__global__ __launch_bounds__(256)
void bdrl_bwd_dwdb_kernel(const T* __restrict__ dout,
                          const T* __restrict__ xsum,
                          const T* __restrict__ dy,
                          const float* __restrict__ mean,
                          const float* __restrict__ rstd,
                          float* __restrict__ part, long R, int H,
                          long rows_per_chunk) {
  constexpr int KINDS = DBIAS ? 3 : 2;
  __shared__ float lds[16][KINDS][64];
  const int quad = threadIdx.x & 15;   // 4-col group within the 64 cols
  const int strip = threadIdx.x >> 4;  // 0..15 row strips
  const int c0 = blockIdx.x * 64 + quad * 4;
  const long r0 = blockIdx.y * rows_per_chunk;
  const long r1 = min(r0 + rows_per_chunk, R);
  float dw[4] = {}, db[4] = {}, dbias[4] = {};
  if (c0 < H) {
    for (long r = r0 + strip; r < r1; r += 16) {
      const float mu = mean[r], rs = rstd[r];
      const v4_t<T> dv = ld4(dout + r * H + c0);
      const v4_t<T> xv = ld4(xsum + r * H + c0);
      v4_t<T> yv;
      if constexpr (DBIAS) yv = ld4(dy + r * H + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = elem<T>(dv, j);
        const float xh = (elem<T>(xv, j) - mu) * rs;
        dw[j] += d * xh;
        db[j] += d;
        if constexpr (DBIAS) dbias[j] += elem<T>(yv, j);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lds[strip][0][quad * 4 + j] = dw[j];
    lds[strip][1][quad * 4 + j] = db[j];
    if constexpr (DBIAS) lds[strip][2][quad * 4 + j] = dbias[j];
  }
  __syncthreads();
  // KINDS*64 threads fold the 16 strips: thread t -> (kind = t/64, col = t%64)
  if (threadIdx.x < KINDS * 64) {
    const int kind = threadIdx.x >> 6, col = threadIdx.x & 63;
    const int gc = blockIdx.x * 64 + col;
    if (gc < H) {
      float s = 0.f;
#pragma unroll
      for (int st = 0; st < 16; ++st) s += lds[st][kind][col];
      part[(long)blockIdx.y * KINDS * H + kind * H + gc] = s;
    }
  }
}

// ---- one-pass forms (H = NV * 256, NV <= 4) --------------------------------
// A lane owns NV vectors of 4 columns (c = lane*4 + k*256), so a whole row
// lives in the wave's registers: every load of a row is issued before the
// first use, xsum is never read back, and a wave that walks several rows
// (grid-stride) loads bias/lnw/lnb once and has the next row's loads in
// flight under the current row's arithmetic. Expressions, column ownership
// and per-lane accumulation order are those of the loop kernels above, so
// every per-row output keeps its bits. That includes which products are
// fused into an add: with every value of a row live at once the compiler
// would choose differently here than in the loops (it did, in dxs), so these
// kernels turn contraction off and write the fused operations the loop
// kernels compile to as fmaf: out = fma(xh, w, b) in the forward;
// dxs = rs * fma(-s2, xh, fma(d, w, -s1)) in the backward; every sum of
// the statistics adds a rounded product. shifted_stats keeps its own setting.
// All of this describes what the compiler in use makes of the loop kernels
// (their statistics loops, for one, stay unfused only because hs * hs and
// dw * xh become packed multiplies before contraction is tried), not a
// property of their source: tests/test_bdrl_onepass_gpu.py holds the two
// sets of kernels together, and if another compiler moves the loop kernels
// it is this list that follows them.
//
// The same goes for a product that is rounded to T. a * b rounded to fp32 and
// then to fp16 is not always the fp16 nearest to a * b, and for fp16 the
// compiler may merge the two steps into one v_fma_mixlo_f16, which rounds
// once. mul_round keeps the two roundings. The loop backward, as compiled,
// rounds dy = dxs * inv_keep once in columns j = 2, 3 of the last iteration
// of an odd trip count (H = 256, 768: the remainder of its two-iteration
// main loop) and twice everywhere else; bdrl_bwd1_kernel does the same.
// That, too, is today's code generation: should a compiler stop doing it,
// drop the single-rounding case below (one fp16 ulp in those dy).

template <typename T>
__device__ __forceinline__ T mul_round(float a, float b) {
  float g = a * b;
  asm("" : "+v"(g));  // the conversion cannot absorb the product
  return from_f32<T>(g);
}

__device__ __forceinline__ __half mul_round_once(float a, float b) {
  unsigned int r;  // the result is the low half
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
  return __ushort_as_half((unsigned short)r);
}

// INFER (serving, DROP = false): as in bdrl_fwd_kernel, only out is stored.
template <typename T, bool DROP, int NV, bool INFER = false>
__global__ __launch_bounds__(256)
void bdrl_fwd1_kernel(const T* __restrict__ y, const T* __restrict__ bias,
                      const T* __restrict__ res, const T* __restrict__ lnw,
                      const T* __restrict__ lnb, T* __restrict__ out,
                      T* __restrict__ xsum,
                      unsigned char* __restrict__ mask_out,
                      float* __restrict__ mean_out,
                      float* __restrict__ rstd_out, float p, float eps,
                      const unsigned long long* __restrict__ seed_base,
                      unsigned long long salt, long R) {
#pragma clang fp contract(off)  // see the note above: fusion is spelled out
  static_assert(!INFER || !DROP, "INFER is a dropout-free form");
  constexpr int H = NV * 256;
  const long nwaves = (long)gridDim.x * 4;
  long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const unsigned long long seed = (DROP ? *seed_base : 0ull) + salt;
  const int lane = threadIdx.x & (WAVE - 1);
  const float inv_keep = 1.f / (1.f - p);

  v4_t<T> bv[NV], wv[NV], lbv[NV], yv[NV], rv[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = lane * 4 + k * 256;
    yv[k] = ld4(y + row * H + c);
    rv[k] = ld4(res + row * H + c);
    bv[k] = ld4(bias + c);
    wv[k] = ld4(lnw + c);
    lbv[k] = ld4(lnb + c);
  }
  const float bias0 = __shfl(elem<T>(bv[0], 0), 0, WAVE);

  for (; row < R; row += nwaves) {
    // the next row's loads go out before this row's arithmetic
    const long nrow = row + nwaves;
    v4_t<T> yn[NV] = {}, rn[NV] = {};
    if (nrow < R) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int c = lane * 4 + k * 256;
        yn[k] = ld4(y + nrow * H + c);
        rn[k] = ld4(res + nrow * H + c);
      }
    }

    // shift = the row's first xsum element, derived as the loop below does
    float shift = __shfl(elem<T>(yv[0], 0), 0, WAVE) + bias0;
    if (DROP) {
      const unsigned int r = hash_rng(seed, row * (unsigned long long)H);
      shift = (r * 2.3283064365386963e-10f) >= p ? shift * inv_keep : 0.f;
    }
    shift = to_f32<T>(
        from_f32<T>(shift + __shfl(elem<T>(rv[0], 0), 0, WAVE)));

    float sum = 0.f, sumsq = 0.f;
    v4_t<T> xv[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = lane * 4 + k * 256;
      uchar4 mv;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float h = elem<T>(yv[k], j) + elem<T>(bv[k], j);
        if (DROP) {
          const unsigned int r =
              hash_rng(seed, row * (unsigned long long)H + c + j);
          const bool live = (r * 2.3283064365386963e-10f) >= p;
          reinterpret_cast<unsigned char*>(&mv)[j] = live;
          h = live ? h * inv_keep : 0.f;
        }
        h += elem<T>(rv[k], j);
        set_elem<T>(xv[k], j, h);
        const float hs = elem<T>(xv[k], j) - shift;
        sum += hs;
        sumsq += hs * hs;
      }
      if (!INFER) st4(xsum + row * H + c, xv[k]);
      if (DROP) *reinterpret_cast<uchar4*>(mask_out + row * H + c) = mv;
    }
    float md, mean, rstd;
    shifted_stats(wave_sum(sum), wave_sum(sumsq), shift, H, eps, md, mean,
                  rstd);
    if (!INFER && lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      v4_t<T> ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xh = (elem<T>(xv[k], j) - shift - md) * rstd;
        set_elem<T>(ov, j, __builtin_fmaf(xh, elem<T>(wv[k], j),
                                          elem<T>(lbv[k], j)));
      }
      st4(out + row * H + lane * 4 + k * 256, ov);
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      yv[k] = yn[k];
      rv[k] = rn[k];
    }
  }
}

// dX and the column sums in one pass. Wave w of the grid walks rows
// w, w + nwaves, ... in ascending order and keeps dlnw / dlnb (/ dbias) of
// its own columns in fp32 registers; after the row loop the BDRL_NW waves
// of a workgroup fold through LDS in wave order, one kind at a time, and the
// workgroup stores one partial row [KINDS][H] with plain stores. No atomics
// and no dependence on arrival order: bdrl_fold_kernel adds the partial
// rows in a fixed order.
constexpr int BDRL_NW = 8;

template <typename T, bool DROP, bool DBIAS, int NV>
__global__ __launch_bounds__(BDRL_NW * WAVE)
void bdrl_bwd1_kernel(const T* __restrict__ dout, const T* __restrict__ xsum,
                      const unsigned char* __restrict__ mask,
                      const T* __restrict__ lnw,
                      const float* __restrict__ mean,
                      const float* __restrict__ rstd, T* __restrict__ dy,
                      T* __restrict__ dres, float* __restrict__ part, float p,
                      long R) {
#pragma clang fp contract(off)  // see the note above: fusion is spelled out
  constexpr int H = NV * 256;
  constexpr int KINDS = DBIAS ? 3 : 2;
  __shared__ float lds[BDRL_NW][H];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const long nwaves = (long)gridDim.x * BDRL_NW;
  long row = (long)blockIdx.x * BDRL_NW + wid;
  const float inv_keep = 1.f / (1.f - p);

  float acc[3][NV][4] = {};  // dlnw, dlnb, dbias of the lane's columns
  v4_t<T> wv[NV], dv[NV], xv[NV];
  uchar4 mv[NV];
  float mu = 0.f, rs = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) wv[k] = ld4(lnw + lane * 4 + k * 256);
  if (row < R) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = lane * 4 + k * 256;
      dv[k] = ld4(dout + row * H + c);
      xv[k] = ld4(xsum + row * H + c);
      if (DROP) mv[k] = *reinterpret_cast<const uchar4*>(mask + row * H + c);
    }
    mu = mean[row];
    rs = rstd[row];
  }

  for (; row < R; row += nwaves) {
    const long nrow = row + nwaves;
    v4_t<T> dn[NV] = {}, xn[NV] = {};
    uchar4 mn[NV] = {};
    float mun = 0.f, rsn = 0.f;
    if (nrow < R) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int c = lane * 4 + k * 256;
        dn[k] = ld4(dout + nrow * H + c);
        xn[k] = ld4(xsum + nrow * H + c);
        if (DROP)
          mn[k] = *reinterpret_cast<const uchar4*>(mask + nrow * H + c);
      }
      mun = mean[nrow];
      rsn = rstd[nrow];
    }

    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dw = elem<T>(dv[k], j) * elem<T>(wv[k], j);
        const float xh = (elem<T>(xv[k], j) - mu) * rs;
        s1 += dw;
        s2 += dw * xh;
      }
    }
    s1 = wave_sum(s1) / H;
    s2 = wave_sum(s2) / H;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int c = lane * 4 + k * 256;
      v4_t<T> dyv, drv;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = elem<T>(dv[k], j);
        const float xh = (elem<T>(xv[k], j) - mu) * rs;
        const float t = __builtin_fmaf(
            -s2, xh, __builtin_fmaf(d, elem<T>(wv[k], j), -s1));
        const T dr = mul_round<T>(rs, t);
        T g = dr;
        if (DROP) {
          const float dxs = rs * t;
          g = mul_round<T>(dxs, inv_keep);
          if constexpr (std::is_same<T, __half>::value)
            if ((NV & 1) && k == NV - 1 && j >= 2)
              g = mul_round_once(dxs, inv_keep);
          if (!reinterpret_cast<unsigned char*>(&mv[k])[j])
            g = from_f32<T>(0.f);
        }
        reinterpret_cast<T*>(&drv)[j] = dr;
        reinterpret_cast<T*>(&dyv)[j] = g;
        acc[0][k][j] = __builtin_fmaf(d, xh, acc[0][k][j]);
        acc[1][k][j] += d;
        // the rounded dy, so dbias is the column sum of the returned dy
        if constexpr (DBIAS) acc[2][k][j] += elem<T>(dyv, j);
      }
      st4(dres + row * H + c, drv);
      st4(dy + row * H + c, dyv);
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      dv[k] = dn[k];
      xv[k] = xn[k];
      mv[k] = mn[k];
    }
    mu = mun;
    rs = rsn;
  }

  // a wave without rows contributes zeros
#pragma unroll
  for (int kind = 0; kind < KINDS; ++kind) {
    if (kind) __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k)
      *reinterpret_cast<float4*>(&lds[wid][lane * 4 + k * 256]) =
          make_float4(acc[kind][k][0], acc[kind][k][1], acc[kind][k][2],
                      acc[kind][k][3]);
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += BDRL_NW * WAVE) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < BDRL_NW; ++w) s += lds[w][c];
      part[((long)blockIdx.x * KINDS + kind) * H + c] = s;
    }
  }
}

// fold [chunks, C] fp32 partial rows into [C] of T for bdrl_bwd1_kernel
// (C = KINDS * H, a multiple of 256). reduce_cols_cast_kernel walks the chunk
// axis 4 ways with dword loads, chunks / 4 dependent steps in a few dozen
// blocks; with up to one partial row per CU this one takes 32 columns x 32
// strips per block with 16-byte loads: lanes 8 apart in a wave hold the same
// columns of different strips and fold by xor-shuffle, the four waves
// through LDS. The order is fixed.
template <typename T>
__global__ __launch_bounds__(256)
void bdrl_fold_kernel(const float* __restrict__ part, T* __restrict__ out,
                      int C, int chunks) {
  __shared__ float lds[4][32];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int quad = lane & 7;
  const int strip = wid * 8 + (lane >> 3);  // 0..31
  const int c = blockIdx.x * 32 + quad * 4;
  float s[4] = {};
  for (int i = strip; i < chunks; i += 32) {
    const float4 v = *reinterpret_cast<const float4*>(part + (long)i * C + c);
    s[0] += v.x;
    s[1] += v.y;
    s[2] += v.z;
    s[3] += v.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int off = 8; off < WAVE; off <<= 1) s[j] += __shfl_xor(s[j], off, WAVE);
    if (lane < 8) lds[wid][quad * 4 + j] = s[j];
  }
  __syncthreads();
  if (threadIdx.x < 32)
    out[blockIdx.x * 32 + threadIdx.x] = from_f32<T>(
        lds[0][threadIdx.x] + lds[1][threadIdx.x] + lds[2][threadIdx.x] +
        lds[3][threadIdx.x]);
}

// run f(std::integral_constant<int, nv>) for nv = 1..4
template <typename F>
void dispatch_nv(int nv, F&& f) {
  switch (nv) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: TORCH_CHECK(false, "bdrl: hidden size must be 256..1024");
  }
}

// PDNLP_BDRL_2PASS (read per call) keeps the loop kernels: the A/B baseline
// and the reference of tests/test_bdrl_onepass_gpu.py
bool bdrl_two_pass() { return getenv("PDNLP_BDRL_2PASS") != nullptr; }

}  // namespace

std::vector<torch::Tensor> bias_dropout_residual_ln_fwd(
    torch::Tensor y, torch::Tensor bias, torch::Tensor res, torch::Tensor lnw,
    torch::Tensor lnb, double p, double eps, torch::Tensor seed_buf,
    long salt) {
  const int H = y.size(-1);
  const long R = y.numel() / H;
  TORCH_CHECK(H % 4 == 0, "bdrl: hidden size must be a multiple of 4");
  auto out = torch::empty_like(y);
  auto xsum = torch::empty_like(y);
  const bool drop = p > 0.0;
  TORCH_CHECK(!drop || (seed_buf.defined() && seed_buf.numel() >= 1 &&
                        seed_buf.is_cuda() &&
                        seed_buf.scalar_type() == torch::kLong),
              "dropout needs a cuda int64 seed buffer");
  auto mask = drop
      ? torch::empty({R, (long)H}, y.options().dtype(torch::kUInt8))
      : torch::empty({0}, y.options().dtype(torch::kUInt8));
  auto mean = torch::empty({R}, y.options().dtype(torch::kFloat32));
  auto rstd = torch::empty({R}, y.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  const long grid = (R + 3) / 4;
  if (H % 256 == 0 && H <= 1024 && !bdrl_two_pass()) {
    // up to eight workgroups of four waves per CU; past that a wave walks rows
    const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    const long grid1 = std::min(grid, 8 * cus);
    DISPATCH_FLOAT_TYPES(y.scalar_type(), "bdrl_fwd", [&] {
      DISPATCH_BOOL(drop, DROP, [&] {
        dispatch_nv(H / 256, [&](auto nv) {
          constexpr int NV = decltype(nv)::value;
          hipLaunchKernelGGL((bdrl_fwd1_kernel<scalar_t, DROP, NV>),
                             dim3(grid1), dim3(256), 0, stream,
                             (const scalar_t*)y.data_ptr(),
                             (const scalar_t*)bias.data_ptr(),
                             (const scalar_t*)res.data_ptr(),
                             (const scalar_t*)lnw.data_ptr(),
                             (const scalar_t*)lnb.data_ptr(),
                             (scalar_t*)out.data_ptr(),
                             (scalar_t*)xsum.data_ptr(),
                             DROP ? mask.data_ptr<unsigned char>() : nullptr,
                             mean.data_ptr<float>(), rstd.data_ptr<float>(),
                             (float)p, (float)eps,
                             DROP ? (const unsigned long long*)
                                        seed_buf.data_ptr()
                                  : nullptr,
                             (unsigned long long)salt, R);
        });
      });
    });
    return {out, xsum, mask, mean, rstd};
  }
  DISPATCH_FLOAT_TYPES(y.scalar_type(), "bdrl_fwd", [&] {
    DISPATCH_BOOL(drop, DROP, [&] {
      hipLaunchKernelGGL((bdrl_fwd_kernel<scalar_t, DROP>), dim3(grid),
                         dim3(256), 0, stream,
                         (const scalar_t*)y.data_ptr(),
                         (const scalar_t*)bias.data_ptr(),
                         (const scalar_t*)res.data_ptr(),
                         (const scalar_t*)lnw.data_ptr(),
                         (const scalar_t*)lnb.data_ptr(),
                         (scalar_t*)out.data_ptr(),
                         (scalar_t*)xsum.data_ptr(),
                         DROP ? mask.data_ptr<unsigned char>() : nullptr,
                         mean.data_ptr<float>(), rstd.data_ptr<float>(), H,
                         (float)p, (float)eps,
                         DROP ? (const unsigned long long*)seed_buf.data_ptr()
                              : nullptr,
                         (unsigned long long)salt, R);
    });
  });
  return {out, xsum, mask, mean, rstd};
}

// Serving form of bias_dropout_residual_ln_fwd at p = 0: the INFER
// instantiations, routed as that function routes. Returns out alone, with
// the bits of that function's out.
torch::Tensor bias_dropout_residual_ln_infer(
    torch::Tensor y, torch::Tensor bias, torch::Tensor res, torch::Tensor lnw,
    torch::Tensor lnb, double eps) {
  const int H = y.size(-1);
  const long R = y.numel() / H;
  TORCH_CHECK(H % 4 == 0, "bdrl: hidden size must be a multiple of 4");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && res.is_contiguous() &&
                  res.numel() == y.numel() &&
                  res.scalar_type() == y.scalar_type() &&
                  bias.numel() == H && lnw.numel() == H && lnb.numel() == H &&
                  bias.scalar_type() == y.scalar_type() &&
                  lnw.scalar_type() == y.scalar_type() &&
                  lnb.scalar_type() == y.scalar_type(),
              "bdrl_infer: y/residual contiguous [.., H], bias/ln_w/ln_b [H], "
              "one dtype");
  auto out = torch::empty_like(y);
  if (R == 0) return out;
  auto stream = at::hip::getCurrentHIPStream();
  const long grid = (R + 3) / 4;
  if (H % 256 == 0 && H <= 1024 && !bdrl_two_pass()) {
    const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    const long grid1 = std::min(grid, 8 * cus);
    DISPATCH_FLOAT_TYPES(y.scalar_type(), "bdrl_infer", [&] {
      dispatch_nv(H / 256, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((bdrl_fwd1_kernel<scalar_t, false, NV, true>),
                           dim3(grid1), dim3(256), 0, stream,
                           (const scalar_t*)y.data_ptr(),
                           (const scalar_t*)bias.data_ptr(),
                           (const scalar_t*)res.data_ptr(),
                           (const scalar_t*)lnw.data_ptr(),
                           (const scalar_t*)lnb.data_ptr(),
                           (scalar_t*)out.data_ptr(), (scalar_t*)nullptr,
                           (unsigned char*)nullptr, (float*)nullptr,
                           (float*)nullptr, 0.f, (float)eps,
                           (const unsigned long long*)nullptr, 0ull, R);
      });
    });
    return out;
  }
  DISPATCH_FLOAT_TYPES(y.scalar_type(), "bdrl_infer", [&] {
    hipLaunchKernelGGL((bdrl_fwd_kernel<scalar_t, false, true>), dim3(grid),
                       dim3(256), 0, stream, (const scalar_t*)y.data_ptr(),
                       (const scalar_t*)bias.data_ptr(),
                       (const scalar_t*)res.data_ptr(),
                       (const scalar_t*)lnw.data_ptr(),
                       (const scalar_t*)lnb.data_ptr(),
                       (scalar_t*)out.data_ptr(), (scalar_t*)nullptr,
                       (unsigned char*)nullptr, (float*)nullptr,
                       (float*)nullptr, H, 0.f, (float)eps,
                       (const unsigned long long*)nullptr, 0ull, R);
  });
  return out;
}

namespace {

// shared host side of the two backward entry points; returns
// {dy, dres, accT} with accT = [dlnw, dlnb(, dbias)] rows
template <bool DBIAS>
std::vector<torch::Tensor> bdrl_bwd_impl(
    torch::Tensor dout, torch::Tensor xsum, torch::Tensor mask,
    torch::Tensor lnw, torch::Tensor mean, torch::Tensor rstd, double p) {
  constexpr int KINDS = DBIAS ? 3 : 2;
  const int H = xsum.size(-1);
  const long R = xsum.numel() / H;
  TORCH_CHECK(H % 256 == 0 && H <= 1024,
              "bdrl: hidden size must be a multiple of 256 and <= 1024");
  auto dy = torch::empty_like(xsum);
  auto dres = torch::empty_like(xsum);
  auto stream = at::hip::getCurrentHIPStream();
  const bool drop = p > 0.0 && mask.numel() > 0;
  if (!bdrl_two_pass()) {
    // one workgroup of BDRL_NW waves per CU at most: that bounds the partial
    // rows (256 on MI355X) whatever R is; past it a wave walks rows
    const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    const long wgs = std::min((R + BDRL_NW - 1) / BDRL_NW, cus);
    auto part = torch::empty({wgs, (long)KINDS, (long)H},
                             xsum.options().dtype(torch::kFloat32));
    auto accT = torch::empty({(long)KINDS, (long)H}, lnw.options());
    DISPATCH_FLOAT_TYPES(xsum.scalar_type(), "bdrl_bwd", [&] {
      DISPATCH_BOOL(drop, DROP, [&] {
        dispatch_nv(H / 256, [&](auto nv) {
          constexpr int NV = decltype(nv)::value;
          hipLaunchKernelGGL((bdrl_bwd1_kernel<scalar_t, DROP, DBIAS, NV>),
                             dim3(wgs), dim3(BDRL_NW * WAVE), 0, stream,
                             (const scalar_t*)dout.data_ptr(),
                             (const scalar_t*)xsum.data_ptr(),
                             DROP ? mask.data_ptr<unsigned char>() : nullptr,
                             (const scalar_t*)lnw.data_ptr(),
                             mean.data_ptr<float>(), rstd.data_ptr<float>(),
                             (scalar_t*)dy.data_ptr(),
                             (scalar_t*)dres.data_ptr(),
                             part.data_ptr<float>(), (float)p, R);
        });
      });
      hipLaunchKernelGGL((bdrl_fold_kernel<scalar_t>),
                         dim3(KINDS * H / 32), dim3(256), 0, stream,
                         part.data_ptr<float>(), (scalar_t*)accT.data_ptr(),
                         KINDS * H, (int)wgs);
    });
    return {dy, dres, accT};
  }
  // 32 chunks: stage-1 grid = (H/64) x 32 (384+ blocks, vectorized) and
  // the strip-parallel reduce folds only 8 serial iterations per thread
  const long rows_per_chunk = (R + 31) / 32;
  const long chunks = (R + rows_per_chunk - 1) / rows_per_chunk;
  auto part = torch::empty({chunks, (long)KINDS, (long)H},
                           xsum.options().dtype(torch::kFloat32));
  auto accT = torch::empty({(long)KINDS, (long)H}, lnw.options());
  const long grid = (R + 3) / 4;
  DISPATCH_FLOAT_TYPES(xsum.scalar_type(), "bdrl_bwd", [&] {
    DISPATCH_BOOL(drop, DROP, [&] {
      hipLaunchKernelGGL((bdrl_bwd_dx_kernel<scalar_t, DROP>), dim3(grid),
                         dim3(256), 0, stream,
                         (const scalar_t*)dout.data_ptr(),
                         (const scalar_t*)xsum.data_ptr(),
                         DROP ? mask.data_ptr<unsigned char>() : nullptr,
                         (const scalar_t*)lnw.data_ptr(),
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),
                         (scalar_t*)dy.data_ptr(), (scalar_t*)dres.data_ptr(),
                         H, (float)p, R);
    });
    dim3 g2((H + 63) / 64, chunks);
    hipLaunchKernelGGL((bdrl_bwd_dwdb_kernel<scalar_t, DBIAS>), g2, dim3(256), 0,
                       stream,
                       (const scalar_t*)dout.data_ptr(),
                       (const scalar_t*)xsum.data_ptr(),
                       (const scalar_t*)dy.data_ptr(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       part.data_ptr<float>(), R, H, rows_per_chunk);
    hipLaunchKernelGGL((reduce_cols_cast_kernel<scalar_t>),
                       dim3((KINDS * H + 63) / 64), dim3(256), 0, stream,
                       part.data_ptr<float>(), (scalar_t*)accT.data_ptr(),
                       (long)(KINDS * H), (int)chunks);
  });
  return {dy, dres, accT};
}

}  // namespace

std::vector<torch::Tensor> bias_dropout_residual_ln_bwd(
    torch::Tensor dout, torch::Tensor xsum, torch::Tensor mask,
    torch::Tensor lnw, torch::Tensor mean, torch::Tensor rstd, double p) {
  auto r = bdrl_bwd_impl<true>(dout, xsum, mask, lnw, mean, rstd, p);
  return {r[0], r[2][2], r[1], r[2][0], r[2][1]};
}

// backward without the projection-bias gradient: {dy, dres, dlnw, dlnb}
std::vector<torch::Tensor> bias_dropout_residual_ln_bwd_nodb(
    torch::Tensor dout, torch::Tensor xsum, torch::Tensor mask,
    torch::Tensor lnw, torch::Tensor mean, torch::Tensor rstd, double p) {
  auto r = bdrl_bwd_impl<false>(dout, xsum, mask, lnw, mean, rstd, p);
  return {r[0], r[1], r[2][0], r[2][1]};
}
