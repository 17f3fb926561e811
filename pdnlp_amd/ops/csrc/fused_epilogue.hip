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
template <typename T, bool DROP>
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
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const unsigned long long seed = (DROP ? *seed_base : 0ull) + salt;
  const int lane = threadIdx.x & (WAVE - 1);
  const T* yr = y + row * H;
  const T* rr = res + row * H;
  T* xr = xsum + row * H;
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
    st4(xr + c, xv);
    if (DROP) *reinterpret_cast<uchar4*>(mask_out + row * H + c) = mv;
  }
  float md, mean, rstd;  // md = mean - shift
  shifted_stats(wave_sum(sum), wave_sum(sumsq), shift, H, eps, md, mean, rstd);
  if (lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
  for (int c = lane * 4; c < H; c += WAVE * 4) {
    const v4_t<T> xv = ld4(xr + c), wv = ld4(lnw + c), bv = ld4(lnb + c);
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
