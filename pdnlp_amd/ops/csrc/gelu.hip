// Bias+GELU forward and GELU/tanh backward epilogue kernels.
// Exact erf GELU (HF "gelu"). Grid-stride, 8 elements per thread iteration,
// vectorized 16-byte loads for bf16/fp16 (G13: hipcc does not auto-vectorize
// scalar bf16 loads).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

__device__ __forceinline__ float gelu_f(float x) {
  return 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
}

__device__ __forceinline__ float gelu_grad_f(float x) {
  const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
  const float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}

template <typename T>
__global__ void bias_gelu_fwd_kernel(const T* __restrict__ x,
                                     const T* __restrict__ b,
                                     T* __restrict__ y, long total, int N) {
  const long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x) * 8;
  const long stride = (long)gridDim.x * blockDim.x * 8;
  for (long i = i0; i < total; i += stride) {
    if (sizeof(T) == 2 && i + 8 <= total) {
      const v4_t<T> x0 = ld4(x + i), x1 = ld4(x + i + 4);
      v4_t<T> y0, y1;
      const int c = (int)(i % N);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        set_elem<T>(y0, j,
                    gelu_f(elem<T>(x0, j) + to_f32<T>(b[(c + j) % N])));
        set_elem<T>(y1, j,
                    gelu_f(elem<T>(x1, j) + to_f32<T>(b[(c + 4 + j) % N])));
      }
      st4(y + i, y0);
      st4(y + i + 4, y1);
    } else {
      for (long k = i; k < min(i + 8, total); ++k) {
        y[k] = from_f32<T>(gelu_f(to_f32<T>(x[k]) + to_f32<T>(b[k % N])));
      }
    }
  }
}

template <typename T>
__global__ void bias_gelu_bwd_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const T* __restrict__ b,
                                     T* __restrict__ dx, long total, int N) {
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < total; i += stride) {
    const float pre = to_f32<T>(x[i]) + to_f32<T>(b[i % N]);
    dx[i] = from_f32<T>(to_f32<T>(dy[i]) * gelu_grad_f(pre));
  }
}

// dgelu on a saved pre-activation (GEMM fused-epilogue backward) —
// grid-stride, 8 elements / 16-B loads per thread iteration
template <typename T>
__global__ void gelu_bwd_kernel(const T* __restrict__ dy,
                                const T* __restrict__ pre,
                                T* __restrict__ dx, long total) {
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  const long stride = (long)gridDim.x * blockDim.x * 8;
  for (long i = i0; i < total; i += stride) {
    if (sizeof(T) == 2 && i + 8 <= total) {
      const v4_t<T> d0 = ld4(dy + i), d1 = ld4(dy + i + 4);
      const v4_t<T> p0 = ld4(pre + i), p1 = ld4(pre + i + 4);
      v4_t<T> o0, o1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        set_elem<T>(o0, j, elem<T>(d0, j) * gelu_grad_f(elem<T>(p0, j)));
        set_elem<T>(o1, j, elem<T>(d1, j) * gelu_grad_f(elem<T>(p1, j)));
      }
      st4(dx + i, o0);
      st4(dx + i + 4, o1);
    } else {
      for (long k = i; k < min(i + 8, total); ++k)
        dx[k] = from_f32<T>(to_f32<T>(dy[k]) * gelu_grad_f(to_f32<T>(pre[k])));
    }
  }
}

template <typename T>
__global__ void tanh_bwd_kernel(const T* __restrict__ dy,
                                const T* __restrict__ pre,
                                T* __restrict__ dx, long total) {
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < total; i += stride) {
    const float t = tanhf(to_f32<T>(pre[i]));
    dx[i] = from_f32<T>(to_f32<T>(dy[i]) * (1.f - t * t));
  }
}


// plain fp32 column sum of a bf16/fp16 [R, N] matrix (projection-bias
// gradients for the fused-QKV GEMM: replaces torch's reduce_kernel)
template <typename T>
__global__ __launch_bounds__(256)
void col_sum_kernel(const T* __restrict__ x, float* __restrict__ part,
                    long R, int N, long rows_per_chunk) {
  // 16 row-strips x 16 col-quads per 64-column group (same structure as
  // bdrl_bwd_dwdb_kernel: vectorized 8-B loads, strips folded through
  // LDS, deterministic partials [chunk][N] for reduce_cols_cast)
  __shared__ float lds[16][64];
  const int quad = threadIdx.x & 15;
  const int strip = threadIdx.x >> 4;
  const int c0 = blockIdx.x * 64 + quad * 4;
  const long r0 = blockIdx.y * rows_per_chunk;
  const long r1 = min(r0 + rows_per_chunk, R);
  float s[4] = {};
  if (c0 < N) {
    for (long r = r0 + strip; r < r1; r += 16) {
      const v4_t<T> v = ld4(x + r * N + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += elem<T>(v, j);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) lds[strip][quad * 4 + j] = s[j];
  __syncthreads();
  if (threadIdx.x < 64) {
    const int gc = blockIdx.x * 64 + threadIdx.x;
    if (gc < N) {
      float acc = 0.f;
#pragma unroll
      for (int st = 0; st < 16; ++st) acc += lds[st][threadIdx.x];
      part[(long)blockIdx.y * N + gc] = acc;
    }
  }
}

int grid_for(long total, int per_thread = 1) {
  const long want = (total + 256L * per_thread - 1) / (256L * per_thread);
  return (int)std::min<long>(want, 2048);  // G11: cap + grid-stride
}

}  // namespace

torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor b) {
  auto y = torch::empty_like(x);
  const long total = x.numel();
  const int N = b.numel();
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_FLOAT_TYPES(x.scalar_type(), "bias_gelu_fwd", [&] {
    hipLaunchKernelGGL((bias_gelu_fwd_kernel<scalar_t>),
                       dim3(grid_for(total, 8)), dim3(256), 0, stream,
                       (const scalar_t*)x.data_ptr(),
                       (const scalar_t*)b.data_ptr(), (scalar_t*)y.data_ptr(),
                       total, N);
  });
  return y;
}

std::vector<torch::Tensor> bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor b) {
  auto dx = torch::empty_like(x);
  const long total = x.numel();
  const int N = b.numel();
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_FLOAT_TYPES(x.scalar_type(), "bias_gelu_bwd", [&] {
    hipLaunchKernelGGL((bias_gelu_bwd_kernel<scalar_t>),
                       dim3(grid_for(total)), dim3(256), 0, stream,
                       (const scalar_t*)dy.data_ptr(),
                       (const scalar_t*)x.data_ptr(),
                       (const scalar_t*)b.data_ptr(),
                       (scalar_t*)dx.data_ptr(), total, N);
  });
  auto db = dx.view({-1, N}).sum(0);
  return {dx, db};
}

torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor pre) {
  auto dx = torch::empty_like(dy);
  const long total = dy.numel();
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_FLOAT_TYPES(dy.scalar_type(), "gelu_bwd", [&] {
    hipLaunchKernelGGL((gelu_bwd_kernel<scalar_t>), dim3(grid_for(total, 8)),
                       dim3(256), 0, stream,
                       (const scalar_t*)dy.data_ptr(),
                       (const scalar_t*)pre.data_ptr(),
                       (scalar_t*)dx.data_ptr(), total);
  });
  return dx;
}

torch::Tensor tanh_bwd(torch::Tensor dy, torch::Tensor pre) {
  auto dx = torch::empty_like(dy);
  const long total = dy.numel();
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_FLOAT_TYPES(dy.scalar_type(), "tanh_bwd", [&] {
    hipLaunchKernelGGL((tanh_bwd_kernel<scalar_t>), dim3(grid_for(total)),
                       dim3(256), 0, stream,
                       (const scalar_t*)dy.data_ptr(),
                       (const scalar_t*)pre.data_ptr(),
                       (scalar_t*)dx.data_ptr(), total);
  });
  return dx;
}

torch::Tensor col_sum(torch::Tensor x) {
  const int N = x.size(-1);
  const long R = x.numel() / N;
  TORCH_CHECK(N % 4 == 0 && x.scalar_type() != torch::kFloat,
              "col_sum: bf16/fp16, N % 4 == 0");
  auto stream = at::hip::getCurrentHIPStream();
  const long rows_per_chunk = (R + 31) / 32;
  const long chunks = (R + rows_per_chunk - 1) / rows_per_chunk;
  auto part = torch::empty({chunks, (long)N},
                           x.options().dtype(torch::kFloat32));
  auto out = torch::empty({(long)N}, x.options());
  dim3 grid((N + 63) / 64, chunks);
  DISPATCH_FLOAT_TYPES(x.scalar_type(), "col_sum", [&] {
    if constexpr (!std::is_same<scalar_t, float>::value) {
      hipLaunchKernelGGL((col_sum_kernel<scalar_t>), grid, dim3(256), 0,
                         stream, (const scalar_t*)x.data_ptr(),
                         part.data_ptr<float>(), R, N, rows_per_chunk);
      hipLaunchKernelGGL((reduce_cols_cast_kernel<scalar_t>),
                         dim3((N + 63) / 64), dim3(256), 0, stream,
                         part.data_ptr<float>(), (scalar_t*)out.data_ptr(),
                         (long)N, (int)chunks);
    }
  });
  return out;
}
