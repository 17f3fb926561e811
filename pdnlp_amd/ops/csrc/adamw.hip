// Multi-tensor AdamW / SGD update + AMP unscale/non-finite check
// (SURVEY.md K12/K13/K15). Packing and launch: multi_tensor.h.
//
// Honors decoupled weight decay (per group), fp32 m/v, optional fp32 master
// weights for bf16/fp16 params, a fused grad-scale-inverse (AMP), and an
// optional device-side gradient-clip coefficient (grad_clip.hip).

#include <optional>

#include "multi_tensor.h"

namespace {

using namespace mt;

// the scale every gradient is multiplied by: the AMP inverse scale times the
// global-norm clip coefficient (grad_clip.hip), a device scalar read once
// per block; nullptr = no clipping
__device__ __forceinline__ float grad_scale(float grad_scale_inv,
                                            const float* grad_coef) {
  return grad_scale_inv * load_or(grad_coef, 1.f);
}

struct AdamWCoef {
  float grad_scale, beta1, beta2, eps, bc2, step_size, wd_factor;
};

// gf is the scaled gradient
__device__ __forceinline__ void adamw_update(const AdamWCoef& c, float gf,
                                             float& w, float& m, float& v) {
  w *= c.wd_factor;
  m = c.beta1 * m + (1.f - c.beta1) * gf;
  v = c.beta2 * v + (1.f - c.beta2) * gf * gf;
  w -= c.step_size * m / (sqrtf(v / c.bc2) + c.eps);
}

// pointer slots: p, g, m, v, mw (mw nullptr when no master weights)
template <typename T, bool MASTER>
__global__ void adamw_kernel(Meta<5> meta, float lr, float beta1,
                             float beta2, float eps, float wd, float bc1,
                             float bc2, float grad_scale_inv,
                             const float* __restrict__ found_inf,
                             const float* __restrict__ grad_coef) {
  // AMP: skip the whole update on overflow, device-side (no host sync —
  // the GradScaler's per-step found_inf.item() stalls the launch pipeline)
  if (load_or(found_inf, 0.f) != 0.f) return;
  const AdamWCoef c{grad_scale(grad_scale_inv, grad_coef), beta1, beta2, eps,
                    bc2, lr / bc1, 1.f - lr * wd};
  const Slot s = find_tensor(meta);
  const long n = meta.numel[s.t];
  T* p = (T*)meta.ptr[0][s.t];
  const T* g = (const T*)meta.ptr[1][s.t];
  float* m = (float*)meta.ptr[2][s.t];
  float* v = (float*)meta.ptr[3][s.t];
  float* mw = MASTER ? (float*)meta.ptr[4][s.t] : nullptr;

  // contiguous ILP elements per thread, vectorized (8 B bf16x4 / 16 B
  // float4) — scalar 2-B loads halve effective HBM bandwidth and this
  // kernel moves ~3 GB per step (params + masters + m + v + grads)
  const long i0 = (s.local_block * BLOCK + threadIdx.x) * (long)ILP;
  // grads may be views into flat DDP buckets at arbitrary offsets — the
  // vector path needs 8-B (16-B fp32) alignment on every pointer
  if (all_aligned(sizeof(v4_t<T>), g, p) && all_aligned(16, m, v, mw) &&
      i0 + ILP <= n) {
    const v4_t<T> gv = ld4(g + i0);
    v4_t<T> pv;
    if (!MASTER) pv = ld4(p + i0);
    float4 mv = ld4(m + i0), vv = ld4(v + i0), wv;
    if (MASTER) wv = ld4(mw + i0);
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
      const float gf = elem<T>(gv, j) * c.grad_scale;
      float w = MASTER ? elem<float>(wv, j) : elem<T>(pv, j);
      float mi = elem<float>(mv, j), vi = elem<float>(vv, j);
      adamw_update(c, gf, w, mi, vi);
      set_elem<float>(mv, j, mi);
      set_elem<float>(vv, j, vi);
      if (MASTER) set_elem<float>(wv, j, w);
      set_elem<T>(pv, j, w);
    }
    st4(m + i0, mv);
    st4(v + i0, vv);
    if (MASTER) st4(mw + i0, wv);
    st4(p + i0, pv);
  } else {
    for (int j = 0; j < ILP; ++j) {
      const long i = i0 + j;
      if (i >= n) break;
      const float gf = to_f32<T>(g[i]) * c.grad_scale;
      float w = MASTER ? mw[i] : to_f32<T>(p[i]);
      float mi = m[i], vi = v[i];
      adamw_update(c, gf, w, mi, vi);
      m[i] = mi;
      v[i] = vi;
      if (MASTER) mw[i] = w;
      p[i] = from_f32<T>(w);
    }
  }
}

// SGD with momentum (the fabric alt-optimizer path):
// buf = mom*buf + (g + wd*w); w -= lr*buf. fp32 momentum, optional fp32
// master weights.
__device__ __forceinline__ void sgd_update(float lr, float momentum, float wd,
                                           float gf, float& w, float& buf) {
  const float gw = gf + wd * w;
  buf = momentum * buf + gw;
  w -= lr * buf;
}

// pointer slots: p, g, buf, mw
template <typename T, bool MASTER>
__global__ void sgd_kernel(Meta<4> meta, float lr, float momentum, float wd,
                           float grad_scale_inv,
                           const float* __restrict__ found_inf,
                           const float* __restrict__ grad_coef) {
  if (load_or(found_inf, 0.f) != 0.f) return;
  const float gs = grad_scale(grad_scale_inv, grad_coef);
  const Slot s = find_tensor(meta);
  const long n = meta.numel[s.t];
  T* p = (T*)meta.ptr[0][s.t];
  const T* g = (const T*)meta.ptr[1][s.t];
  float* buf = (float*)meta.ptr[2][s.t];
  float* mw = MASTER ? (float*)meta.ptr[3][s.t] : nullptr;
  const long i0 = (s.local_block * BLOCK + threadIdx.x) * (long)ILP;
  for (int j = 0; j < ILP; ++j) {
    const long i = i0 + j;
    if (i >= n) break;
    const float gf = to_f32<T>(g[i]) * gs;
    float w = MASTER ? mw[i] : to_f32<T>(p[i]);
    float b = buf[i];
    sgd_update(lr, momentum, wd, gf, w, b);
    buf[i] = b;
    if (MASTER) mw[i] = w;
    p[i] = from_f32<T>(w);
  }
}

template <typename T>
__global__ void unscale_kernel(Meta<1> meta, float* found_inf,
                               float inv_scale) {
  const Slot s = find_tensor(meta);
  bool bad = false;
  map_inplace((T*)meta.ptr[0][s.t], meta.numel[s.t], s.local_block,
              [&](float x) {
                x *= inv_scale;
                if (!isfinite(x)) bad = true;
                return x;
              });
  if (__any(bad) && (threadIdx.x & (WAVE - 1)) == 0) *found_inf = 1.f;
}

const float* coef_ptr(const std::optional<torch::Tensor>& c) {
  return c.has_value() ? nullable_scalar_ptr(*c, "grad_coef") : nullptr;
}

}  // namespace

void multi_tensor_adamw(std::vector<torch::Tensor> params,
                        std::vector<torch::Tensor> grads,
                        std::vector<torch::Tensor> exp_avgs,
                        std::vector<torch::Tensor> exp_avg_sqs,
                        std::vector<torch::Tensor> masters, double lr,
                        double beta1, double beta2, double eps,
                        double weight_decay, double bc1, double bc2,
                        double grad_scale_inv, torch::Tensor found_inf,
                        std::optional<torch::Tensor> grad_coef) {
  TORCH_CHECK(!params.empty());
  const float* finf = nullable_scalar_ptr(found_inf, "found_inf");
  const float* gcoef = coef_ptr(grad_coef);
  auto stream = at::hip::getCurrentHIPStream();
  for_each_chunk<5>(
      {&params, &grads, &exp_avgs, &exp_avg_sqs, &masters}, elementwise_blocks,
      [&](const Meta<5>& meta, int blocks) {
        DISPATCH_FLOAT_TYPES(params[0].scalar_type(), "multi_tensor_adamw", [&] {
          DISPATCH_BOOL(!masters.empty(), MASTER, [&] {
            hipLaunchKernelGGL((adamw_kernel<scalar_t, MASTER>), dim3(blocks),
                               dim3(BLOCK), 0, stream, meta, (float)lr,
                               (float)beta1, (float)beta2, (float)eps,
                               (float)weight_decay, (float)bc1, (float)bc2,
                               (float)grad_scale_inv, finf, gcoef);
          });
        });
      });
}

void multi_tensor_sgd(std::vector<torch::Tensor> params,
                      std::vector<torch::Tensor> grads,
                      std::vector<torch::Tensor> bufs,
                      std::vector<torch::Tensor> masters, double lr,
                      double momentum, double weight_decay,
                      double grad_scale_inv, torch::Tensor found_inf,
                      std::optional<torch::Tensor> grad_coef) {
  TORCH_CHECK(!params.empty());
  const float* finf = nullable_scalar_ptr(found_inf, "found_inf");
  const float* gcoef = coef_ptr(grad_coef);
  auto stream = at::hip::getCurrentHIPStream();
  for_each_chunk<4>(
      {&params, &grads, &bufs, &masters}, elementwise_blocks,
      [&](const Meta<4>& meta, int blocks) {
        DISPATCH_FLOAT_TYPES(params[0].scalar_type(), "multi_tensor_sgd", [&] {
          DISPATCH_BOOL(!masters.empty(), MASTER, [&] {
            hipLaunchKernelGGL((sgd_kernel<scalar_t, MASTER>), dim3(blocks),
                               dim3(BLOCK), 0, stream, meta, (float)lr,
                               (float)momentum, (float)weight_decay,
                               (float)grad_scale_inv, finf, gcoef);
          });
        });
      });
}

void multi_tensor_unscale(std::vector<torch::Tensor> grads,
                          torch::Tensor found_inf, double inv_scale) {
  TORCH_CHECK(!grads.empty());
  float* finf = scalar_ptr(found_inf, "found_inf");
  auto stream = at::hip::getCurrentHIPStream();
  for_each_chunk<1>(
      {&grads}, elementwise_blocks, [&](const Meta<1>& meta, int blocks) {
        DISPATCH_FLOAT_TYPES(grads[0].scalar_type(), "multi_tensor_unscale", [&] {
          hipLaunchKernelGGL((unscale_kernel<scalar_t>), dim3(blocks),
                             dim3(BLOCK), 0, stream, meta, finf,
                             (float)inv_scale);
        });
      });
}
