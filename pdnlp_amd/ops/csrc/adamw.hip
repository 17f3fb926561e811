// Multi-tensor AdamW update + AMP unscale/non-finite check
// (SURVEY.md K12/K13).
//
// Chunked multi-tensor launch: up to 32 tensors per launch packed into the
// kernel-argument block (pointer arrays + per-tensor block-offset prefix
// sums; the kernel finds its tensor by scanning the 33-entry prefix array —
// trivially cheap on the scalar unit). Replaces torch's per-tensor foreach
// launches with one launch per ~32 tensors: the reference's AdamW walks 201
// BERT tensors per step.
//
// Honors decoupled weight decay (per group), fp32 m/v, optional fp32 master
// weights for bf16/fp16 params, a fused grad-scale-inverse (AMP), and an
// optional device-side gradient-clip coefficient (grad_clip.hip).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <optional>

#include "common.h"

namespace {

constexpr int MAXT = 32;

// 4-element vector chunk: 8 B for bf16/fp16, 16 B for fp32
template <typename TT> struct V4A { using type = short4; };
template <> struct V4A<float> { using type = float4; };
template <typename TT> using v4_t = typename V4A<TT>::type;
constexpr int BLOCK = 256;
constexpr int ILP = 4;

struct AdamWMeta {
  const void* g[MAXT];
  void* p[MAXT];
  float* m[MAXT];
  float* v[MAXT];
  float* mw[MAXT];  // nullptr when no master weights
  long numel[MAXT];
  int block_prefix[MAXT + 1];
  int ntensors;
};

template <typename T, bool MASTER>
__global__ void adamw_kernel(AdamWMeta meta, float lr, float beta1,
                             float beta2, float eps, float wd, float bc1,
                             float bc2, float grad_scale_inv,
                             const float* __restrict__ found_inf,
                             const float* __restrict__ grad_coef) {
  // AMP: skip the whole update on overflow, device-side (no host sync —
  // the GradScaler's per-step found_inf.item() stalls the launch pipeline)
  if (found_inf != nullptr && *found_inf != 0.f) return;
  // global-norm clip: device coefficient (grad_clip.hip), read once per
  // block and folded into the scale the gradients are multiplied by anyway
  if (grad_coef != nullptr) grad_scale_inv *= *grad_coef;
  // find tensor for this block
  int t = 0;
  while (t + 1 < meta.ntensors && blockIdx.x >= meta.block_prefix[t + 1]) ++t;
  const long local_block = blockIdx.x - meta.block_prefix[t];
  const long n = meta.numel[t];
  const T* g = (const T*)meta.g[t];
  T* p = (T*)meta.p[t];
  float* m = meta.m[t];
  float* v = meta.v[t];
  float* mw = MASTER ? meta.mw[t] : nullptr;

  const float step_size = lr / bc1;
  const float wd_factor = 1.f - lr * wd;
  // contiguous ILP elements per thread, vectorized (8 B bf16x4 / 16 B
  // float4) — scalar 2-B loads halve effective HBM bandwidth and this
  // kernel moves ~3 GB per step (params + masters + m + v + grads)
  const long i0 = (local_block * BLOCK + threadIdx.x) * (long)ILP;
  // grads may be views into flat DDP buckets at arbitrary offsets — the
  // vector path needs 8-B (16-B fp32) alignment on every pointer
  const bool aligned =
      ((((unsigned long)g | (unsigned long)p) & (sizeof(v4_t<T>) - 1)) |
       (((unsigned long)m | (unsigned long)v |
         (MASTER ? (unsigned long)mw : 0ul)) & 15ul)) == 0;
  if (aligned && i0 + ILP <= n) {
    v4_t<T> gv = *reinterpret_cast<const v4_t<T>*>(g + i0);
    v4_t<T> pv;
    if (!MASTER) pv = *reinterpret_cast<const v4_t<T>*>(p + i0);
    float4 mv = *reinterpret_cast<const float4*>(m + i0);
    float4 vv = *reinterpret_cast<const float4*>(v + i0);
    float4 wv;
    if (MASTER) wv = *reinterpret_cast<const float4*>(mw + i0);
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
      const float gf =
          to_f32<T>(reinterpret_cast<const T*>(&gv)[j]) * grad_scale_inv;
      float w = MASTER ? reinterpret_cast<float*>(&wv)[j]
                       : to_f32<T>(reinterpret_cast<const T*>(&pv)[j]);
      w *= wd_factor;
      const float mi =
          beta1 * reinterpret_cast<float*>(&mv)[j] + (1.f - beta1) * gf;
      const float vi =
          beta2 * reinterpret_cast<float*>(&vv)[j] + (1.f - beta2) * gf * gf;
      reinterpret_cast<float*>(&mv)[j] = mi;
      reinterpret_cast<float*>(&vv)[j] = vi;
      w -= step_size * mi / (sqrtf(vi / bc2) + eps);
      if (MASTER) reinterpret_cast<float*>(&wv)[j] = w;
      reinterpret_cast<T*>(&pv)[j] = from_f32<T>(w);
    }
    *reinterpret_cast<float4*>(m + i0) = mv;
    *reinterpret_cast<float4*>(v + i0) = vv;
    if (MASTER) *reinterpret_cast<float4*>(mw + i0) = wv;
    *reinterpret_cast<v4_t<T>*>(p + i0) = pv;
  } else {
    for (int j = 0; j < ILP; ++j) {
      const long i = i0 + j;
      if (i >= n) break;
      const float gf = to_f32<T>(g[i]) * grad_scale_inv;
      float w = MASTER ? mw[i] : to_f32<T>(p[i]);
      w *= wd_factor;
      const float mi = beta1 * m[i] + (1.f - beta1) * gf;
      const float vi = beta2 * v[i] + (1.f - beta2) * gf * gf;
      m[i] = mi;
      v[i] = vi;
      w -= step_size * mi / (sqrtf(vi / bc2) + eps);
      if (MASTER) mw[i] = w;
      p[i] = from_f32<T>(w);
    }
  }
}

// SGD with momentum (SURVEY.md K15 — the fabric alt-optimizer path):
// buf = mom*buf + (g + wd*w); w -= lr*buf. fp32 momentum, optional fp32
// master weights, same multi-tensor packing as AdamW.
struct SgdMeta {
  const void* g[MAXT];
  void* p[MAXT];
  float* buf[MAXT];
  float* mw[MAXT];
  long numel[MAXT];
  int block_prefix[MAXT + 1];
  int ntensors;
};

template <typename T, bool MASTER>
__global__ void sgd_kernel(SgdMeta meta, float lr, float momentum, float wd,
                           float grad_scale_inv,
                           const float* __restrict__ found_inf,
                           const float* __restrict__ grad_coef) {
  if (found_inf != nullptr && *found_inf != 0.f) return;
  if (grad_coef != nullptr) grad_scale_inv *= *grad_coef;
  int t = 0;
  while (t + 1 < meta.ntensors && blockIdx.x >= meta.block_prefix[t + 1]) ++t;
  const long local_block = blockIdx.x - meta.block_prefix[t];
  const long n = meta.numel[t];
  const T* g = (const T*)meta.g[t];
  T* p = (T*)meta.p[t];
  float* buf = meta.buf[t];
  float* mw = MASTER ? meta.mw[t] : nullptr;
  const long i0 = (local_block * BLOCK + threadIdx.x) * (long)ILP;
  for (int j = 0; j < ILP; ++j) {
    const long i = i0 + j;
    if (i >= n) break;
    const float gf = to_f32<T>(g[i]) * grad_scale_inv;
    float w = MASTER ? mw[i] : to_f32<T>(p[i]);
    const float gw = gf + wd * w;
    const float b = momentum * buf[i] + gw;
    buf[i] = b;
    w -= lr * b;
    if (MASTER) mw[i] = w;
    p[i] = from_f32<T>(w);
  }
}

struct UnscaleMeta {
  void* g[MAXT];
  long numel[MAXT];
  int block_prefix[MAXT + 1];
  int ntensors;
};

template <typename T>
__global__ void unscale_kernel(UnscaleMeta meta, float* found_inf,
                               float inv_scale) {
  int t = 0;
  while (t + 1 < meta.ntensors && blockIdx.x >= meta.block_prefix[t + 1]) ++t;
  const long local_block = blockIdx.x - meta.block_prefix[t];
  const long n = meta.numel[t];
  T* g = (T*)meta.g[t];
  bool bad = false;
  const long i0 = (local_block * BLOCK + threadIdx.x) * (long)ILP;
  if ((((unsigned long)g) & (sizeof(v4_t<T>) - 1)) == 0 && i0 + ILP <= n) {
    v4_t<T> gv = *reinterpret_cast<const v4_t<T>*>(g + i0);
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
      const float x = to_f32<T>(reinterpret_cast<const T*>(&gv)[j]) * inv_scale;
      if (!isfinite(x)) bad = true;
      reinterpret_cast<T*>(&gv)[j] = from_f32<T>(x);
    }
    *reinterpret_cast<v4_t<T>*>(g + i0) = gv;
  } else {
    for (int j = 0; j < ILP; ++j) {
      const long i = i0 + j;
      if (i >= n) break;
      const float x = to_f32<T>(g[i]) * inv_scale;
      if (!isfinite(x)) bad = true;
      g[i] = from_f32<T>(x);
    }
  }
  if (__any(bad) && (threadIdx.x & (WAVE - 1)) == 0) *found_inf = 1.f;
}

// nullable device clip coefficient (fp32[1]); nullptr = no clipping
const float* coef_ptr(const std::optional<torch::Tensor>& c) {
  if (!c.has_value() || !c->defined() || c->numel() == 0) return nullptr;
  TORCH_CHECK(c->is_cuda() && c->numel() == 1 &&
                  c->scalar_type() == at::ScalarType::Float,
              "grad_coef must be a 1-element fp32 device tensor");
  return c->data_ptr<float>();
}

int blocks_of(long numel) {
  return (int)((numel + (long)BLOCK * ILP - 1) / ((long)BLOCK * ILP));
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
  const float* finf = (found_inf.defined() && found_inf.numel() > 0)
                          ? found_inf.data_ptr<float>()
                          : nullptr;
  const float* gcoef = coef_ptr(grad_coef);
  const bool master = !masters.empty();
  auto stream = at::hip::getCurrentHIPStream();
  const auto dtype = params[0].scalar_type();
  size_t i = 0;
  while (i < params.size()) {
    AdamWMeta meta{};
    int nt = 0;
    int blocks = 0;
    while (i < params.size() && nt < MAXT) {
      auto& p = params[i];
      TORCH_CHECK(p.scalar_type() == dtype, "mixed dtypes in one chunk");
      meta.p[nt] = p.data_ptr();
      meta.g[nt] = grads[i].data_ptr();
      meta.m[nt] = exp_avgs[i].data_ptr<float>();
      meta.v[nt] = exp_avg_sqs[i].data_ptr<float>();
      meta.mw[nt] = master ? masters[i].data_ptr<float>() : nullptr;
      meta.numel[nt] = p.numel();
      meta.block_prefix[nt] = blocks;
      blocks += blocks_of(p.numel());
      ++nt;
      ++i;
    }
    meta.block_prefix[nt] = blocks;
    meta.ntensors = nt;
    DISPATCH_FLOAT_TYPES(dtype, "multi_tensor_adamw", [&] {
      if (master) {
        hipLaunchKernelGGL((adamw_kernel<scalar_t, true>), dim3(blocks),
                           dim3(BLOCK), 0, stream, meta, (float)lr,
                           (float)beta1, (float)beta2, (float)eps,
                           (float)weight_decay, (float)bc1, (float)bc2,
                           (float)grad_scale_inv, finf, gcoef);
      } else {
        hipLaunchKernelGGL((adamw_kernel<scalar_t, false>), dim3(blocks),
                           dim3(BLOCK), 0, stream, meta, (float)lr,
                           (float)beta1, (float)beta2, (float)eps,
                           (float)weight_decay, (float)bc1, (float)bc2,
                           (float)grad_scale_inv, finf, gcoef);
      }
    });
  }
}

void multi_tensor_sgd(std::vector<torch::Tensor> params,
                      std::vector<torch::Tensor> grads,
                      std::vector<torch::Tensor> bufs,
                      std::vector<torch::Tensor> masters, double lr,
                      double momentum, double weight_decay,
                      double grad_scale_inv, torch::Tensor found_inf,
                        std::optional<torch::Tensor> grad_coef) {
  TORCH_CHECK(!params.empty());
  const float* finf = (found_inf.defined() && found_inf.numel() > 0)
                          ? found_inf.data_ptr<float>()
                          : nullptr;
  const float* gcoef = coef_ptr(grad_coef);
  const bool master = !masters.empty();
  auto stream = at::hip::getCurrentHIPStream();
  const auto dtype = params[0].scalar_type();
  size_t i = 0;
  while (i < params.size()) {
    SgdMeta meta{};
    int nt = 0;
    int blocks = 0;
    while (i < params.size() && nt < MAXT) {
      auto& p = params[i];
      TORCH_CHECK(p.scalar_type() == dtype, "mixed dtypes in one chunk");
      meta.p[nt] = p.data_ptr();
      meta.g[nt] = grads[i].data_ptr();
      meta.buf[nt] = bufs[i].data_ptr<float>();
      meta.mw[nt] = master ? masters[i].data_ptr<float>() : nullptr;
      meta.numel[nt] = p.numel();
      meta.block_prefix[nt] = blocks;
      blocks += blocks_of(p.numel());
      ++nt;
      ++i;
    }
    meta.block_prefix[nt] = blocks;
    meta.ntensors = nt;
    DISPATCH_FLOAT_TYPES(dtype, "multi_tensor_sgd", [&] {
      if (master) {
        hipLaunchKernelGGL((sgd_kernel<scalar_t, true>), dim3(blocks),
                           dim3(BLOCK), 0, stream, meta, (float)lr,
                           (float)momentum, (float)weight_decay,
                           (float)grad_scale_inv, finf, gcoef);
      } else {
        hipLaunchKernelGGL((sgd_kernel<scalar_t, false>), dim3(blocks),
                           dim3(BLOCK), 0, stream, meta, (float)lr,
                           (float)momentum, (float)weight_decay,
                           (float)grad_scale_inv, finf, gcoef);
      }
    });
  }
}

void multi_tensor_unscale(std::vector<torch::Tensor> grads,
                          torch::Tensor found_inf, double inv_scale) {
  TORCH_CHECK(!grads.empty());
  auto stream = at::hip::getCurrentHIPStream();
  const auto dtype = grads[0].scalar_type();
  size_t i = 0;
  while (i < grads.size()) {
    UnscaleMeta meta{};
    int nt = 0;
    int blocks = 0;
    while (i < grads.size() && nt < MAXT) {
      meta.g[nt] = grads[i].data_ptr();
      meta.numel[nt] = grads[i].numel();
      meta.block_prefix[nt] = blocks;
      blocks += blocks_of(grads[i].numel());
      ++nt;
      ++i;
    }
    meta.block_prefix[nt] = blocks;
    meta.ntensors = nt;
    DISPATCH_FLOAT_TYPES(dtype, "multi_tensor_unscale", [&] {
      hipLaunchKernelGGL((unscale_kernel<scalar_t>), dim3(blocks), dim3(BLOCK),
                         0, stream, meta, found_inf.data_ptr<float>(),
                         (float)inv_scale);
    });
  }
}
