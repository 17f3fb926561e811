// Fused cross-entropy forward/backward: log-softmax + NLL
// on [B, C] logits (C = 6 for the reference task), one wavefront per row,
// fp32 throughout. Forward returns per-row losses (binding takes the mean)
// and saves log-probs for a one-pass backward.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

__global__ void ce_fwd_kernel(const float* __restrict__ logits,
                              const long* __restrict__ labels,
                              float* __restrict__ losses,
                              float* __restrict__ logprobs, int C) {
  const long row = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const float* lr = logits + row * C;
  float* lpr = logprobs + row * C;
  float m = -3.4e38f;
  for (int c = lane; c < C; c += WAVE) m = fmaxf(m, lr[c]);
  m = wave_max(m);
  float sum = 0.f;
  for (int c = lane; c < C; c += WAVE) sum += __expf(lr[c] - m);
  sum = wave_sum(sum);
  const float lse = m + __logf(sum);
  for (int c = lane; c < C; c += WAVE) lpr[c] = lr[c] - lse;
  if (lane == 0) losses[row] = lse - lr[labels[row]];
}

__global__ void ce_bwd_kernel(const float* __restrict__ dloss,
                              const float* __restrict__ logprobs,
                              const long* __restrict__ labels,
                              float* __restrict__ dlogits, int C, float invB) {
  const long row = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const float d = dloss[0] * invB;
  for (int c = lane; c < C; c += WAVE) {
    const float p = __expf(logprobs[row * C + c]);
    dlogits[row * C + c] = d * (p - (c == labels[row] ? 1.f : 0.f));
  }
}

// ---- ignore_index variants -------------------------------------------------
// A row whose label equals ignore_index carries no sentence (the empty
// sequences that round a packed batch up to a fixed count): it never indexes
// logits with its label, adds 0 to the loss and gets a zero gradient row.
// The mean runs over the valid rows only; their count is taken on the device
// by ce_reduce_ignore_kernel and read from device memory by the backward, so
// one captured launch is right for any mix of valid and ignored rows.

__global__ void ce_fwd_ignore_kernel(const float* __restrict__ logits,
                                     const long* __restrict__ labels,
                                     float* __restrict__ losses,
                                     float* __restrict__ logprobs, int C,
                                     long ignore_index) {
  const long row = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const float* lr = logits + row * C;
  float* lpr = logprobs + row * C;
  float m = -3.4e38f;
  for (int c = lane; c < C; c += WAVE) m = fmaxf(m, lr[c]);
  m = wave_max(m);
  float sum = 0.f;
  for (int c = lane; c < C; c += WAVE) sum += __expf(lr[c] - m);
  sum = wave_sum(sum);
  const float lse = m + __logf(sum);
  for (int c = lane; c < C; c += WAVE) lpr[c] = lr[c] - lse;
  if (lane == 0) {
    const long label = labels[row];
    losses[row] = label == ignore_index ? 0.f : lse - lr[label];
  }
}

// one block: loss = sum(losses) / #valid, nvalid = #valid. Each thread adds
// its rows in a fixed order and block_sum folds in a fixed tree, so the
// result is deterministic (no atomics). The count is exact in fp32 for
// B < 2^24 (checked by the caller).
__global__ __launch_bounds__(256)
void ce_reduce_ignore_kernel(const float* __restrict__ losses,
                             const long* __restrict__ labels,
                             float* __restrict__ loss,
                             float* __restrict__ nvalid, long B,
                             long ignore_index) {
  __shared__ float lds[4];
  float s = 0.f, n = 0.f;
  for (long r = threadIdx.x; r < B; r += 256) {
    s += losses[r];
    n += labels[r] != ignore_index ? 1.f : 0.f;
  }
  s = block_sum<4>(s, lds);
  n = block_sum<4>(n, lds);
  if (threadIdx.x == 0) {
    loss[0] = s / n;
    nvalid[0] = n;
  }
}

__global__ void ce_bwd_ignore_kernel(const float* __restrict__ dloss,
                                     const float* __restrict__ logprobs,
                                     const long* __restrict__ labels,
                                     const float* __restrict__ nvalid,
                                     float* __restrict__ dlogits, int C,
                                     long ignore_index) {
  const long row = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const long label = labels[row];
  if (label == ignore_index) {
    for (int c = lane; c < C; c += WAVE) dlogits[row * C + c] = 0.f;
    return;
  }
  const float d = dloss[0] / nvalid[0];
  for (int c = lane; c < C; c += WAVE) {
    const float p = __expf(logprobs[row * C + c]);
    dlogits[row * C + c] = d * (p - (c == label ? 1.f : 0.f));
  }
}

}  // namespace

std::vector<torch::Tensor> cross_entropy_fwd(torch::Tensor logits,
                                             torch::Tensor labels) {
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32);
  const int C = logits.size(-1);
  const long B = logits.size(0);
  auto losses = torch::empty({B}, logits.options());
  auto logprobs = torch::empty_like(logits);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(B), dim3(WAVE), 0, stream,
                     logits.data_ptr<float>(), labels.data_ptr<long>(),
                     losses.data_ptr<float>(), logprobs.data_ptr<float>(), C);
  return {losses.mean(), logprobs};
}

torch::Tensor cross_entropy_bwd(torch::Tensor dloss, torch::Tensor logprobs,
                                torch::Tensor labels) {
  const int C = logprobs.size(-1);
  const long B = logprobs.size(0);
  auto dlogits = torch::empty_like(logprobs);
  auto stream = at::hip::getCurrentHIPStream();
  auto d = dloss.to(torch::kFloat32).contiguous();
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(B), dim3(WAVE), 0, stream,
                     d.data_ptr<float>(), logprobs.data_ptr<float>(),
                     labels.data_ptr<long>(), dlogits.data_ptr<float>(), C,
                     1.f / B);
  return dlogits;
}

// returns {loss (mean over rows with label != ignore_index), logprobs,
// nvalid fp32[1] (device-resident count of those rows)}
std::vector<torch::Tensor> cross_entropy_ignore_fwd(torch::Tensor logits,
                                                    torch::Tensor labels,
                                                    long ignore_index) {
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32);
  TORCH_CHECK(labels.scalar_type() == torch::kLong && labels.is_contiguous());
  const int C = logits.size(-1);
  const long B = logits.size(0);
  TORCH_CHECK(B > 0 && B < (1L << 24) && labels.numel() == B);
  auto losses = torch::empty({B}, logits.options());
  auto logprobs = torch::empty_like(logits);
  auto loss = torch::empty({}, logits.options());
  auto nvalid = torch::empty({1}, logits.options());
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(ce_fwd_ignore_kernel, dim3(B), dim3(WAVE), 0, stream,
                     logits.data_ptr<float>(), labels.data_ptr<long>(),
                     losses.data_ptr<float>(), logprobs.data_ptr<float>(), C,
                     ignore_index);
  hipLaunchKernelGGL(ce_reduce_ignore_kernel, dim3(1), dim3(256), 0, stream,
                     losses.data_ptr<float>(), labels.data_ptr<long>(),
                     loss.data_ptr<float>(), nvalid.data_ptr<float>(), B,
                     ignore_index);
  return {loss, logprobs, nvalid};
}

torch::Tensor cross_entropy_ignore_bwd(torch::Tensor dloss,
                                       torch::Tensor logprobs,
                                       torch::Tensor labels,
                                       torch::Tensor nvalid,
                                       long ignore_index) {
  const int C = logprobs.size(-1);
  const long B = logprobs.size(0);
  auto dlogits = torch::empty_like(logprobs);
  auto stream = at::hip::getCurrentHIPStream();
  auto d = dloss.to(torch::kFloat32).contiguous();
  hipLaunchKernelGGL(ce_bwd_ignore_kernel, dim3(B), dim3(WAVE), 0, stream,
                     d.data_ptr<float>(), logprobs.data_ptr<float>(),
                     labels.data_ptr<long>(), nvalid.data_ptr<float>(),
                     dlogits.data_ptr<float>(), C, ignore_index);
  return dlogits;
}
