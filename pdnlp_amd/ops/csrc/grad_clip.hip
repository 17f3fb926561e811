// Global-norm gradient clipping: multi-tensor sum of squares, the clip
// coefficient, and an in-place multi-tensor scale.
//
// The training step needs ||g||_2 over ~200 gradient tensors and then
// g * min(1, max_norm / (||g|| + 1e-6)). The norm is one read pass over the
// gradients (this file); the multiply is folded into the optimizer kernels
// (adamw.hip reads the device coefficient), so gradients are never
// rewritten on the fused path. multi_tensor_scale_ serves the in-place API.
//
// Sum of squares, deterministic, no atomics:
//   stage 1  one block per EPB = 16384 elements of one tensor (packing and
//            launch: multi_tensor.h). A thread makes K 16-byte loads (bf16/fp16:
//            8 lanes x K=8, fp32: 4 lanes x K=16), strided by the block so
//            a wave reads contiguous 1-KiB rows, and keeps one fp32
//            accumulator PER VECTOR LANE. The block writes one fp32 partial
//            to partials[part_base + blockIdx.x] - every launch of a call
//            writes its own slice of one workspace.
//   stage 2  ONE 1024-thread block folds all P partials of the call in
//            fixed order and (optionally) finishes norm + coefficient.
//
// Rounding depth (every add is fp32, u = 2^-24), P <= 65536 partials
// (1.07e9 elements per call, checked on the host):
//   L = 16  longest per-accumulator sequential chain (fp32: K = 16 loads;
//           bf16/fp16: 8)
//   D = 101 = 3 (fold 8 lane accumulators) + 1 (unaligned head element)
//           + 6 (wave butterfly) + 4 (fold 4 waves)
//           + 64 (stage-2 per-thread chain, ceil(P/1024)) + 6 (wave)
//           + 16 (fold 16 waves) + 1 (accumulate into out)
//   (L + D) * 2^-24 = 117 * 5.96e-8 = 6.97e-6 <= 1e-5.
//
// Alignment: gradients are views into flat DDP/ZeRO buffers at arbitrary
// element offsets. `head` is the number of elements before the first 16-byte
// boundary; those (< 8) are read with scalar loads by block 0, the body
// behind them is 16-byte aligned, and the last partial vector is read scalar.

#include <optional>

#include "multi_tensor.h"

namespace {

using namespace mt;

constexpr int NW = BLOCK / WAVE;
constexpr int EPB = 16384;       // elements per stage-1 block, every dtype
constexpr int FOLD_BLOCK = 1024;
constexpr int FOLD_NW = FOLD_BLOCK / WAVE;
constexpr long MAX_PARTIALS = 65536;  // keeps the stage-2 chain at <= 64

// elements of a tensor before the first 16-byte boundary (<= numel)
__host__ __device__ inline long head_elems(const void* p, long esize,
                                           long numel) {
  const long head = (long)(((16ul - ((unsigned long)p & 15ul)) & 15ul) / esize);
  return head < numel ? head : numel;
}

// stage-1 blocks of a tensor; one that is all head still needs its block 0
int sumsq_blocks(const torch::Tensor& t) {
  const long nb =
      t.numel() - head_elems(t.data_ptr(), t.element_size(), t.numel());
  return (int)(nb > 0 ? (nb + EPB - 1) / EPB : 1);
}

template <typename T>
__global__ __launch_bounds__(BLOCK)
void sumsq_partial_kernel(Meta<1> meta, float* __restrict__ partials) {
  constexpr int VEC = 16 / sizeof(T);
  constexpr int K = EPB / (BLOCK * VEC);
  __shared__ float lds[NW];
  const Slot slot = find_tensor(meta);
  const long local_block = slot.local_block;
  const long numel = meta.numel[slot.t];
  const T* g = (const T*)meta.ptr[0][slot.t];
  const int head = (int)head_elems(g, sizeof(T), numel);
  const T* body = g + head;      // 16-byte aligned
  const long nb = numel - head;  // >= 0

  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  const long base = local_block * (long)EPB + (long)threadIdx.x * VEC;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long i = base + (long)k * (BLOCK * VEC);
    if (i + VEC <= nb) {
      const uint4 raw = *reinterpret_cast<const uint4*>(body + i);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float x = to_f32<T>(reinterpret_cast<const T*>(&raw)[j]);
        acc[j] += x * x;
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (i + j < nb) {
          const float x = to_f32<T>(body[i + j]);
          acc[j] += x * x;
        }
      }
    }
  }
  // pairwise fold of the lane accumulators
#pragma unroll
  for (int w = VEC / 2; w > 0; w >>= 1) {
#pragma unroll
    for (int j = 0; j < w; ++j) acc[j] += acc[j + w];
  }
  float s = acc[0];
  if (local_block == 0 && (int)threadIdx.x < head) {
    const float x = to_f32<T>(g[threadIdx.x]);
    s += x * x;
  }
  s = wave_sum(s);
  if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) r += lds[i];
    partials[blockIdx.x] = r;
  }
}

__device__ __forceinline__ void write_coef(float sumsq, float max_norm,
                                           float* coef_out, float* norm_out) {
  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1);
  // a NaN ratio fails the comparison and propagates, like torch.clamp
  const float norm = sqrtf(sumsq);
  const float c = max_norm / (norm + 1e-6f);
  *coef_out = (c > 1.f) ? 1.f : c;
  *norm_out = norm;
}

// stage 2: fixed-order fold of P partials by one block; coef_out == nullptr
// skips the finalisation (ZeRO all-reduces `out` first)
__global__ __launch_bounds__(FOLD_BLOCK)
void sumsq_fold_kernel(const float* __restrict__ partials, int P,
                       float* __restrict__ out, int accumulate,
                       float max_norm, float* __restrict__ coef_out,
                       float* __restrict__ norm_out) {
  __shared__ float lds[FOLD_NW];
  float s = 0.f;
  for (int i = threadIdx.x; i < P; i += FOLD_BLOCK) s += partials[i];
  s = wave_sum(s);
  if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < FOLD_NW; ++i) r += lds[i];
    if (accumulate) r += *out;
    *out = r;
    if (coef_out != nullptr) write_coef(r, max_norm, coef_out, norm_out);
  }
}

__global__ void clip_coef_kernel(const float* __restrict__ sumsq,
                                 float max_norm, float* __restrict__ coef_out,
                                 float* __restrict__ norm_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    write_coef(*sumsq, max_norm, coef_out, norm_out);
}

// ---- in-place scale by a device scalar -------------------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK)
void scale_kernel(Meta<1> meta, const float* __restrict__ coef) {
  const float c = *coef;
  // below the clip threshold the coefficient is exactly 1: leave the
  // gradients untouched instead of rewriting them with themselves
  if (c == 1.f) return;
  const Slot s = find_tensor(meta);
  map_inplace((T*)meta.ptr[0][s.t], meta.numel[s.t], s.local_block,
              [c](float x) { return x * c; });
}

}  // namespace

void multi_tensor_sumsq(std::vector<torch::Tensor> tensors, torch::Tensor out,
                        bool accumulate, double max_norm,
                        std::optional<torch::Tensor> coef_out,
                        std::optional<torch::Tensor> norm_out) {
  float* outp = scalar_ptr(out, "out");
  const bool finalize = coef_out.has_value() && coef_out->defined();
  float* coefp = finalize ? scalar_ptr(*coef_out, "coef_out") : nullptr;
  float* normp = nullptr;
  if (finalize) {
    TORCH_CHECK(norm_out.has_value(), "norm_out is required with coef_out");
    normp = scalar_ptr(*norm_out, "norm_out");
  }
  auto stream = at::hip::getCurrentHIPStream();

  const auto live = live_tensors(tensors, "multi_tensor_sumsq");
  long total_blocks = 0;
  for (auto& t : live) total_blocks += (t.numel() + EPB - 1) / EPB;
  TORCH_CHECK(total_blocks <= MAX_PARTIALS,
              "multi_tensor_sumsq: more than ", MAX_PARTIALS * (long)EPB,
              " elements in one call; split the list and accumulate");

  torch::Tensor partials;
  float* partp = nullptr;
  if (total_blocks > 0) {
    partials = torch::empty({total_blocks},
                            out.options().dtype(at::ScalarType::Float));
    partp = partials.data_ptr<float>();
    // every launch of the call writes its own slice of the one workspace
    long part_base = 0;
    for_each_chunk<1>({&live}, sumsq_blocks, [&](const Meta<1>& meta,
                                                 int blocks) {
      DISPATCH_FLOAT_TYPES(live[0].scalar_type(), "multi_tensor_sumsq", [&] {
        hipLaunchKernelGGL((sumsq_partial_kernel<scalar_t>), dim3(blocks),
                           dim3(BLOCK), 0, stream, meta, partp + part_base);
      });
      part_base += blocks;
    });
    total_blocks = part_base;
  }
  hipLaunchKernelGGL(sumsq_fold_kernel, dim3(1), dim3(FOLD_BLOCK), 0, stream,
                     partp, (int)total_blocks, outp, accumulate ? 1 : 0,
                     (float)max_norm, coefp, normp);
}

void clip_coef_from_sumsq(torch::Tensor sumsq, double max_norm,
                          torch::Tensor coef_out, torch::Tensor norm_out) {
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(WAVE), 0, stream,
                     scalar_ptr(sumsq, "sumsq"), (float)max_norm,
                     scalar_ptr(coef_out, "coef_out"),
                     scalar_ptr(norm_out, "norm_out"));
}

void multi_tensor_scale_(std::vector<torch::Tensor> tensors,
                         torch::Tensor coef) {
  const float* coefp = scalar_ptr(coef, "coef");
  auto stream = at::hip::getCurrentHIPStream();
  const auto live = live_tensors(tensors, "multi_tensor_scale_");
  if (live.empty()) return;
  for_each_chunk<1>(
      {&live}, elementwise_blocks, [&](const Meta<1>& meta, int blocks) {
        DISPATCH_FLOAT_TYPES(live[0].scalar_type(), "multi_tensor_scale_", [&] {
          hipLaunchKernelGGL((scale_kernel<scalar_t>), dim3(blocks),
                             dim3(BLOCK), 0, stream, meta, coefp);
        });
      });
}
