// Multi-tensor launch: one kernel launch per 32 tensors instead of one per
// tensor (AdamW walks 201 BERT tensors per step).
//
// Up to MAXT tensors are packed into the kernel-argument block: NP pointer
// arrays, the element counts, and the prefix sums of the blocks each tensor
// gets. A block finds its tensor by scanning the 33-entry prefix array,
// which is trivially cheap on the scalar unit. A new multi-tensor kernel
// supplies the pointer count NP, a blocks-per-tensor rule and its
// per-element function; packing, chunking and lookup live here.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <array>
#include <vector>

#include "common.h"

namespace mt {

constexpr int MAXT = 32;   // tensors per launch
constexpr int BLOCK = 256;
constexpr int ILP = 4;     // contiguous elements per thread, one v4_t
constexpr long ELEMS_PER_BLOCK = (long)BLOCK * ILP;

// NP = 5 (AdamW) is 1.7 KB of the 4 KB kernel-argument limit
template <int NP>
struct Meta {
  void* ptr[NP][MAXT];  // nullptr for a list the call leaves empty
  long numel[MAXT];
  int block_prefix[MAXT + 1];
  int ntensors;
};

struct Slot {
  int t;             // tensor index in the Meta
  long local_block;  // this block's index inside that tensor
};

template <int NP>
__device__ __forceinline__ Slot find_tensor(const Meta<NP>& meta) {
  int t = 0;
  while (t + 1 < meta.ntensors && blockIdx.x >= meta.block_prefix[t + 1]) ++t;
  return {t, (long)blockIdx.x - meta.block_prefix[t]};
}

// true when every pointer is aligned to `bytes` (a power of two)
template <typename... P>
__device__ __forceinline__ bool all_aligned(unsigned long bytes, P... p) {
  return ((... | (unsigned long)p) & (bytes - 1)) == 0;
}

// g[i] = f(g[i]) over this block's BLOCK * ILP elements of an n-element
// tensor: one v4_t per thread where g is aligned for it (gradients may be
// views into flat DDP buckets at arbitrary offsets) and the vector is whole,
// element by element otherwise. f maps float to float.
template <typename T, typename F>
__device__ __forceinline__ void map_inplace(T* g, long n, long local_block,
                                            F f) {
  const long i0 = (local_block * BLOCK + threadIdx.x) * (long)ILP;
  if (all_aligned(sizeof(v4_t<T>), g) && i0 + ILP <= n) {
    v4_t<T> gv = ld4(g + i0);
#pragma unroll
    for (int j = 0; j < ILP; ++j) set_elem<T>(gv, j, f(elem<T>(gv, j)));
    st4(g + i0, gv);
  } else {
    for (int j = 0; j < ILP; ++j) {
      const long i = i0 + j;
      if (i >= n) break;
      g[i] = from_f32<T>(f(to_f32<T>(g[i])));
    }
  }
}

inline int elementwise_blocks(const torch::Tensor& t) {
  return (int)((t.numel() + ELEMS_PER_BLOCK - 1) / ELEMS_PER_BLOCK);
}

// Walks NP parallel tensor lists in chunks of MAXT and calls
// launch(meta, blocks) per chunk. lists[0] sets the length, the element
// counts and the dtype; an empty list fills its slot with nullptr.
// blocks_of(tensor of lists[0]) is the number of blocks that tensor gets.
template <int NP, typename BlocksOf, typename Launch>
void for_each_chunk(
    const std::array<const std::vector<torch::Tensor>*, NP>& lists,
    BlocksOf blocks_of, Launch launch) {
  const auto& first = *lists[0];
  size_t i = 0;
  while (i < first.size()) {
    Meta<NP> meta{};
    int nt = 0;
    int blocks = 0;
    for (; i < first.size() && nt < MAXT; ++i, ++nt) {
      TORCH_CHECK(first[i].scalar_type() == first[0].scalar_type(),
                  "mixed dtypes in one call");
      for (int k = 0; k < NP; ++k) {
        const auto& list = *lists[k];
        meta.ptr[k][nt] = list.empty() ? nullptr : list[i].data_ptr();
      }
      meta.numel[nt] = first[i].numel();
      meta.block_prefix[nt] = blocks;
      blocks += blocks_of(first[i]);
    }
    meta.block_prefix[nt] = blocks;
    meta.ntensors = nt;
    launch(meta, blocks);
  }
}

// the non-empty tensors of a list, checked contiguous and on the device
// (for_each_chunk checks that they are of one dtype)
inline std::vector<torch::Tensor> live_tensors(
    const std::vector<torch::Tensor>& tensors, const char* op) {
  std::vector<torch::Tensor> live;
  for (auto& t : tensors) {
    if (t.numel() == 0) continue;
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(), op,
                ": tensors must be contiguous device tensors");
    live.push_back(t);
  }
  return live;
}

// device scalars (fp32[1]): loss-scale flag, clip coefficient, norms
inline float* scalar_ptr(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.numel() == 1 &&
                  t.scalar_type() == at::ScalarType::Float,
              name, " must be a 1-element fp32 device tensor");
  return t.data_ptr<float>();
}
// nullptr when the tensor is absent (undefined or empty)
inline float* nullable_scalar_ptr(const torch::Tensor& t, const char* name) {
  return (t.defined() && t.numel() > 0) ? scalar_ptr(t, name) : nullptr;
}
// *p, or `otherwise` for an absent scalar
__device__ __forceinline__ float load_or(const float* p, float otherwise) {
  return p != nullptr ? *p : otherwise;
}

}  // namespace mt
