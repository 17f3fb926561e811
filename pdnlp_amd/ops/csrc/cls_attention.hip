// One-query-row-per-sequence attention for gfx950: the first token of every
// sequence of a packed stream attends to the keys of its own sequence.
//
// A sequence classifier reads only the first-token row of the last encoder
// layer, so that layer's attention needs one query row per sequence. The
// flash kernels of attention.hip work on 64-row query tiles, the wrong shape
// for this; here the problem is a batch of GEMVs (q·K^T, then P·V) that reads
// K and V once and is bound by that read.
//
//  - Works DIRECTLY on the packed QKV projection [T, 3H] in the layout
//    attention.hip documents (head h's q/k/v at columns h*64 / H+h*64 /
//    2H+h*64, head_dim 64) and writes o [rows_out, H]: row i < B is the
//    output of sequence i's first token, every other row exactly zero.
//  - One wave per (sequence, head); a block is four waves = four heads of one
//    sequence. A head's K (or V) row is 128 B = 8 lanes x 16 B, so a wave
//    reads 8 keys per step with one 16-byte load per lane: lane = (key
//    sub-slot, 8-column chunk). Each 8-lane group keeps an online softmax
//    (m, l, 8 output columns) over its keys j = sub, sub+8, ...; the eight
//    groups are merged once at the end by wave shuffles. No LDS, no MFMA,
//    no barrier.
//  - fp32 scores, softmax and accumulation; P stays fp32 (never rounded to
//    the 16-bit type as the MFMA kernels must).
//  - Each wave owns every element it writes: o[i, h*64..], lse[h, i], the k
//    and v columns of head h in its sequence's rows of dqkv and the q columns
//    of the first row. No atomics; all sums run in a fixed order, so results
//    are bit-reproducible.
//  - Dropout on P is the flash kernels' scheme: device seed + salt, keep
//    where hash_rng32(drop_idx<VARLEN>(h*T + first row, key)) * 2^-32 >= p.
//    With the same (seed, salt) the kept set equals the one
//    flash_attn_varlen_fwd keeps on that row. Backward recomputes it; nothing
//    is saved but (o, lse).
//  - The grid is (rows_out, ceil(nh/4)) and cu_seqlens is read on the device
//    only: no host sync, and a captured graph serves any boundaries.
//  - Zeros: the forward grid covers every (row, head) of o, so the kernel
//    writes the zero rows itself and o needs no fill launch. dqkv [T, 3H] is
//    zero-filled by the host (as flash_attn_varlen_bwd does): the rows outside
//    every sequence belong to no wave.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "attn_common.h"

namespace {

constexpr int CLS_THREADS = 256;  // 4 waves = 4 heads of one sequence
constexpr float LOG2E = 1.4426950408889634f;

// 8 contiguous elements (16 B) <-> fp32
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ p, float* f) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  const T* e = reinterpret_cast<const T*>(&u);
#pragma unroll
  for (int d = 0; d < 8; ++d) f[d] = to_f32<T>(e[d]);
}
template <typename T>
__device__ __forceinline__ void store8(T* __restrict__ p, const float* f) {
  uint4 u;
  T* e = reinterpret_cast<T*>(&u);
#pragma unroll
  for (int d = 0; d < 8; ++d) e[d] = from_f32<T>(f[d]);
  *reinterpret_cast<uint4*>(p) = u;
}

// sum over the 8 lanes of a group (lanes that share lane>>3)
__device__ __forceinline__ float group_sum(float x) {
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}
// sum / max over the 8 groups (lanes that share lane&7)
__device__ __forceinline__ float cross_sum(float x) {
#pragma unroll
  for (int off = 8; off < WAVE; off <<= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}
__device__ __forceinline__ float cross_max(float x) {
#pragma unroll
  for (int off = 8; off < WAVE; off <<= 1)
    x = fmaxf(x, __shfl_xor(x, off, WAVE));
  return x;
}

// The wave's (sequence, head): first packed row and clamped length. len <= 0
// for rows past the batch, empty sequences and a cu_seqlens entry outside
// the stream. Wave-uniform.
__device__ __forceinline__ int cls_bounds(const int* __restrict__ cu_seqlens,
                                          int i, int B, int T_rows,
                                          long& row0) {
  row0 = 0;
  if (i >= B) return 0;
  row0 = cu_seqlens[i];
  if (row0 < 0 || row0 >= T_rows) return 0;
  return varlen_len(cu_seqlens, i, row0, T_rows);
}

// ---------------------------------------------------------------------------
// forward. INFER: the same arithmetic, no lse store.
// ---------------------------------------------------------------------------

template <typename T, bool DROP, bool INFER>
__global__ __launch_bounds__(CLS_THREADS)
void cls_attn_fwd_kernel(const T* __restrict__ qkv,
                         const int* __restrict__ cu_seqlens,
                         T* __restrict__ o, float* __restrict__ lse,
                         const unsigned long long* __restrict__ seed_base,
                         unsigned long long salt, float scale, float p, int nh,
                         int T_rows, int B, int rows_out) {
  static_assert(!(INFER && DROP), "the serving form has no dropout");
  const int lane = threadIdx.x & (WAVE - 1);
  const int i = blockIdx.x;                           // output row = sequence
  const int h = blockIdx.y * 4 + (threadIdx.x >> 6);  // one wave per head
  if (h >= nh) return;  // wave-uniform; the kernel has no barrier
  const int sub = lane >> 3, c = lane & 7;
  const long H = (long)nh * 64, ld = 3 * H;
  T* orow = o + (long)i * H + h * 64 + c * 8;

  long row0;
  const int len = cls_bounds(cu_seqlens, i, B, T_rows, row0);
  if (len <= 0) {  // wave-uniform: this wave owns a zero slice of o
    if (sub == 0) *reinterpret_cast<uint4*>(orow) = make_uint4(0u, 0u, 0u, 0u);
    if (!INFER && lane == 0) lse[(long)h * rows_out + i] = 0.f;
    return;
  }

  const T* qp = qkv + row0 * ld + h * 64 + c * 8;
  const T* kp = qp + H;
  const T* vp = qp + 2 * H;
  const unsigned long long seed = DROP ? (*seed_base + salt) : 0ull;
  const unsigned int seed32 = (unsigned int)(seed ^ (seed >> 32));
  const float inv_keep = DROP ? 1.f / (1.f - p) : 1.f;
  const unsigned int qrow = (unsigned int)((long)h * T_rows + row0);

  float q[8];
  load8<T>(qp, q);
#pragma unroll
  for (int d = 0; d < 8; ++d) q[d] *= scale * LOG2E;  // exp2 domain

  // the group's online softmax over keys sub, sub + 8, ...
  float m = -INFINITY, l = 0.f, acc[8] = {};
  for (int j0 = 0; j0 < len; j0 += 8) {  // wave-uniform trip count
    const int key = j0 + sub;
    const bool valid = key < len;
    const long kr = valid ? key : len - 1;  // tail: a clamped copy, P = 0
    float k[8], v[8];
    load8<T>(kp + kr * ld, k);
    load8<T>(vp + kr * ld, v);
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) s += q[d] * k[d];
    s = group_sum(s);
    const float mn = valid ? fmaxf(m, s) : m;
    const float alpha = m == -INFINITY ? 0.f : exp2f(m - mn);
    const float pj = valid ? exp2f(s - mn) : 0.f;
    m = mn;
    l = l * alpha + pj;  // the denominator sums the undropped P
    float pk = pj;
    if (DROP) {
      const unsigned int rr = hash_rng32(
          seed32, drop_idx<true>(qrow, (unsigned int)key, T_rows));
      pk = (rr * 2.3283064365386963e-10f) >= p ? pj * inv_keep : 0.f;
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] = acc[d] * alpha + pk * v[d];
  }

  // merge the eight groups; group 0 always holds key 0, so M is finite
  const float M = cross_max(m);
  const float w = m == -INFINITY ? 0.f : exp2f(m - M);
  l = cross_sum(l * w);
  const float invl = 1.f / l;  // l >= 1: the key at the maximum gives P = 1
#pragma unroll
  for (int d = 0; d < 8; ++d) acc[d] = cross_sum(acc[d] * w) * invl;
  if (sub == 0) store8<T>(orow, acc);
  if (!INFER && lane == 0) lse[(long)h * rows_out + i] = M + log2f(l);
}

// ---------------------------------------------------------------------------
// backward: recompute P from lse; the wave writes dK and dV of its sequence's
// rows and dQ of the first row. dqkv arrives zero-filled.
// ---------------------------------------------------------------------------

template <typename T, bool DROP>
__global__ __launch_bounds__(CLS_THREADS)
void cls_attn_bwd_kernel(const T* __restrict__ dout,
                         const T* __restrict__ qkv, const T* __restrict__ o,
                         const float* __restrict__ lse,
                         const int* __restrict__ cu_seqlens,
                         T* __restrict__ dqkv,
                         const unsigned long long* __restrict__ seed_base,
                         unsigned long long salt, float scale, float p, int nh,
                         int T_rows, int B, int rows_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int i = blockIdx.x;
  const int h = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (h >= nh) return;  // wave-uniform
  const int sub = lane >> 3, c = lane & 7;
  const long H = (long)nh * 64, ld = 3 * H;

  long row0;
  const int len = cls_bounds(cu_seqlens, i, B, T_rows, row0);
  if (len <= 0) return;  // wave-uniform: nothing of dqkv belongs to this wave

  const long col = (long)h * 64 + c * 8;
  const T* qp = qkv + row0 * ld + col;
  const T* kp = qp + H;
  const T* vp = qp + 2 * H;
  T* dqp = dqkv + row0 * ld + col;
  T* dkp = dqp + H;
  T* dvp = dqp + 2 * H;
  const unsigned long long seed = DROP ? (*seed_base + salt) : 0ull;
  const unsigned int seed32 = (unsigned int)(seed ^ (seed >> 32));
  const float inv_keep = DROP ? 1.f / (1.f - p) : 1.f;
  const unsigned int qrow = (unsigned int)((long)h * T_rows + row0);

  float q[8], dO[8], ov[8];
  load8<T>(qp, q);
  load8<T>(dout + (long)i * H + col, dO);
  load8<T>(o + (long)i * H + col, ov);
  // D = dO·O = sum_j P_j dP_j, also under dropout (O holds the kept P)
  float dsum = 0.f;
#pragma unroll
  for (int d = 0; d < 8; ++d) dsum += dO[d] * ov[d];
  const float D = group_sum(dsum);
  const float L = lse[(long)h * rows_out + i];
  const float scale2 = scale * LOG2E;

  float dq[8] = {};
  for (int j0 = 0; j0 < len; j0 += 8) {  // wave-uniform trip count
    const int key = j0 + sub;
    const bool valid = key < len;
    const long kr = valid ? key : len - 1;
    float k[8], v[8];
    load8<T>(kp + kr * ld, k);
    load8<T>(vp + kr * ld, v);
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      s += q[d] * k[d];
      dp += dO[d] * v[d];
    }
    s = group_sum(s);
    dp = group_sum(dp);
    const float P = exp2f(s * scale2 - L);
    float keep = 1.f;
    if (DROP) {
      const unsigned int rr = hash_rng32(
          seed32, drop_idx<true>(qrow, (unsigned int)key, T_rows));
      keep = (rr * 2.3283064365386963e-10f) >= p ? inv_keep : 0.f;
    }
    const float dS = valid ? P * (dp * keep - D) * scale : 0.f;
    const float pd = P * keep;
    float dk[8], dv[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      dk[d] = dS * q[d];
      dv[d] = pd * dO[d];
      dq[d] += dS * k[d];
    }
    if (valid) {
      store8<T>(dkp + kr * ld, dk);
      store8<T>(dvp + kr * ld, dv);
    }
  }
#pragma unroll
  for (int d = 0; d < 8; ++d) dq[d] = cross_sum(dq[d]);
  if (sub == 0) store8<T>(dqp, dq);
}

void check_cls_args(const torch::Tensor& qkv, const torch::Tensor& cu_seqlens,
                    long rows_out, long max_seqlen, long nh) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 2,
              "cls_attn: qkv must be contiguous [T, 3H]");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 ||
                  qkv.scalar_type() == torch::kHalf,
              "cls_attn: bf16/fp16 only");
  TORCH_CHECK(nh >= 1 && qkv.size(1) == 3 * nh * 64,
              "cls_attn: head_dim must be 64 and qkv last dim 3*nh*64");
  TORCH_CHECK(qkv.size(0) > 0 && nh * qkv.size(0) <= (1L << 22),
              "cls_attn: T must be positive and nh*T <= 2^22 (32-bit dropout "
              "counter)");
  TORCH_CHECK((size_t)qkv.data_ptr() % 16 == 0,
              "cls_attn: qkv must be 16-byte aligned");
  TORCH_CHECK(cu_seqlens.is_cuda() && cu_seqlens.is_contiguous() &&
                  cu_seqlens.dim() == 1 && cu_seqlens.numel() >= 2 &&
                  cu_seqlens.scalar_type() == torch::kInt,
              "cls_attn: cu_seqlens must be a contiguous cuda int32 [B+1]");
  TORCH_CHECK(rows_out >= cu_seqlens.numel() - 1,
              "cls_attn: rows_out must be at least the number of sequences");
  TORCH_CHECK(max_seqlen >= 1 && max_seqlen <= 1024,
              "cls_attn: max_seqlen must be in [1, 1024]");
}

const unsigned long long* cls_seed(double p, const torch::Tensor& seed_buf) {
  if (!(p > 0.0)) return nullptr;
  TORCH_CHECK(p < 1.0 && seed_buf.defined() && seed_buf.is_cuda() &&
                  seed_buf.scalar_type() == torch::kLong,
              "cls_attn: dropout needs p < 1 and a cuda int64 seed buffer");
  return (const unsigned long long*)seed_buf.data_ptr();
}

// runs the lambda with scalar_t bound to the 16-bit type (check_cls_args)
#define CLS_DISPATCH(DTYPE, ...)                                               \
  [&] {                                                                        \
    if ((DTYPE) == at::ScalarType::BFloat16) {                                 \
      using scalar_t = __hip_bfloat16;                                         \
      return __VA_ARGS__();                                                    \
    } else {                                                                   \
      using scalar_t = __half;                                                 \
      return __VA_ARGS__();                                                    \
    }                                                                          \
  }()

template <bool INFER>
void cls_fwd_launch(const torch::Tensor& qkv, const torch::Tensor& cu_seqlens,
                    torch::Tensor& o, float* lse, long rows_out, long nh,
                    double scale, double p,
                    const unsigned long long* seed, long salt) {
  const dim3 grid(rows_out, (nh + 3) / 4);
  const int B = (int)cu_seqlens.numel() - 1;
  CLS_DISPATCH(qkv.scalar_type(), [&] {
    DISPATCH_BOOL(seed != nullptr, DROP_, [&] {
      constexpr bool DROP = DROP_ && !INFER;
      hipLaunchKernelGGL(
          (cls_attn_fwd_kernel<scalar_t, DROP, INFER>), grid,
          dim3(CLS_THREADS), 0, at::hip::getCurrentHIPStream(),
          (const scalar_t*)qkv.data_ptr(), (const int*)cu_seqlens.data_ptr(),
          (scalar_t*)o.data_ptr(), lse, seed, (unsigned long long)salt,
          (float)scale, (float)p, (int)nh, (int)qkv.size(0), B,
          (int)rows_out);
    });
  });
}

}  // namespace

// The launch shape is a function of (rows_out, nh) alone; max_seqlen is
// validated against the 1024-key clamp of varlen_len and otherwise unused.
std::vector<torch::Tensor> cls_attn_fwd(torch::Tensor qkv,
                                        torch::Tensor cu_seqlens,
                                        long rows_out, long max_seqlen,
                                        long nh, double scale, double p,
                                        torch::Tensor seed_buf, long salt) {
  check_cls_args(qkv, cu_seqlens, rows_out, max_seqlen, nh);
  const unsigned long long* seed = cls_seed(p, seed_buf);
  // no fill launch: every (row, head) slice of o and lse has an owner
  auto o = torch::empty({rows_out, nh * 64}, qkv.options());
  auto lse = torch::empty({nh, rows_out}, qkv.options().dtype(torch::kFloat));
  cls_fwd_launch<false>(qkv, cu_seqlens, o, (float*)lse.data_ptr(), rows_out,
                        nh, scale, p, seed, salt);
  return {o, lse};
}

// Serving form: the bits of cls_attn_fwd's o at p = 0, no lse.
torch::Tensor cls_attn_infer(torch::Tensor qkv, torch::Tensor cu_seqlens,
                             long rows_out, long max_seqlen, long nh,
                             double scale) {
  check_cls_args(qkv, cu_seqlens, rows_out, max_seqlen, nh);
  auto o = torch::empty({rows_out, nh * 64}, qkv.options());
  cls_fwd_launch<true>(qkv, cu_seqlens, o, nullptr, rows_out, nh, scale, 0.0,
                       nullptr, 0);
  return o;
}

torch::Tensor cls_attn_bwd(torch::Tensor dout, torch::Tensor qkv,
                           torch::Tensor o, torch::Tensor lse,
                           torch::Tensor cu_seqlens, long max_seqlen, long nh,
                           double scale, double p, torch::Tensor seed_buf,
                           long salt) {
  TORCH_CHECK(dout.dim() == 2, "cls_attn: dout must be [rows_out, H]");
  const long rows_out = dout.size(0), H = nh * 64;
  check_cls_args(qkv, cu_seqlens, rows_out, max_seqlen, nh);
  TORCH_CHECK(dout.is_cuda() && dout.is_contiguous() &&
                  dout.scalar_type() == qkv.scalar_type() &&
                  dout.size(1) == H && (size_t)dout.data_ptr() % 16 == 0,
              "cls_attn: dout must be contiguous [rows_out, H] of qkv dtype");
  TORCH_CHECK(o.is_cuda() && o.is_contiguous() &&
                  o.scalar_type() == qkv.scalar_type() &&
                  o.sizes() == dout.sizes() &&
                  (size_t)o.data_ptr() % 16 == 0 && lse.is_cuda() &&
                  lse.is_contiguous() &&
                  lse.scalar_type() == torch::kFloat &&
                  lse.numel() == nh * rows_out,
              "cls_attn: o [rows_out, H] / lse [nh, rows_out] from the "
              "forward");
  const unsigned long long* seed = cls_seed(p, seed_buf);
  // zero-filled: q columns of the non-first rows and every row outside the
  // sequences have no owner in the kernel
  auto dqkv = torch::zeros_like(qkv);
  const dim3 grid(rows_out, (nh + 3) / 4);
  const int B = (int)cu_seqlens.numel() - 1;
  CLS_DISPATCH(qkv.scalar_type(), [&] {
    DISPATCH_BOOL(seed != nullptr, DROP, [&] {
      hipLaunchKernelGGL(
          (cls_attn_bwd_kernel<scalar_t, DROP>), grid, dim3(CLS_THREADS), 0,
          at::hip::getCurrentHIPStream(), (const scalar_t*)dout.data_ptr(),
          (const scalar_t*)qkv.data_ptr(), (const scalar_t*)o.data_ptr(),
          (const float*)lse.data_ptr(), (const int*)cu_seqlens.data_ptr(),
          (scalar_t*)dqkv.data_ptr(), seed, (unsigned long long)salt,
          (float)scale, (float)p, (int)nh, (int)qkv.size(0), B,
          (int)rows_out);
    });
  });
  return dqkv;
}
