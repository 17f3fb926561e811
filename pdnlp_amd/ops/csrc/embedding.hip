// Fused embedding gather + add + LayerNorm and its backward
// (embedding scatter-add, SURVEY.md K11 note).
//
// Forward: one wavefront per token row; gathers word/position/token-type
// rows, sums in fp32, LayerNorm with fp32 stats — one kernel instead of the
// reference's three embedding gathers + add + LN (vendor kernels inside HF
// BERT, reference call site multi-gpu-distributed-cls.py:132-136).
//
// Backward, without float atomics, fp32 tables or fill/cast pairs:
//  (1) row pass: one wave per token row recomputes the summed embedding
//      (gather is cheaper than saving [R,H]), applies the LN-input gradient
//      formula and stores dsum once as an fp32 contribution row ws[R,H]. dsum
//      is the gradient of ALL THREE tables at this row's indices;
//  (2) index pass: per destination (a row of the word, position or type
//      table) the number of contribution rows and the first of them, by
//      integer atomics whose result does not depend on their order;
//  (3) sum pass: one workgroup per destination row finds its rows in
//      ascending order, sums them in that order and writes the row once in
//      the table dtype — zeros for an untouched row. A destination with more
//      than CH rows (token type 0: every row; pad id 0 of a padded batch) is
//      split into row ranges of CH summed by separate workgroups, (4) whose
//      partials are added in range order;
//  (5, 6) dLNw/dLNb: deterministic two-stage column reduction.
// Every sum has a fixed order, so all five results repeat bit for bit.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <climits>

#include "common.h"

namespace {

template <typename T>
__global__ void emb_ln_fwd_kernel(
    const long* __restrict__ ids, const long* __restrict__ type_ids,
    const long* __restrict__ pos_ids, const T* __restrict__ word,
    const T* __restrict__ pos, const T* __restrict__ type_,
    const T* __restrict__ w, const T* __restrict__ b, T* __restrict__ y,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, int H,
    float eps) {
  const int row = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const T* wr = word + (long)ids[row] * H;
  const T* pr = pos + (long)pos_ids[row] * H;
  const T* tr = type_ + (long)type_ids[row] * H;
  T* yr = y + (long)row * H;

  // one-pass statistics of x - shift (see shifted_stats in common.h)
  const float shift = to_f32<T>(wr[0]) + to_f32<T>(pr[0]) + to_f32<T>(tr[0]);
  float sum = 0.f, sumsq = 0.f;
  for (int c = lane; c < H; c += WAVE) {
    const float v =
        to_f32<T>(wr[c]) + to_f32<T>(pr[c]) + to_f32<T>(tr[c]) - shift;
    sum += v;
    sumsq += v * v;
  }
  float md, mean, rstd;  // md = mean - shift
  shifted_stats(wave_sum(sum), wave_sum(sumsq), shift, H, eps, md, mean, rstd);
  if (lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
  for (int c = lane; c < H; c += WAVE) {
    const float v = to_f32<T>(wr[c]) + to_f32<T>(pr[c]) + to_f32<T>(tr[c]);
    yr[c] = from_f32<T>((v - shift - md) * rstd * to_f32<T>(w[c]) +
                        to_f32<T>(b[c]));
  }
}

// ---- backward --------------------------------------------------------------

constexpr int EMB_LIST_MAX = 1024;  // longest row list one workgroup sums

// The three tables as one destination space [0, D): word rows, then position
// rows, then type rows. Selected by wave-uniform compares, never indexed.
struct EmbTabs {
  const long* idx0; const long* idx1; const long* idx2;  // [R] row -> index
  void* out0; void* out1; void* out2;                    // [rows_t, H]
  int rows0, rows1, rows2;
};

// int workspace: count[D], head[D], nheavy, heavy[maxslot]
struct EmbIndex {
  int* count;   // contribution rows of a destination
  int* head;    // the first of them
  int* nheavy;  // destinations with more than ch rows ...
  int* heavy;   // ... and their list, in no particular order
  int D, ch, nch, maxslot;
};

// (1) One wave per token row: ws[row] = dsum in fp32. The wave also clears
// its share of the index workspace, which the next launch fills.
template <typename T>
__global__ void emb_ln_bwd_row_kernel(
    const T* __restrict__ dy, const long* __restrict__ ids,
    const long* __restrict__ type_ids, const long* __restrict__ pos_ids,
    const T* __restrict__ word, const T* __restrict__ pos,
    const T* __restrict__ type_, const T* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ ws, EmbIndex ix, int H) {
  const int row = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  for (long i = (long)row * WAVE + lane; i < ix.D;
       i += (long)gridDim.x * WAVE) {
    ix.count[i] = 0;
    ix.head[i] = INT_MAX;
  }
  if (row == 0 && lane == 0) *ix.nheavy = 0;

  const T* dyr = dy + (long)row * H;
  const T* wr = word + (long)ids[row] * H;
  const T* pr = pos + (long)pos_ids[row] * H;
  const T* tr = type_ + (long)type_ids[row] * H;
  const float mu = mean[row], rs = rstd[row];

  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < H; c += WAVE) {
    const float dyw = to_f32<T>(dyr[c]) * to_f32<T>(w[c]);
    const float x = to_f32<T>(wr[c]) + to_f32<T>(pr[c]) + to_f32<T>(tr[c]);
    const float xh = (x - mu) * rs;
    s1 += dyw;
    s2 += dyw * xh;
  }
  s1 = wave_sum(s1) / H;
  s2 = wave_sum(s2) / H;
  for (int c = lane; c < H; c += WAVE) {
    const float dyw = to_f32<T>(dyr[c]) * to_f32<T>(w[c]);
    const float x = to_f32<T>(wr[c]) + to_f32<T>(pr[c]) + to_f32<T>(tr[c]);
    const float xh = (x - mu) * rs;
    ws[(long)row * H + c] = rs * (dyw - s1 - xh * s2);
  }
}

// (2) Thread per (row, table): count and first row of every destination.
// Lanes of a wave that share a destination go through their lowest lane (the
// lowest row), so token type 0 costs one atomic per wave, not one per row.
// The arrival that takes a count past ch enters the destination in the heavy
// list; its slot number depends on timing, the sums do not.
__global__ __launch_bounds__(256)
void emb_ln_bwd_index_kernel(EmbTabs tb, EmbIndex ix, int R) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = blockIdx.y;
  const long* idx = t == 0 ? tb.idx0 : t == 1 ? tb.idx1 : tb.idx2;
  const int rows = t == 0 ? tb.rows0 : t == 1 ? tb.rows1 : tb.rows2;
  const int off = t == 0 ? 0 : t == 1 ? tb.rows0 : tb.rows0 + tb.rows1;
  long v = -1;
  if (r < R) v = idx[r];
  const bool valid = v >= 0 && v < rows;
  const int d = off + (int)v;
  bool leader = false;
  int n = 0;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int l = __ffsll((long long)todo) - 1;
    const int dl = __shfl(d, l, WAVE);
    const unsigned long long m = __ballot(valid && d == dl);
    if (lane == l) {
      leader = true;
      n = __popcll(m);
    }
    todo &= ~m;
  }
  if (leader) {
    const int old = atomicAdd(ix.count + d, n);
    atomicMin(ix.head + d, r);
    if (old <= ix.ch && old + n > ix.ch) {
      const int s = atomicAdd(ix.nheavy, 1);
      if (s < ix.maxslot) ix.heavy[s] = d;
    }
  }
}

// table, index array and output row of destination d (block-uniform)
__device__ __forceinline__ void emb_dest(const EmbTabs& tb, int d,
                                         const long*& idx, long& v,
                                         void*& out) {
  if (d < tb.rows0) {
    idx = tb.idx0; v = d; out = tb.out0;
  } else if (d < tb.rows0 + tb.rows1) {
    idx = tb.idx1; v = d - tb.rows0; out = tb.out1;
  } else {
    idx = tb.idx2; v = d - tb.rows0 - tb.rows1; out = tb.out2;
  }
}

typedef float emb_f4 __attribute__((ext_vector_type(4)));

// sum of the n rows list[0..n) of ws at 4 columns, in list order, 8 loads in
// flight; the tail repeats the last row's load and drops the value.
// `round_t`: each term is rounded to T first. The position and type tables
// have always summed the T-rounded dsum (their kernels read a [R,H]
// workspace of T); keeping that keeps their bf16/fp16 gradients at what
// they were up to the order of the fp32 additions.
template <typename T>
__device__ __forceinline__ emb_f4 emb_sum_rows(const float* __restrict__ ws,
                                               const int* list, int n, int H,
                                               int col, bool round_t) {
  emb_f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < n; k += 8) {
    emb_f4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = list[min(k + j, n - 1)];
      v[j] = *reinterpret_cast<const emb_f4*>(ws + (long)row * H + col);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool keep = k + j < n;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float x = v[j][q];
        if (round_t) x = to_f32<T>(from_f32<T>(x));
        acc[q] += keep ? x : 0.f;
      }
    }
  }
  return acc;
}

template <typename T>
__device__ __forceinline__ void emb_store_row(void* out, long v, int H,
                                              int col, emb_f4 acc) {
  v4_t<T> o;
#pragma unroll
  for (int q = 0; q < 4; ++q) set_elem<T>(o, q, acc[q]);
  st4<T>((T*)out + v * H + col, o);
}

// (3) Workgroups [0, maxslot*nch): range c of heavy slot s -> part[s][c][H].
// Workgroups behind them: one destination row each, written in T. Wave w of
// a workgroup owns columns [256w, 256w+256), 4 per lane; wave 0 finds the
// rows: it compares 256 indices per round trip and appends the matches in
// ascending row order.
template <typename T>
__global__ void emb_ln_bwd_sum_kernel(const float* __restrict__ ws,
                                      EmbTabs tb, EmbIndex ix,
                                      float* __restrict__ part, int R,
                                      int H) {
  __shared__ int list[EMB_LIST_MAX];
  __shared__ int nlist;
  const int lane = threadIdx.x & (WAVE - 1);
  const int col = (threadIdx.x >> 6) * 256 + lane * 4;
  const bool colok = col < H;
  const int nitems = ix.maxslot * ix.nch;
  const bool item = (int)blockIdx.x < nitems;

  int d, r0, r1, want;
  long pslab = 0;
  if (item) {
    const int s = blockIdx.x / ix.nch, c = blockIdx.x % ix.nch;
    if (s >= min(*ix.nheavy, ix.maxslot)) return;
    d = ix.heavy[s];
    r0 = c * ix.ch;
    r1 = min(R, r0 + ix.ch);
    want = ix.ch;
    pslab = (long)blockIdx.x * H;
  } else {
    d = blockIdx.x - nitems;
    want = ix.count[d];
    if (want > ix.ch) return;  // heavy: the items above and the fold
    r0 = ix.head[d];
    r1 = R;
  }
  const long* idx;
  long v;
  void* out;
  emb_dest(tb, d, idx, v, out);
  if (want == 0) {
    if (colok) emb_store_row<T>(out, v, H, col, emb_f4{0.f, 0.f, 0.f, 0.f});
    return;
  }

  if (threadIdx.x < WAVE) {
    int found = 0;
    if (!item && want == 1) {
      if (lane == 0) list[0] = r0;
      found = 1;
    } else {
      for (int base = r0; base < r1 && found < want; base += 4 * WAVE) {
        long x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = base + j * WAVE + lane;
          x[j] = idx[min(r, r1 - 1)];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = base + j * WAVE + lane;
          const bool hit = r < r1 && x[j] == v;
          const unsigned long long m = __ballot(hit);
          const int at = found + __popcll(m & ((1ull << lane) - 1ull));
          if (hit && at < EMB_LIST_MAX) list[at] = r;
          found += __popcll(m);
        }
      }
    }
    if (lane == 0) nlist = min(found, EMB_LIST_MAX);
  }
  __syncthreads();
  if (!colok) return;
  const emb_f4 acc = emb_sum_rows<T>(ws, list, nlist, H, col, d >= tb.rows0);
  if (item)
    *reinterpret_cast<emb_f4*>(part + pslab + col) = acc;
  else
    emb_store_row<T>(out, v, H, col, acc);
}

// (4) One workgroup per heavy slot: its range partials in range order.
template <typename T>
__global__ void emb_ln_bwd_fold_kernel(const float* __restrict__ part,
                                       EmbTabs tb, EmbIndex ix, int H) {
  const int s = blockIdx.x;
  if (s >= min(*ix.nheavy, ix.maxslot)) return;
  const int col = (threadIdx.x >> 6) * 256 + (threadIdx.x & (WAVE - 1)) * 4;
  if (col >= H) return;
  const long* idx;
  long v;
  void* out;
  emb_dest(tb, ix.heavy[s], idx, v, out);
  const float* p = part + (long)s * ix.nch * H + col;
  emb_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int c = 0; c < ix.nch; ++c) {
    const emb_f4 x = *reinterpret_cast<const emb_f4*>(p + (long)c * H);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += x[q];
  }
  emb_store_row<T>(out, v, H, col, acc);
}

// (5) dLNw/dLNb partials [chunk][2][H], laid out as bdrl_bwd_dwdb_kernel
// (fused_epilogue.hip): block = 16 row strips x 16 column quads over 64
// columns, 4-element loads, strips folded through LDS in strip order. x-hat
// is recomputed from the three gathered rows as the row pass does.
template <typename T>
__global__ __launch_bounds__(256)
void emb_ln_bwd_dwdb_kernel(
    const T* __restrict__ dy, const long* __restrict__ ids,
    const long* __restrict__ type_ids, const long* __restrict__ pos_ids,
    const T* __restrict__ word, const T* __restrict__ pos,
    const T* __restrict__ type_, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ part, int R, int H,
    int rows_per_chunk) {
  __shared__ float lds[16][2][64];
  const int quad = threadIdx.x & 15;
  const int strip = threadIdx.x >> 4;
  const int c0 = blockIdx.x * 64 + quad * 4;
  const int r0 = blockIdx.y * rows_per_chunk;
  const int r1 = min(r0 + rows_per_chunk, R);
  float dw[4] = {}, db[4] = {};
  if (c0 < H) {
    for (int r = r0 + strip; r < r1; r += 16) {
      const float mu = mean[r], rs = rstd[r];
      const v4_t<T> dv = ld4(dy + (long)r * H + c0);
      const v4_t<T> wv = ld4(word + (long)ids[r] * H + c0);
      const v4_t<T> pv = ld4(pos + (long)pos_ids[r] * H + c0);
      const v4_t<T> tv = ld4(type_ + (long)type_ids[r] * H + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = elem<T>(dv, j);
        const float x = elem<T>(wv, j) + elem<T>(pv, j) + elem<T>(tv, j);
        const float xh = (x - mu) * rs;
        dw[j] += d * xh;
        db[j] += d;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lds[strip][0][quad * 4 + j] = dw[j];
    lds[strip][1][quad * 4 + j] = db[j];
  }
  __syncthreads();
  if (threadIdx.x < 2 * 64) {
    const int kind = threadIdx.x >> 6, colb = threadIdx.x & 63;
    const int gc = blockIdx.x * 64 + colb;
    if (gc < H) {
      float s = 0.f;
#pragma unroll
      for (int st = 0; st < 16; ++st) s += lds[st][kind][colb];
      part[(long)blockIdx.y * 2 * H + kind * H + gc] = s;
    }
  }
}

}  // namespace

std::vector<torch::Tensor> embedding_ln_fwd(
    torch::Tensor ids, torch::Tensor type_ids, torch::Tensor pos_ids,
    torch::Tensor word, torch::Tensor pos, torch::Tensor type_,
    torch::Tensor w, torch::Tensor b, double eps) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == torch::kLong);
  const int H = word.size(1);
  const long R = ids.numel();
  auto y = torch::empty({ids.size(0), ids.size(1), H}, word.options());
  auto mean = torch::empty({R}, word.options().dtype(torch::kFloat32));
  auto rstd = torch::empty({R}, word.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_FLOAT_TYPES(word.scalar_type(), "embedding_ln_fwd", [&] {
    hipLaunchKernelGGL((emb_ln_fwd_kernel<scalar_t>), dim3(R), dim3(WAVE), 0,
                       stream,
                       ids.data_ptr<long>(), type_ids.data_ptr<long>(),
                       pos_ids.data_ptr<long>(),
                       (const scalar_t*)word.data_ptr(),
                       (const scalar_t*)pos.data_ptr(),
                       (const scalar_t*)type_.data_ptr(),
                       (const scalar_t*)w.data_ptr(),
                       (const scalar_t*)b.data_ptr(), (scalar_t*)y.data_ptr(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), H,
                       (float)eps);
  });
  return {y, mean, rstd};
}

std::vector<torch::Tensor> embedding_ln_bwd(
    torch::Tensor dy, torch::Tensor ids, torch::Tensor type_ids,
    torch::Tensor pos_ids, torch::Tensor word, torch::Tensor pos,
    torch::Tensor type_, torch::Tensor w, torch::Tensor mean,
    torch::Tensor rstd) {
  const int H = word.size(1);
  const long R = ids.numel();
  TORCH_CHECK(H % 4 == 0 && H <= 4096,
              "embedding_ln_bwd: hidden size must be a multiple of 4, <= 4096");
  TORCH_CHECK(R > 0 && R < INT_MAX / WAVE, "embedding_ln_bwd: bad row count");
  TORCH_CHECK(ids.is_contiguous() && type_ids.is_contiguous() &&
              pos_ids.is_contiguous() && dy.is_contiguous());
  const long D = word.size(0) + pos.size(0) + type_.size(0);
  TORCH_CHECK(D < INT_MAX, "embedding_ln_bwd: tables too large");

  // A destination with more than ch rows is summed in row ranges of ch by
  // separate workgroups: ch rows of 1 KiB per wave is about one round of
  // latency-bound reading, and R / 32 keeps the ranges of a destination that
  // takes every row (a token type) at 32, whatever R is.
  EmbIndex ix;
  ix.ch = (int)std::min<long>(EMB_LIST_MAX, std::max<long>(128, (R + 31) / 32));
  ix.nch = (int)((R + ix.ch - 1) / ix.ch);
  ix.maxslot = 3 * ix.nch;  // more than ch rows each, R rows per table
  ix.D = (int)D;

  auto opts32 = word.options().dtype(torch::kFloat32);
  auto ws = torch::empty({R, (long)H}, opts32);
  auto ibuf = torch::empty({2 * D + 1 + ix.maxslot},
                           word.options().dtype(torch::kInt32));
  auto part = torch::empty({(long)ix.maxslot * ix.nch, (long)H}, opts32);
  const int rows_per_chunk = (int)((R + 31) / 32);
  const int chunks = (int)((R + rows_per_chunk - 1) / rows_per_chunk);
  auto cpart = torch::empty({(long)chunks, 2L, (long)H}, opts32);
  auto dword = torch::empty({word.size(0), (long)H}, word.options());
  auto dpos = torch::empty({pos.size(0), (long)H}, word.options());
  auto dtype_ = torch::empty({type_.size(0), (long)H}, word.options());
  auto dln = torch::empty({2L, (long)H}, word.options());

  ix.count = ibuf.data_ptr<int>();
  ix.head = ix.count + D;
  ix.nheavy = ix.head + D;
  ix.heavy = ix.nheavy + 1;
  EmbTabs tb;
  tb.idx0 = ids.data_ptr<long>();
  tb.idx1 = pos_ids.data_ptr<long>();
  tb.idx2 = type_ids.data_ptr<long>();
  tb.out0 = dword.data_ptr();
  tb.out1 = dpos.data_ptr();
  tb.out2 = dtype_.data_ptr();
  tb.rows0 = (int)word.size(0);
  tb.rows1 = (int)pos.size(0);
  tb.rows2 = (int)type_.size(0);

  auto stream = at::hip::getCurrentHIPStream();
  const int ncg = (H + 255) / 256;  // waves per destination row
  DISPATCH_FLOAT_TYPES(word.scalar_type(), "embedding_ln_bwd", [&] {
    hipLaunchKernelGGL((emb_ln_bwd_row_kernel<scalar_t>), dim3(R), dim3(WAVE),
                       0, stream,
                       (const scalar_t*)dy.data_ptr(), ids.data_ptr<long>(),
                       type_ids.data_ptr<long>(), pos_ids.data_ptr<long>(),
                       (const scalar_t*)word.data_ptr(),
                       (const scalar_t*)pos.data_ptr(),
                       (const scalar_t*)type_.data_ptr(),
                       (const scalar_t*)w.data_ptr(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), ws.data_ptr<float>(), ix, H);
    hipLaunchKernelGGL(emb_ln_bwd_index_kernel, dim3((R + 255) / 256, 3),
                       dim3(256), 0, stream, tb, ix, (int)R);
    hipLaunchKernelGGL((emb_ln_bwd_sum_kernel<scalar_t>),
                       dim3(ix.maxslot * ix.nch + (int)D), dim3(WAVE * ncg), 0,
                       stream, ws.data_ptr<float>(), tb, ix,
                       part.data_ptr<float>(), (int)R, H);
    hipLaunchKernelGGL((emb_ln_bwd_fold_kernel<scalar_t>), dim3(ix.maxslot),
                       dim3(WAVE * ncg), 0, stream, part.data_ptr<float>(),
                       tb, ix, H);
    hipLaunchKernelGGL((emb_ln_bwd_dwdb_kernel<scalar_t>),
                       dim3((H + 63) / 64, chunks), dim3(256), 0, stream,
                       (const scalar_t*)dy.data_ptr(), ids.data_ptr<long>(),
                       type_ids.data_ptr<long>(), pos_ids.data_ptr<long>(),
                       (const scalar_t*)word.data_ptr(),
                       (const scalar_t*)pos.data_ptr(),
                       (const scalar_t*)type_.data_ptr(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       cpart.data_ptr<float>(), (int)R, H, rows_per_chunk);
    hipLaunchKernelGGL((reduce_cols_cast_kernel<scalar_t>),
                       dim3((2 * H + 63) / 64), dim3(256), 0, stream,
                       cpart.data_ptr<float>(), (scalar_t*)dln.data_ptr(),
                       (long)(2 * H), chunks);
  });
  return {dword, dpos, dtype_, dln[0], dln[1]};
}
