// Conventions shared by every attention kernel over a packed token stream
// (attention.hip, cls_attention.hip): the dropout counter and the clamp of a
// sequence's length. One definition, so the kernels cannot drift apart: the
// CLS-only kernel must keep exactly the probabilities the flash kernels keep.
#pragma once

#include "common.h"

// dropout counter for probability (qrow, key): qrow is the head-major row
// (padded: bh*S + row; VARLEN: h*T + packed row), key the key index inside
// the sequence. Identical in forward, dQ and dK/dV. VARLEN strides rows by
// the 1024 key cap instead of S, so nh*T <= 2^22 (host-checked) cannot wrap.
template <bool VARLEN>
__device__ __forceinline__ unsigned int drop_idx(unsigned int qrow,
                                                 unsigned int key, int S) {
  return VARLEN ? (qrow << 10) + key : qrow * S + key;
}

// VARLEN sequence length of batch entry b, clamped so that a bad cu_seqlens
// can neither leave the [T] stream nor the 1024-entry LDS rows
__device__ __forceinline__ int varlen_len(const int* cu_seqlens, long b,
                                          long row0, int T) {
  const long len = cu_seqlens[b + 1] - row0;
  const long cap = T - row0 < 1024 ? T - row0 : 1024;
  return (int)(len < cap ? len : cap);
}
