// Device and launch helpers shared by the toolbox units only (ot.hip, gpr.hip, register.hip, neighbors.hip).  The step
// engine's units do not include this header: what they compile from does not change when it does.
#pragma once
#include "common.hpp"

namespace gpsa {

// Maximum over the 64 lanes of a wave, returned in every lane: wave_sum's moves with fmax in place of +
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, dpp_move<0xB1>(v));
  v = fmax(v, dpp_move<0x4E>(v));
  v = fmax(v, dpp_move<0x141>(v));
  v = fmax(v, dpp_move<0x140>(v));
  return fmax(fmax(lane_value(v, 0), lane_value(v, 16)), fmax(lane_value(v, 32), lane_value(v, 48)));
}

// (d, j) < (bd, bj) in the order of the key (distance, index): a total order, so a minimum or a sorted list by it does
// not depend on how the candidates were cut into slices
__device__ __forceinline__ bool key_less(double d, int j, double bd, int bj) {
  return d < bd || (d == bd && j < bj);
}

// The closing of a 256-thread workgroup over three sums: every thread's (s0, s1, s2) into red, then the LDS tree
// h = 128 .. 1, thread t adding element t + h to its own.  On return red[q][0] is sum q, visible to every thread.
__device__ __forceinline__ void fold3_256(double s0, double s1, double s2, double (*red)[256]) {
  const int tid = threadIdx.x;
  red[0][tid] = s0, red[1][tid] = s1, red[2][tid] = s2;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[0][tid] += red[0][tid + h], red[1][tid] += red[1][tid + h], red[2][tid] += red[2][tid + h];
    __syncthreads();
  }
}

// ... over the triples part [nblk][3] of earlier workgroups: thread t takes blocks t, t + 256, ... in order
__device__ __forceinline__ void fold3_partials(const double* __restrict__ part, long long nblk, double (*red)[256]) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long b = threadIdx.x; b < nblk; b += 256) s0 += part[b * 3], s1 += part[b * 3 + 1], s2 += part[b * 3 + 2];
  fold3_256(s0, s1, s2, red);
}

// rows [r0, r0 + 64) of X [n, D] into LDS, padded with zeros to MAXD coordinates and beyond n; t = 0 .. 63 is the
// staging thread's row (any other t: not a staging thread)
__device__ __forceinline__ void stage_rows64(const double* __restrict__ X, long long n, int D, long long r0, int t,
                                             double (*xs)[MAXD]) {
  if (t >= 0 && t < 64) {
    const long long r = r0 + t;
#pragma unroll
    for (int d = 0; d < MAXD; ++d) xs[t][d] = (r < n && d < D) ? X[r * D + d] : 0.0;
  }
}

// The number of slices of a streamed axis of axis_len rows: the caller's (at most one per row), or for 0 enough of them
// that about four workgroups per compute unit are in flight next to the `blocks` workgroups of one slice, each slice at
// least one LDS tile long; max_parts at most
static inline int slice_parts(long long blocks, long long axis_len, long long tile, long long max_parts, int caller_parts) {
  long long p = caller_parts;
  if (p == 0) {
    const long long want = 4LL * num_cus();
    p = blocks >= want ? 1 : cdiv(want, blocks);
    p = min(p, cdiv(axis_len, tile));
  }
  p = min(p, axis_len);
  p = min(p, max_parts);
  return (int)max(p, 1LL);
}

}  // namespace gpsa
