// What counts.hip, counts_sparse.hip and moments.hip share (no other unit includes this): how a wave walks a row of a
// dense column tile or of a CSR matrix inside a column tile, the Poisson term of the deviance, the order in which four
// partial sums meet, the host checks of the entries.  Each kernel keeps its own accumulation; the tile and group
// constants stay in the units and come in as arguments.  Device code is compiled with floating-point contraction on: a
// function here is the statements its callers had, in their operand order (tests/test_count_walk_bits_gpu.py).
#pragma once
#include <math.h>

#include "common.hpp"

namespace gpsa {

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// the column inside the tile of a lane's k-th value (VEC: float4 loads, quads of consecutive columns per lane)
template <bool VEC>
__device__ __forceinline__ int tile_col(int lane, int k) {
  return VEC ? (k >> 2) * 256 + lane * 4 + (k & 3) : k * WAVE + lane;
}

// a lane's PER_LANE values of the row at `row` in the tile that starts at column c0; columns beyond P read as 0
template <bool VEC, int PER_LANE>
__device__ __forceinline__ void load_row(const float* row, long long c0, long long P, int lane, float (&v)[PER_LANE]) {
  if (VEC) {
#pragma unroll
    for (int j = 0; j < PER_LANE / 4; ++j) {
      const long long c = c0 + j * 256 + lane * 4;
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < P) q = *reinterpret_cast<const float4*>(row + c);  // P % 4 == 0: c + 3 < P
      v[4 * j] = q.x, v[4 * j + 1] = q.y, v[4 * j + 2] = q.z, v[4 * j + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      const long long c = c0 + k * WAVE + lane;
      v[k] = c < P ? row[c] : 0.f;
    }
  }
}

// One wave, row i of a CSR matrix, the column tile [c0, c1), c1 <= P: entry(cc, y) is called by the lane that holds it
// for every stored entry with c0 <= column < c1 (cc = column - c0), 64 entries at a time in storage order.  The row's
// range is clamped to [0, nnz] and a row with keep[i] == 0 has no entries: a malformed matrix is never followed outside
// col / val.  Where the row's part of the tile starts is found by a 64-way search over its sorted column indices, one
// load per round and lane, until 64 or fewer candidates remain.
template <class Entry>
__device__ __forceinline__ void csr_row_in_tile(const long long* __restrict__ crow, const int* __restrict__ col,
                                                const float* __restrict__ val, const unsigned char* __restrict__ keep,
                                                long long i, long long nnz, long long c0, long long c1, int lane,
                                                Entry entry) {
  const long long s = clampll(crow[i], 0, nnz), e = clampll(crow[i + 1], s, nnz);
  const long long len = (keep != nullptr && keep[i] == 0) ? 0 : e - s;
  // the first entry at or beyond c0 lies in [lo, hi]: 64 probes per round (wave-uniform lo, hi)
  long long lo = 0, hi = len;
  while (hi - lo > WAVE) {
    const long long step = (hi - lo + WAVE - 1) / WAVE, p = lo + lane * step;
    const bool before = p < hi && (long long)col[s + p] < c0;
    const long long cnt = __popcll(__builtin_amdgcn_ballot_w64(before));
    if (cnt == 0) {
      hi = lo;
    } else {
      hi = min(hi, lo + cnt * step);
      lo = lo + (cnt - 1) * step + 1;
    }
  }
  for (long long pos = lo; pos < len; pos += WAVE) {
    const long long k = pos + lane;
    long long c = c1;
    float y = 0.f;
    if (k < len) c = col[s + k], y = val[s + k];
    const bool below = k < len && c < c1;
    if (below && c >= c0) entry((int)(c - c0), y);  // c0 <= c < c1 <= P: inside the tile, inside the plane
    if (__popcll(__builtin_amdgcn_ballot_w64(below)) < WAVE) break;  // the row's end, or an entry beyond the tile
  }
}

// the workgroup (256 threads) fills table[t] = t log t, 0 at t = 0; synchronise before poisson_terms
template <int TABLE>
__device__ __forceinline__ void ylogy_fill(double* table) {
  for (int t = threadIdx.x; t < TABLE; t += 256) table[t] = t > 0 ? (double)t * log((double)t) : 0.0;
}
// t1 = y log y (from the table for a whole number below TABLE), t2 = y log_sz of a stored y > 0: the one expression
// behind the dense and the CSR deviance, which agree bit for bit wherever their sums run in the same order
template <int TABLE>
__device__ __forceinline__ void poisson_terms(const double* table, float yf, double log_sz, double& t1, double& t2) {
  const double y = (double)yf;
  const int yi = yf < (float)TABLE ? (int)yf : 0;
  t1 = (yi > 0 && (float)yi == yf) ? table[yi] : y * log(y);
  t2 = y * log_sz;
}

// four partial sums (the waves' columns in LDS, the fold's segments) meet left to right
__device__ __forceinline__ double sum4(double a, double b, double c, double d) { return ((a + b) + c) + d; }
template <int W>
__device__ __forceinline__ double meet4(const double (&rows)[4][W], int cc) {
  return sum4(rows[0][cc], rows[1][cc], rows[2][cc], rows[3][cc]);
}

// host: view_off [V + 1] rises strictly from 0 to N (an empty view has no moments), V >= 1: 0 or the refusal
static inline int view_off_check(const long long* view_off, int V, long long N) {
  if (view_off == nullptr || V < 1 || view_off[0] != 0 || view_off[V] != N) return GPSA_EINVAL;
  for (int v = 0; v < V; ++v)
    if (view_off[v + 1] <= view_off[v]) return GPSA_EINVAL;
  return 0;
}
// host: what every CSR entry asks of (crow, col, val, N, P, nnz): 0 or the refusal
static inline int csr_shape_check(const void* crow, const void* col, const void* val, long long N, long long P,
                                  long long nnz) {
  if (crow == nullptr || N < 1 || P < 1 || P > 0x7fffffffLL || N > 0x7fffffffLL) return GPSA_EINVAL;
  if (nnz < 0 || nnz > N * P) return GPSA_EINVAL;  // (N, P < 2^31: no overflow)
  if (nnz > 0 && (col == nullptr || val == nullptr)) return GPSA_EINVAL;
  return 0;
}

}  // namespace gpsa
