// Spatial autocorrelation on a sparse weight graph in CSR on the device: crow [n + 1] int64, col [nnz] int32 ascending
// within a row, w [nnz] fp64.  Three families:
//
//   * the graph out of the kNN lists (graph_count_kernel, graph_scan_kernel, graph_write_kernel): a row's ascending
//     out-list (its k nearest) and ascending in-list (the rows that list it) are merged by one thread per row - as they
//     are ("none"), their union or their intersection ("mutual").  Count, scan, write, as image.hip compacts: the count
//     and the write walk the same merge, the scan is one workgroup's exclusive prefix over the row counts;
//   * a caller's graph checked (graph_check_kernel) and any graph's sums S0, S1, S2 (graph_sums_kernel), a thread per
//     row, 256 rows per workgroup; the workgroup's rows meet in row order in LDS, the workgroups in order in a fold;
//   * the permuted statistic (autocorr_perm_kernel, autocorr_fold_kernel), the hot path:
//       Moran  num[r, p] = sum_i Z[pi_r(i), p] * sum_{j in row i} w_ij Z[pi_r(j), p]
//       Geary  num[r, p] = sum_i sum_{j in row i} w_ij (Z[pi_r(i), p] - Z[pi_r(j), p])^2
//     A wave owns (64 consecutive genes, a row group, PERM_W permutations): its lanes are the genes, so a gathered row
//     of Z is one coalesced 512-byte read, and the PERM_W rows of one neighbour position are in flight together.  The
//     row's col / w are loaded once by the lanes (64 positions at a time, so a hub row is a loop), each lane looks its
//     column up in the PERM_W permutations, and the walk over the positions takes them out of the lanes by readlane.
//     The four waves of a workgroup take the next permutations of the same rows: the structure is read once per
//     workgroup from memory.  The rows of a group ascend in the wave's program order, j runs in CSR order, every
//     product is an explicit fma: (r, p)'s partial of a group is one fixed chain of operations, whatever the launch
//     holds beside it.  The groups - AC_MAX_GROUPS at most, a function of n alone - meet in ascending order in the
//     fold.  No atomics anywhere; a repeated call, or the same permutation in another call, gives the same bits.
//
// Bounds.  Every row range is clamped to [0, nnz].  An entry of perms or col outside [0, n) is never followed: a bad
// pi_r(i) drops row i of permutation r, a bad col or pi_r(j) drops that edge.  autocorr_bad_kernel counts the bad
// entries of perms and col (each once) into block partials, the fold adds them into n_bad.
#include <math.h>

#include "common.hpp"

namespace gpsa {

constexpr int AC_MAX_GROUPS = 32;  // row groups of the permuted statistic, at most: the partials are 8 G R P bytes
constexpr int AC_ROWS_MIN = 32;    // rows of a group, at least
constexpr int PERM_W = 4;          // permutations a wave carries: that many gathered rows in flight per position
constexpr int AC_BAD_BLOCKS = 256; // workgroups of the bad-entry count, at most
constexpr int GRAPH_ROWS = 256;    // rows of a workgroup in the check and the sums

enum { GRAPH_NONE = 0, GRAPH_UNION = 1, GRAPH_MUTUAL = 2 };

static long long ac_rows_per_group(long long n) {
  const long long r = cdiv(n, (long long)AC_MAX_GROUPS);
  return r < AC_ROWS_MIN ? AC_ROWS_MIN : r;
}
static long long ac_groups(long long n) { return cdiv(n, ac_rows_per_group(n)); }

__device__ __forceinline__ long long ac_clamp(long long v, long long lo, long long hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// ---- the graph out of the kNN lists -----------------------------------------------------------------------------------
// row i: a = out [i, 0..k) ascending, b = in_src [in_ptr[i] .. in_ptr[i + 1]) ascending (both without duplicates);
// emit(j) for every column of the row, ascending
template <typename F>
__device__ __forceinline__ void graph_merge_row(const int* __restrict__ out, const long long* __restrict__ in_ptr,
                                                const int* __restrict__ in_src, long long i, int k, long long E, int kind,
                                                F emit) {
  const int* a = out + i * k;
  if (kind == GRAPH_NONE) {
    for (int x = 0; x < k; ++x) emit(a[x]);
    return;
  }
  const long long b0 = ac_clamp(in_ptr[i], 0, E), b1 = ac_clamp(in_ptr[i + 1], b0, E);
  int x = 0;
  long long y = b0;
  while (x < k && y < b1) {
    const int ja = a[x], jb = in_src[y];
    if (ja == jb) {
      emit(ja);
      ++x, ++y;
    } else if (ja < jb) {
      if (kind == GRAPH_UNION) emit(ja);
      ++x;
    } else {
      if (kind == GRAPH_UNION) emit(jb);
      ++y;
    }
  }
  if (kind == GRAPH_UNION) {
    for (; x < k; ++x) emit(a[x]);
    for (; y < b1; ++y) emit(in_src[y]);
  }
}

// crow[i + 1] = the length of row i (crow[0] = 0); graph_scan_kernel turns the lengths into offsets
__global__ void __launch_bounds__(256)
graph_count_kernel(const int* __restrict__ out, const long long* __restrict__ in_ptr, const int* __restrict__ in_src,
                   long long n, int k, int kind, long long* __restrict__ crow) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= n) return;
  long long deg = 0;
  graph_merge_row(out, in_ptr, in_src, i, k, n * k, kind, [&](int) { ++deg; });
  crow[i + 1] = deg;
  if (i == 0) crow[0] = 0;
}

// one workgroup of 1024 threads: v[1 .. n] becomes its inclusive prefix sum, in place (integers: exact in any order)
__global__ void __launch_bounds__(1024)
graph_scan_kernel(long long* __restrict__ v, long long n) {
  __shared__ long long tot[1024];
  const long long per = (n + 1023) / 1024;
  const long long a = 1 + threadIdx.x * per, b = a + per < n + 1 ? a + per : n + 1;
  long long s = 0;
  for (long long i = a; i < b; ++i) s += v[i];
  tot[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int t = 0; t < 1024; ++t) {
      const long long here = tot[t];
      tot[t] = run;
      run += here;
    }
  }
  __syncthreads();
  long long run = tot[threadIdx.x];
  for (long long i = a; i < b; ++i) {
    run += v[i];
    v[i] = run;
  }
}

__global__ void __launch_bounds__(256)
graph_write_kernel(const int* __restrict__ out, const long long* __restrict__ in_ptr, const int* __restrict__ in_src,
                   long long n, int k, int kind, int row_standardize, const long long* __restrict__ crow, long long nnz,
                   int* __restrict__ col, double* __restrict__ w) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= n) return;
  const long long s = ac_clamp(crow[i], 0, nnz), e = ac_clamp(crow[i + 1], s, nnz);
  const double wt = (row_standardize && e > s) ? 1.0 / (double)(e - s) : 1.0;
  long long pos = s;
  graph_merge_row(out, in_ptr, in_src, i, k, n * k, kind, [&](int j) {
    if (pos < e) col[pos] = j, w[pos] = wt;
    ++pos;
  });
}

// ---- a graph checked, a graph's sums ------------------------------------------------------------------------------------
// the 256 values of a workgroup meet in thread order: the result in thread 0
__device__ __forceinline__ double meet_in_order(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int t = 0; t < GRAPH_ROWS; ++t) s += sh[t];
  return s;
}

// part [blocks, 8]: crow violations (crow[0] != 0, a decrease, crow[n] != nnz), columns outside [0, n), places inside a
// row where the column does not strictly increase, self edges, weights that are not finite or < 0
__global__ void __launch_bounds__(GRAPH_ROWS)
graph_check_kernel(const long long* __restrict__ crow, const int* __restrict__ col, const double* __restrict__ w,
                   long long n, long long nnz, double* __restrict__ part) {
  __shared__ double sh[GRAPH_ROWS];
  const long long i = blockIdx.x * (long long)GRAPH_ROWS + threadIdx.x;
  double v_crow = 0.0, v_range = 0.0, v_order = 0.0, v_self = 0.0, v_w = 0.0;
  if (i < n) {
    const long long here = crow[i], next = crow[i + 1];
    if (i == 0 && here != 0) v_crow += 1.0;
    if (i == n - 1 && next != nnz) v_crow += 1.0;
    if (next < here) v_crow += 1.0;
    const long long s = ac_clamp(here, 0, nnz), e = ac_clamp(next, s, nnz);
    for (long long q = s; q < e; ++q) {
      const long long c = col[q];
      const double wt = w[q];
      if (c < 0 || c >= n) v_range += 1.0;
      if (c == i) v_self += 1.0;
      if (q > s && c <= col[q - 1]) v_order += 1.0;
      if (!(wt >= 0.0 && wt < INFINITY)) v_w += 1.0;
    }
  }
  double* mine = part + 8 * (long long)blockIdx.x;
  double t = meet_in_order(v_crow, sh);
  if (threadIdx.x == 0) mine[0] = t;
  t = meet_in_order(v_range, sh);
  if (threadIdx.x == 0) mine[1] = t;
  t = meet_in_order(v_order, sh);
  if (threadIdx.x == 0) mine[2] = t;
  t = meet_in_order(v_self, sh);
  if (threadIdx.x == 0) mine[3] = t;
  t = meet_in_order(v_w, sh);
  if (threadIdx.x == 0) mine[4] = t;
}

// part [blocks, 8]: the workgroup's rows' shares of S0, S1, S2.  Row i gives  sum_j w_ij;  per stored edge (i, j)
// 1/2 (w_ij + w_ji)^2 where (j, i) is stored (found by binary search in row j's ascending columns: both directions carry
// a half) and w_ij^2 where it is not;  (w_i. + w_.i)^2 with the column sum over the transposed structure: tperm
// [tptr[i] .. tptr[i + 1]) are the positions of the entries of column i, ascending.
__global__ void __launch_bounds__(GRAPH_ROWS)
graph_sums_kernel(const long long* __restrict__ crow, const int* __restrict__ col, const double* __restrict__ w,
                  const long long* __restrict__ tptr, const long long* __restrict__ tperm, long long n, long long nnz,
                  double* __restrict__ part) {
  __shared__ double sh[GRAPH_ROWS];
  const long long i = blockIdx.x * (long long)GRAPH_ROWS + threadIdx.x;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  if (i < n) {
    const long long s = ac_clamp(crow[i], 0, nnz), e = ac_clamp(crow[i + 1], s, nnz);
    for (long long q = s; q < e; ++q) {
      const long long j = col[q];
      const double wij = w[q];
      s0 += wij;
      double wji = 0.0;
      bool back = false;
      if (j >= 0 && j < n) {
        long long lo = ac_clamp(crow[j], 0, nnz), hi = ac_clamp(crow[j + 1], lo, nnz);
        while (lo < hi) {  // the first position of row j whose column is >= i
          const long long mid = lo + (hi - lo) / 2;
          if (col[mid] < i) lo = mid + 1; else hi = mid;
        }
        if (lo < ac_clamp(crow[j + 1], 0, nnz) && col[lo] == i) back = true, wji = w[lo];
      }
      s1 += back ? 0.5 * (wij + wji) * (wij + wji) : wij * wij;
    }
    double cs = 0.0;
    const long long t0 = ac_clamp(tptr[i], 0, nnz), t1 = ac_clamp(tptr[i + 1], t0, nnz);
    for (long long q = t0; q < t1; ++q) {
      const long long at = tperm[q];
      if (at >= 0 && at < nnz) cs += w[at];
    }
    s2 = (s0 + cs) * (s0 + cs);
  }
  double* mine = part + 8 * (long long)blockIdx.x;
  double t = meet_in_order(s0, sh);
  if (threadIdx.x == 0) mine[0] = t;
  t = meet_in_order(s1, sh);
  if (threadIdx.x == 0) mine[1] = t;
  t = meet_in_order(s2, sh);
  if (threadIdx.x == 0) mine[2] = t;
}

// one workgroup: thread q < nq adds part[., q] over the blocks in order
template <typename TO>
__global__ void __launch_bounds__(64)
graph_fold_kernel(const double* __restrict__ part, long long blocks, int nq, TO* __restrict__ out) {
  if ((int)threadIdx.x >= nq) return;
  double s = 0.0;
  for (long long b = 0; b < blocks; ++b) s += part[8 * b + threadIdx.x];
  out[threadIdx.x] = (TO)s;
}

// ---- the permuted statistic ---------------------------------------------------------------------------------------------
// bad [gridDim.x]: the entries of perms [R n] and of col [nnz] outside [0, n), a grid-stride count per workgroup
__global__ void __launch_bounds__(256)
autocorr_bad_kernel(const int* __restrict__ perms, long long total, const int* __restrict__ col, long long nnz,
                    long long n, double* __restrict__ bad) {
  __shared__ double red[4];
  const long long tid = blockIdx.x * 256LL + threadIdx.x, nthreads = gridDim.x * 256LL;
  double c = 0.0;
  for (long long q = tid; q < total; q += nthreads) {
    const long long v = perms[q];
    if (v < 0 || v >= n) c += 1.0;
  }
  for (long long q = tid; q < nnz; q += nthreads) {
    const long long v = col[q];
    if (v < 0 || v >= n) c += 1.0;
  }
  c = block_sum(c, red);
  if (threadIdx.x == 0) bad[blockIdx.x] = c;
}

// workgroup (blockIdx.x = gene tile, blockIdx.y = row group, blockIdx.z = a block of 4 PERM_W permutations); wave w
// takes the permutations (4 blockIdx.z + w) PERM_W ..; see the head of the file.  part [G, R, P].
template <int MODE>
__global__ void __launch_bounds__(256)
autocorr_perm_kernel(const double* __restrict__ Z, long long n, long long P, const long long* __restrict__ crow,
                     const int* __restrict__ col, const double* __restrict__ w, long long nnz,
                     const int* __restrict__ perms, long long R, long long rows_per_group, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long p = blockIdx.x * 64LL + lane;
  const bool active = p < P;
  const long long g = blockIdx.y;
  const long long r0 = ((long long)blockIdx.z * 4 + wv) * PERM_W;
  if (r0 >= R) return;  // (no barrier below: a wave may leave)
  const int nq = (int)(R - r0 < PERM_W ? R - r0 : PERM_W);
  const long long i0 = g * rows_per_group, i1 = i0 + rows_per_group < n ? i0 + rows_per_group : n;
  const double* Zp = Z + (active ? p : 0);
  double acc[PERM_W];
#pragma unroll
  for (int q = 0; q < PERM_W; ++q) acc[q] = 0.0;

  for (long long i = i0; i < i1; ++i) {
    const long long s = ac_clamp(crow[i], 0, nnz), e = ac_clamp(crow[i + 1], s, nnz);
    double zi[PERM_W], lag[PERM_W];
    bool oki[PERM_W];
#pragma unroll
    for (int q = 0; q < PERM_W; ++q) {
      long long pi = -1;
      if (q < nq) pi = perms[(r0 + q) * n + i];
      oki[q] = pi >= 0 && pi < n;
      zi[q] = (oki[q] && active) ? Zp[pi * P] : 0.0;
      lag[q] = 0.0;
    }
    for (long long base = s; base < e; base += 64) {
      const int cnt = (int)(e - base < 64 ? e - base : 64);
      // the lanes take 64 positions of the row: column, weight, and the column's row under each permutation (-1: skip)
      int myc = -1;
      double myw = 0.0;
      if (lane < cnt) myc = col[base + lane], myw = w[base + lane];
      const bool cok = myc >= 0 && (long long)myc < n;
      int myp[PERM_W];
#pragma unroll
      for (int q = 0; q < PERM_W; ++q) {
        int v = -1;
        if (cok && q < nq && oki[q]) v = perms[(r0 + q) * n + myc];
        myp[q] = (v >= 0 && (long long)v < n) ? v : -1;
      }
      for (int t = 0; t < cnt; ++t) {
        const double wt = lane_value(myw, t);
        int pj[PERM_W];
        double zj[PERM_W];
#pragma unroll
        for (int q = 0; q < PERM_W; ++q) pj[q] = __builtin_amdgcn_readlane(myp[q], t);
#pragma unroll
        for (int q = 0; q < PERM_W; ++q) zj[q] = (pj[q] >= 0 && active) ? Zp[(long long)pj[q] * P] : 0.0;
#pragma unroll
        for (int q = 0; q < PERM_W; ++q) {
          if (pj[q] < 0) continue;  // wave-uniform
          if (MODE == 0) {
            lag[q] = fma(wt, zj[q], lag[q]);
          } else {
            const double d = zi[q] - zj[q];
            acc[q] = fma(wt * d, d, acc[q]);
          }
        }
      }
    }
    if (MODE == 0) {
#pragma unroll
      for (int q = 0; q < PERM_W; ++q)
        if (oki[q]) acc[q] = fma(zi[q], lag[q], acc[q]);
    }
  }
  if (active) {
#pragma unroll
    for (int q = 0; q < PERM_W; ++q)
      if (q < nq) part[(g * R + r0 + q) * P + p] = acc[q];
  }
}

// num [R P] = the groups' partials added in ascending order; the first thread also folds the bad-entry counts
__global__ void __launch_bounds__(256)
autocorr_fold_kernel(const double* __restrict__ part, long long G, long long RP, double* __restrict__ num,
                     const double* __restrict__ bad, int bad_blocks, long long* __restrict__ n_bad) {
  const long long x = blockIdx.x * 256LL + threadIdx.x;
  if (x == 0) {
    double c = 0.0;
    for (int b = 0; b < bad_blocks; ++b) c += bad[b];
    *n_bad = (long long)c;
  }
  if (x >= RP) return;
  double s = 0.0;
  for (long long g = 0; g < G; ++g) s += part[g * RP + x];
  num[x] = s;
}

static long long graph_blocks(long long n) { return cdiv(n, (long long)GRAPH_ROWS); }

}  // namespace gpsa

extern "C" {

long long gpsa_graph_workspace(long long n) {
  if (n < 1) return 0;
  return 8 * 8 * gpsa::graph_blocks(n);
}

static int graph_lists_check(const int* out, const long long* in_ptr, const int* in_src, long long n, int k, int kind) {
  if (out == nullptr || n < 1 || k < 1 || kind < 0 || kind > 2) return GPSA_EINVAL;
  if (kind != gpsa::GRAPH_NONE && (in_ptr == nullptr || in_src == nullptr)) return GPSA_EINVAL;
  if (n >= (1LL << 31)) return GPSA_EUNSUPPORTED;
  return 0;
}

int gpsa_graph_merge_count(const int* out, const long long* in_ptr, const int* in_src, long long n, int k, int kind,
                           long long* crow, void* stream) {
  const int rc = graph_lists_check(out, in_ptr, in_src, n, k, kind);
  if (rc) return rc;
  if (crow == nullptr) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  gpsa::graph_count_kernel<<<(unsigned)cdiv(n, 256), 256, 0, st>>>(out, in_ptr, in_src, n, k, kind, crow);
  GPSA_LAUNCH_CHECK();
  gpsa::graph_scan_kernel<<<1, 1024, 0, st>>>(crow, n);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_graph_merge_write(const int* out, const long long* in_ptr, const int* in_src, long long n, int k, int kind,
                           int row_standardize, const long long* crow, long long nnz, int* col, double* w,
                           void* stream) {
  const int rc = graph_lists_check(out, in_ptr, in_src, n, k, kind);
  if (rc) return rc;
  if (crow == nullptr || nnz < 0 || (nnz > 0 && (col == nullptr || w == nullptr))) return GPSA_EINVAL;
  if (nnz == 0) return 0;
  gpsa::graph_write_kernel<<<(unsigned)cdiv(n, 256), 256, 0, as_stream(stream)>>>(out, in_ptr, in_src, n, k, kind,
                                                                                   row_standardize, crow, nnz, col, w);
  GPSA_LAUNCH_CHECK();
  return 0;
}

static int graph_csr_check(const long long* crow, const int* col, const double* w, long long n, long long nnz) {
  if (crow == nullptr || n < 1 || nnz < 0 || (nnz > 0 && (col == nullptr || w == nullptr))) return GPSA_EINVAL;
  if (n >= (1LL << 31)) return GPSA_EUNSUPPORTED;
  return 0;
}

int gpsa_graph_check_f64(const long long* crow, const int* col, const double* w, long long n, long long nnz,
                         long long* out, void* workspace, long long workspace_bytes, void* stream) {
  const int rc = graph_csr_check(crow, col, w, n, nnz);
  if (rc) return rc;
  if (out == nullptr) return GPSA_EINVAL;
  if (workspace == nullptr || workspace_bytes < gpsa_graph_workspace(n)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const long long blocks = gpsa::graph_blocks(n);
  gpsa::graph_check_kernel<<<(unsigned)blocks, gpsa::GRAPH_ROWS, 0, st>>>(crow, col, w, n, nnz, (double*)workspace);
  GPSA_LAUNCH_CHECK();
  gpsa::graph_fold_kernel<long long><<<1, 64, 0, st>>>((const double*)workspace, blocks, 5, out);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_graph_sums_f64(const long long* crow, const int* col, const double* w, const long long* tptr,
                        const long long* tperm, long long n, long long nnz, double* out, void* workspace,
                        long long workspace_bytes, void* stream) {
  const int rc = graph_csr_check(crow, col, w, n, nnz);
  if (rc) return rc;
  if (out == nullptr || tptr == nullptr || (nnz > 0 && tperm == nullptr)) return GPSA_EINVAL;
  if (workspace == nullptr || workspace_bytes < gpsa_graph_workspace(n)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const long long blocks = gpsa::graph_blocks(n);
  gpsa::graph_sums_kernel<<<(unsigned)blocks, gpsa::GRAPH_ROWS, 0, st>>>(crow, col, w, tptr, tperm, n, nnz,
                                                                         (double*)workspace);
  GPSA_LAUNCH_CHECK();
  gpsa::graph_fold_kernel<double><<<1, 64, 0, st>>>((const double*)workspace, blocks, 3, out);
  GPSA_LAUNCH_CHECK();
  return 0;
}

long long gpsa_autocorr_perm_workspace(long long n, long long P, long long R) {
  if (n < 1 || P < 1 || R < 1) return 0;
  return 8 * (gpsa::ac_groups(n) * R * P + gpsa::AC_BAD_BLOCKS);
}

int gpsa_autocorr_perm_f64(const double* Z, long long n, long long P, const long long* crow, const int* col,
                           const double* w, long long nnz, const int* perms, long long R, int mode, double* num,
                           long long* n_bad, void* workspace, long long workspace_bytes, void* stream) {
  if (Z == nullptr || crow == nullptr || perms == nullptr || num == nullptr || n_bad == nullptr) return GPSA_EINVAL;
  if (n < 1 || P < 1 || R < 1 || nnz < 0 || (mode != 0 && mode != 1)) return GPSA_EINVAL;
  if (nnz > 0 && (col == nullptr || w == nullptr)) return GPSA_EINVAL;
  const long long zblocks = cdiv(R, 4LL * gpsa::PERM_W);
  if (n >= (1LL << 31) || P >= (1LL << 31) || zblocks > 65535 || cdiv(R * P, 256LL) >= (1LL << 31))
    return GPSA_EUNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < gpsa_autocorr_perm_workspace(n, P, R)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const long long rpg = gpsa::ac_rows_per_group(n), G = gpsa::ac_groups(n);
  double* part = (double*)workspace;
  double* bad = part + G * R * P;
  const long long most = R * n > nnz ? R * n : nnz;
  const int bad_blocks = (int)(cdiv(most, 256LL) < gpsa::AC_BAD_BLOCKS ? cdiv(most, 256LL) : gpsa::AC_BAD_BLOCKS);
  gpsa::autocorr_bad_kernel<<<bad_blocks, 256, 0, st>>>(perms, R * n, col, nnz, n, bad);
  GPSA_LAUNCH_CHECK();
  const dim3 grid((unsigned)cdiv(P, 64LL), (unsigned)G, (unsigned)zblocks);
  if (mode == 0)
    gpsa::autocorr_perm_kernel<0><<<grid, 256, 0, st>>>(Z, n, P, crow, col, w, nnz, perms, R, rpg, part);
  else
    gpsa::autocorr_perm_kernel<1><<<grid, 256, 0, st>>>(Z, n, P, crow, col, w, nnz, perms, R, rpg, part);
  GPSA_LAUNCH_CHECK();
  gpsa::autocorr_fold_kernel<<<(unsigned)cdiv(R * P, 256LL), 256, 0, st>>>(part, G, R * P, num, bad, bad_blocks, n_bad);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
