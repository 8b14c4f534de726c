// Rigid pre-registration of slices on the device: the score of many candidate transforms of slice B against slice A.
// Replaces the hand-tuned rotation the reference's experiment scripts apply to a slice before the fit
// (slideseq_alignment.py: angle = 1.45; two_slice_alignment.py: three quarter turns "manually"): register.py searches
// rotations, reflections and shifts with this entry as its only device work.
//
// gpsa_rigid_scores_f64, D = 2.  For candidate k (a row of T [K, 6]: R row-major, then t) and row i of B the transformed
// point is q_d = fma(R_d0, x0, fma(R_d1, x1, t_d)); its nearest row of A is the smallest key (d2, index), d2 accumulated
// as knn_scan_kernel does (u = q - r; s = fma(u, u, s)), a NaN distance counted as +inf - a total order, so the answer
// does not depend on how the scan was cut.  Row i is matched iff d2 <= max_d2, and per candidate
//   sse = sum_{i matched} sum_p (double(YB[i, p]) - double(YA[nn, p]))^2,  d2_sum = sum_{i matched} d2,  n_matched.
//
// The scan is NOT K launches of the kNN kernel: a thread owns one row of B and RG_C candidates at once - RG_C
// transformed points and RG_C running (d2, index) minima in registers - and A streams through LDS a tile at a time; every
// lane reads the same address (a broadcast), and one LDS read feeds RG_C candidates.  The references arrive in ascending
// index, so a strict d2 < best is the key's order within a slice (a tie keeps the lower index), and a NaN or +inf distance
// never enters: a thread that took nothing ends at (+inf, the slice's first row), the key's minimum there.
// blockIdx.y takes groups of RG_C candidates, blockIdx.z slices of the A axis; with more than one slice a second kernel
// merges the slices' minima by the same key, as knn_merge_kernel does.
//
// The closing kernel gathers YA[nn] (lanes over genes, 256 / TX rows of B in flight per workgroup): workgroup (row group
// g, candidate k) walks its rows in ascending order, every thread one fixed fma chain, the 256 threads meet in a fixed
// LDS tree; the row groups - RG_MAX_GROUPS at most, a function of n alone - are added in ascending order by a last
// kernel.  No atomics, one writer per output element: sse / d2_sum / n_matched of a candidate depend on its own row of T
// and on (n, P) alone - the same bits for every chunking of the candidates, every split of the A axis, every repeat.
#include <limits.h>
#include <math.h>

#include "toolbox.hpp"

namespace gpsa {

constexpr int RG_ROWS = 256;        // rows of B of a scan workgroup: one per thread
constexpr int RG_TILE = 1024;       // rows of A staged in LDS at a time (D = 2: 16 KB)
constexpr int RG_C = 8;             // candidates a thread carries: 7 VGPRs each (q0, q1, d2: 2 each; index: 1), no scratch
constexpr int RG_MAX_GROUPS = 32;   // row groups of the closing sums, at most
constexpr int RG_GROUP_MIN = 32;    // rows of a group, at least
constexpr int RG_MAXPARTS = 64;     // slices of the A axis, at most

static long long rg_rows_per_group(long long n) {
  const long long r = cdiv(n, (long long)RG_MAX_GROUPS);
  return r < RG_GROUP_MIN ? RG_GROUP_MIN : r;
}
static long long rg_groups(long long n) { return cdiv(n, rg_rows_per_group(n)); }

// rows [blockIdx.x * 256 ..) of B, candidates [blockIdx.y * RG_C ..), rows [lo, hi) of A of slice blockIdx.z.
// od / oi [gridDim.z][K][n] (one slice: the tables nn / d2 themselves)
__global__ void __launch_bounds__(RG_ROWS)
rigid_scan_kernel(const double* __restrict__ XA, long long m, const double* __restrict__ XB, long long n,
                  const double* __restrict__ T, long long K, long long chunk, int* __restrict__ oi,
                  double* __restrict__ od) {
  __shared__ double rs[RG_TILE * 2];
  const long long i = blockIdx.x * (long long)RG_ROWS + threadIdx.x;
  const bool live = i < n;
  const long long k0 = (long long)blockIdx.y * RG_C;
  const long long lo = (long long)blockIdx.z * chunk;
  const long long hi = min(m, lo + chunk);
  const double x0 = live ? XB[i * 2] : 0.0, x1 = live ? XB[i * 2 + 1] : 0.0;
  double q0[RG_C], q1[RG_C], bd[RG_C];
  int bi[RG_C];
#pragma unroll
  for (int c = 0; c < RG_C; ++c) {
    const double* t = T + min(k0 + c, K - 1) * 6;  // a candidate past the table repeats the last one and is not written
    q0[c] = fma(t[0], x0, fma(t[1], x1, t[4]));
    q1[c] = fma(t[2], x0, fma(t[3], x1, t[5]));
    bd[c] = INFINITY;
    bi[c] = INT_MAX;
  }
  for (long long r0 = lo; r0 < hi; r0 += RG_TILE) {
    const int cnt = (int)min((long long)RG_TILE, hi - r0);
    __syncthreads();  // the previous tile has been consumed
    for (int t = threadIdx.x; t < cnt * 2; t += RG_ROWS) rs[t] = XA[r0 * 2 + t];
    __syncthreads();
    if (live) {
      const int j0 = (int)r0;
#pragma unroll 4
      for (int r = 0; r < cnt; ++r) {
        const double a0 = rs[2 * r], a1 = rs[2 * r + 1];
#pragma unroll
        for (int c = 0; c < RG_C; ++c) {
          const double u0 = q0[c] - a0, u1 = q1[c] - a1;
          const double s = fma(u1, u1, u0 * u0);  // = fma(u1, u1, fma(u0, u0, 0.0))
          const bool take = s < bd[c];            // false for a NaN
          bd[c] = take ? s : bd[c];
          bi[c] = take ? j0 + r : bi[c];
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < RG_C; ++c)
    if (k0 + c < K) {
      const long long o = ((long long)blockIdx.z * K + (k0 + c)) * n + i;
      // nothing below +inf in this slice: its first row, at +inf (an empty last slice: a row of A all the same)
      oi[o] = bi[c] == INT_MAX ? (int)min(lo, m - 1) : bi[c];
      od[o] = bd[c];
    }
}

// the slices' minima pd / pi [parts][K n] -> nn / d2 [K n] by the key (d2, index)
__global__ void __launch_bounds__(256)
rigid_merge_kernel(const double* __restrict__ pd, const int* __restrict__ pi, long long total, int parts,
                   int* __restrict__ nn, double* __restrict__ d2) {
  const long long e = blockIdx.x * 256LL + threadIdx.x;
  if (e >= total) return;
  double bd = pd[e];
  int bi = pi[e];
  for (int p = 1; p < parts; ++p) {
    const double d = pd[p * total + e];
    const int j = pi[p * total + e];
    const bool take = key_less(d, j, bd, bi);
    bd = take ? d : bd;
    bi = take ? j : bi;
  }
  nn[e] = bi;
  d2[e] = bd;
}

// workgroup (blockIdx.x = row group g, blockIdx.y = candidate k): thread (ty, tx) takes rows i0 + ty, i0 + ty + TY, ...
// of the group and genes tx, tx + TX, ...;  part [K][G][3] = the group's sse, d2_sum, n_matched (a double: exact)
template <int TX>
__global__ void __launch_bounds__(256)
rigid_close_kernel(const float* __restrict__ YA, long long m, const float* __restrict__ YB, long long n, int P,
                   const int* __restrict__ nn, const double* __restrict__ d2, double max_d2, long long rows_per_group,
                   double* __restrict__ part) {
  constexpr int TY = 256 / TX;
  __shared__ double red[3][256];
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const long long g = blockIdx.x, k = blockIdx.y;
  const long long i0 = g * rows_per_group, i1 = min(n, i0 + rows_per_group);
  double sse = 0.0, dsum = 0.0, cnt = 0.0;
  for (long long i = i0 + ty; i < i1; i += TY) {
    const double d = d2[k * n + i];
    const long long j = nn[k * n + i];
    if (!(d <= max_d2) || j < 0 || j >= m) continue;  // unmatched; an index outside A is not followed
    const float* __restrict__ yb = YB + i * P;
    const float* __restrict__ ya = YA + j * P;
    for (int p = tx; p < P; p += TX) {
      const double u = (double)yb[p] - (double)ya[p];
      sse = fma(u, u, sse);
    }
    if (tx == 0) {
      dsum += d;
      cnt += 1.0;
    }
  }
  fold3_256(sse, dsum, cnt, red);
  if (threadIdx.x < 3) part[(k * gridDim.x + g) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// candidate k: its groups' partials in ascending order
__global__ void __launch_bounds__(256)
rigid_fold_kernel(const double* __restrict__ part, long long K, int G, double* __restrict__ sse,
                  long long* __restrict__ n_matched, double* __restrict__ d2_sum) {
  const long long k = blockIdx.x * 256LL + threadIdx.x;
  if (k >= K) return;
  double s = 0.0, d = 0.0, c = 0.0;
  for (int g = 0; g < G; ++g) {
    const double* p = part + (k * G + g) * 3;
    s += p[0];
    d += p[1];
    c += p[2];
  }
  sse[k] = s;
  d2_sum[k] = d;
  n_matched[k] = (long long)c;
}

// slices of the A axis (slice_parts): a slice's scan is cdiv(n, RG_ROWS) x cdiv(K, RG_C) workgroups
static int rg_parts(long long n, long long m, long long K, int parts) {
  return slice_parts(cdiv(n, RG_ROWS) * cdiv(K, RG_C), m, RG_TILE, RG_MAXPARTS, parts);
}

// the workspace, in this order (every piece a multiple of 8 bytes): the partials [K][G][3] fp64;  d2 then nn [K n] where
// the caller keeps no tables;  the slices' minima, d2 then index [parts][K n], with more than one slice
struct RgLayout {
  long long part, tables, slices, total;
};
static RgLayout rg_layout(long long n, long long K, int parts, bool own_tables) {
  RgLayout L;
  const long long e = K * n, i4 = cdiv(e * 4, 8) * 8;
  L.part = 8 * K * rg_groups(n) * 3;
  L.tables = own_tables ? e * 8 + i4 : 0;
  L.slices = parts > 1 ? parts * e * 8 + cdiv(parts * e * 4, 8) * 8 : 0;
  L.total = L.part + L.tables + L.slices;
  return L;
}

static bool rg_sizes_ok(long long n, long long m, long long K, long long P) {
  return n >= 1 && m >= 1 && K >= 1 && P >= 1;
}
static bool rg_sizes_supported(long long n, long long m, long long K, long long P) {
  // indices are int32; the closing grid's y extent is K; the merge runs a thread per element of a table
  return m <= 0x7fffffffLL && n <= 0x7fffffffLL && P <= 0x7fffffffLL && K <= 65535 && K * n <= (1LL << 38);
}

}  // namespace gpsa

extern "C" {

long long gpsa_rigid_scores_workspace(long long n, long long m, long long K, int P, int parts, int tables) {
  if (!gpsa::rg_sizes_ok(n, m, K, P) || !gpsa::rg_sizes_supported(n, m, K, P) || parts < 0) return 0;
  return gpsa::rg_layout(n, K, gpsa::rg_parts(n, m, K, parts), tables == 0).total;
}

int gpsa_rigid_scores_f64(const double* XA, const float* YA, long long m, const double* XB, const float* YB,
                          long long n, int P, const double* T, long long K, double max_d2, int parts, double* sse,
                          long long* n_matched, double* d2_sum, int* nn, double* d2, void* workspace,
                          long long workspace_bytes, void* stream) {
  if (!XA || !YA || !XB || !YB || !T || !sse || !n_matched || !d2_sum) return GPSA_EINVAL;
  if ((nn == nullptr) != (d2 == nullptr)) return GPSA_EINVAL;
  if (!gpsa::rg_sizes_ok(n, m, K, P) || parts < 0) return GPSA_EINVAL;
  if (!(max_d2 >= 0.0) || isinf(max_d2)) return GPSA_EINVAL;
  if (!gpsa::rg_sizes_supported(n, m, K, P)) return GPSA_EUNSUPPORTED;
  const int np = gpsa::rg_parts(n, m, K, parts);
  const gpsa::RgLayout L = gpsa::rg_layout(n, K, np, nn == nullptr);
  if (workspace == nullptr || workspace_bytes < L.total) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const long long e = K * n;
  char* ws = (char*)workspace;
  double* part = (double*)ws;
  if (nn == nullptr) {
    d2 = (double*)(ws + L.part);
    nn = (int*)(ws + L.part + e * 8);
  }
  const dim3 grid((unsigned)cdiv(n, gpsa::RG_ROWS), (unsigned)cdiv(K, gpsa::RG_C), (unsigned)np);
  if (np == 1) {
    gpsa::rigid_scan_kernel<<<grid, gpsa::RG_ROWS, 0, st>>>(XA, m, XB, n, T, K, m, nn, d2);
    GPSA_LAUNCH_CHECK();
  } else {
    double* pd = (double*)(ws + L.part + L.tables);
    int* pi = (int*)(pd + (long long)np * e);
    gpsa::rigid_scan_kernel<<<grid, gpsa::RG_ROWS, 0, st>>>(XA, m, XB, n, T, K, cdiv(m, np), pi, pd);
    GPSA_LAUNCH_CHECK();
    gpsa::rigid_merge_kernel<<<(unsigned)cdiv(e, 256), 256, 0, st>>>(pd, pi, e, np, nn, d2);
    GPSA_LAUNCH_CHECK();
  }
  const long long rpg = gpsa::rg_rows_per_group(n);
  const int G = (int)gpsa::rg_groups(n);
  const dim3 cgrid((unsigned)G, (unsigned)K);
  if (P <= 16)
    gpsa::rigid_close_kernel<16><<<cgrid, 256, 0, st>>>(YA, m, YB, n, P, nn, d2, max_d2, rpg, part);
  else
    gpsa::rigid_close_kernel<64><<<cgrid, 256, 0, st>>>(YA, m, YB, n, P, nn, d2, max_d2, rpg, part);
  GPSA_LAUNCH_CHECK();
  gpsa::rigid_fold_kernel<<<(unsigned)cdiv(K, 256), 256, 0, st>>>(part, K, G, sse, n_matched, d2_sum);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
