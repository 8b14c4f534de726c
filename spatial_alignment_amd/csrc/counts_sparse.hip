// Count preprocessing from a sparse count matrix in CSR on the device: crow [N + 1] int64, col [nnz] int32, val [nnz]
// fp32 (counts held as floats).  The margins and the Poisson deviance of counts.hip are sums over the entries > 0 only,
// so they never need the dense [N, P] matrix; only the selected block does, and csr_gather_kernel writes it.  As in
// counts.hip every sum is fp64 in a fixed order, no output element has two writers and a repeated call gives the same
// bits.  For integer counts the sums are exact, so they equal the dense entries' results bit for bit; other values agree
// to rounding (the order of the additions differs).
//
// The two reductions are ONE walk, csr_walk_kernel, over a grid of (column tile t, row group g):
//   * the rows are cut into G <= CSR_MAX_GROUPS groups of R consecutive rows (csr_rows_per_group: at least CSR_ROWS_MIN),
//     the columns into T = ceil(P / CSR_COL_TILE) tiles; workgroup (t, g) owns that block of the matrix;
//   * wave w takes the rows w, w + 4, ... of the group one after the other.  Each wave owns a private plane of the tile's
//     columns in LDS (two doubles per column); a lane adds an entry to the plane at the entry's column.  The columns
//     inside a row of a checked matrix are distinct, so no two lanes of the wave meet, and the rows follow each other in
//     the wave's program order: every plane element is added to in row order;
//   * a row's part of the tile is swept by row_walk.hpp's csr_row_in_tile (a 64-way search for its start, then 64
//     entries at a time), shared with moments.hip; the Poisson term is the dense walk's function.  Every entry is
//     consumed by exactly one tile: the matrix is read once;
//   * the four planes meet in wave order and go to the group's row of two partial planes pa / pb [G, P];
//   * a row's total over the tile is a wave sum, written by lane 0 to rpa / rpn [T, N] (margins only);
//   * csr_fold_kernel folds pa / pb over the groups and rpa / rpn over the tiles, both in order, and sums the
//     workgroups' counts of invalid values.
// Workspace (gpsa_count_csr_workspace): pa, pb [G, P], rpa [T, N] doubles, rpn [T, N] int32, bad [G * T] doubles and the
// check's partials [CSR_CHECK_BLOCKS, 4] doubles: 16 G P + 12 T N bytes and change, independent of nnz.
//
// Bounds.  gpsa_csr_check reports a malformed matrix and reads only crow [0, N], col / val [0, nnz) and rows clamped to
// [0, nnz].  The three compute kernels clamp every row range to [0, nnz] themselves and skip a column index outside
// [0, P) (the gather: a slot outside [0, G), a row outside [0, N)), so an unchecked matrix gives wrong sums but is never
// followed outside its buffers.  A `keep` mask of N bytes (0: the row is skipped as if absent; NULL: all rows) is
// honoured by the two reductions.
#include <math.h>

#include "row_walk.hpp"

namespace gpsa {

constexpr int CSR_COL_TILE = 512;       // columns of a tile: 4 planes x 2 doubles x 512 = 32 KiB of LDS
constexpr int CSR_ROWS_MIN = 16;        // rows of a group, at least (4 per wave)
constexpr int CSR_MAX_GROUPS = 32;      // groups, at most: the column partials are 16 G P bytes
constexpr int CSR_LOG_TABLE = 256;      // y log y of the counts below this comes from a table in LDS (deviance)
constexpr int CSR_CHECK_BLOCKS = 1024;  // workgroups of the check, at most
constexpr int CSR_GATHER_TILE = 8192;   // output columns assembled in LDS at a time (32 KiB)

enum { CSR_MARGINS = 0, CSR_DEVIANCE = 1 };

static long long csr_rows_per_group(long long N) {
  const long long r = cdiv(N, (long long)CSR_MAX_GROUPS);
  return r < CSR_ROWS_MIN ? CSR_ROWS_MIN : r;
}

struct CsrWorkspace {
  double *pa = nullptr, *pb = nullptr, *rpa = nullptr, *bad = nullptr, *chk = nullptr;
  int* rpn = nullptr;
  long long doubles;
  CsrWorkspace(void* ws, long long N, long long P) {
    const long long G = cdiv(N, csr_rows_per_group(N)), T = cdiv(P, (long long)CSR_COL_TILE);
    const long long o_rpa = 2 * G * P, o_rpn = o_rpa + T * N, o_bad = o_rpn + (T * N + 1) / 2, o_chk = o_bad + G * T;
    doubles = o_chk + 4 * CSR_CHECK_BLOCKS;
    if (ws == nullptr) return;  // the size alone
    pa = (double*)ws, pb = pa + G * P, rpa = pa + o_rpa, rpn = (int*)(pa + o_rpn), bad = pa + o_bad, chk = pa + o_chk;
  }
};

__device__ __forceinline__ long long cdivd(long long a, long long b) { return (a + b - 1) / b; }

// block (blockIdx.x = t, blockIdx.y = g) of the matrix; see the head of the file.
//   CSR_MARGINS:  pa = sums, pb = entries > 0 per column; rpa / rpn the same per row; bad = values NaN, +-inf or < 0
//   CSR_DEVIANCE: aux = log_sz [N]; pa = sum y log y - y log_sz, pb = sum |y log y| + |y log_sz| (y <= 0: no term)
template <int MODE>
__global__ void __launch_bounds__(256)
csr_walk_kernel(const long long* __restrict__ crow, const int* __restrict__ col, const float* __restrict__ val,
                const unsigned char* __restrict__ keep, long long N, long long P, long long nnz, long long R,
                const double* __restrict__ aux, double* __restrict__ pa, double* __restrict__ pb,
                double* __restrict__ rpa, int* __restrict__ rpn, double* __restrict__ bad) {
  __shared__ double ca[4][CSR_COL_TILE], cb[4][CSR_COL_TILE];
  __shared__ double red[4];
  __shared__ double ylogy[MODE == CSR_DEVIANCE ? CSR_LOG_TABLE : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long t = blockIdx.x, g = blockIdx.y;
  const long long c0 = t * CSR_COL_TILE, c1 = min(P, c0 + CSR_COL_TILE);
  const long long r0 = g * R, r1 = min(N, r0 + R);
  for (int cc = threadIdx.x; cc < 4 * CSR_COL_TILE; cc += 256) (&ca[0][0])[cc] = 0.0, (&cb[0][0])[cc] = 0.0;
  if (MODE == CSR_DEVIANCE) ylogy_fill<CSR_LOG_TABLE>(ylogy);
  __syncthreads();
  double nbad = 0.0;
  for (long long i = r0 + w; i < r1; i += 4) {
    const double lsz = MODE == CSR_DEVIANCE ? aux[i] : 0.0;
    double srow = 0.0;
    float nrow = 0.f;
    csr_row_in_tile(crow, col, val, keep, i, nnz, c0, c1, lane, [&](int cc, float y) {
      if (MODE == CSR_MARGINS) {
        const bool positive = y > 0.f;
        ca[w][cc] += (double)y;
        cb[w][cc] += positive ? 1.0 : 0.0;
        srow += (double)y;
        nrow += positive ? 1.f : 0.f;
        nbad += (y >= 0.f && y < INFINITY) ? 0.0 : 1.0;
      } else if (y > 0.f) {
        double t1, t2;
        poisson_terms<CSR_LOG_TABLE>(ylogy, y, lsz, t1, t2);
        ca[w][cc] += t1 - t2;
        cb[w][cc] += fabs(t1) + fabs(t2);
      }
    });
    if (MODE == CSR_MARGINS) {
      srow = wave_sum(srow);
      nrow = wave_sum(nrow);
      if (lane == 0) rpa[t * N + i] = srow, rpn[t * N + i] = (int)nrow;
    }
  }
  __syncthreads();
  // the four waves' columns meet in wave order
  for (int cc = threadIdx.x; cc < (int)(c1 - c0); cc += 256) {
    pa[g * P + c0 + cc] = meet4(ca, cc);
    pb[g * P + c0 + cc] = meet4(cb, cc);
  }
  if (MODE == CSR_MARGINS) {
    const double tot = block_sum(nbad, red);
    if (threadIdx.x == 0) bad[g * gridDim.x + t] = tot;
  }
}

// pa / pb [G, P] folded over the groups, rpa / rpn [T, N] folded over the tiles, both in order.  The first cdiv(P, 256)
// workgroups take a column per thread, the next cdiv(N, 256) a row per thread (CSR_MARGINS), the last sums bad [G * T].
//   CSR_MARGINS:  oa = col_sum, ob = col_nnz (int64), row_a = row_sum, row_b = row_nnz
//   CSR_DEVIANCE: oa = ll_sat, ob = abs_sat (double)
template <int MODE>
__global__ void __launch_bounds__(256)
csr_fold_kernel(const double* __restrict__ pa, const double* __restrict__ pb, const double* __restrict__ rpa,
                const int* __restrict__ rpn, const double* __restrict__ bad, long long G, long long T, long long N,
                long long P, double* __restrict__ oa, void* __restrict__ ob, double* __restrict__ row_a,
                long long* __restrict__ row_b, long long* __restrict__ n_invalid) {
  __shared__ double red[4];
  const long long cblocks = cdivd(P, 256), rblocks = MODE == CSR_MARGINS ? cdivd(N, 256) : 0;
  const long long b = blockIdx.x;
  if (b < cblocks) {
    const long long c = b * 256 + threadIdx.x;
    if (c >= P) return;
    double a = 0.0, n = 0.0;
    for (long long g = 0; g < G; ++g) a += pa[g * P + c], n += pb[g * P + c];
    oa[c] = a;
    if (MODE == CSR_MARGINS)
      ((long long*)ob)[c] = (long long)n;
    else
      ((double*)ob)[c] = n;
  } else if (b < cblocks + rblocks) {
    const long long i = (b - cblocks) * 256 + threadIdx.x;
    if (i >= N) return;
    double a = 0.0;
    long long n = 0;
    for (long long t = 0; t < T; ++t) a += rpa[t * N + i], n += rpn[t * N + i];
    row_a[i] = a, row_b[i] = n;
  } else {
    double s = 0.0;
    for (long long k = threadIdx.x; k < G * T; k += 256) s += bad[k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) *n_invalid = (long long)s;
  }
}

// part [gridDim.x, 4]: crow violations (crow[0] != 0, a decrease, crow[N] != nnz), column indices outside [0, P), places
// inside a row where the column index does not strictly increase, stored values equal to 0.  Counts: exact in any order.
__global__ void __launch_bounds__(256)
csr_check_kernel(const long long* __restrict__ crow, const int* __restrict__ col, const float* __restrict__ val,
                 long long N, long long P, long long nnz, double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  const long long tid = blockIdx.x * 256LL + threadIdx.x, nthreads = gridDim.x * 256LL;
  double v_crow = 0.0, v_range = 0.0, v_order = 0.0, v_zero = 0.0;
  for (long long i = tid; i <= N; i += nthreads) {  // crow over [0, N]
    const long long here = crow[i];
    if (i == 0 && here != 0) v_crow += 1.0;
    if (i == N && here != nnz) v_crow += 1.0;
    if (i < N && crow[i + 1] < here) v_crow += 1.0;
  }
  for (long long k = tid; k < nnz; k += nthreads) {  // col and val flat over [0, nnz)
    const long long c = col[k];
    if (c < 0 || c >= P) v_range += 1.0;
    if (val[k] == 0.f) v_zero += 1.0;
  }
  // a wave per row, the row's bounds clamped to [0, nnz]
  for (long long i = tid >> 6; i < N; i += nthreads >> 6) {
    const long long s = clampll(crow[i], 0, nnz), e = clampll(crow[i + 1], s, nnz);
    for (long long k = s + 1 + lane; k < e; k += WAVE)
      if (col[k] <= col[k - 1]) v_order += 1.0;
  }
  double* mine = part + 4 * (long long)blockIdx.x;
  double tot = block_sum(v_crow, red);
  if (threadIdx.x == 0) mine[0] = tot;
  tot = block_sum(v_range, red);
  if (threadIdx.x == 0) mine[1] = tot;
  tot = block_sum(v_order, red);
  if (threadIdx.x == 0) mine[2] = tot;
  tot = block_sum(v_zero, red);
  if (threadIdx.x == 0) mine[3] = tot;
}

// one workgroup: out[q] = sum over the blocks of part[., q]
__global__ void __launch_bounds__(256)
csr_check_fold_kernel(const double* __restrict__ part, int blocks, long long* __restrict__ out) {
  __shared__ double red[4];
  for (int q = 0; q < 4; ++q) {
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256) s += part[4 * b + q];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[q] = (long long)s;
  }
}

// workgroup j assembles row rows[j] of the selected block in LDS, CSR_GATHER_TILE output columns at a time, and stores
// it coalesced: every element of out [n_rows, G] is written exactly once, zeros included.
__global__ void __launch_bounds__(256)
csr_gather_kernel(const long long* __restrict__ crow, const int* __restrict__ col, const float* __restrict__ val,
                  long long N, long long P, long long nnz, const long long* __restrict__ rows,
                  const int* __restrict__ slot, long long G, float* __restrict__ out) {
  __shared__ float buf[CSR_GATHER_TILE];
  const long long j = blockIdx.x, i = rows[j];
  long long s = 0, e = 0;
  if (i >= 0 && i < N) s = clampll(crow[i], 0, nnz), e = clampll(crow[i + 1], s, nnz);
  for (long long g0 = 0; g0 < G; g0 += CSR_GATHER_TILE) {
    const int width = (int)min((long long)CSR_GATHER_TILE, G - g0);
    for (int q = threadIdx.x; q < width; q += 256) buf[q] = 0.f;
    __syncthreads();
    for (long long k = s + threadIdx.x; k < e; k += 256) {
      const long long c = col[k];
      if (c < 0 || c >= P) continue;
      const long long q = (long long)slot[c] - g0;
      if (q >= 0 && q < width) buf[q] = val[k];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < width; q += 256) out[j * G + g0 + q] = buf[q];
    __syncthreads();  // before the next tile's zeros
  }
}

template <int MODE>
static int csr_reduce(const long long* crow, const int* col, const float* val, const unsigned char* keep, long long N,
                      long long P, long long nnz, const double* aux, double* oa, void* ob, double* row_a,
                      long long* row_b, long long* n_invalid, void* workspace, hipStream_t st) {
  const CsrWorkspace ws(workspace, N, P);
  const long long R = csr_rows_per_group(N), G = cdiv(N, R), T = cdiv(P, (long long)CSR_COL_TILE);
  csr_walk_kernel<MODE><<<dim3((unsigned)T, (unsigned)G), 256, 0, st>>>(crow, col, val, keep, N, P, nnz, R, aux, ws.pa,
                                                                          ws.pb, ws.rpa, ws.rpn, ws.bad);
  GPSA_LAUNCH_CHECK();
  const long long blocks = cdiv(P, 256) + (MODE == CSR_MARGINS ? cdiv(N, 256) + 1 : 0);
  csr_fold_kernel<MODE><<<(unsigned)blocks, 256, 0, st>>>(ws.pa, ws.pb, ws.rpa, ws.rpn, ws.bad, G, T, N, P, oa, ob, row_a,
                                                          row_b, n_invalid);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // namespace gpsa

extern "C" {

long long gpsa_count_csr_workspace(long long N, long long P) {
  if (N < 1 || P < 1) return 0;
  return 8 * gpsa::CsrWorkspace(nullptr, N, P).doubles;
}

int gpsa_csr_check(const long long* crow, const int* col, const float* val, long long N, long long P, long long nnz,
                   long long* out, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (int rc = csr_shape_check(crow, col, val, N, P, nnz)) return rc;
  if (out == nullptr) return GPSA_EINVAL;
  if (workspace == nullptr || workspace_bytes < gpsa_count_csr_workspace(N, P)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const CsrWorkspace ws(workspace, N, P);
  const long long work = cdiv((nnz > 64 * N ? nnz : 64 * N) + 1, 256);
  const int blocks = (int)(work < CSR_CHECK_BLOCKS ? work : CSR_CHECK_BLOCKS);
  csr_check_kernel<<<blocks, 256, 0, st>>>(crow, col, val, N, P, nnz, ws.chk);
  GPSA_LAUNCH_CHECK();
  csr_check_fold_kernel<<<1, 256, 0, st>>>(ws.chk, blocks, out);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_count_margins_csr_f32(const long long* crow, const int* col, const float* val, const unsigned char* keep,
                               long long N, long long P, long long nnz, double* row_sum, double* col_sum,
                               long long* row_nnz, long long* col_nnz, long long* n_invalid, void* workspace,
                               long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (int rc = csr_shape_check(crow, col, val, N, P, nnz)) return rc;
  if (!row_sum || !col_sum || !row_nnz || !col_nnz || !n_invalid) return GPSA_EINVAL;
  if (workspace == nullptr || workspace_bytes < gpsa_count_csr_workspace(N, P)) return GPSA_EWORKSPACE;
  return csr_reduce<CSR_MARGINS>(crow, col, val, keep, N, P, nnz, nullptr, col_sum, col_nnz, row_sum, row_nnz, n_invalid,
                                 workspace, as_stream(stream));
}

int gpsa_count_deviance_csr_f32(const long long* crow, const int* col, const float* val, const unsigned char* keep,
                                long long N, long long P, long long nnz, const double* log_sz, double* ll_sat,
                                double* abs_sat, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (int rc = csr_shape_check(crow, col, val, N, P, nnz)) return rc;
  if (!log_sz || !ll_sat || !abs_sat) return GPSA_EINVAL;
  if (workspace == nullptr || workspace_bytes < gpsa_count_csr_workspace(N, P)) return GPSA_EWORKSPACE;
  return csr_reduce<CSR_DEVIANCE>(crow, col, val, keep, N, P, nnz, log_sz, ll_sat, abs_sat, nullptr, nullptr, nullptr,
                                  workspace, as_stream(stream));
}

int gpsa_csr_gather_dense_f32(const long long* crow, const int* col, const float* val, long long N, long long P,
                              long long nnz, const long long* rows, long long n_rows, const int* slot, long long G,
                              float* out, void* stream) {
  using namespace gpsa;
  if (int rc = csr_shape_check(crow, col, val, N, P, nnz)) return rc;
  if (!rows || !slot || !out || n_rows < 1 || n_rows > 0x7fffffffLL || G < 1 || G > P) return GPSA_EINVAL;
  csr_gather_kernel<<<(unsigned)n_rows, 256, 0, as_stream(stream)>>>(crow, col, val, N, P, nnz, rows, slot, G, out);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
