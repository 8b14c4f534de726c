// Per-(view, column) moments of a matrix on the device: what the dispersion-based gene selection (counts.py:
// highly_variable_genes) and the per-view variance filter (column_moments) reduce the data to.  For every view v (a range
// of consecutive rows, view_off [V + 1] on the host) and column c
//     s1[v, c] = sum t,   s2[v, c] = sum t^2,   abs1[v, c] = sum |t|        (fp64)
// over the view's rows, where t is formed in fp64 from the stored fp32 value y:
//     MOM_IDENTITY  t = y                     (any sign: the variance filter on transformed data)
//     MOM_EXPM1     t = expm1(y)              (the matrix is log1p(normalised counts), scanpy's convention)
//     MOM_SCALE     t = y * scale_i           (scale [N] fp64, target / row sum: the normalised counts from raw counts,
//                                              without the N x P normalised matrix)
// and one int64: the number of t that are NaN or +-inf.  The caller closes mean and variance.  The rules of counts.hip and
// counts_sparse.hip hold: every sum is fp64 in a fixed order, no output element has two writers, a repeated call gives
// the same bits, nothing of N * P elements is allocated.  Integer values in MOM_IDENTITY give exact sums, so the dense
// and the CSR entry agree bit for bit there; other values agree to rounding.
//
// Dense (moments_walk_kernel), the structure of counts.hip's walk.  The views are walked one after the other (a launch
// per view: a row group never mixes two views).  A view's n rows are cut into G <= MOM_MAX_GROUPS groups of R
// consecutive rows (mom_rows_per_group: at least MOM_ROWS_MIN); workgroup g owns group g and walks the column tiles of
// MOM_COL_TILE columns.  Inside a tile wave w takes the rows w, w + 4, ... of the group, a lane holds 8 columns of the
// tile and three fp64 accumulators per column in registers, the next row's loads are in flight while a row is consumed.
// At the end of a tile the four waves' accumulators meet in LDS in wave order, one quantity after the other through one
// [4][MOM_COL_TILE] buffer, and go to the group's row of the three partial planes p [3][Gb, P].
//
// CSR (moments_csr_walk_kernel), the structure of counts_sparse.hip's walk over a grid of (column tile, row group) per
// view, G <= MOM_CSR_MAX_GROUPS: each wave owns a private plane of the tile's columns in LDS (three doubles per column)
// and adds the rows' entries to it in row order; the planes meet in wave order.  The tile loader and the CSR row sweep
// are row_walk.hpp's, the ones counts.hip and counts_sparse.hip use.  Unstored entries contribute exactly 0
// in all three modes (expm1(0) = 0), so the sums run over the stored entries; a row with keep == 0 contributes nothing.
// Every row range is clamped to [0, nnz] and a column index outside the tile (so outside [0, P)) is skipped: a malformed
// matrix gives wrong sums but is never followed outside its buffers.
//
// moments_fold_kernel folds the planes over the groups in order (64 columns x 4 contiguous segments per workgroup, the
// segments combined in order) into row v of s1 / s2 / abs1; its last workgroup sums the groups' counts of non-finite
// values into the view's slot, and moments_finish_kernel adds the views' slots into the one int64.
// Workspace: the three planes, the groups' counts and the views' slots; the planes are reused from view to view (the
// launches of one call are ordered on the stream).
#include <math.h>

#include "row_walk.hpp"

namespace gpsa {

constexpr int MOM_COL_TILE = 512;        // columns of a tile: 8 per lane (dense), a plane's width in LDS (CSR)
constexpr int MOM_ROWS_MIN = 16;         // rows of a group, at least (4 per wave)
constexpr int MOM_MAX_GROUPS = 512;      // dense: groups of a view, at most (the planes are 24 G P bytes)
constexpr int MOM_CSR_MAX_GROUPS = 16;   // CSR: groups of a view, at most
constexpr int MOM_PER_LANE = MOM_COL_TILE / WAVE;

enum { MOM_IDENTITY = 0, MOM_EXPM1 = 1, MOM_SCALE = 2 };

static long long mom_rows_per_group(long long n, int max_groups) {
  const long long r = cdiv(n, (long long)max_groups);
  return r < MOM_ROWS_MIN ? MOM_ROWS_MIN : r;
}
// the most groups any n <= N is cut into (the views share the planes)
static long long mom_groups_bound(long long N, int max_groups) {
  const long long g = cdiv(N, (long long)MOM_ROWS_MIN);
  return g < max_groups ? g : max_groups;
}

// planes [3][Gb, P], bad [nbad], badv [V]   (doubles); nbad = Gb (dense) or Gb * T (CSR)
struct MomWorkspace {
  double *p[3] = {nullptr, nullptr, nullptr}, *bad = nullptr, *badv = nullptr;
  long long doubles;
  MomWorkspace(void* ws, long long N, long long P, int V, bool csr) {
    const long long gb = mom_groups_bound(N, csr ? MOM_CSR_MAX_GROUPS : MOM_MAX_GROUPS);
    const long long nbad = csr ? gb * cdiv(P, (long long)MOM_COL_TILE) : gb;
    doubles = 3 * gb * P + nbad + V;
    if (ws == nullptr) return;  // the size alone
    p[0] = (double*)ws, p[1] = p[0] + gb * P, p[2] = p[1] + gb * P, bad = p[2] + gb * P, badv = bad + nbad;
  }
};

template <int MODE>
__device__ __forceinline__ double mom_value(float y, double sc) {
  const double yd = (double)y;
  return MODE == MOM_IDENTITY ? yd : (MODE == MOM_EXPM1 ? expm1(yd) : yd * sc);
}
__device__ __forceinline__ double mom_nonfinite(double t) { return fabs(t) < INFINITY ? 0.0 : 1.0; }  // (a NaN: 1)

// rows [blockIdx.x * R, ...) of the view Y [n, P] (scale: the view's first entry); see the head of the file
template <int MODE, bool VEC>
__global__ void __launch_bounds__(256)
moments_walk_kernel(const float* __restrict__ Y, long long n, long long P, int R, const double* __restrict__ scale,
                    double* __restrict__ p0, double* __restrict__ p1, double* __restrict__ p2, double* __restrict__ bad) {
  __shared__ double cs[4][MOM_COL_TILE];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * R;
  const int rows = (int)min((long long)R, n - r0);
  const float* Yg = Y + r0 * P;
  double* const planes[3] = {p0, p1, p2};
  double nbad = 0.0;
  for (long long c0 = 0; c0 < P; c0 += MOM_COL_TILE) {
    double a[3][MOM_PER_LANE];
#pragma unroll
    for (int k = 0; k < MOM_PER_LANE; ++k) a[0][k] = 0.0, a[1][k] = 0.0, a[2][k] = 0.0;
    float cur[MOM_PER_LANE] = {}, nxt[MOM_PER_LANE] = {};
    if (w < rows) load_row<VEC, MOM_PER_LANE>(Yg + (long long)w * P, c0, P, lane, cur);
    for (int r = w; r < rows; r += 4) {
      if (r + 4 < rows) load_row<VEC, MOM_PER_LANE>(Yg + (long long)(r + 4) * P, c0, P, lane, nxt);
      const double sc = MODE == MOM_SCALE ? scale[r0 + r] : 0.0;
#pragma unroll
      for (int k = 0; k < MOM_PER_LANE; ++k) {
        const double t = mom_value<MODE>(cur[k], sc);
        a[0][k] += t;
        a[1][k] += t * t;
        a[2][k] += fabs(t);
        // a column beyond P read as 0, and 0 times a non-finite scale is a NaN that no entry of the matrix holds
        nbad += (c0 + tile_col<VEC>(lane, k) < P) ? mom_nonfinite(t) : 0.0;
      }
#pragma unroll
      for (int k = 0; k < MOM_PER_LANE; ++k) cur[k] = nxt[k];
    }
    // the four waves' columns meet in wave order, one quantity after the other
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int k = 0; k < MOM_PER_LANE; ++k) cs[w][tile_col<VEC>(lane, k)] = a[q][k];
      __syncthreads();
      for (int cc = threadIdx.x; cc < MOM_COL_TILE; cc += 256) {
        const long long c = c0 + cc;
        if (c >= P) break;
        planes[q][(long long)blockIdx.x * P + c] = meet4(cs, cc);
      }
      __syncthreads();  // before the next quantity lands in cs
    }
  }
  const double tot = block_sum(nbad, red);
  if (threadIdx.x == 0) bad[blockIdx.x] = tot;
}

// block (blockIdx.x = column tile, blockIdx.y = row group) of the view's rows [a, a + n) of the CSR matrix; scale and
// keep are indexed by the row of the whole matrix; see the head of the file
template <int MODE>
__global__ void __launch_bounds__(256)
moments_csr_walk_kernel(const long long* __restrict__ crow, const int* __restrict__ col, const float* __restrict__ val,
                        const unsigned char* __restrict__ keep, long long a, long long n, long long P, long long nnz,
                        long long R, const double* __restrict__ scale, double* __restrict__ p0, double* __restrict__ p1,
                        double* __restrict__ p2, double* __restrict__ bad) {
  __shared__ double c1s[4][MOM_COL_TILE], c2s[4][MOM_COL_TILE], c3s[4][MOM_COL_TILE];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long t = blockIdx.x, g = blockIdx.y;
  const long long c0 = t * MOM_COL_TILE, c1 = min(P, c0 + MOM_COL_TILE);
  const long long r0 = a + g * R, r1 = min(a + n, r0 + R);
  for (int cc = threadIdx.x; cc < 4 * MOM_COL_TILE; cc += 256)
    (&c1s[0][0])[cc] = 0.0, (&c2s[0][0])[cc] = 0.0, (&c3s[0][0])[cc] = 0.0;
  __syncthreads();
  double nbad = 0.0;
  for (long long i = r0 + w; i < r1; i += 4) {
    const double sc = MODE == MOM_SCALE ? scale[i] : 0.0;
    csr_row_in_tile(crow, col, val, keep, i, nnz, c0, c1, lane, [&](int cc, float y) {
      const double tv = mom_value<MODE>(y, sc);
      c1s[w][cc] += tv;
      c2s[w][cc] += tv * tv;
      c3s[w][cc] += fabs(tv);
      nbad += mom_nonfinite(tv);
    });
  }
  __syncthreads();
  // the four waves' columns meet in wave order
  for (int cc = threadIdx.x; cc < (int)(c1 - c0); cc += 256) {
    p0[g * P + c0 + cc] = meet4(c1s, cc);
    p1[g * P + c0 + cc] = meet4(c2s, cc);
    p2[g * P + c0 + cc] = meet4(c3s, cc);
  }
  const double tot = block_sum(nbad, red);
  if (threadIdx.x == 0) bad[g * gridDim.x + t] = tot;
}

// the planes [G, P] folded over the groups in order -> o0 / o1 / o2 [P] (the view's row of s1 / s2 / abs1); one more
// workgroup, the last, sums bad [nbad] into the view's slot.  64 columns x 4 contiguous segments of the groups per
// workgroup; the segments meet in LDS in order.
__global__ void __launch_bounds__(256)
moments_fold_kernel(const double* __restrict__ p0, const double* __restrict__ p1, const double* __restrict__ p2,
                    long long G, long long P, double* __restrict__ o0, double* __restrict__ o1, double* __restrict__ o2,
                    const double* __restrict__ bad, long long nbad, double* __restrict__ slot) {
  __shared__ double s0[4][WAVE], s1[4][WAVE], s2[4][WAVE];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  if (blockIdx.x == gridDim.x - 1) {
    double s = 0.0;
    for (long long k = threadIdx.x; k < nbad; k += 256) s += bad[k];
    s = block_sum(s, &s0[0][0]);
    if (threadIdx.x == 0) *slot = s;
    return;
  }
  const long long c = blockIdx.x * (long long)WAVE + lane;
  const long long per = (G + 3) / 4, g_lo = seg * per, g_hi = min(G, g_lo + per);
  double x0 = 0.0, x1 = 0.0, x2 = 0.0;
  if (c < P) {
#pragma unroll 4
    for (long long g = g_lo; g < g_hi; ++g) x0 += p0[g * P + c], x1 += p1[g * P + c], x2 += p2[g * P + c];
  }
  s0[seg][lane] = x0, s1[seg][lane] = x1, s2[seg][lane] = x2;
  __syncthreads();
  if (seg != 0 || c >= P) return;
  o0[c] = sum4(x0, s0[1][lane], s0[2][lane], s0[3][lane]);
  o1[c] = sum4(x1, s1[1][lane], s1[2][lane], s1[3][lane]);
  o2[c] = sum4(x2, s2[1][lane], s2[2][lane], s2[3][lane]);
}

// one workgroup: the views' counts (whole numbers held as doubles: exact in any order) -> the one int64
__global__ void __launch_bounds__(256)
moments_finish_kernel(const double* __restrict__ slot, int V, long long* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int v = threadIdx.x; v < V; v += 256) s += slot[v];
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out = (long long)s;
}

// what both entries ask of (mode, scale, view_off, V, the outputs): 0 or the refusal
static int mom_args_check(int mode, const void* scale, const long long* view_off, int V, long long N, const void* s1,
                          const void* s2, const void* abs1, const void* n_nonfinite) {
  if (mode < MOM_IDENTITY || mode > MOM_SCALE || (mode == MOM_SCALE && scale == nullptr)) return GPSA_EINVAL;
  if (!s1 || !s2 || !abs1 || !n_nonfinite) return GPSA_EINVAL;
  return view_off_check(view_off, V, N);
}

static int mom_fold(hipStream_t st, const MomWorkspace& ws, long long G, long long P, long long nbad, int v, double* s1,
                    double* s2, double* abs1) {
  const unsigned blocks = (unsigned)cdiv(P, WAVE) + 1u;
  moments_fold_kernel<<<blocks, 256, 0, st>>>(ws.p[0], ws.p[1], ws.p[2], G, P, s1 + v * P, s2 + v * P, abs1 + v * P,
                                              ws.bad, nbad, ws.badv + v);
  GPSA_LAUNCH_CHECK();
  return 0;
}

template <int MODE>
static int mom_dense(hipStream_t st, const float* Y, long long P, const double* scale, const long long* view_off, int V,
                     double* s1, double* s2, double* abs1, long long* n_nonfinite, const MomWorkspace& ws) {
  for (int v = 0; v < V; ++v) {
    const long long a = view_off[v], n = view_off[v + 1] - a;
    const int R = (int)mom_rows_per_group(n, MOM_MAX_GROUPS);
    const long long G = cdiv(n, R);
    const float* Yv = Y + a * P;
    const double* sv = MODE == MOM_SCALE ? scale + a : nullptr;
    if (P % 4 == 0 && ((uintptr_t)Yv % 16) == 0)
      moments_walk_kernel<MODE, true><<<(unsigned)G, 256, 0, st>>>(Yv, n, P, R, sv, ws.p[0], ws.p[1], ws.p[2], ws.bad);
    else
      moments_walk_kernel<MODE, false><<<(unsigned)G, 256, 0, st>>>(Yv, n, P, R, sv, ws.p[0], ws.p[1], ws.p[2], ws.bad);
    GPSA_LAUNCH_CHECK();
    if (int rc = mom_fold(st, ws, G, P, G, v, s1, s2, abs1)) return rc;
  }
  moments_finish_kernel<<<1, 256, 0, st>>>(ws.badv, V, n_nonfinite);
  GPSA_LAUNCH_CHECK();
  return 0;
}

template <int MODE>
static int mom_csr(hipStream_t st, const long long* crow, const int* col, const float* val, const unsigned char* keep,
                   long long P, long long nnz, const double* scale, const long long* view_off, int V, double* s1,
                   double* s2, double* abs1, long long* n_nonfinite, const MomWorkspace& ws) {
  const long long T = cdiv(P, (long long)MOM_COL_TILE);
  for (int v = 0; v < V; ++v) {
    const long long a = view_off[v], n = view_off[v + 1] - a;
    const long long R = mom_rows_per_group(n, MOM_CSR_MAX_GROUPS), G = cdiv(n, R);
    moments_csr_walk_kernel<MODE><<<dim3((unsigned)T, (unsigned)G), 256, 0, st>>>(crow, col, val, keep, a, n, P, nnz, R,
                                                                                  scale, ws.p[0], ws.p[1], ws.p[2], ws.bad);
    GPSA_LAUNCH_CHECK();
    if (int rc = mom_fold(st, ws, G, P, G * T, v, s1, s2, abs1)) return rc;
  }
  moments_finish_kernel<<<1, 256, 0, st>>>(ws.badv, V, n_nonfinite);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // namespace gpsa

extern "C" {

long long gpsa_column_moments_workspace(long long N, long long P, int V) {
  if (N < 1 || P < 1 || V < 1) return 0;
  return 8 * gpsa::MomWorkspace(nullptr, N, P, V, false).doubles;
}

long long gpsa_column_moments_csr_workspace(long long N, long long P, int V) {
  if (N < 1 || P < 1 || V < 1) return 0;
  return 8 * gpsa::MomWorkspace(nullptr, N, P, V, true).doubles;
}

int gpsa_column_moments_f32(int mode, const float* Y, long long N, long long P, const double* scale,
                            const long long* view_off, int V, double* s1, double* s2, double* abs1,
                            long long* n_nonfinite, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (Y == nullptr || N < 1 || P < 1) return GPSA_EINVAL;
  if (P > 0x7fffffffLL || N > 0x7fffffffLL * (long long)MOM_ROWS_MIN) return GPSA_EINVAL;  // the grids' extents
  if (int rc = mom_args_check(mode, scale, view_off, V, N, s1, s2, abs1, n_nonfinite)) return rc;
  if (workspace == nullptr || workspace_bytes < gpsa_column_moments_workspace(N, P, V)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const MomWorkspace ws(workspace, N, P, V, false);
  switch (mode) {
    case MOM_IDENTITY:
      return mom_dense<MOM_IDENTITY>(st, Y, P, scale, view_off, V, s1, s2, abs1, n_nonfinite, ws);
    case MOM_EXPM1:
      return mom_dense<MOM_EXPM1>(st, Y, P, scale, view_off, V, s1, s2, abs1, n_nonfinite, ws);
    default:
      return mom_dense<MOM_SCALE>(st, Y, P, scale, view_off, V, s1, s2, abs1, n_nonfinite, ws);
  }
}

int gpsa_column_moments_csr_f32(int mode, const long long* crow, const int* col, const float* val,
                                const unsigned char* keep, long long N, long long P, long long nnz, const double* scale,
                                const long long* view_off, int V, double* s1, double* s2, double* abs1,
                                long long* n_nonfinite, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (int rc = csr_shape_check(crow, col, val, N, P, nnz)) return rc;
  if (int rc = mom_args_check(mode, scale, view_off, V, N, s1, s2, abs1, n_nonfinite)) return rc;
  if (workspace == nullptr || workspace_bytes < gpsa_column_moments_csr_workspace(N, P, V)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const MomWorkspace ws(workspace, N, P, V, true);
  switch (mode) {
    case MOM_IDENTITY:
      return mom_csr<MOM_IDENTITY>(st, crow, col, val, keep, P, nnz, scale, view_off, V, s1, s2, abs1, n_nonfinite, ws);
    case MOM_EXPM1:
      return mom_csr<MOM_EXPM1>(st, crow, col, val, keep, P, nnz, scale, view_off, V, s1, s2, abs1, n_nonfinite, ws);
    default:
      return mom_csr<MOM_SCALE>(st, crow, col, val, keep, P, nnz, scale, view_off, V, s1, s2, abs1, n_nonfinite, ws);
  }
}

}  // extern "C"
