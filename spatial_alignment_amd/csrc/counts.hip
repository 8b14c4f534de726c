// Count preprocessing on the device: what turns a raw count matrix Y [N, P] (fp32, row-major, counts held as floats)
// into what the likelihoods take - the margins, the Poisson deviance per gene, the analytic residuals / log1p, the
// per-view z-score.  All four entries are streaming passes: Y is read once per reduction and once per transform, every
// sum is fp64 in a fixed order, nothing of N * P elements is allocated, and no output element has two writers.
//
// The reductions (margins, deviance, per-view moments) are ONE walk, count_walk_kernel:
//   * the rows are cut into G groups of R consecutive rows (count_rows_per_group: at least COUNT_ROWS_MIN, so that 8 000
//     rows already make 500 workgroups; at most COUNT_MAX_GROUPS groups while R stays <= COUNT_ROWS_MAX, so that the
//     column partials stay a small fraction of Y);
//   * workgroup g owns group g and walks the column tiles of COUNT_COL_TILE columns.  Inside a tile wave w takes the
//     rows w, w + 4, ... of the group, a lane holds 8 columns of the tile in registers (two 16-byte loads per row where
//     the pitch allows it, P % 4 == 0 and an aligned base; eight 4-byte loads, lane-contiguous, otherwise), the next
//     row's loads are in flight while a row is consumed;
//   * a row's total over the tile is a wave sum, added by lane 0 to the row's accumulator in LDS: the rows' results are
//     complete inside the workgroup;
//   * at the end of a tile the four waves' column accumulators meet in LDS in wave order and go to the group's row of
//     two partial planes pa / pb [G, P];
//   * count_fold_kernel folds the planes over the groups in order (64 columns x 4 contiguous segments per workgroup,
//     the segments combined in order), so the finishing launch has P / 64 workgroups of its own.
// The moments of the z-score are Welford's update per lane (the count is the wave's row count: one reciprocal per row)
// combined by Chan's formula across waves and groups - never E[y^2] - E[y]^2.
//
// The transforms are elementwise: fp64 arithmetic per element, rounded once to fp32, `out` may be Y itself (an element
// is read and written by the same thread).
//
// The tile loader, the Poisson term, the meet of four partial sums and the view_off check are row_walk.hpp's, shared
// with counts_sparse.hip and moments.hip.
#include <math.h>

#include "row_walk.hpp"

namespace gpsa {

constexpr int COUNT_COL_TILE = 512;     // columns of a tile: 8 per lane
constexpr int COUNT_ROWS_MIN = 16;      // rows of a group, at least (4 per wave)
constexpr int COUNT_ROWS_MAX = 512;     // ... at most (the rows' accumulators live in LDS)
constexpr int COUNT_MAX_GROUPS = 1024;  // groups, at most, while COUNT_ROWS_MAX allows it
constexpr int COUNT_PER_LANE = COUNT_COL_TILE / WAVE;
constexpr int COUNT_LOG_TABLE = 256;    // y log y of the counts below this comes from a table in LDS (deviance)

enum { WALK_MARGINS = 0, WALK_DEVIANCE = 1, WALK_MOMENTS = 2 };
enum { TR_PEARSON = 0, TR_NB_DEVIANCE = 1, TR_POISSON_DEVIANCE = 2, TR_LOG1P = 3, TR_ZSCORE = 4 };

static long long count_rows_per_group(long long n) {
  long long r = cdiv(n, (long long)COUNT_MAX_GROUPS);
  r = r < COUNT_ROWS_MIN ? COUNT_ROWS_MIN : r;
  return r > COUNT_ROWS_MAX ? COUNT_ROWS_MAX : r;
}
// the most groups any n <= N is cut into (the views of the z-score share one workspace)
static long long count_groups_bound(long long N) {
  if (N <= (long long)COUNT_MAX_GROUPS * COUNT_ROWS_MAX) {
    const long long g = cdiv(N, (long long)COUNT_ROWS_MIN);
    return g < COUNT_MAX_GROUPS ? g : COUNT_MAX_GROUPS;
  }
  return cdiv(N, (long long)COUNT_ROWS_MAX);
}
// workspace layout: pa [Gb, P], pb [Gb, P], bad [Gb], mean [P], istd [P]   (doubles)
static long long count_workspace_doubles(long long N, long long P) {
  const long long gb = count_groups_bound(N);
  return 2 * gb * P + gb + 2 * P;
}

// (n, mean, M2) of a set joined with (nb, mb, qb) of the rows after it
__device__ __forceinline__ void chan_join(double& n, double& mean, double& m2, double nb, double mb, double qb) {
  if (nb == 0.0) return;
  if (n == 0.0) {
    n = nb, mean = mb, m2 = qb;
    return;
  }
  const double tot = n + nb, d = mb - mean;
  mean += d * (nb / tot);
  m2 += qb + d * d * (n * nb / tot);
  n = tot;
}

// rows [blockIdx.x * R, ...) of Y [n, P]; see the head of the file.
//   WALK_MARGINS:  pa = sums, pb = entries > 0 per column; row_a / row_b the same per row; bad[g] = entries that are
//                  NaN, +-inf or < 0
//   WALK_DEVIANCE: aux = log_sz [n]; pa = sum y log y - y log_sz, pb = sum |y log y| + |y log_sz| (y = 0: 0)
//   WALK_MOMENTS:  pa = mean, pb = sum of squared deviations from it, of the group's rows
template <int MODE, bool VEC>
__global__ void __launch_bounds__(256)
count_walk_kernel(const float* __restrict__ Y, long long n, long long P, int R, const double* __restrict__ aux,
                  double* __restrict__ pa, double* __restrict__ pb, double* __restrict__ row_a,
                  long long* __restrict__ row_b, double* __restrict__ bad) {
  __shared__ double ca[4][COUNT_COL_TILE], cb[4][COUNT_COL_TILE];
  __shared__ double ra[MODE == WALK_MARGINS ? COUNT_ROWS_MAX : 1];
  __shared__ int rn[MODE == WALK_MARGINS ? COUNT_ROWS_MAX : 1];
  __shared__ double red[4];
  __shared__ double ylogy[MODE == WALK_DEVIANCE ? COUNT_LOG_TABLE : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * R;
  const int rows = (int)min((long long)R, n - r0);
  const float* Yg = Y + r0 * P;
  if (MODE == WALK_MARGINS) {
    for (int t = threadIdx.x; t < rows; t += 256) ra[t] = 0.0, rn[t] = 0;
    __syncthreads();
  }
  if (MODE == WALK_DEVIANCE) {
    ylogy_fill<COUNT_LOG_TABLE>(ylogy);
    __syncthreads();
  }
  double nbad = 0.0;
  for (long long c0 = 0; c0 < P; c0 += COUNT_COL_TILE) {
    double a[COUNT_PER_LANE], b[COUNT_PER_LANE];
#pragma unroll
    for (int k = 0; k < COUNT_PER_LANE; ++k) a[k] = 0.0, b[k] = 0.0;
    float cur[COUNT_PER_LANE] = {}, nxt[COUNT_PER_LANE] = {};
    if (w < rows) load_row<VEC, COUNT_PER_LANE>(Yg + (long long)w * P, c0, P, lane, cur);
    int seen = 0;
    for (int r = w; r < rows; r += 4) {
      if (r + 4 < rows) load_row<VEC, COUNT_PER_LANE>(Yg + (long long)(r + 4) * P, c0, P, lane, nxt);
      if (MODE == WALK_MARGINS) {
        double s = 0.0;
        float z = 0.f;
#pragma unroll
        for (int k = 0; k < COUNT_PER_LANE; ++k) {
          const float y = cur[k];
          const bool pos = y > 0.f;
          a[k] += (double)y;
          b[k] += pos ? 1.0 : 0.0;
          s += (double)y;
          z += pos ? 1.f : 0.f;
          nbad += (y >= 0.f && y < INFINITY) ? 0.0 : 1.0;
        }
        s = wave_sum(s);
        z = wave_sum(z);
        if (lane == 0) ra[r] += s, rn[r] += (int)z;  // row r belongs to this wave alone
      } else if (MODE == WALK_DEVIANCE) {
        const double lsz = aux[r0 + r];
#pragma unroll
        for (int k = 0; k < COUNT_PER_LANE; ++k) {
          if ((double)cur[k] > 0.0) {
            double t1, t2;
            poisson_terms<COUNT_LOG_TABLE>(ylogy, cur[k], lsz, t1, t2);
            a[k] += t1 - t2;
            b[k] += fabs(t1) + fabs(t2);
          }
        }
      } else {
        seen += 1;
        const double inv = 1.0 / (double)seen;
#pragma unroll
        for (int k = 0; k < COUNT_PER_LANE; ++k) {
          const double y = (double)cur[k], d = y - a[k];
          a[k] = fma(d, inv, a[k]);
          b[k] = fma(d, y - a[k], b[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < COUNT_PER_LANE; ++k) cur[k] = nxt[k];
    }
    // the four waves' columns meet in wave order
#pragma unroll
    for (int k = 0; k < COUNT_PER_LANE; ++k) {
      ca[w][tile_col<VEC>(lane, k)] = a[k];
      cb[w][tile_col<VEC>(lane, k)] = b[k];
    }
    __syncthreads();
    for (int cc = threadIdx.x; cc < COUNT_COL_TILE; cc += 256) {
      const long long c = c0 + cc;
      if (c >= P) break;
      double va, vb;
      if (MODE == WALK_MOMENTS) {
        double cnt = 0.0;
        va = 0.0, vb = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double nu = rows > u ? (double)((rows - u + 3) / 4) : 0.0;  // rows u, u + 4, ... below `rows`
          chan_join(cnt, va, vb, nu, ca[u][cc], cb[u][cc]);
        }
      } else {
        va = meet4(ca, cc);
        vb = meet4(cb, cc);
      }
      pa[(long long)blockIdx.x * P + c] = va;
      pb[(long long)blockIdx.x * P + c] = vb;
    }
    __syncthreads();  // before the next tile's columns land in ca / cb
  }
  if (MODE == WALK_MARGINS) {
    for (int t = threadIdx.x; t < rows; t += 256) row_a[r0 + t] = ra[t], row_b[r0 + t] = (long long)rn[t];
    const double tot = block_sum(nbad, red);
    if (threadIdx.x == 0) bad[blockIdx.x] = tot;
  }
}

// the planes pa / pb [G, P] folded over the groups in order -> per column
//   WALK_MARGINS:  oa = col_sum, ob = col_nnz (int64); one more workgroup, the last, sums bad [G] into n_invalid
//   WALK_DEVIANCE: oa = ll_sat, ob = abs_sat (double)
//   WALK_MOMENTS:  oa = mean, ob = 1 / std of the n rows (population), 0 where the column is constant (M2 == 0 exactly:
//                  every Welford and Chan step of a constant column is exact)
// 64 columns x 4 contiguous segments of the groups per workgroup; the segments meet in LDS in order.
template <int MODE>
__global__ void __launch_bounds__(256)
count_fold_kernel(const double* __restrict__ pa, const double* __restrict__ pb, long long G, long long P, int R,
                  long long n, double* __restrict__ oa, void* __restrict__ ob, const double* __restrict__ bad,
                  long long* __restrict__ n_invalid) {
  __shared__ double sa[4][WAVE], sb[4][WAVE], sn[4][WAVE];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  if (MODE == WALK_MARGINS && blockIdx.x == gridDim.x - 1) {
    double s = 0.0;
    for (long long g = threadIdx.x; g < G; g += 256) s += bad[g];
    s = block_sum(s, &sa[0][0]);
    if (threadIdx.x == 0) *n_invalid = (long long)s;
    return;
  }
  const long long c = blockIdx.x * (long long)WAVE + lane;
  const long long per = (G + 3) / 4, g_lo = seg * per, g_hi = min(G, g_lo + per);
  double a = 0.0, b = 0.0, cnt = 0.0;
  if (c < P) {
#pragma unroll 4
    for (long long g = g_lo; g < g_hi; ++g) {
      const double va = pa[g * P + c], vb = pb[g * P + c];
      if (MODE == WALK_MOMENTS) {
        chan_join(cnt, a, b, (double)min((long long)R, n - g * R), va, vb);
      } else {
        a += va;
        b += vb;
      }
    }
  }
  sa[seg][lane] = a, sb[seg][lane] = b, sn[seg][lane] = cnt;
  __syncthreads();
  if (seg != 0 || c >= P) return;
  if (MODE == WALK_MOMENTS) {
    for (int u = 1; u < 4; ++u) chan_join(cnt, a, b, sn[u][lane], sa[u][lane], sb[u][lane]);
    oa[c] = a;
    ((double*)ob)[c] = b > 0.0 ? 1.0 / sqrt(b / (double)n) : 0.0;
  } else {
    a = sum4(a, sa[1][lane], sa[2][lane], sa[3][lane]);
    b = sum4(b, sb[1][lane], sb[2][lane], sb[3][lane]);
    oa[c] = a;
    if (MODE == WALK_MARGINS)
      ((long long*)ob)[c] = (long long)b;
    else
      ((double*)ob)[c] = b;
  }
}

// the columns of a view whose 1 / std was set to 0 (constant within the view): one workgroup
__global__ void __launch_bounds__(256)
count_constant_kernel(const double* __restrict__ istd, long long P, long long* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (long long c = threadIdx.x; c < P; c += 256) s += istd[c] == 0.0 ? 1.0 : 0.0;
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out = (long long)s;
}

// one element.  u: the row's sum (TR_ZSCORE: the column's 1 / std; TR_LOG1P: target / the row's sum, 0 in an empty row),
// v: the column's sum (TR_ZSCORE: its mean); inv_total = 1 / total, inv_theta = 1 / theta (0 for theta = inf)
template <int MODE>
__device__ __forceinline__ float transform_one(float yf, double u, double v, double inv_total, double theta,
                                               double inv_theta, double clip) {
  const double y = (double)yf;
  double z;
  if (MODE == TR_ZSCORE) {
    z = (y - v) * u;
  } else if (MODE == TR_LOG1P) {
    z = y > 0.0 ? log1p(y * u) : 0.0;
  } else {
    const double mu = u * v * inv_total;
    if (!(mu > 0.0)) return 0.f;  // an empty row or column: the reference divides 0 by 0 there
    if (MODE == TR_PEARSON) {
      z = (y - mu) * rsqrt(fma(mu * mu, inv_theta, mu));
      if (clip > 0.0) z = z > clip ? clip : (z < -clip ? -clip : z);
    } else {
      const double xl = y > 0.0 ? y * log(y / mu) : 0.0;
      double t = MODE == TR_POISSON_DEVIANCE ? 2.0 * (xl - (y - mu))
                                             : 2.0 * (xl - (y + theta) * log((y + theta) / (mu + theta)));
      t = t > 0.0 ? t : 0.0;
      z = y > mu ? sqrt(t) : (y < mu ? -sqrt(t) : 0.0);
    }
  }
  return (float)z;
}

// what an element takes from its row: the row's sum, or for TR_LOG1P target / the row's sum (0 in an empty row)
template <int MODE>
__device__ __forceinline__ double row_factor(const double* __restrict__ u, long long i, double target) {
  if (MODE == TR_ZSCORE) return 0.0;
  const double ui = u[i];
  if (MODE == TR_LOG1P) return ui > 0.0 ? target / ui : 0.0;
  return ui;
}

// grid-stride over the quads (VEC) or the elements of Y [N, P].  Y and out are not restrict: they may be one array.
template <int MODE, bool VEC>
__global__ void __launch_bounds__(256)
count_transform_kernel(const float* Y, long long N, long long P, const double* __restrict__ u, const double* __restrict__ v,
                       double total, double theta, double clip, double target, float* out) {
  const long long step = (long long)gridDim.x * 256;
  const double inv_total = 1.0 / total, inv_theta = 1.0 / theta;
  if (VEC) {
    const long long pq = P / 4, nq = N * pq;
    for (long long q = blockIdx.x * 256LL + threadIdx.x; q < nq; q += step) {
      const long long i = q / pq, c = (q - i * pq) * 4;
      const float4 y = *reinterpret_cast<const float4*>(Y + i * P + c);
      const float yy[4] = {y.x, y.y, y.z, y.w};
      const double ui = row_factor<MODE>(u, i, target);
      float oo[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        oo[e] = transform_one<MODE>(yy[e], MODE == TR_ZSCORE ? u[c + e] : ui, MODE == TR_LOG1P ? 0.0 : v[c + e], inv_total,
                                    theta, inv_theta, clip);
      *reinterpret_cast<float4*>(out + i * P + c) = make_float4(oo[0], oo[1], oo[2], oo[3]);
    }
  } else {
    const long long ne = N * P;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < ne; e += step) {
      const long long i = e / P, c = e - i * P;
      out[e] = transform_one<MODE>(Y[e], MODE == TR_ZSCORE ? u[c] : row_factor<MODE>(u, i, target),
                                   MODE == TR_LOG1P ? 0.0 : v[c], inv_total, theta, inv_theta, clip);
    }
  }
}

static bool count_vec_ok(const void* a, const void* b, long long P) {
  return P % 4 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0;
}

template <int MODE>
static int launch_walk(hipStream_t st, const float* Y, long long n, long long P, const double* aux, double* pa, double* pb,
                       double* row_a, long long* row_b, double* bad) {
  const int R = (int)count_rows_per_group(n);
  const unsigned G = (unsigned)cdiv(n, R);
  if (count_vec_ok(Y, Y, P))
    count_walk_kernel<MODE, true><<<G, 256, 0, st>>>(Y, n, P, R, aux, pa, pb, row_a, row_b, bad);
  else
    count_walk_kernel<MODE, false><<<G, 256, 0, st>>>(Y, n, P, R, aux, pa, pb, row_a, row_b, bad);
  GPSA_LAUNCH_CHECK();
  return 0;
}

template <int MODE>
static int launch_fold(hipStream_t st, const double* pa, const double* pb, long long n, long long P, double* oa, void* ob,
                       const double* bad, long long* n_invalid) {
  const int R = (int)count_rows_per_group(n);
  const long long G = cdiv(n, R);
  const unsigned blocks = (unsigned)cdiv(P, WAVE) + (MODE == WALK_MARGINS ? 1u : 0u);
  count_fold_kernel<MODE><<<blocks, 256, 0, st>>>(pa, pb, G, P, R, n, oa, ob, bad, n_invalid);
  GPSA_LAUNCH_CHECK();
  return 0;
}

template <int MODE>
static int launch_transform(hipStream_t st, const float* Y, long long N, long long P, const double* u, const double* v,
                            double total, double theta, double clip, double target, float* out) {
  const bool vec = count_vec_ok(Y, out, P);
  const long long work = cdiv(vec ? N * (P / 4) : N * P, 256), cap = 16LL * num_cus();
  const unsigned grid = (unsigned)(work < cap ? work : cap);
  if (vec)
    count_transform_kernel<MODE, true><<<grid, 256, 0, st>>>(Y, N, P, u, v, total, theta, clip, target, out);
  else
    count_transform_kernel<MODE, false><<<grid, 256, 0, st>>>(Y, N, P, u, v, total, theta, clip, target, out);
  GPSA_LAUNCH_CHECK();
  return 0;
}

// what every entry asks of (Y, N, P): 0 or the refusal
static int count_shape_check(const void* Y, long long N, long long P) {
  if (Y == nullptr || N < 1 || P < 1) return GPSA_EINVAL;
  if (P > 0x7fffffffLL || N > 0x7fffffffLL * (long long)COUNT_ROWS_MIN) return GPSA_EINVAL;  // the grids' extents
  return 0;
}

struct CountWorkspace {
  double *pa, *pb, *bad, *mean, *istd;
  CountWorkspace(void* ws, long long N, long long P) {
    const long long gb = count_groups_bound(N);
    pa = (double*)ws, pb = pa + gb * P, bad = pb + gb * P, mean = bad + gb, istd = mean + P;
  }
};

}  // namespace gpsa

extern "C" {

long long gpsa_count_workspace(long long N, long long P) {
  if (N < 1 || P < 1) return 0;
  return 8 * gpsa::count_workspace_doubles(N, P);
}

int gpsa_count_margins_f32(const float* Y, long long N, long long P, double* row_sum, double* col_sum, long long* row_nnz,
                           long long* col_nnz, long long* n_invalid, void* workspace, long long workspace_bytes,
                           void* stream) {
  using namespace gpsa;
  if (int rc = count_shape_check(Y, N, P)) return rc;
  if (!row_sum || !col_sum || !row_nnz || !col_nnz || !n_invalid) return GPSA_EINVAL;
  if (workspace == nullptr || workspace_bytes < gpsa_count_workspace(N, P)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const CountWorkspace ws(workspace, N, P);
  if (int rc = launch_walk<WALK_MARGINS>(st, Y, N, P, nullptr, ws.pa, ws.pb, row_sum, row_nnz, ws.bad)) return rc;
  return launch_fold<WALK_MARGINS>(st, ws.pa, ws.pb, N, P, col_sum, col_nnz, ws.bad, n_invalid);
}

int gpsa_count_deviance_f32(const float* Y, long long N, long long P, const double* log_sz, double* ll_sat, double* abs_sat,
                            void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (int rc = count_shape_check(Y, N, P)) return rc;
  if (!log_sz || !ll_sat || !abs_sat) return GPSA_EINVAL;
  if (workspace == nullptr || workspace_bytes < gpsa_count_workspace(N, P)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const CountWorkspace ws(workspace, N, P);
  if (int rc = launch_walk<WALK_DEVIANCE>(st, Y, N, P, log_sz, ws.pa, ws.pb, nullptr, nullptr, nullptr)) return rc;
  return launch_fold<WALK_DEVIANCE>(st, ws.pa, ws.pb, N, P, ll_sat, abs_sat, nullptr, nullptr);
}

int gpsa_count_transform_f32(int mode, const float* Y, long long N, long long P, const double* row_sum,
                             const double* col_sum, double total, double theta, double clip, double target, float* out,
                             void* stream) {
  using namespace gpsa;
  if (int rc = count_shape_check(Y, N, P)) return rc;
  if (mode < TR_PEARSON || mode > TR_LOG1P) return GPSA_EINVAL;
  if (out == nullptr || row_sum == nullptr) return GPSA_EINVAL;
  if (mode == TR_LOG1P) {
    if (!(target > 0.0) || !(target < INFINITY)) return GPSA_EINVAL;
  } else {
    if (col_sum == nullptr || !(total > 0.0) || !(total < INFINITY)) return GPSA_EINVAL;
    if (mode != TR_POISSON_DEVIANCE && !(theta > 0.0)) return GPSA_EINVAL;  // (also a NaN)
    if (mode == TR_NB_DEVIANCE && !(theta < INFINITY)) return GPSA_EINVAL;  // theta = inf is TR_POISSON_DEVIANCE
    if (mode == TR_PEARSON && !(clip >= 0.0)) return GPSA_EINVAL;
  }
  hipStream_t st = as_stream(stream);
  switch (mode) {
    case TR_PEARSON:
      return launch_transform<TR_PEARSON>(st, Y, N, P, row_sum, col_sum, total, theta, clip, target, out);
    case TR_NB_DEVIANCE:
      return launch_transform<TR_NB_DEVIANCE>(st, Y, N, P, row_sum, col_sum, total, theta, clip, target, out);
    case TR_POISSON_DEVIANCE:
      return launch_transform<TR_POISSON_DEVIANCE>(st, Y, N, P, row_sum, col_sum, total, theta, clip, target, out);
    default:
      return launch_transform<TR_LOG1P>(st, Y, N, P, row_sum, col_sum, total, theta, clip, target, out);
  }
}

int gpsa_standardize_views_f32(const float* Y, long long N, long long P, const long long* view_off, int V, float* out,
                               long long* n_constant, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (int rc = count_shape_check(Y, N, P)) return rc;
  if (!out || !n_constant) return GPSA_EINVAL;
  if (int rc = view_off_check(view_off, V, N)) return rc;
  if (workspace == nullptr || workspace_bytes < gpsa_count_workspace(N, P)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const CountWorkspace ws(workspace, N, P);
  for (int v = 0; v < V; ++v) {
    const long long a = view_off[v], n = view_off[v + 1] - a;
    const float* Yv = Y + a * P;
    if (int rc = launch_walk<WALK_MOMENTS>(st, Yv, n, P, nullptr, ws.pa, ws.pb, nullptr, nullptr, nullptr)) return rc;
    if (int rc = launch_fold<WALK_MOMENTS>(st, ws.pa, ws.pb, n, P, ws.mean, ws.istd, nullptr, nullptr)) return rc;
    count_constant_kernel<<<1, 256, 0, st>>>(ws.istd, P, n_constant + v);
    GPSA_LAUNCH_CHECK();
    if (int rc = launch_transform<TR_ZSCORE>(st, Yv, n, P, ws.istd, ws.mean, 1.0, 1.0, 0.0, 1.0, out + a * P)) return rc;
  }
  return 0;
}

}  // extern "C"
