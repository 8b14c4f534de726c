// Optimal-transport slice alignment on the device (ot.py): the kernels of an entropic fused Gromov-Wasserstein solve
// between two slices (Peyre, Cuturi and Solomon 2016: projected gradient, each step a log-domain Sinkhorn solve), next
// to the dense fp64 products that exist already (gpsa_gemm).  All fp64; the expression matrices are read as fp32.
//
//   C1 = |x_i - x_k|, C2 = |y_j - y_l|                         ot_dist_kernel (the tile scheme of gpr_cov_kernel, `same`)
//   cA = (C1 o C1) a                                           ot_sqmatvec_kernel
//   P = (Y + 0.01) / row sum, log P, sum_p P log P             ot_expr_rows_kernel ("kl"; "euclidean": Y, sum_p y^2)
//   M = term_i - (P log Q^T)_ij   |   r_i + r_j - 2 (A B^T)_ij  ot_expr_cost_kernel, in place over the product
//   cost = (1 - alpha) M + 2 alpha (cA 1^T + 1 cB^T - 2 G)      ot_cost_kernel, in place over G = C1 T C2, reducing
//                                                              sum |cost|, <M, T>, <cA' 1^T + 1 cB'^T - 2 G, T>
//   f_i = -e LSE_j((g_j - cost_ij) / e + log b_j)              ot_sink_row_kernel: a wave per row, online (max, sum)
//   g_j = -e LSE_i((f_i - cost_ij) / e + log a_i)              ot_sink_col_kernel + ot_sink_merge_kernel
//   T_ij = a_i b_j exp((f_i + g_j - cost_ij) / e)              ot_plan_kernel, reducing T 1, T^T 1, |T - T_old|_1
//
// Every sum runs in a fixed order without atomics: a repeated call gives the same bits.  A row is never split over
// workgroups in the row pass.  The column pass and the plan cut the n rows into G <= OT_MAX_GROUPS groups of R
// consecutive rows (ot_rows_per_group: at least OT_ROWS_MIN); workgroup (t, g) owns columns 64 t .. 64 t + 63 of group g,
// a lane holds one column, wave w takes the rows w, w + 4, ... of the group, the four waves meet in LDS in wave order and
// a (max, sum) partial per (group, column) goes to the workspace, where the groups are merged in order (the pattern of
// gpsa_count_margins_f32).  Every exponential has the running maximum subtracted: |cost| / e in the thousands neither
// overflows nor gives a NaN.  e is read from a device double.  Nothing of n m elements is allocated here.
#include <math.h>

#include "toolbox.hpp"

namespace gpsa {

constexpr int OT_T = 64;             // tile edge of the distance kernel; columns of a tile in the column pass and the plan
constexpr int OT_ROWS_MIN = 64;      // rows of a group, at least
constexpr int OT_MAX_GROUPS = 128;   // groups, at most
constexpr int OT_COST_BLOCKS = 1024; // workgroups of the cost pass, at most
enum { OT_KL = 0, OT_EUCLIDEAN = 1 };

static long long ot_rows_per_group(long long n) {
  const long long r = cdiv(n, (long long)OT_MAX_GROUPS);
  return r < OT_ROWS_MIN ? OT_ROWS_MIN : r;
}
static long long ot_groups(long long n) { return cdiv(n, ot_rows_per_group(n)); }
static long long ot_col_tiles(long long m) { return cdiv(m, (long long)OT_T); }
static long long ot_cost_blocks(long long n) { return n < OT_COST_BLOCKS ? n : OT_COST_BLOCKS; }

// one more term v of a running log-sum-exp held as (mx, s): the sum of exp(. - mx)
__device__ __forceinline__ void ot_lse_add(double v, double& mx, double& s) {
  if (v > mx) {
    s = s * exp(mx - v) + 1.0;  // (mx = -inf at the start: 0 * 0 + 1)
    mx = v;
  } else {
    s += exp(v - mx);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// distances
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
ot_dist_kernel(const double* __restrict__ X, long long n, int D, double* __restrict__ Cm) {
  __shared__ double xa[OT_T][MAXD], xb[OT_T][MAXD];
  __shared__ double tile[OT_T][OT_T + 1];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;  // block-uniform: the mirror of (bj, bi) writes this tile
  const long long i0 = (long long)bi * OT_T, j0 = (long long)bj * OT_T;
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  if (tid < 2 * OT_T) {  // what stage_rows64 writes, both tiles in one branch: two calls change this kernel's registers
    const int t = tid & 63;
    const long long r = (tid < OT_T ? i0 : j0) + t;
    double(*xs)[MAXD] = tid < OT_T ? xa : xb;
#pragma unroll
    for (int d = 0; d < MAXD; ++d) xs[t][d] = (r < n && d < D) ? X[r * D + d] : 0.0;
  }
  __syncthreads();
  const long long j = j0 + tx;
  for (int r = ty; r < OT_T; r += 4) {
    const long long i = i0 + r;
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < MAXD; ++d) {
      const double t = xa[r][d] - xb[tx][d];
      s += t * t;
    }
    const double v = sqrt(s);
    if (i < n && j < n) Cm[i * n + j] = v;
    tile[r][tx] = v;
  }
  if (bi != bj) {
    __syncthreads();
    const long long ii = i0 + tx;
    for (int r = ty; r < OT_T; r += 4) {
      const long long jj = j0 + r;
      if (jj < n && ii < n) Cm[jj * n + ii] = tile[tx][r];
    }
  }
}

// out_i = sum_k C_ik^2 v_k: a wave per row of C [n, ncol]
__global__ void __launch_bounds__(256)
ot_sqmatvec_kernel(const double* __restrict__ Cm, long long n, long long ncol, const double* __restrict__ v,
                   double* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + w;
  if (row >= n) return;
  const double* c = Cm + row * ncol;
  double s = 0.0;
  for (long long k = lane; k < ncol; k += WAVE) s += c[k] * c[k] * v[k];
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// expression rows and the expression cost
// ---------------------------------------------------------------------------------------------------------------------
// a wave per row of Y [n, P] fp32.  OT_KL: Pm = (y + 0.01) / row sum, Lg = log Pm, term = sum_p Pm Lg, bad = the row's
// entries that are negative, NaN or inf.  OT_EUCLIDEAN: Pm = y, term = sum_p y^2, bad = the NaN or inf entries.
template <int MODE>
__global__ void __launch_bounds__(256)
ot_expr_rows_kernel(const float* __restrict__ Y, long long n, long long P, double* __restrict__ Pm,
                    double* __restrict__ Lg, double* __restrict__ term, double* __restrict__ bad) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + w;
  if (row >= n) return;
  const float* y = Y + row * P;
  double s = 0.0, nb = 0.0;
  for (long long p = lane; p < P; p += WAVE) {
    const double v = (double)y[p];
    const bool finite = fabs(v) < INFINITY;  // (a NaN: false)
    nb += (MODE == OT_KL ? (finite && v >= 0.0) : finite) ? 0.0 : 1.0;
    s += MODE == OT_KL ? v + 0.01 : v * v;
  }
  s = wave_sum(s);
  nb = wave_sum(nb);
  double t = s;
  if (MODE == OT_KL) {
    t = 0.0;
    for (long long p = lane; p < P; p += WAVE) {
      const double pv = ((double)y[p] + 0.01) / s, lp = log(pv);
      Pm[row * P + p] = pv;
      Lg[row * P + p] = lp;
      t += pv * lp;
    }
    t = wave_sum(t);
  } else {
    for (long long p = lane; p < P; p += WAVE) Pm[row * P + p] = (double)y[p];
  }
  if (lane == 0) term[row] = t, bad[row] = nb;
}

// one workgroup: whole numbers held as doubles (exact in any order) -> the one int64
__global__ void __launch_bounds__(256)
ot_count_kernel(const double* __restrict__ bad, long long n, long long* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (long long k = threadIdx.x; k < n; k += 256) s += bad[k];
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out = (long long)s;
}

// in place over G [n, m]: OT_KL  M = ra_i - G_ij (G = P log Q^T);  OT_EUCLIDEAN  M = max(0, ra_i + rb_j - 2 G_ij) (G = A B^T)
template <int MODE>
__global__ void __launch_bounds__(256)
ot_expr_cost_kernel(double* __restrict__ G, long long n, long long m, const double* __restrict__ ra,
                    const double* __restrict__ rb) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const double bj = MODE == OT_EUCLIDEAN ? rb[j] : 0.0;
  for (long long i = blockIdx.y; i < n; i += gridDim.y) {
    const double g = G[i * m + j];
    G[i * m + j] = MODE == OT_KL ? ra[i] - g : fmax(0.0, (ra[i] + bj) - 2.0 * g);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the cost of an outer step, in place over G = C1 T C2, and the three sums of the same pass
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
ot_cost_kernel(double* __restrict__ G, const double* __restrict__ M, const double* __restrict__ T,
               const double* __restrict__ cA, const double* __restrict__ cB, const double* __restrict__ cAt,
               const double* __restrict__ cBt, double alpha, long long n, long long m, double* __restrict__ part) {
  __shared__ double red[3][4];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long i = blockIdx.x; i < n; i += gridDim.x) {
    const double ai = cA[i], ati = cAt[i];
    for (long long j = threadIdx.x; j < m; j += 256) {
      const long long idx = i * m + j;
      const double g = G[idx], mm = M[idx], t = T[idx];
      const double c = (1.0 - alpha) * mm + 2.0 * alpha * ((ai + cB[j]) - 2.0 * g);
      G[idx] = c;
      s0 += fabs(c);
      s1 += mm * t;
      s2 += ((ati + cBt[j]) - 2.0 * g) * t;
    }
  }
  s0 = block_sum(s0, red[0]);
  s1 = block_sum(s1, red[1]);
  s2 = block_sum(s2, red[2]);
  if (threadIdx.x == 0) part[blockIdx.x * 3] = s0, part[blockIdx.x * 3 + 1] = s1, part[blockIdx.x * 3 + 2] = s2;
}

// the workgroups' triples in one fixed order -> out[0..2]
__global__ void __launch_bounds__(256)
ot_close3_kernel(const double* __restrict__ part, long long nblk, double* __restrict__ out) {
  __shared__ double red[3][256];
  fold3_partials(part, nblk, red);
  if (threadIdx.x < 3) out[threadIdx.x] = red[threadIdx.x][0];
}

// ---------------------------------------------------------------------------------------------------------------------
// the Sinkhorn sweep
// ---------------------------------------------------------------------------------------------------------------------
// f_i = -e LSE_j((g_j - cost_ij) / e + log b_j): a wave per row, a lane the columns lane, lane + 64, ...; the lanes'
// (max, sum) pairs meet at the wave's maximum and are added by wave_sum
__global__ void __launch_bounds__(256)
ot_sink_row_kernel(const double* __restrict__ cost, long long n, long long m, const double* __restrict__ g,
                   const double* __restrict__ logb, const double* __restrict__ eps_p, double* __restrict__ f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + w;
  if (row >= n) return;
  const double eps = *eps_p;
  const double* c = cost + row * m;
  double mx = -INFINITY, s = 0.0;
  long long j = lane;
  for (; j + 3 * WAVE < m; j += 4 * WAVE) {  // four loads in flight
    const double c0 = c[j], c1 = c[j + WAVE], c2 = c[j + 2 * WAVE], c3 = c[j + 3 * WAVE];
    ot_lse_add((g[j] - c0) / eps + logb[j], mx, s);
    ot_lse_add((g[j + WAVE] - c1) / eps + logb[j + WAVE], mx, s);
    ot_lse_add((g[j + 2 * WAVE] - c2) / eps + logb[j + 2 * WAVE], mx, s);
    ot_lse_add((g[j + 3 * WAVE] - c3) / eps + logb[j + 3 * WAVE], mx, s);
  }
  for (; j < m; j += WAVE) ot_lse_add((g[j] - c[j]) / eps + logb[j], mx, s);
  const double top = wave_max(mx);                  // finite: m >= 1, lane 0 holds a column
  s = wave_sum(s == 0.0 ? 0.0 : s * exp(mx - top)); // (a lane without a column: s = 0, mx = -inf)
  if (lane == 0) f[row] = -eps * (top + log(s));
}

// the (max, sum) of exp((f_i - cost_ij) / e + log a_i) over the rows of group blockIdx.y, per column: pm, ps [G, m]
__global__ void __launch_bounds__(256)
ot_sink_col_kernel(const double* __restrict__ cost, long long n, long long m, long long R, const double* __restrict__ f,
                   const double* __restrict__ loga, const double* __restrict__ eps_p, double* __restrict__ pm,
                   double* __restrict__ ps) {
  __shared__ double lm[4][WAVE], ls[4][WAVE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long j = (long long)blockIdx.x * OT_T + lane, grp = blockIdx.y;
  const long long r0 = grp * R, r1 = min(n, r0 + R);
  const double eps = *eps_p;
  double mx = -INFINITY, s = 0.0;
  if (j < m) {
    long long i = r0 + w;
    for (; i + 4 < r1; i += 8) {  // two loads in flight
      const double c0 = cost[i * m + j], c1 = cost[(i + 4) * m + j];
      ot_lse_add((f[i] - c0) / eps + loga[i], mx, s);
      ot_lse_add((f[i + 4] - c1) / eps + loga[i + 4], mx, s);
    }
    for (; i < r1; i += 4) ot_lse_add((f[i] - cost[i * m + j]) / eps + loga[i], mx, s);
  }
  lm[w][lane] = mx, ls[w][lane] = s;
  __syncthreads();
  if (w != 0 || j >= m) return;
  // the four waves in wave order (wave 0 holds row r0: the maximum is finite)
  const double top = fmax(fmax(lm[0][lane], lm[1][lane]), fmax(lm[2][lane], lm[3][lane]));
  double tot = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) tot += ls[k][lane] == 0.0 ? 0.0 : ls[k][lane] * exp(lm[k][lane] - top);
  pm[grp * m + j] = top;
  ps[grp * m + j] = tot;
}

// the groups' pairs merged in group order: g_j = -e (max + log sum)
__global__ void __launch_bounds__(256)
ot_sink_merge_kernel(const double* __restrict__ pm, const double* __restrict__ ps, long long G, long long m,
                     const double* __restrict__ eps_p, double* __restrict__ g) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  double top = -INFINITY;
  for (long long k = 0; k < G; ++k) top = fmax(top, pm[k * m + j]);
  double tot = 0.0;
  for (long long k = 0; k < G; ++k) tot += ps[k * m + j] * exp(pm[k * m + j] - top);
  g[j] = -(*eps_p) * (top + log(tot));
}

// ---------------------------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------------------------
// tile (blockIdx.x: 64 columns, blockIdx.y: a row group) of T = a_i b_j exp((f_i + g_j - cost_ij) / e), written over T_old;
// rowpart [n, Tc]: the row's sum inside the tile; colpart [G, m]: the column's sum inside the group; chg [G Tc]: the
// tile's sum of |T - T_old|
__global__ void __launch_bounds__(256)
ot_plan_kernel(const double* __restrict__ cost, long long n, long long m, long long R, const double* __restrict__ f,
               const double* __restrict__ g, const double* __restrict__ a, const double* __restrict__ b,
               const double* __restrict__ eps_p, double* __restrict__ T, double* __restrict__ rowpart,
               double* __restrict__ colpart, double* __restrict__ chg) {
  __shared__ double cs[4][WAVE];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long j = (long long)blockIdx.x * OT_T + lane, grp = blockIdx.y, Tc = gridDim.x;
  const long long r0 = grp * R, r1 = min(n, r0 + R);
  const double eps = *eps_p;
  const bool in = j < m;
  const double gj = in ? g[j] : 0.0, bj = in ? b[j] : 0.0;
  double col = 0.0, d = 0.0;
  for (long long i = r0 + w; i < r1; i += 4) {  // (wave-uniform trip count: wave_sum below is whole)
    double t = 0.0;
    if (in) {
      const long long idx = i * m + j;
      t = a[i] * bj * exp(((f[i] + gj) - cost[idx]) / eps);
      d += fabs(t - T[idx]);
      T[idx] = t;
      col += t;
    }
    const double rs = wave_sum(t);
    if (lane == 0) rowpart[i * Tc + blockIdx.x] = rs;
  }
  cs[w][lane] = col;
  __syncthreads();
  if (w == 0 && in) colpart[grp * m + j] = ((cs[0][lane] + cs[1][lane]) + cs[2][lane]) + cs[3][lane];
  const double tot = block_sum(d, red);
  if (threadIdx.x == 0) chg[grp * Tc + blockIdx.x] = tot;
}

// out[k] = sum_t part[k * inner + t * stride] over t < count, in order (rows: inner = Tc, stride = 1; columns: inner = 1,
// stride = m)
__global__ void __launch_bounds__(256)
ot_fold_kernel(const double* __restrict__ part, long long len, long long inner, long long stride, long long count,
               double* __restrict__ out) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= len) return;
  double s = 0.0;
  for (long long t = 0; t < count; ++t) s += part[k * inner + t * stride];
  out[k] = s;
}

// one workgroup: out[0] = |rowsum - a|_1, out[1] = |colsum - b|_1, out[2] = sum chg, each in one fixed order
__global__ void __launch_bounds__(256)
ot_plan_close_kernel(const double* __restrict__ rowsum, const double* __restrict__ a, long long n,
                     const double* __restrict__ colsum, const double* __restrict__ b, long long m,
                     const double* __restrict__ chg, long long nchg, double* __restrict__ out) {
  __shared__ double red[3][256];
  const int tid = threadIdx.x;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long k = tid; k < n; k += 256) s0 += fabs(rowsum[k] - a[k]);
  for (long long k = tid; k < m; k += 256) s1 += fabs(colsum[k] - b[k]);
  for (long long k = tid; k < nchg; k += 256) s2 += chg[k];
  fold3_256(s0, s1, s2, red);
  if (tid < 3) out[tid] = red[tid][0];
}

static inline bool ot_size_ok(long long n, long long m) {
  return n <= 0x7fffffffLL && m <= 0x7fffffffLL;  // every grid extent and every n m index in 63 bits
}

}  // namespace gpsa

extern "C" {

int gpsa_ot_dist_f64(const double* X, long long n, int D, double* Cm, void* stream) {
  using namespace gpsa;
  if (!X || !Cm || n < 1 || D < 1) return GPSA_EINVAL;
  if (D > MAXD || cdiv(n, (long long)OT_T) > 65535) return GPSA_EUNSUPPORTED;
  const unsigned t = (unsigned)cdiv(n, (long long)OT_T);
  ot_dist_kernel<<<dim3(t, t), 256, 0, as_stream(stream)>>>(X, n, D, Cm);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_ot_sqmatvec_f64(const double* Cm, long long n, long long ncol, const double* v, double* out, void* stream) {
  using namespace gpsa;
  if (!Cm || !v || !out || n < 1 || ncol < 1) return GPSA_EINVAL;
  if (!ot_size_ok(n, ncol)) return GPSA_EUNSUPPORTED;
  ot_sqmatvec_kernel<<<(unsigned)cdiv(n, 4LL), 256, 0, as_stream(stream)>>>(Cm, n, ncol, v, out);
  GPSA_LAUNCH_CHECK();
  return 0;
}

long long gpsa_ot_expr_rows_workspace(long long n) { return n < 1 ? 0 : 8 * n; }

int gpsa_ot_expr_rows_f32(int mode, const float* Y, long long n, long long P, double* Pm, double* Lg, double* term,
                          long long* n_invalid, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!Y || !Pm || !term || !n_invalid || n < 1 || P < 1) return GPSA_EINVAL;
  if (mode != OT_KL && mode != OT_EUCLIDEAN) return GPSA_EINVAL;
  if (mode == OT_KL && !Lg) return GPSA_EINVAL;
  if (!ot_size_ok(n, P)) return GPSA_EUNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < gpsa_ot_expr_rows_workspace(n)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  double* bad = (double*)workspace;
  const unsigned blocks = (unsigned)cdiv(n, 4LL);
  if (mode == OT_KL) ot_expr_rows_kernel<OT_KL><<<blocks, 256, 0, st>>>(Y, n, P, Pm, Lg, term, bad);
  else ot_expr_rows_kernel<OT_EUCLIDEAN><<<blocks, 256, 0, st>>>(Y, n, P, Pm, Lg, term, bad);
  GPSA_LAUNCH_CHECK();
  ot_count_kernel<<<1, 256, 0, st>>>(bad, n, n_invalid);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_ot_expr_cost_f64(int mode, double* G, long long n, long long m, const double* ra, const double* rb,
                          void* stream) {
  using namespace gpsa;
  if (!G || !ra || n < 1 || m < 1) return GPSA_EINVAL;
  if (mode != OT_KL && mode != OT_EUCLIDEAN) return GPSA_EINVAL;
  if (mode == OT_EUCLIDEAN && !rb) return GPSA_EINVAL;
  if (!ot_size_ok(n, m)) return GPSA_EUNSUPPORTED;
  const dim3 grid((unsigned)cdiv(m, 256LL), (unsigned)(n < 4096 ? n : 4096));
  hipStream_t st = as_stream(stream);
  if (mode == OT_KL) ot_expr_cost_kernel<OT_KL><<<grid, 256, 0, st>>>(G, n, m, ra, rb);
  else ot_expr_cost_kernel<OT_EUCLIDEAN><<<grid, 256, 0, st>>>(G, n, m, ra, rb);
  GPSA_LAUNCH_CHECK();
  return 0;
}

long long gpsa_ot_cost_workspace(long long n, long long m) {
  if (n < 1 || m < 1) return 0;
  return 8 * 3 * gpsa::ot_cost_blocks(n);
}

int gpsa_ot_cost_f64(double* G, const double* M, const double* T, const double* cA, const double* cB, const double* cAt,
                     const double* cBt, double alpha, long long n, long long m, double* sums, void* workspace,
                     long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!G || !M || !T || !cA || !cB || !cAt || !cBt || !sums || n < 1 || m < 1) return GPSA_EINVAL;
  if (!(alpha >= 0.0 && alpha <= 1.0)) return GPSA_EINVAL;
  if (!ot_size_ok(n, m)) return GPSA_EUNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < gpsa_ot_cost_workspace(n, m)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const long long nblk = ot_cost_blocks(n);
  double* part = (double*)workspace;
  ot_cost_kernel<<<(unsigned)nblk, 256, 0, st>>>(G, M, T, cA, cB, cAt, cBt, alpha, n, m, part);
  GPSA_LAUNCH_CHECK();
  ot_close3_kernel<<<1, 256, 0, st>>>(part, nblk, sums);
  GPSA_LAUNCH_CHECK();
  return 0;
}

long long gpsa_ot_sinkhorn_workspace(long long n, long long m) {
  if (n < 1 || m < 1) return 0;
  return 8 * 2 * gpsa::ot_groups(n) * m;
}

int gpsa_ot_sinkhorn_f64(const double* cost, long long n, long long m, const double* loga, const double* logb,
                         const double* eps, double* f, double* g, int iters, void* workspace,
                         long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!cost || !loga || !logb || !eps || !f || !g || n < 1 || m < 1 || iters < 0) return GPSA_EINVAL;
  if (!ot_size_ok(n, m)) return GPSA_EUNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < gpsa_ot_sinkhorn_workspace(n, m)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const long long R = ot_rows_per_group(n), G = ot_groups(n);
  double *pm = (double*)workspace, *ps = pm + G * m;
  const dim3 cgrid((unsigned)ot_col_tiles(m), (unsigned)G);
  for (int it = 0; it < iters; ++it) {
    ot_sink_row_kernel<<<(unsigned)cdiv(n, 4LL), 256, 0, st>>>(cost, n, m, g, logb, eps, f);
    GPSA_LAUNCH_CHECK();
    ot_sink_col_kernel<<<cgrid, 256, 0, st>>>(cost, n, m, R, f, loga, eps, pm, ps);
    GPSA_LAUNCH_CHECK();
    ot_sink_merge_kernel<<<(unsigned)cdiv(m, 256LL), 256, 0, st>>>(pm, ps, G, m, eps, g);
    GPSA_LAUNCH_CHECK();
  }
  return 0;
}

long long gpsa_ot_plan_workspace(long long n, long long m) {
  if (n < 1 || m < 1) return 0;
  const long long G = gpsa::ot_groups(n), Tc = gpsa::ot_col_tiles(m);
  return 8 * (n * Tc + G * m + G * Tc);
}

int gpsa_ot_plan_f64(const double* cost, long long n, long long m, const double* f, const double* g, const double* a,
                     const double* b, const double* eps, double* T, double* rowsum, double* colsum, double* sums,
                     void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!cost || !f || !g || !a || !b || !eps || !T || !rowsum || !colsum || !sums || n < 1 || m < 1) return GPSA_EINVAL;
  if (!ot_size_ok(n, m)) return GPSA_EUNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < gpsa_ot_plan_workspace(n, m)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const long long R = ot_rows_per_group(n), G = ot_groups(n), Tc = ot_col_tiles(m);
  double *rowpart = (double*)workspace, *colpart = rowpart + n * Tc, *chg = colpart + G * m;
  ot_plan_kernel<<<dim3((unsigned)Tc, (unsigned)G), 256, 0, st>>>(cost, n, m, R, f, g, a, b, eps, T, rowpart, colpart, chg);
  GPSA_LAUNCH_CHECK();
  ot_fold_kernel<<<(unsigned)cdiv(n, 256LL), 256, 0, st>>>(rowpart, n, Tc, 1, Tc, rowsum);
  GPSA_LAUNCH_CHECK();
  ot_fold_kernel<<<(unsigned)cdiv(m, 256LL), 256, 0, st>>>(colpart, m, 1, m, G, colsum);
  GPSA_LAUNCH_CHECK();
  ot_plan_close_kernel<<<1, 256, 0, st>>>(rowsum, a, n, colsum, b, m, chg, G * Tc, sums);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
