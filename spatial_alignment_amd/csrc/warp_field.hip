// The learned warp as a function of the point: its mean, its Jacobian, the Jacobian's determinant, and its inverse.
// For a non-fixed view the warp GP's conditional mean (vgpsa.py:174-204, mean only) is closed form in x:
//   g(x)    = x A + b + k(x, Z) beta,          beta = K_uu^-1 (delta_G - (Z A + b))   [M, D], formed by the caller
//   J[j, d] = d g_j / d x_d = A[d, j] + sum_m beta[m, j] cd(x, z_m) (x[d] - z_m[d])
// with cd the derivative coefficient of cov_eval (kmat_cov.hpp: dk/dz_d = cd (z_d - x_d), so dk/dx_d = cd (x_d - z_d)).
// Everything is fp64; k(X, Z) never exists in memory.
//
// Both entries evaluate g and J through ONE device function, warp_eval, templated on the covariance kind, on D and on
// whether J is wanted - the forward and the inverse cannot disagree.
//
// A workgroup (256 threads) covers WF_TR = 32 rows x WF_SL = 8 slices of the inducing points: thread (row, slice) sums
// the points m = slice, slice + 8, ... of every slab of WF_SLAB points (Z and beta staged in LDS slab by slab: at
// M = 1000, D = 4 they are 64 KB and do not fit whole), the slices' partial sums meet through LDS and are added in the
// order slice 0, 1, ..., 7.  One thread per row would put 79 waves on the chip at n = 20 000.  No atomics; a row's
// result depends on its x, on M and on nothing else - not on n, not on the launch it is part of, not on its neighbours.
//
// gpsa_warp_invert_f64 runs exactly `iters` undamped Newton updates x <- x - J(x)^-1 (g(x) - target) in one launch (the
// trip count is the caller's, there is no early exit and no loop on data), then evaluates g once more AT THE RETURNED x
// for the residual |g(x) - target|_2.  The D x D solve is unrolled elimination with partial pivoting in registers (row
// swaps as selects: no run-time register index).  A zero or non-finite pivot or a non-finite iterate marks the row
// failed for good: X = NaN, residual = +inf.
#include <math.h>

#include "common.hpp"
#include "kmat_cov.hpp"

namespace gpsa {

constexpr int WF_TR = 32;     // rows per workgroup
constexpr int WF_SL = 8;      // slices of the inducing points per row
constexpr int WF_SLAB = 256;  // inducing points staged in LDS at a time

static_assert(WF_TR * WF_SL == 256, "a workgroup is rows x slices");

// LDS of a workgroup.  The slab and the slices' partial sums are never alive together, but they are kept apart: the
// largest instantiation (D = 4 with J) is 16 + 40 + 5 + 1 = 62 KB, D = 2 is 8 + 12 + 1.5 + 0.5 = 22 KB.
template <int D, int NV>
struct WarpLds {
  double z[WF_SLAB * D];
  double beta[WF_SLAB * D];
  double part[WF_SL][NV][WF_TR];  // [slice][value][row]: a wave's lanes read and write consecutive doubles
  double tot[NV][WF_TR];
  double x[D][WF_TR];  // the invert kernel's iterate, handed from a row's owner to its slices
};

// The hyper-parameters and the affine part, uniform over the launch
template <int D>
struct WarpModel {
  const double* Z;
  const double* beta;
  const double* A;  // [D, D]: g gets x A
  const double* b;  // [D]
  double ell, inv_ell, var;
  int M;
};

// g(x) and, with WANT_J, J(x) of row `row` of the tile, x in registers of all WF_SL threads of the row.  Cooperative:
// every thread of the workgroup calls it (it stages slabs and passes barriers).  The sums are returned to the row's OWNER
// (slice 0) only: G[j] = g_j, Jm[j][d] = d g_j / d x_d; the other threads' outputs are not meaningful.
template <int KIND, int D, bool WANT_J, int NV>
__device__ __forceinline__ void warp_eval(const WarpModel<D>& mdl, WarpLds<D, NV>& lds, int row, int slice,
                                          const double (&x)[D], double (&G)[D], double (&Jm)[D][D]) {
  static_assert(NV >= D + (WANT_J ? D * D : 0), "room for the values reduced");
  constexpr int NR = D + (WANT_J ? D * D : 0);  // values reduced over the slices
  const int tid = threadIdx.x;
  double accG[D], accJ[D][D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    accG[j] = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) accJ[j][d] = 0.0;
  }
  double xx[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) xx[d] = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) xx[d] = x[d];

  for (int m0 = 0; m0 < mdl.M; m0 += WF_SLAB) {
    const int cnt = min(WF_SLAB, mdl.M - m0);
    __syncthreads();  // the previous slab (or the previous call's sums) has been consumed
    for (int i = tid; i < cnt * D; i += 256) {
      lds.z[i] = mdl.Z[(long long)m0 * D + i];
      lds.beta[i] = mdl.beta[(long long)m0 * D + i];
    }
    __syncthreads();
    for (int mm = slice; mm < cnt; mm += WF_SL) {
      double zz[MAXD];
#pragma unroll
      for (int d = 0; d < MAXD; ++d) zz[d] = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) zz[d] = lds.z[mm * D + d];
      double k, cd, pl;
      cov_eval<double, KIND>(zz, xx, D, mdl.ell, mdl.inv_ell, mdl.var, k, cd, pl);
      double bt[D];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        bt[j] = lds.beta[mm * D + j];
        accG[j] = fma(bt[j], k, accG[j]);
      }
      if (WANT_J) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const double w = cd * (xx[d] - zz[d]);  // dk / dx_d
#pragma unroll
          for (int j = 0; j < D; ++j) accJ[j][d] = fma(bt[j], w, accJ[j][d]);
        }
      }
    }
  }
  // the slices' partial sums -> LDS; thread (row, slice) then adds values slice, slice + 8, ... over the slices in the
  // order 0..7, and the row's owner collects the NR totals
#pragma unroll
  for (int j = 0; j < D; ++j) lds.part[slice][j][row] = accG[j];
  if (WANT_J) {
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
      for (int d = 0; d < D; ++d) lds.part[slice][D + j * D + d][row] = accJ[j][d];
  }
  __syncthreads();
  for (int v = slice; v < NR; v += WF_SL) {
    double t = lds.part[0][v][row];
#pragma unroll
    for (int s = 1; s < WF_SL; ++s) t += lds.part[s][v][row];
    lds.tot[v][row] = t;
  }
  __syncthreads();
  if (slice == 0) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double gj = mdl.b[j];
#pragma unroll
      for (int d = 0; d < D; ++d) gj = fma(x[d], mdl.A[d * D + j], gj);
      G[j] = gj + lds.tot[j][row];
    }
    if (WANT_J) {
#pragma unroll
      for (int j = 0; j < D; ++j)
#pragma unroll
        for (int d = 0; d < D; ++d) Jm[j][d] = mdl.A[d * D + j] + lds.tot[D + j * D + d][row];
    }
  }
}

template <int D>
__device__ __forceinline__ double det_small(const double (&a)[D][D]) {
  if constexpr (D == 1) {
    return a[0][0];
  } else if constexpr (D == 2) {
    return fma(a[0][0], a[1][1], -(a[0][1] * a[1][0]));
  } else if constexpr (D == 3) {
    const double c0 = fma(a[1][1], a[2][2], -(a[1][2] * a[2][1]));
    const double c1 = fma(a[1][0], a[2][2], -(a[1][2] * a[2][0]));
    const double c2 = fma(a[1][0], a[2][1], -(a[1][1] * a[2][0]));
    return fma(a[0][0], c0, fma(-a[0][1], c1, a[0][2] * c2));
  } else {
    // 2 x 2 minors of rows 0, 1 against the complementary minors of rows 2, 3
    const double s0 = fma(a[0][0], a[1][1], -(a[1][0] * a[0][1]));
    const double s1 = fma(a[0][0], a[1][2], -(a[1][0] * a[0][2]));
    const double s2 = fma(a[0][0], a[1][3], -(a[1][0] * a[0][3]));
    const double s3 = fma(a[0][1], a[1][2], -(a[1][1] * a[0][2]));
    const double s4 = fma(a[0][1], a[1][3], -(a[1][1] * a[0][3]));
    const double s5 = fma(a[0][2], a[1][3], -(a[1][2] * a[0][3]));
    const double c5 = fma(a[2][2], a[3][3], -(a[3][2] * a[2][3]));
    const double c4 = fma(a[2][1], a[3][3], -(a[3][1] * a[2][3]));
    const double c3 = fma(a[2][1], a[3][2], -(a[3][1] * a[2][2]));
    const double c2 = fma(a[2][0], a[3][3], -(a[3][0] * a[2][3]));
    const double c1 = fma(a[2][0], a[3][2], -(a[3][0] * a[2][2]));
    const double c0 = fma(a[2][0], a[3][1], -(a[3][0] * a[2][1]));
    return fma(s0, c5, fma(-s1, c4, fma(s2, c3, fma(s3, c2, fma(-s4, c1, s5 * c0)))));
  }
}

__device__ __forceinline__ bool wf_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

// a dx = r by elimination with partial pivoting, fully unrolled (a and r are destroyed).  false: a pivot was zero or
// not finite (dx is then not meaningful)
template <int D>
__device__ __forceinline__ bool solve_small(double (&a)[D][D], double (&r)[D], double (&dx)[D]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    int p = c;
    double best = fabs(a[c][c]);
#pragma unroll
    for (int i = c + 1; i < D; ++i) {
      const double v = fabs(a[i][c]);
      const bool up = v > best;  // (a NaN never wins; it is caught as the pivot or spreads into the later ones)
      best = up ? v : best;
      p = up ? i : p;
    }
#pragma unroll
    for (int i = c + 1; i < D; ++i) {
      const bool sw = p == i;
#pragma unroll
      for (int k = c; k < D; ++k) {
        const double top = a[c][k], low = a[i][k];
        a[c][k] = sw ? low : top;
        a[i][k] = sw ? top : low;
      }
      const double top = r[c], low = r[i];
      r[c] = sw ? low : top;
      r[i] = sw ? top : low;
    }
    const double piv = a[c][c];
    ok = ok && piv != 0.0 && wf_finite(piv);
    const double inv = 1.0 / piv;
#pragma unroll
    for (int i = c + 1; i < D; ++i) {
      const double f = a[i][c] * inv;
#pragma unroll
      for (int k = c + 1; k < D; ++k) a[i][k] = fma(-f, a[c][k], a[i][k]);
      r[i] = fma(-f, r[c], r[i]);
    }
  }
#pragma unroll
  for (int c = D - 1; c >= 0; --c) {
    double s = r[c];
#pragma unroll
    for (int k = c + 1; k < D; ++k) s = fma(-a[c][k], dx[k], s);
    dx[c] = s / a[c][c];
  }
  return ok;
}

template <int D>
__device__ __forceinline__ WarpModel<D> warp_model(const double* Z, const double* beta, const double* A,
                                                   const double* b, const double* ls_u, const double* var_u, int M) {
  WarpModel<D> m;
  m.Z = Z;
  m.beta = beta;
  m.A = A;
  m.b = b;
  m.ell = exp(ls_u[0]);
  m.inv_ell = 1.0 / m.ell;
  m.var = exp(var_u[0]);
  m.M = M;
  return m;
}

template <int KIND, int D, bool WANT_J>
__global__ void __launch_bounds__(256)
warp_field_kernel(const double* __restrict__ Z, const double* __restrict__ beta, const double* __restrict__ A,
                  const double* __restrict__ b, const double* __restrict__ ls_u, const double* __restrict__ var_u,
                  const double* __restrict__ X, long long n, int M, double* __restrict__ G, double* __restrict__ J,
                  double* __restrict__ det) {
  constexpr int NV = D + (WANT_J ? D * D : 0);
  __shared__ WarpLds<D, NV> lds;
  const int row = threadIdx.x & (WF_TR - 1), slice = threadIdx.x / WF_TR;
  const long long r = (long long)blockIdx.x * WF_TR + row;
  const bool live = r < n;
  const WarpModel<D> mdl = warp_model<D>(Z, beta, A, b, ls_u, var_u, M);
  double x[D];
#pragma unroll
  for (int d = 0; d < D; ++d) x[d] = live ? X[r * D + d] : 0.0;  // rows past the edge run on the origin, store nothing
  double g[D], Jm[D][D];
  warp_eval<KIND, D, WANT_J, NV>(mdl, lds, row, slice, x, g, Jm);
  if (slice == 0 && live) {
#pragma unroll
    for (int j = 0; j < D; ++j) G[r * D + j] = g[j];
    if (WANT_J) {
      if (J != nullptr) {
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
          for (int d = 0; d < D; ++d) J[(r * D + j) * D + d] = Jm[j][d];
      }
      if (det != nullptr) det[r] = det_small<D>(Jm);
    }
  }
}

template <int KIND, int D>
__global__ void __launch_bounds__(256)
warp_invert_kernel(const double* __restrict__ Z, const double* __restrict__ beta, const double* __restrict__ A,
                   const double* __restrict__ b, const double* __restrict__ ls_u, const double* __restrict__ var_u,
                   const double* __restrict__ target, const double* __restrict__ x0, int iters, long long n, int M,
                   double* __restrict__ X, double* __restrict__ residual) {
  constexpr int NV = D + D * D;
  __shared__ WarpLds<D, NV> lds;
  const int row = threadIdx.x & (WF_TR - 1), slice = threadIdx.x / WF_TR;
  const long long r = (long long)blockIdx.x * WF_TR + row;
  const bool live = r < n;
  const WarpModel<D> mdl = warp_model<D>(Z, beta, A, b, ls_u, var_u, M);
  double x[D], t[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = live ? x0[r * D + d] : 0.0;
    t[d] = live ? target[r * D + d] : 0.0;
  }
  bool ok = true;  // the owner's: sticky once false
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    double g[D], Jm[D][D];
    warp_eval<KIND, D, true, NV>(mdl, lds, row, slice, x, g, Jm);
    if (slice == 0) {
      double res[D], dx[D];
#pragma unroll
      for (int d = 0; d < D; ++d) res[d] = g[d] - t[d];
      ok = solve_small<D>(Jm, res, dx) && ok;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double xn = x[d] - dx[d];
        ok = ok && wf_finite(xn);
        lds.x[d][row] = xn;
      }
      if (!ok) {  // a failed row goes on as NaN: every later value of it is NaN too
#pragma unroll
        for (int d = 0; d < D; ++d) lds.x[d][row] = NAN;
      }
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = lds.x[d][row];
    // (the next evaluation's first barrier separates these reads from the next iteration's writes)
  }
  double g[D], Jm[D][D];
  warp_eval<KIND, D, false, NV>(mdl, lds, row, slice, x, g, Jm);
  if (slice == 0 && live) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double e = g[d] - t[d];
      s = fma(e, e, s);
      ok = ok && wf_finite(x[d]);
    }
    const double rn = sqrt(s);
    ok = ok && wf_finite(rn);
#pragma unroll
    for (int d = 0; d < D; ++d) X[r * D + d] = ok ? x[d] : (double)NAN;
    residual[r] = ok ? rn : (double)INFINITY;
  }
}

template <int KIND, int D>
static int launch_warp_field(dim3 grid, hipStream_t st, const double* Z, const double* beta, const double* A,
                             const double* b, const double* ls_u, const double* var_u, const double* X, long long n,
                             int M, double* G, double* J, double* det) {
  if (J != nullptr || det != nullptr)
    warp_field_kernel<KIND, D, true><<<grid, 256, 0, st>>>(Z, beta, A, b, ls_u, var_u, X, n, M, G, J, det);
  else
    warp_field_kernel<KIND, D, false><<<grid, 256, 0, st>>>(Z, beta, A, b, ls_u, var_u, X, n, M, G, nullptr, nullptr);
  GPSA_LAUNCH_CHECK();
  return 0;
}

template <int KIND>
static int launch_warp_field_d(int D, dim3 grid, hipStream_t st, const double* Z, const double* beta, const double* A,
                               const double* b, const double* ls_u, const double* var_u, const double* X, long long n,
                               int M, double* G, double* J, double* det) {
  switch (D) {
    case 1: return launch_warp_field<KIND, 1>(grid, st, Z, beta, A, b, ls_u, var_u, X, n, M, G, J, det);
    case 2: return launch_warp_field<KIND, 2>(grid, st, Z, beta, A, b, ls_u, var_u, X, n, M, G, J, det);
    case 3: return launch_warp_field<KIND, 3>(grid, st, Z, beta, A, b, ls_u, var_u, X, n, M, G, J, det);
    case 4: return launch_warp_field<KIND, 4>(grid, st, Z, beta, A, b, ls_u, var_u, X, n, M, G, J, det);
    default: return GPSA_EUNSUPPORTED;
  }
}

template <int KIND>
static int launch_warp_invert_d(int D, dim3 grid, hipStream_t st, const double* Z, const double* beta, const double* A,
                                const double* b, const double* ls_u, const double* var_u, const double* target,
                                const double* x0, int iters, long long n, int M, double* X, double* residual) {
#define GPSA_WI_CASE(DD)                                                                                             \
  case DD:                                                                                                           \
    warp_invert_kernel<KIND, DD><<<grid, 256, 0, st>>>(Z, beta, A, b, ls_u, var_u, target, x0, iters, n, M, X, residual); \
    break;
  switch (D) {
    GPSA_WI_CASE(1)
    GPSA_WI_CASE(2)
    GPSA_WI_CASE(3)
    GPSA_WI_CASE(4)
    default: return GPSA_EUNSUPPORTED;
  }
#undef GPSA_WI_CASE
  GPSA_LAUNCH_CHECK();
  return 0;
}

// the checks both entries share, made before any launch: 0, GPSA_EINVAL or GPSA_EUNSUPPORTED
static int warp_args_check(int kind, const void* Z, const void* beta, const void* A, const void* b, const void* ls_u,
                           const void* var_u, long long n, int M, int D) {
  if (Z == nullptr || beta == nullptr || A == nullptr || b == nullptr || ls_u == nullptr || var_u == nullptr)
    return GPSA_EINVAL;
  if (n < 1 || M < 1 || D < 1) return GPSA_EINVAL;
  if (kind != GPSA_K_RBF && kind != GPSA_K_MATERN12 && kind != GPSA_K_MATERN32) return GPSA_EINVAL;
  if (D > MAXD) return GPSA_EUNSUPPORTED;
  if (cdiv(n, WF_TR) > 0x7fffffffLL) return GPSA_EINVAL;
  return 0;
}

}  // namespace gpsa

extern "C" {

int gpsa_warp_field_f64(int kind, const double* Z, const double* beta, const double* A, const double* b,
                        const double* ls_u, const double* var_u, const double* X, long long n, int M, int D, double* G,
                        double* J, double* det, void* stream) {
  const int bad = gpsa::warp_args_check(kind, Z, beta, A, b, ls_u, var_u, n, M, D);
  if (bad) return bad;
  if (X == nullptr || G == nullptr) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)cdiv(n, gpsa::WF_TR));
  switch (kind) {
    case GPSA_K_RBF:
      return gpsa::launch_warp_field_d<GPSA_K_RBF>(D, grid, st, Z, beta, A, b, ls_u, var_u, X, n, M, G, J, det);
    case GPSA_K_MATERN12:
      return gpsa::launch_warp_field_d<GPSA_K_MATERN12>(D, grid, st, Z, beta, A, b, ls_u, var_u, X, n, M, G, J, det);
    default:
      return gpsa::launch_warp_field_d<GPSA_K_MATERN32>(D, grid, st, Z, beta, A, b, ls_u, var_u, X, n, M, G, J, det);
  }
}

int gpsa_warp_invert_f64(int kind, const double* Z, const double* beta, const double* A, const double* b,
                         const double* ls_u, const double* var_u, const double* target, const double* x0, int iters,
                         long long n, int M, int D, double* X, double* residual, void* stream) {
  const int bad = gpsa::warp_args_check(kind, Z, beta, A, b, ls_u, var_u, n, M, D);
  if (bad) return bad;
  if (target == nullptr || x0 == nullptr || X == nullptr || residual == nullptr || iters < 0) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)cdiv(n, gpsa::WF_TR));
  switch (kind) {
    case GPSA_K_RBF:
      return gpsa::launch_warp_invert_d<GPSA_K_RBF>(D, grid, st, Z, beta, A, b, ls_u, var_u, target, x0, iters, n, M, X,
                                                    residual);
    case GPSA_K_MATERN12:
      return gpsa::launch_warp_invert_d<GPSA_K_MATERN12>(D, grid, st, Z, beta, A, b, ls_u, var_u, target, x0, iters, n,
                                                         M, X, residual);
    default:
      return gpsa::launch_warp_invert_d<GPSA_K_MATERN32>(D, grid, st, Z, beta, A, b, ls_u, var_u, target, x0, iters, n,
                                                         M, X, residual);
  }
}

}  // extern "C"
