// Exact GP regression on the device (gpr.py): the three kernels that sklearn's GaussianProcessRegressor with
// ``[C *] k + WhiteKernel`` needs next to the factorisation and the dense products that exist already
// (gpsa_chol_inv_blocked_f64, gpsa_gemm).  All fp64.
//
//   K(theta) = a k(X, X; l) + (tau2 + jitter) I,   theta = (log a, log l, log tau2) on the DEVICE (the optimiser never
//   syncs to pass parameters); a = 1 unless `amplitude`.  sklearn's kernel forms, isotropic l:
//     rbf       exp(-d^2 / (2 l^2))                     d k / d log l = k d^2 / l^2
//     matern32  (1 + r) exp(-r),  r = sqrt(3) d / l                     r^2 exp(-r)
//     matern12  exp(-r),          r = d / l                             r exp(-r)
//   d^2 in difference form, summed over the coordinates in order (at d = 0 every form is 1 with derivative 0: no 0 / 0).
//
// gpr_cov_kernel     a 64 x 64 tile of K per workgroup.  With `same` only the tiles (I, J <= I) run; an off-diagonal
//                    tile goes through LDS to its mirror position, so K is symmetric to the bit and each pair is
//                    evaluated once.
// gpr_grad_kernel    the marginal likelihood's gradient 1/2 sum_ij W_ij dK_ij with W = alpha alpha^T - P K^-1, one
//                    workgroup per tile (I, J <= I): alpha_I alpha_J^T on v_mfma_f64_16x16x4_f64 (each wave a 32 x 32
//                    quadrant, P zero-padded to a multiple of 4 in registers), minus P Kinv_IJ, times k and dk / dlog l
//                    evaluated from X_I, X_J on the fly; off-diagonal tiles count twice.  Neither alpha alpha^T nor a dK
//                    matrix exists in memory.  Three partials per workgroup, added in a fixed order by
//                    gpr_grad_close_kernel: no atomics, a repeated call gives the same bits.
// gpr_mean_kernel    a k(X*, X) alpha: a workgroup owns 16 test rows; alpha is staged in LDS 64 training rows x 64 outputs at
//                    a time and wave w takes rows 16 w .. 16 w + 15 of every such chunk: each lane evaluates k(x*_row, x_t)
//                    for ITS (row, t) of the 16 x 4 A operand and the MFMA contracts it with alpha's rows t.  No [ns, N]
//                    matrix exists.  A wave's sum runs over the chunks in order, the four waves' sums are added as
//                    (w0 + w1) + (w2 + w3): one order for every row, whatever rows the caller passes together.
#include <math.h>

#include "toolbox.hpp"

namespace gpsa {

constexpr int GPR_T = 64;       // tile edge of all three kernels
constexpr int GPR_ALD = 68;     // pitch of the mean kernel's alpha chunk in LDS
typedef double gpr_acc_t __attribute__((ext_vector_type(4)));

// k and dk / dlog l (both without the amplitude) at squared distance d2
template <int KIND>
__device__ __forceinline__ void gpr_k(double d2, double inv_l, double& k, double& dk) {
  if (KIND == GPSA_K_RBF) {
    const double s = d2 * inv_l * inv_l;
    k = exp(-0.5 * s);
    dk = k * s;
  } else if (KIND == GPSA_K_MATERN32) {
    const double r = sqrt(3.0 * d2) * inv_l, e = exp(-r);
    k = (1.0 + r) * e;
    dk = r * r * e;
  } else {
    const double r = sqrt(d2) * inv_l;
    k = exp(-r);
    dk = r * k;
  }
}

__device__ __forceinline__ double gpr_d2(const double* __restrict__ u, const double* __restrict__ v) {
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < MAXD; ++d) {
    const double t = u[d] - v[d];
    s += t * t;
  }
  return s;
}

template <int KIND>
__global__ void __launch_bounds__(256)
gpr_cov_kernel(const double* __restrict__ XA, long long na, const double* __restrict__ XB, long long nb, int D,
               const double* __restrict__ theta, int amplitude, int same, double jitter, double* __restrict__ K) {
  __shared__ double xa[GPR_T][MAXD], xb[GPR_T][MAXD];
  __shared__ double tile[GPR_T][GPR_T + 1];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (same && bj > bi) return;  // block-uniform: the mirror of (bj, bi) writes this tile
  const long long i0 = (long long)bi * GPR_T, j0 = (long long)bj * GPR_T;
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  stage_rows64(XA, na, D, i0, tid, xa);
  stage_rows64(XB, nb, D, j0, tid - GPR_T, xb);
  __syncthreads();
  const double a = amplitude ? exp(theta[0]) : 1.0, inv_l = exp(-theta[1]), tau2 = exp(theta[2]);
  const long long j = j0 + tx;
  for (int r = ty; r < GPR_T; r += 4) {
    const long long i = i0 + r;
    double k, dk;
    gpr_k<KIND>(gpr_d2(xa[r], xb[tx]), inv_l, k, dk);
    double v = a * k;
    if (same && i == j) v = (v + tau2) + jitter;
    if (i < na && j < nb) K[i * nb + j] = v;
    tile[r][tx] = v;
  }
  if (same && bi != bj) {
    __syncthreads();
    const long long ii = i0 + tx;
    for (int r = ty; r < GPR_T; r += 4) {
      const long long jj = j0 + r;
      if (jj < nb && ii < na) K[jj * nb + ii] = tile[tx][r];  // na == nb
    }
  }
}

template <int KIND>
__global__ void __launch_bounds__(256)
gpr_grad_kernel(const double* __restrict__ X, long long N, int D, const double* __restrict__ theta,
                const double* __restrict__ alpha, int P, const double* __restrict__ Kinv, double* __restrict__ part) {
  __shared__ double xi[GPR_T][MAXD], xj[GPR_T][MAXD];
  __shared__ double red[4][3];
  // workgroup b -> tile (bi, bj <= bi) of the lower triangle, row by row
  const long long b = blockIdx.x;
  long long bi = (long long)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= b) ++bi;
  while (bi * (bi + 1) / 2 > b) --bi;
  const long long bj = b - bi * (bi + 1) / 2;
  const long long i0 = bi * GPR_T, j0 = bj * GPR_T;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 32, j = lane & 15, kq = lane >> 4;
  stage_rows64(X, N, D, i0, tid, xi);
  stage_rows64(X, N, D, j0, tid - GPR_T, xj);
  __syncthreads();

  // alpha_I alpha_J^T: A operand lane (row j, k kq) = alpha[row][p0 + kq], B operand lane (k kq, col j) the same of J
  gpr_acc_t acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = (gpr_acc_t){0.0, 0.0, 0.0, 0.0};
  const long long ra0 = i0 + wm + j, ra1 = ra0 + 16, cb0 = j0 + wn + j, cb1 = cb0 + 16;
  for (int p0 = 0; p0 < P; p0 += 4) {
    const int p = p0 + kq;
    const bool ok = p < P;  // the K dimension padded with zeros in registers
    const double a0 = (ok && ra0 < N) ? alpha[ra0 * P + p] : 0.0;
    const double a1 = (ok && ra1 < N) ? alpha[ra1 * P + p] : 0.0;
    const double b0 = (ok && cb0 < N) ? alpha[cb0 * P + p] : 0.0;
    const double b1 = (ok && cb1 < N) ? alpha[cb1 * P + p] : 0.0;
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }

  // C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
  const double inv_l = exp(-theta[1]), Pd = (double)P;
  double sa = 0.0, sl = 0.0, st = 0.0;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wm + 16 * ti + kq + 4 * r, lc = wn + 16 * tj + j;
        const long long row = i0 + lr, col = j0 + lc;
        if (row < N && col < N) {
          const double W = acc[ti][tj][r] - Pd * Kinv[row * N + col];
          double k, dk;
          gpr_k<KIND>(gpr_d2(xi[lr], xj[lc]), inv_l, k, dk);
          sa += W * k;
          sl += W * dk;
          if (row == col) st += W;
        }
      }
  sa = wave_sum(sa);
  sl = wave_sum(sl);
  st = wave_sum(st);
  if (lane == 0) red[w][0] = sa, red[w][1] = sl, red[w][2] = st;
  __syncthreads();
  if (tid < 3) {
    const double s = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    part[b * 3 + tid] = (bi == bj) ? s : 2.0 * s;  // an off-diagonal tile stands for its mirror too
  }
}

// the workgroups' partials in one fixed order -> out[0..2] = dLML / d(log a, log l, log tau2)
__global__ void __launch_bounds__(256)
gpr_grad_close_kernel(const double* __restrict__ part, long long nblk, const double* __restrict__ theta, int amplitude,
                      double* __restrict__ out) {
  __shared__ double red[3][256];
  fold3_partials(part, nblk, red);
  if (threadIdx.x == 0) {
    const double a = amplitude ? exp(theta[0]) : 1.0, tau2 = exp(theta[2]);
    out[0] = 0.5 * a * red[0][0];
    out[1] = 0.5 * a * red[1][0];
    out[2] = 0.5 * tau2 * red[2][0];
  }
}

template <int KIND>
__global__ void __launch_bounds__(256)
gpr_mean_kernel(const double* __restrict__ XS, long long ns, const double* __restrict__ X, long long N, int D,
                const double* __restrict__ theta, int amplitude, const double* __restrict__ alpha, int P,
                double* __restrict__ out) {
  __shared__ double xt[GPR_T][MAXD];
  __shared__ double al[GPR_T][GPR_ALD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, kq = lane >> 4;
  const long long rbase = (long long)blockIdx.x * 16;  // the workgroup's 16 test rows
  const int c0 = blockIdx.y * GPR_T;                   // ... and 64 outputs
  double xs[MAXD];
#pragma unroll
  for (int d = 0; d < MAXD; ++d) xs[d] = (rbase + j < ns && d < D) ? XS[(rbase + j) * D + d] : 0.0;
  const double inv_l = exp(-theta[1]);
  gpr_acc_t acc[4];
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) acc[tj] = (gpr_acc_t){0.0, 0.0, 0.0, 0.0};
  for (long long n0 = 0; n0 < N; n0 += GPR_T) {
    __syncthreads();  // the previous chunk has been read
    stage_rows64(X, N, D, n0, tid, xt);
    for (int e = tid; e < GPR_T * GPR_T; e += 256) {
      const int r = e >> 6, c = e & 63;
      al[r][c] = (n0 + r < N && c0 + c < P) ? alpha[(n0 + r) * P + c0 + c] : 0.0;  // rows beyond N contribute k * 0
    }
    __syncthreads();
    // wave w takes the chunk's training rows 16 w .. 16 w + 15: the kernel is evaluated once per (test row, training row)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int t = (w * 4 + kk) * 4 + kq;
      double k, dk;
      gpr_k<KIND>(gpr_d2(xs, xt[t]), inv_l, k, dk);  // the A operand: lane (row j, k kq) of the 16 x 4 kernel tile
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
        if (c0 + 16 * tj < P) acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, al[t][16 * tj + j], acc[tj], 0, 0, 0);
    }
  }
  // the four waves' sums meet in LDS and are added in one order: (w0 + w1) + (w2 + w3)
  __syncthreads();
  double* red = &al[0][0];  // 4 waves x 16 accumulator values x 64 lanes = 4096 doubles <= 64 * GPR_ALD
#pragma unroll
  for (int tj = 0; tj < 4; ++tj)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[((w * 16) + tj * 4 + r) * 64 + lane] = acc[tj][r];
  __syncthreads();
  const double a = amplitude ? exp(theta[0]) : 1.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int o = tid + 256 * q, v = o >> 6, ln = o & 63;  // accumulator value v = 4 tj + r of lane ln
    const double s = (red[v * 64 + ln] + red[(16 + v) * 64 + ln]) + (red[(32 + v) * 64 + ln] + red[(48 + v) * 64 + ln]);
    const long long row = rbase + (ln >> 4) + 4 * (v & 3);
    const int col = c0 + 16 * (v >> 2) + (ln & 15);
    if (row < ns && col < P) out[row * P + col] = a * s;
  }
}

static inline long long gpr_tiles(long long N) {
  const long long T = cdiv(N, (long long)GPR_T);
  return T * (T + 1) / 2;
}

static inline bool gpr_kind_ok(int kind) {
  return kind == GPSA_K_RBF || kind == GPSA_K_MATERN12 || kind == GPSA_K_MATERN32;
}

}  // namespace gpsa

extern "C" {

int gpsa_gpr_cov_f64(int kind, const double* XA, long long na, const double* XB, long long nb, int D, const double* theta,
                     int amplitude, int same, double jitter, double* K, void* stream) {
  using namespace gpsa;
  if (!XA || !XB || !theta || !K || na < 1 || nb < 1 || D < 1 || !gpr_kind_ok(kind) || !(jitter >= 0.0))
    return GPSA_EINVAL;
  if (same && (na != nb || XA != XB)) return GPSA_EINVAL;
  if (D > MAXD || cdiv(na, (long long)GPR_T) > 65535 || cdiv(nb, (long long)GPR_T) > 0x7fffffffLL) return GPSA_EUNSUPPORTED;
  const dim3 grid((unsigned)cdiv(nb, (long long)GPR_T), (unsigned)cdiv(na, (long long)GPR_T));
  hipStream_t st = as_stream(stream);
#define GPSA_GPR_COV(KD) \
  gpr_cov_kernel<KD><<<grid, 256, 0, st>>>(XA, na, XB, nb, D, theta, amplitude ? 1 : 0, same ? 1 : 0, jitter, K)
  if (kind == GPSA_K_RBF) GPSA_GPR_COV(GPSA_K_RBF);
  else if (kind == GPSA_K_MATERN32) GPSA_GPR_COV(GPSA_K_MATERN32);
  else GPSA_GPR_COV(GPSA_K_MATERN12);
#undef GPSA_GPR_COV
  GPSA_LAUNCH_CHECK();
  return 0;
}

long long gpsa_gpr_lml_grad_workspace(long long N, int P) {
  if (N < 1 || P < 1) return 0;
  return 8 * 3 * gpsa::gpr_tiles(N);
}

int gpsa_gpr_lml_grad_f64(int kind, const double* X, long long N, int D, const double* theta, int amplitude,
                          const double* alpha, int P, const double* Kinv, double* out, void* workspace,
                          long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!X || !theta || !alpha || !Kinv || !out || N < 1 || D < 1 || P < 1 || !gpr_kind_ok(kind)) return GPSA_EINVAL;
  if (D > MAXD || N > 65535LL * GPR_T || gpr_tiles(N) > 0x7fffffffLL) return GPSA_EUNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < gpsa_gpr_lml_grad_workspace(N, P)) return GPSA_EWORKSPACE;
  const long long nblk = gpr_tiles(N);
  double* part = (double*)workspace;
  hipStream_t st = as_stream(stream);
#define GPSA_GPR_GRAD(KD) gpr_grad_kernel<KD><<<(unsigned)nblk, 256, 0, st>>>(X, N, D, theta, alpha, P, Kinv, part)
  if (kind == GPSA_K_RBF) GPSA_GPR_GRAD(GPSA_K_RBF);
  else if (kind == GPSA_K_MATERN32) GPSA_GPR_GRAD(GPSA_K_MATERN32);
  else GPSA_GPR_GRAD(GPSA_K_MATERN12);
#undef GPSA_GPR_GRAD
  GPSA_LAUNCH_CHECK();
  gpr_grad_close_kernel<<<1, 256, 0, st>>>(part, nblk, theta, amplitude ? 1 : 0, out);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_gpr_mean_f64(int kind, const double* XS, long long ns, const double* X, long long N, int D, const double* theta,
                      int amplitude, const double* alpha, int P, double* out, void* stream) {
  using namespace gpsa;
  if (!XS || !X || !theta || !alpha || !out || ns < 1 || N < 1 || D < 1 || P < 1 || !gpr_kind_ok(kind))
    return GPSA_EINVAL;
  if (D > MAXD || cdiv(ns, 16LL) > 0x7fffffffLL || cdiv((long long)P, (long long)GPR_T) > 65535)
    return GPSA_EUNSUPPORTED;
  const dim3 grid((unsigned)cdiv(ns, 16LL), (unsigned)cdiv((long long)P, (long long)GPR_T));
  hipStream_t st = as_stream(stream);
#define GPSA_GPR_MEAN(KD) gpr_mean_kernel<KD><<<grid, 256, 0, st>>>(XS, ns, X, N, D, theta, amplitude ? 1 : 0, alpha, P, out)
  if (kind == GPSA_K_RBF) GPSA_GPR_MEAN(GPSA_K_RBF);
  else if (kind == GPSA_K_MATERN32) GPSA_GPR_MEAN(GPSA_K_MATERN32);
  else GPSA_GPR_MEAN(GPSA_K_MATERN12);
#undef GPSA_GPR_MEAN
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
