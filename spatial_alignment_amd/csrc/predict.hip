// Closed-form predictive moments of the data GP: the other closing of the layer that data_sample_fwd_kernel closes with
// a draw.  From a row chunk's per-sample conditional mean / quadratic form (meanT, v [L, S*c], column s*c + r; q [S*c])
// it forms, per row r and output p, the moments of the mixture over the S warp samples and, with observations, the
// held-out log predictive density - all S samples reduced inside the kernel, nothing of size S*c*L or S*c*P written.
// Reference: the conditional of gpsa/models/vgpsa.py:174-204, the LMC mix of :428-432 and the likelihood scale of
// :532-538; it replaces the draw-and-average idiom of experiments/expression/slideseq/slideseq_prediction.py:360-368.
//
// HBM-bound: 2 L S c 4 bytes in, 2 c P 4 bytes out.  The inputs are L-major with rows contiguous, the results [c, P]
// row-major: a workgroup owns 32 rows, stages one sample's [32 outputs x 32 rows] slab through LDS (loads: 128 contiguous
// bytes per output row) and keeps its (row, output) accumulators in registers with half a wave per row (stores: 128
// contiguous bytes per row).  All arithmetic behind the loads is fp64: the between-sample variance is a difference of
// nearly equal numbers once the model is trained, and the kernel waits for memory either way.
#include <math.h>

#include "common.hpp"

namespace gpsa {

constexpr double PRED_TWO_JITTER = 2e-5;  // diagonal_offset added twice (vgpsa.py:191/201 and :204), quirk 3
constexpr int PRED_TR = 32;               // rows of the chunk per workgroup
constexpr int PRED_TP = 32;               // outputs per pass: a wave stores 32 consecutive outputs of two rows
constexpr int PRED_RPT = PRED_TR / 8;     // rows per thread (half-wave h of 8 owns rows h, h + 8, ...)
constexpr int PRED_LMAX = 64;             // latent outputs an LMC mix can take (W's slab is LDS-resident)

// LMC: m_s = mu_s W, u_s = sigma2_s (W o W) with W's [L x 32] slab and its square resident in LDS (L <= 64), mixed per
// sample BEFORE the reduction over s (the between-sample term is a variance of m_s, not of mu_s).  !LMC: P == L, m_s = mu_s.
template <bool LMC>
__global__ void __launch_bounds__(256)
predict_moments_kernel(const float* __restrict__ meanT, const float* __restrict__ v, const double* __restrict__ q,
                       const float* __restrict__ var_u, long long c, int S, int L, int P,
                       const float* __restrict__ W, const float* __restrict__ noise_u, int include_noise,
                       const float* __restrict__ Y, float* __restrict__ F_mean, float* __restrict__ F_var,
                       double* __restrict__ lpd) {
  constexpr int NL = LMC ? PRED_LMAX : PRED_TP;  // latent outputs staged per sample
  __shared__ float s_mu[NL][PRED_TR + 1];
  __shared__ double s_sig[NL][PRED_TR + 1];
  __shared__ float s_w[LMC ? PRED_LMAX : 1][PRED_TP], s_w2[LMC ? PRED_LMAX : 1][PRED_TP];

  const int tid = threadIdx.x;
  const int px = tid & 31, ry = tid >> 5;      // accumulation: output px of the pass, rows ry + 8 j
  const int sr = tid & 31, sl = tid >> 5;      // staging: row sr of the tile, outputs sl + 8 k
  const long long r0 = (long long)blockIdx.x * PRED_TR;
  const long long SC = (long long)S * c;
  const double var0 = exp((double)var_u[0]);
  double tau2 = 0.0;
  if (noise_u != nullptr) {
    const double tau = exp((double)noise_u[0]) + 1e-5;  // vgpsa.py:217; used as a standard deviation (quirk 5)
    tau2 = tau * tau;
  }
  const double inv_S = 1.0 / (double)S;
  const bool has_y = Y != nullptr;
  constexpr double LOG_2PI = 1.8378770664093454835606594728112;

  double lp[PRED_RPT];
#pragma unroll
  for (int j = 0; j < PRED_RPT; ++j) lp[j] = 0.0;

  for (int p0 = 0; p0 < P; p0 += PRED_TP) {
    const int p = p0 + px;
    const int l0 = LMC ? 0 : p0;  // first latent output staged in this pass
    if (LMC) {
      __syncthreads();  // the previous pass has finished reading the slab
      for (int e = tid; e < PRED_LMAX * PRED_TP; e += 256) {
        const int l = e >> 5, pp = e & 31;
        const float w = (l < L && p0 + pp < P) ? W[(long long)l * P + p0 + pp] : 0.f;
        s_w[LMC ? l : 0][pp] = w;
        s_w2[LMC ? l : 0][pp] = w * w;
      }
    }
    double m0[PRED_RPT], sd[PRED_RPT], sdd[PRED_RPT], su[PRED_RPT], mx[PRED_RPT], acc[PRED_RPT], y[PRED_RPT];
#pragma unroll
    for (int j = 0; j < PRED_RPT; ++j) {
      m0[j] = sd[j] = sdd[j] = su[j] = acc[j] = 0.0;
      mx[j] = -INFINITY;
      const long long r = r0 + ry + 8 * j;
      y[j] = (has_y && r < c && p < P) ? (double)Y[r * P + p] : (double)NAN;
    }
    for (int s = 0; s < S; ++s) {
      __syncthreads();  // the previous sample's slab has been consumed
      {
        const long long r = r0 + sr;
        const long long col = (long long)s * c + r;
        // sigma^2 - q formed in fp64 before anything is rounded: it cancels to ~1e-3 sigma^2 for dense inducing sets
        const double resid = (r < c) ? (var0 - q[col]) + PRED_TWO_JITTER : 0.0;
#pragma unroll
        for (int k = 0; k < NL; k += 8) {
          const int l = l0 + sl + k;
          float mu = 0.f;
          double sg = 0.0;
          if (r < c && l < L) {
            const long long o = (long long)l * SC + col;
            mu = meanT[o];
            sg = resid + (double)v[o];
          }
          s_mu[sl + k][sr] = mu;
          s_sig[sl + k][sr] = sg;
        }
      }
      __syncthreads();
      double m[PRED_RPT], u[PRED_RPT];
      if (LMC) {
#pragma unroll
        for (int j = 0; j < PRED_RPT; ++j) m[j] = u[j] = 0.0;
        for (int l = 0; l < L; ++l) {
          const double w = (double)s_w[LMC ? l : 0][px], w2 = (double)s_w2[LMC ? l : 0][px];
#pragma unroll
          for (int j = 0; j < PRED_RPT; ++j) {
            m[j] = fma((double)s_mu[l][ry + 8 * j], w, m[j]);
            u[j] = fma(s_sig[l][ry + 8 * j], w2, u[j]);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < PRED_RPT; ++j) {
          m[j] = (double)s_mu[px][ry + 8 * j];
          u[j] = s_sig[px][ry + 8 * j];
        }
      }
#pragma unroll
      for (int j = 0; j < PRED_RPT; ++j) {
        // between-sample term from values centred on the first sample, fp64 sums (never E[m^2] - E[m]^2 of raw values)
        if (s == 0) m0[j] = m[j];
        const double d = m[j] - m0[j];
        sd[j] += d;
        sdd[j] = fma(d, d, sdd[j]);
        su[j] += u[j];
        // log-sum-exp over the samples through a running maximum: far-apart components do not underflow to -inf
        // (selects, no branches: one exp per sample; NaN observations are skipped).  The logarithm and the exponential
        // themselves are fp32 calls on fp64 arguments and sums: 1e-7 absolute on terms of order one, and their fp64
        // versions' constants do not fit the scalar registers next to this kernel's arguments
        const double wv = u[j] + tau2, e = y[j] - m[j];
        const double t = -0.5 * (LOG_2PI + (double)logf((float)wv) + e * e / wv);
        const double dt = t - mx[j];  // +inf at the first sample (mx = -inf)
        const double ex = (double)expf((float)(-fabs(dt)));
        const bool valid = y[j] == y[j], up = dt > 0.0;
        const double acc_new = up ? fma(acc[j], ex, 1.0) : acc[j] + ex;
        acc[j] = valid ? acc_new : acc[j];
        mx[j] = (valid && up) ? t : mx[j];
      }
    }
#pragma unroll
    for (int j = 0; j < PRED_RPT; ++j) {
      const long long r = r0 + ry + 8 * j;
      if (r < c && p < P) {
        const double mean_d = sd[j] * inv_S;  // mean of the centred values
        const double between = fmax(sdd[j] * inv_S - mean_d * mean_d, 0.0);
        F_mean[r * P + p] = (float)(m0[j] + mean_d);
        F_var[r * P + p] = (float)(su[j] * inv_S + between + (include_noise ? tau2 : 0.0));
        if (y[j] == y[j]) lp[j] += mx[j] + (double)logf((float)(acc[j] * inv_S));
      }
    }
  }
  if (lpd != nullptr) {  // the rows' sums over the outputs, through LDS in a fixed order (the workgroup owns its rows)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PRED_RPT; ++j) s_sig[px][ry + 8 * j] = lp[j];
    __syncthreads();
    if (tid < PRED_TR && r0 + tid < c) {
      double tot = 0.0;
      for (int k = 0; k < PRED_TP; ++k) tot += s_sig[k][tid];
      lpd[r0 + tid] = tot;
    }
  }
}

}  // namespace gpsa

extern "C" int gpsa_predict_moments_f32(const float* meanT, const float* v, const double* q, const float* var_u,
                                        long long c, int S, int L, int P, const float* W, const float* noise_u,
                                        int include_noise, const float* Y, float* F_mean, float* F_var,
                                        float* Fl_mean, float* Fl_var, double* lpd, void* stream) {
  if (c < 1 || S < 1 || L < 1 || P < 1) return GPSA_EINVAL;
  if (meanT == nullptr || v == nullptr || q == nullptr || var_u == nullptr || F_mean == nullptr || F_var == nullptr)
    return GPSA_EINVAL;
  if (W == nullptr && P != L) return GPSA_EINVAL;
  if ((Y != nullptr || include_noise) && noise_u == nullptr) return GPSA_EINVAL;
  if ((Y == nullptr) != (lpd == nullptr)) return GPSA_EINVAL;
  if ((Fl_mean == nullptr) != (Fl_var == nullptr)) return GPSA_EINVAL;
  if (W != nullptr && L > gpsa::PRED_LMAX) return GPSA_EUNSUPPORTED;  // W's slab is LDS-resident (as lmc_mfma_kernel)
  const long long blocks = cdiv(c, gpsa::PRED_TR);
  if (blocks > 0x7fffffffLL) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)blocks);
  if (W != nullptr)
    gpsa::predict_moments_kernel<true><<<grid, 256, 0, st>>>(meanT, v, q, var_u, c, S, L, P, W, noise_u, include_noise,
                                                              Y, F_mean, F_var, lpd);
  else
    gpsa::predict_moments_kernel<false><<<grid, 256, 0, st>>>(meanT, v, q, var_u, c, S, L, P, nullptr, noise_u,
                                                               include_noise, Y, F_mean, F_var, lpd);
  GPSA_LAUNCH_CHECK();
  if (Fl_mean != nullptr) {  // the latent outputs' own moments: the unmixed closing, never with the observation noise
    gpsa::predict_moments_kernel<false><<<grid, 256, 0, st>>>(meanT, v, q, var_u, c, S, L, L, nullptr, nullptr, 0,
                                                               nullptr, Fl_mean, Fl_var, nullptr);
    GPSA_LAUNCH_CHECK();
  }
  return 0;
}
