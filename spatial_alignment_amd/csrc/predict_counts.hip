// Count predictions: the data GP's closing under a Poisson likelihood with a log link.  The sibling of predict.hip - same
// inputs (a row chunk's per-sample conditional mean / quadratic form: meanT, v [L, S*c], column s*c + r; q [S*c]), same
// layout, same per-sample log-rate moments m_s, u_s (LMC mix per sample, +2e-5, no tau) - closed on the scale of the
// counts: with eta ~ Normal(mu, u), mu = m_s + log_offset[r], u = u_s, per row r and output p
//   lam_s  = exp(mu + u/2)                                              (the lognormal's mean)
//   Y_mean = mean_s lam_s
//   Y_var  = Y_mean + mean_s[lam_s^2 expm1(u)] + var_s(lam_s)           (Poisson + within-sample + between-sample)
//   lpd[r] = sum_p log mean_s Int Poisson(y; e^eta) Normal(eta; mu, u) d eta          (NaN entries of Y contribute 0)
// The Poisson-lognormal integral has no closed form.  It is taken by Gauss-Hermite quadrature CENTRED ON THE INTEGRAND'S
// MODE (Laplace's centre and scale; the rule is then exact for the Gaussian part and sees the rest as a smooth factor):
//   h(eta) = y eta - e^eta - (eta - mu)^2 / (2u),  concave;   Newton from e0 = min(mu + u y, max(mu, log y)), which lies at
//   or to the right of the mode (h' <= 0 there: monotone convergence, no overshoot into exp's overflow), exactly
//   PCNT_NEWTON iterations, no data-dependent loop;   s^2 = 1 / (e^e^ + 1/u),   eta_k = e^ + sqrt(2 s^2) x_k,
//   log Int = log sum_k exp(h(eta_k) + x_k^2 + log w_k) + (1/2) log(2 s^2) - (1/2) log(2 pi u) - lgamma(y + 1).
// The node terms are summed relative to h(e^): h is concave with its maximum next to e^ and every x_k^2 + log w_k is
// negative, so no term exceeds it by more than Newton's residual and nothing overflows; the samples are then mixed through
// a running maximum of h(e^) as predict.hip mixes its Gaussian components (far-apart components do not underflow to -inf).
// Measured against a dense trapezoid integral in fp64 (tests/test_predict_counts.py): |error| / max(1, |lpd|) per entry
// 1.9e-10 for u <= 0.5, 2.0e-8 for u <= 1, 1.8e-6 for u <= 2, 4.6e-5 for u <= 4; nothing is measured beyond u = 4.
//
// Compute-bound, unlike its sibling: with Y about PCNT_NEWTON + 1 + 2 * 20 + 3 exponentials per (row, output, sample), all
// fp64 (the bars are held against an fp64 integral and the kernel does nothing else with its time).  Without Y neither
// the mode nor the quadrature is computed: HAS_Y is a template argument, the decision is the launch's, not a lane's.
#include <math.h>

#include "common.hpp"

namespace gpsa {

constexpr double PCNT_TWO_JITTER = 2e-5;  // diagonal_offset added twice (vgpsa.py:191/201 and :204), quirk 3
constexpr int PCNT_TR = 32;               // rows of the chunk per workgroup
constexpr int PCNT_TP = 32;               // outputs per pass: a wave stores 32 consecutive outputs of two rows
constexpr int PCNT_RPT = PCNT_TR / 8;     // rows per thread (half-wave h of 8 owns rows h, h + 8, ...)
constexpr int PCNT_LMAX = 64;             // latent outputs an LMC mix can take (W's slab is LDS-resident)
constexpr int PCNT_NEWTON = 8;            // Newton iterations for the mode (4 fail by orders of magnitude)
constexpr int PCNT_HALF_Q = 10;           // Q = 20 Gauss-Hermite nodes, +-x_k in pairs

// the positive half of the 20-node Gauss-Hermite rule: {x_k, log w_k + x_k^2} (the other half mirrors it); the same
// numbers as predict.GH_NODES, which tests/test_predict_counts.py pins against a brute-force integral
__constant__ double PCNT_GH[PCNT_HALF_Q][2] = {
    {0.24534070830090124, -0.7114710404116901},
    {0.7374737285453944, -0.7055368459223146},
    {1.234076215395323, -0.6933054504113765},
    {1.7385377121165861, -0.6739741099862373},
    {2.2549740020892757, -0.6461102649118216},
    {2.7888060584281305, -0.6072415536850873},
    {3.3478545673832163, -0.5529289199616052},
    {3.944764040115625, -0.4743672219775181},
    {4.603682449550744, -0.35050407841539055},
    {5.387480890011233, -0.10692622802020324},
};

// log of Int e^{h(eta)} d eta / sqrt(2 pi u), split as ref + log(amp) - log(pi)/2: ref = h(e^), amp = sqrt(s^2 / u) sum_k e^{...}
__device__ __forceinline__ void pcnt_integral(double y, double mu, double u, double logy, double& ref, double& amp) {
  double e = fmin(fma(u, y, mu), fmax(mu, logy));
#pragma unroll 1
  for (int it = 0; it < PCNT_NEWTON; ++it) {
    const double E = exp(e);
    e += (u * (y - E) - (e - mu)) / fma(u, E, 1.0);  // e - h'(e) / h''(e), both multiplied by u
  }
  const double E = exp(e);
  const double g = 1.0 / fma(u, E, 1.0);  // s^2 / u
  const double sc = sqrt(2.0 * u * g);    // sqrt(2 s^2)
  const double d0 = e - mu, i2u = 0.5 / u;
  ref = y * e - E - d0 * d0 * i2u;
  double T = 0.0;
#pragma unroll 1
  for (int k = 0; k < PCNT_HALF_Q; ++k) {
    const double t = sc * PCNT_GH[k][0], lw = PCNT_GH[k][1] - ref;
    const double ea = e + t, eb = e - t, da = d0 + t, db = d0 - t;
    T += exp(fma(y, ea, lw) - exp(ea) - da * da * i2u);
    T += exp(fma(y, eb, lw) - exp(eb) - db * db * i2u);
  }
  amp = T * sqrt(g);
}

// fp64 logarithm from the fp32 one and the fp64 exponential: l0 = logf(x) is good to ~1e-7 l0, r = x e^{-l0} - 1 is that
// error exactly, and log(1 + r) = r - r^2/2 to r^3/3 < 1e-15.  The library's fp64 log brings a second set of fp64
// constants, which do not fit the scalar registers next to the exponential's and this kernel's arguments (predict.hip
// notes the same).  x in (0, FLT_MAX); the callers see to that.
__device__ __forceinline__ double pcnt_log(double x) {
  const double l0 = (double)logf((float)x);
  const double r = fma(x, exp(-l0), -1.0);
  return l0 + fma(-0.5 * r, r, r);
}

// lgamma(x) + log(pi)/2 for x > 0 (the quadrature's constant rides along) by Stirling's series at z >= 8 (x < 8 is
// shifted up by 7 through the recurrence): absolute error below 3e-13, next to log densities of order one and more
__device__ __forceinline__ double pcnt_lgamma_half_log_pi(double x) {
  const bool low = x < 8.0;
  const double prod = x * (x + 1.0) * (x + 2.0) * (x + 3.0) * (x + 4.0) * (x + 5.0) * (x + 6.0);
  const double z = low ? x + 7.0 : x;
  const double iz = 1.0 / z, iz2 = iz * iz;
  constexpr double HALF_LOG_2PI_PI = 0.91893853320467274178 + 0.57236494292470008707;  // (log 2 pi + log pi) / 2
  double t = fma(iz2, 1.0 / 1188.0, -1.0 / 1680.0);
  t = fma(iz2, t, 1.0 / 1260.0);
  t = fma(iz2, t, -1.0 / 360.0);
  t = fma(iz2, t, 1.0 / 12.0);
  const double st = fma(z - 0.5, pcnt_log(z), -z) + fma(t, iz, HALF_LOG_2PI_PI);
  return st - pcnt_log(low ? prod : 1.0);
}

// expm1(u), u >= 0, from exp and log alone (Kahan): (w - 1) u / log w with w = exp(u) cancels the rounding of w; beyond
// u = 40, w - 1 is w
__device__ __forceinline__ double pcnt_expm1(double u) {
  const double w = exp(u);
  const bool big = u > 40.0, tiny = w == 1.0;
  const double k = (w - 1.0) * u / pcnt_log((big || tiny) ? 2.0 : w);
  return big ? w : (tiny ? u : k);
}

// LMC: m_s = mu_s W, u_s = sigma2_s (W o W) with W's [L x 32] slab and its square resident in LDS (L <= 64), mixed per
// sample BEFORE anything is exponentiated.  !LMC: P == L, m_s = mu_s.  The staging is predict.hip's, restated (that
// unit's device code is not touched), with one difference: a thread closes its PCNT_RPT rows one after the other, each
// over all S samples, and the slab is staged again for each.  With Y the closing costs some 2000 fp64 instructions per
// (row, output, sample) against 8 bytes staged, and one entry's state per thread is what keeps the kernel free of spills
// (four entries at once: 356 registers and up to 158 scalar spills): 144-148 VGPRs, three waves per SIMD (the LMC
// variant's 41.7 KB of LDS allows three workgroups per CU as well).  Without Y the kernel is NOT compute-bound (about
// four exponentials per entry) and still reads meanT, v and q four times and passes twice the barriers of its sibling;
// the repeats come from a slab the same workgroup has just read and are expected to be served by L2, but nothing of that
// is measured.  It keeps the one structure so that its moments are the Y variant's bit for bit (96-112 VGPRs, 4-5 waves
// per SIMD); staging once with four entries' state is open for it if the call's time ever shows it.
template <bool LMC, bool HAS_Y>
__global__ void __launch_bounds__(256)
predict_counts_kernel(const float* __restrict__ meanT, const float* __restrict__ v, const double* __restrict__ q,
                      const float* __restrict__ var_u, long long c, int S, int L, int P, const float* __restrict__ W,
                      const float* __restrict__ log_offset, const float* __restrict__ Y, float* __restrict__ Y_mean,
                      float* __restrict__ Y_var, double* __restrict__ lpd) {
  constexpr int NL = LMC ? PCNT_LMAX : PCNT_TP;  // latent outputs staged per sample
  // the loads of a slab in flight together: all of them where the kernel waits for memory (no Y); one by one next to the
  // quadrature, whose constants need the scalar registers that the unrolled loads' eight edge masks would take
  constexpr int STAGE_UNROLL = HAS_Y ? 1 : NL / 8;
  __shared__ float s_mu[NL][PCNT_TR + 1];
  __shared__ double s_sig[NL][PCNT_TR + 1];
  __shared__ float s_w[LMC ? PCNT_LMAX : 1][PCNT_TP], s_w2[LMC ? PCNT_LMAX : 1][PCNT_TP];

  const int tid = threadIdx.x;
  const int px = tid & 31, ry = tid >> 5;  // accumulation: output px of the pass, rows ry + 8 j
  const int sr = tid & 31, sl = tid >> 5;  // staging: row sr of the tile, outputs sl + 8 k
  const long long r0 = (long long)blockIdx.x * PCNT_TR;
  const long long SC = (long long)S * c;
  const double var0 = exp((double)var_u[0]);
  const double inv_S = 1.0 / (double)S;

  // this thread's entry (row ry, output px) of the three [c, P] arrays and its row of lpd, as per-thread pointers: formed
  // once, they take the four base pointers out of the scalar registers for the rest of the kernel
  const long long e00 = (r0 + ry) * (long long)P + px;
  const float* y_at = HAS_Y ? Y + e00 : nullptr;
  float* mean_at = Y_mean + e00;
  float* var_at = Y_var + e00;
  double* lpd_at = HAS_Y ? lpd + (r0 + (tid & (PCNT_TR - 1))) : nullptr;
  // the rows' offsets and log densities live in registers across the passes; jj below is a run-time index, so both are
  // read and written through selects over the four
  double lp[PCNT_RPT], offs[PCNT_RPT];
#pragma unroll
  for (int j = 0; j < PCNT_RPT; ++j) {
    const long long r = r0 + ry + 8 * j;
    lp[j] = 0.0;
    offs[j] = (log_offset != nullptr && r < c) ? (double)log_offset[r] : 0.0;
  }

  for (int p0 = 0; p0 < P; p0 += PCNT_TP) {
    const int p = p0 + px;
    const int l0 = LMC ? 0 : p0;  // first latent output staged in this pass
    if (LMC) {
      __syncthreads();  // the previous pass has finished reading the slab
      for (int e = tid; e < PCNT_LMAX * PCNT_TP; e += 256) {
        const int l = e >> 5, pp = e & 31;
        const float w = (l < L && p0 + pp < P) ? W[(long long)l * P + p0 + pp] : 0.f;
        s_w[LMC ? l : 0][pp] = w;
        s_w2[LMC ? l : 0][pp] = w * w;
      }
    }
#pragma unroll 1
    for (int jj = 0; jj < PCNT_RPT; ++jj) {
      const int row = ry + 8 * jj;
      const long long ra = r0 + row;
      const bool inside = ra < c && p < P;
      const long long at = 8LL * jj * P + p0;  // from (row ry, output px) to (row, output p)
      double off = offs[0];
#pragma unroll
      for (int j = 1; j < PCNT_RPT; ++j) off = (j == jj) ? offs[j] : off;
      double y = 0.0, logy = 0.0;
      bool valid = false;
      if (HAS_Y) {
        const double yv = inside ? (double)y_at[at] : (double)NAN;
        valid = yv == yv;
        y = valid ? yv : 0.0;  // a missing entry runs the arithmetic of a zero and is left out of every sum
        logy = y > 0.0 ? pcnt_log(y) : -INFINITY;  // y = 0: the start is then mu
      }
      double lam0 = 0.0, sd = 0.0, sdd = 0.0, sw = 0.0, acc = 0.0, mx = -INFINITY;
      for (int s = 0; s < S; ++s) {
        __syncthreads();  // the previous slab has been consumed
        {
          const long long r = r0 + sr;
          const long long col = (long long)s * c + r;
          // sigma^2 - q formed in fp64 before anything is rounded: it cancels to ~1e-3 sigma^2 for dense inducing sets
          const double resid = (r < c) ? (var0 - q[col]) + PCNT_TWO_JITTER : 0.0;
#pragma unroll STAGE_UNROLL
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
        double m, u;
        if (LMC) {
          m = u = 0.0;
          for (int l = 0; l < L; ++l) {
            m = fma((double)s_mu[l][row], (double)s_w[LMC ? l : 0][px], m);
            u = fma(s_sig[l][row], (double)s_w2[LMC ? l : 0][px], u);
          }
        } else {
          m = (double)s_mu[px][row];
          u = s_sig[px][row];
        }
        const double mu = m + off;
        const double lam = exp(fma(0.5, u, mu));
        // between-sample term from values centred on the first sample, fp64 sums (never E[lam^2] - E[lam]^2)
        if (s == 0) lam0 = lam;
        const double d = lam - lam0;
        sd += d;
        sdd = fma(d, d, sdd);
        sw = fma(lam * lam, pcnt_expm1(u), sw);
        if (HAS_Y) {
          // u = 0 (rows and outputs past the edge; an all-zero column of W) is the limit of a point mass at mu: the floor
          // keeps 1/u finite and gives exactly that limit (the mode stays at mu, the node terms become -x_k^2)
          double ref, amp;
          pcnt_integral(y, mu, fmax(u, 0x1p-500), logy, ref, amp);
          // mixture over the samples through a running maximum (selects, no branches; one exp per sample)
          const double dt = ref - mx;  // +inf at the first sample (mx = -inf)
          const double ex = exp(-fabs(dt));
          const bool up = dt > 0.0;
          const double acc_new = up ? fma(acc, ex, amp) : fma(amp, ex, acc);
          acc = valid ? acc_new : acc;
          mx = (valid && up) ? ref : mx;
        }
      }
      if (inside) {
        const double mean_d = sd * inv_S;  // mean of the centred values
        const double between = fmax(fma(sdd, inv_S, -(mean_d * mean_d)), 0.0);
        const double mean = lam0 + mean_d;
        mean_at[at] = (float)mean;
        var_at[at] = (float)(mean + fma(sw, inv_S, between));
      }
      if (HAS_Y) {
        const double term = (inside && valid) ? mx + pcnt_log(acc * inv_S) - pcnt_lgamma_half_log_pi(y + 1.0) : 0.0;
#pragma unroll
        for (int j = 0; j < PCNT_RPT; ++j) lp[j] += (j == jj) ? term : 0.0;
      }
    }
  }
  if (HAS_Y) {  // the rows' sums over the outputs, through LDS in a fixed order (the workgroup owns its rows)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PCNT_RPT; ++j) s_sig[px][ry + 8 * j] = lp[j];
    __syncthreads();
    if (tid < PCNT_TR && r0 + tid < c) {
      double tot = 0.0;
      for (int k = 0; k < PCNT_TP; ++k) tot += s_sig[k][tid];
      *lpd_at = tot;
    }
  }
}

template <bool LMC>
static int launch_predict_counts(dim3 grid, hipStream_t st, const float* meanT, const float* v, const double* q,
                                 const float* var_u, long long c, int S, int L, int P, const float* W,
                                 const float* log_offset, const float* Y, float* Y_mean, float* Y_var, double* lpd) {
  if (Y != nullptr)
    predict_counts_kernel<LMC, true><<<grid, 256, 0, st>>>(meanT, v, q, var_u, c, S, L, P, W, log_offset, Y, Y_mean,
                                                            Y_var, lpd);
  else
    predict_counts_kernel<LMC, false><<<grid, 256, 0, st>>>(meanT, v, q, var_u, c, S, L, P, W, log_offset, nullptr,
                                                             Y_mean, Y_var, nullptr);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // namespace gpsa

extern "C" int gpsa_predict_counts_f32(const float* meanT, const float* v, const double* q, const float* var_u,
                                       long long c, int S, int L, int P, const float* W, const float* log_offset,
                                       const float* Y, float* Y_mean, float* Y_var, double* lpd, void* stream) {
  if (c < 1 || S < 1 || L < 1 || P < 1) return GPSA_EINVAL;
  if (meanT == nullptr || v == nullptr || q == nullptr || var_u == nullptr || Y_mean == nullptr || Y_var == nullptr)
    return GPSA_EINVAL;
  if (W == nullptr && P != L) return GPSA_EINVAL;
  if ((Y == nullptr) != (lpd == nullptr)) return GPSA_EINVAL;
  if (W != nullptr && L > gpsa::PCNT_LMAX) return GPSA_EUNSUPPORTED;  // W's slab is LDS-resident (as predict.hip)
  const long long blocks = cdiv(c, gpsa::PCNT_TR);
  if (blocks > 0x7fffffffLL) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)blocks);
  if (W != nullptr)
    return gpsa::launch_predict_counts<true>(grid, st, meanT, v, q, var_u, c, S, L, P, W, log_offset, Y, Y_mean, Y_var,
                                             lpd);
  return gpsa::launch_predict_counts<false>(grid, st, meanT, v, q, var_u, c, S, L, P, nullptr, log_offset, Y, Y_mean,
                                            Y_var, lpd);
}
