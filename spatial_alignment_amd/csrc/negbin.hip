// Count outputs (model.likelihood = "negative_binomial"): the per-element kernels of the negative binomial likelihood term with a
// trainable dispersion per output, rho [P], r_p = exp(rho_p).
//   nb_const_kernel / gpsa_nb_const   the draw-independent pieces, once per step: per view the sums of
//                                     lgamma(y + r) - lgamma(r), per output the weighted sums of r (psi(y + r) - psi(r))
//   loglik_nb_kernel<BWD>             sums of t = y a - (y + r) softplus(a) per (view, block) / dF = gloss w_v ((y + r)
//                                     sigma(a) - y) / S and the per-output sums of u = -r softplus(a) + (y + r) sigma(a) - y
//                                     (the closing pair gpsa_elbo_loss_nb_fwd / _bwd of loss_views.hip launches it)
//   gpsa_lmc_loglik_fused_nb_f32      the fused LMC pass (lmc_mfma_nb_kernel, lmc.hip) and the reduction of its partials
// a = F + log_offset[row] - rho_p.  No exp(eta) appears, so nothing overflows for a large eta; expf / log1pf are the exact
// ones.  Per-element terms are fp32, every sum is fp64 in a fixed order; the y-only pieces are fp64 throughout (r (psi(y + r)
// - psi(r)) cancels badly for a large r).  Y is not validated.  The NaN test is y == y (no fast-math flag in the build).
// Every kernel here is a column reduction over [rows, P]: thread (tx, ty) of a block owns column c0 + tx and the rows ty,
// ty + rl, .. of the block's row range (cw columns x rl = 256 / cw row lanes: consecutive threads read consecutive p), the
// row lanes are folded through LDS in a fixed tree, and the per-(view, row block) column partials are summed in order by a
// finishing launch.
#include "internal.hpp"

namespace gpsa {

// digamma for x > 0 in fp64: psi(x) = psi(x + 1) - 1 / x up to x >= 8, then the asymptotic series through x^-14
// (x <= 0: NaN - the recurrence would not end for a far negative argument)
__device__ __forceinline__ double digamma_pos(double x) {
  if (!(x > 0.0)) return __builtin_nan("");
  double s = 0.0;
  while (x < 8.0) {
    s -= 1.0 / x;
    x += 1.0;
  }
  const double i = 1.0 / x, i2 = i * i;
  // B_2k / (2k): 1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12
  const double ser =
      i2 * (1.0 / 12.0 -
            i2 * (1.0 / 120.0 -
                  i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 - i2 * (691.0 / 32760.0 - i2 * (1.0 / 12.0)))))));
  return s + log(x) - 0.5 * i - ser;
}

// fold the rl = 256 / cw row lanes of every column: red[256], thread (tx, ty) at ty * cw + tx; the sum lands in ty == 0
__device__ __forceinline__ double fold_rows(double v, double* red, int cw) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= cw; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[threadIdx.x];
}

NbGrid nb_grid(long long rows, int V, int P) {
  NbGrid g;
  g.cw = 1;
  while (g.cw < 64 && g.cw < P) g.cw <<= 1;
  const long long ct = cdiv(P, g.cw);
  g.gx = (int)(ct < 16 ? ct : 16);
  long long nrb = cdiv(rows, 4LL * (256 / g.cw));  // four rows per thread and more
  const long long cap = 4096 / ((long long)V * g.gx);  // V <= 64, gx <= 16: cap >= 4
  if (nrb > cap) nrb = cap;
  if (nrb > 1024) nrb = 1024;  // (enough row blocks to fill the device at a narrow P; the finish walks them per output)
  if (nrb < 1) nrb = 1;
  g.nrb = (int)nrb;
  return g;
}

// Y [N, P], rho [P]; grid (gx, nrb, V).  cpart[(v * nrb + b) * gx + x] = the block's sum of lgamma(y + r) - lgamma(r);
// dpart[(v * nrb + b) * P + p] = the row block's sum of r (psi(y + r) - psi(r)) in column p
__global__ void __launch_bounds__(256)
nb_const_kernel(const float* __restrict__ Y, const float* __restrict__ rho, long long P, ViewRows vr, int cw, int skip,
                double* __restrict__ cpart, double* __restrict__ dpart) {
  __shared__ double red[256];
  __shared__ double red4[4];
  const int v = blockIdx.z, b = blockIdx.y, nrb = gridDim.y, rl = 256 / cw;
  const int tx = threadIdx.x & (cw - 1), ty = threadIdx.x / cw;
  const long long lo = vr.off[v], rows = vr.off[v + 1] - lo, chunk = (rows + nrb - 1) / nrb;
  const long long q0 = b * chunk, q1 = (q0 + chunk < rows) ? q0 + chunk : rows;
  double ctot = 0.0;
  for (long long c0 = (long long)blockIdx.x * cw; c0 < P; c0 += (long long)gridDim.x * cw) {
    const long long p = c0 + tx;
    double cs = 0.0, ds = 0.0;
    if (p < P) {
      const double r = exp((double)rho[p]);
      const double lgr = lgamma(r), psr = digamma_pos(r);
      for (long long q = q0 + ty; q < q1; q += rl) {
        const float y = Y[(lo + q) * P + p];
        if (!skip || y == y) {
          const double yr = (double)y + r;
          cs += lgamma(yr) - lgr;
          ds += r * (digamma_pos(yr) - psr);
        }
      }
    }
    ds = fold_rows(ds, red, cw);
    if (ty == 0 && p < P) dpart[((long long)v * nrb + b) * P + p] = ds;
    ctot += cs;
  }
  ctot = block_sum(ctot, red4);
  if (threadIdx.x == 0) cpart[((long long)v * nrb + b) * gridDim.x + blockIdx.x] = ctot;
}

// csum[v] = view v's block partials in order (block 0);  dconst[p] = sum_v w_v sum_b dpart[(v nrb + b) P + p], views and
// row blocks in order, one thread per output
__global__ void __launch_bounds__(256)
nb_const_finish_kernel(const double* __restrict__ cpart, const double* __restrict__ dpart, int V, int nrb, int gx,
                       long long P, const double* __restrict__ w, double* __restrict__ csum, double* __restrict__ dconst) {
  __shared__ double red4[4];
  const long long p = blockIdx.x * 256LL + threadIdx.x;
  if (p < P) {
    double tot = 0.0;
    for (int v = 0; v < V; ++v) {
      double s = 0.0;
      for (int b = 0; b < nrb; ++b) s += dpart[((long long)v * nrb + b) * P + p];
      tot += (w != nullptr ? w[v] : 1.0) * s;
    }
    dconst[p] = tot;
  }
  if (blockIdx.x == 0) {
    const int per = nrb * gx;
    for (int v = 0; v < V; ++v) {
      double s = 0.0;
      for (int k = threadIdx.x; k < per; k += 256) s += cpart[(long long)v * per + k];
      s = block_sum(s, red4);
      if (threadIdx.x == 0) csum[v] = s;
      __syncthreads();
    }
  }
}

// F [S, N, P], Y [N, P], off [N] or nullptr, rho [P]; grid (gx, nrb, V) over the S * rows_v rows (s, n) of view v
template <bool BWD>
__global__ void __launch_bounds__(256)
loglik_nb_kernel(const float* __restrict__ F, const float* __restrict__ Y, const float* __restrict__ off,
                 const float* __restrict__ rho, int S, long long N, long long P, ViewRows vr, int cw,
                 const double* __restrict__ w, const float* __restrict__ gloss, int skip, float* __restrict__ dF,
                 double* __restrict__ part, double* __restrict__ upart) {
  __shared__ double red[256];
  __shared__ double red4[4];
  const int v = blockIdx.z, b = blockIdx.y, nrb = gridDim.y, rl = 256 / cw;
  const int tx = threadIdx.x & (cw - 1), ty = threadIdx.x / cw;
  const long long lo = vr.off[v], rv = vr.off[v + 1] - lo, rows = rv * S, chunk = (rows + nrb - 1) / nrb;
  const long long q0 = b * chunk, q1 = (q0 + chunk < rows) ? q0 + chunk : rows;
  const double wv = w != nullptr ? w[v] : 1.0;
  const float coef = BWD ? (float)((double)gloss[0] * wv / (double)S) : 0.f;
  double ttot = 0.0;
  for (long long c0 = (long long)blockIdx.x * cw; c0 < P; c0 += (long long)gridDim.x * cw) {
    const long long p = c0 + tx;
    double acc = 0.0;
    if (p < P) {
      const float rh = rho[p], r = expf(rh);
      // (s, n) of row q: one division for the thread's first row, then steps of rl rows
      long long sm = (q0 + ty < q1) ? (q0 + ty) / rv : 0, nn = (q0 + ty < q1) ? (q0 + ty) - sm * rv : 0;
      for (long long q = q0 + ty; q < q1; q += rl) {
        const long long n = lo + nn;
        const long long i = (sm * N + n) * P + p;
        const float y = Y[n * P + p];
        const float a = F[i] + (off != nullptr ? off[n] : 0.f) - rh;
        const float e = expf(-fabsf(a));                 // in (0, 1]: nothing overflows
        const float sp = fmaxf(a, 0.f) + log1pf(e);      // softplus(a)
        const float sg = (a >= 0.f ? 1.f : e) / (1.f + e);  // sigma(a)
        const float yr = y + r;
        const bool obs = !skip || y == y;
        if (BWD) {
          const float d = fmaf(yr, sg, -y);
          dF[i] = obs ? coef * d : 0.f;
          acc += obs ? (double)fmaf(-r, sp, d) : 0.0;
        } else {
          acc += obs ? (double)fmaf(y, a, -yr * sp) : 0.0;
        }
        nn += rl;
        while (nn >= rv) {
          nn -= rv;
          ++sm;
        }
      }
    }
    if (BWD) {
      acc = fold_rows(acc, red, cw);
      if (ty == 0 && p < P) upart[((long long)v * nrb + b) * P + p] = acc;
    } else {
      ttot += acc;
    }
  }
  if (!BWD) {
    ttot = block_sum(ttot, red4);
    if (threadIdx.x == 0) part[(long long)v * (nrb * gridDim.x) + (long long)b * gridDim.x + blockIdx.x] = ttot;
  }
}

int nb_loglik_launch(bool bwd, const float* F, const float* Y, const float* log_offset, const float* log_disp, int S,
                     long long N, int P, const ViewRows& vr, int V, const NbGrid& g, const double* w, const float* gloss,
                     int skip, float* dF, double* part, double* upart, hipStream_t st) {
  const dim3 grid(g.gx, g.nrb, V);
  if (bwd)
    loglik_nb_kernel<true><<<grid, 256, 0, st>>>(F, Y, log_offset, log_disp, S, N, P, vr, g.cw, w, gloss, skip, dF,
                                                 nullptr, upart);
  else
    loglik_nb_kernel<false><<<grid, 256, 0, st>>>(F, Y, log_offset, log_disp, S, N, P, vr, g.cw, w, nullptr, skip, nullptr,
                                                  part, nullptr);
  GPSA_LAUNCH_CHECK();
  return 0;
}

// one thread per output, views and row blocks in order
__global__ void __launch_bounds__(256)
nb_ddisp_kernel(const double* __restrict__ upart, int V, int nrb, long long P, const double* __restrict__ w, int S,
                const double* __restrict__ dconst, const float* __restrict__ gloss, float* __restrict__ ddisp) {
  const long long p = blockIdx.x * 256LL + threadIdx.x;
  if (p >= P) return;
  double tot = 0.0;
  for (int v = 0; v < V; ++v) {
    double s = 0.0;
    for (int b = 0; b < nrb; ++b) s += upart[((long long)v * nrb + b) * P + p];
    tot += (w != nullptr ? w[v] : 1.0) * s;
  }
  ddisp[p] = (float)(-(double)gloss[0] * (tot / (double)S + dconst[p]));
}

int nb_ddisp_launch(const double* upart, int V, int nrb, int P, const double* w, int S, const double* dconst,
                    const float* gloss, float* ddisp, hipStream_t st) {
  nb_ddisp_kernel<<<(unsigned)cdiv(P, 256), 256, 0, st>>>(upart, V, nrb, P, w, S, dconst, gloss, ddisp);
  GPSA_LAUNCH_CHECK();
  return 0;
}

// bytes of gpsa_nb_const's partials for one term: [V][nrb][P] column partials and [V][nrb][gx] block sums
static long long nb_const_bytes(long long N, int P, int V) {
  const NbGrid g = nb_grid(N, V, P);  // (a view has at most N rows: the launch's nrb is no larger)
  return 8LL * V * g.nrb * ((long long)P + g.gx);
}

}  // namespace gpsa

extern "C" {

long long gpsa_nb_const_workspace(long long N, int P, int n_views) {
  if (N < 1 || P < 1 || n_views < 1 || n_views > gpsa::LOSS_MAX_VIEWS) return 0;
  return gpsa::nb_const_bytes(N, P, n_views);
}

int gpsa_nb_const(int n_ll, const float* const* Y, const long long* N, const int* P, const float* const* log_disp,
                  const int* n_views, const long long* const* view_off, const double* const* w, int skip,
                  double* const* csum, double* const* dconst, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (n_ll < 1 || n_ll > GPSA_MAX_MODS || !Y || !N || !P || !log_disp || !csum || !dconst || !workspace)
    return GPSA_EINVAL;
  if ((n_views == nullptr) != (view_off == nullptr) || (w != nullptr && n_views == nullptr)) return GPSA_EINVAL;
  for (int i = 0; i < n_ll; ++i) {
    if (!Y[i] || !log_disp[i] || !csum[i] || !dconst[i] || N[i] < 1 || P[i] < 1) return GPSA_EINVAL;
    if (n_views && !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
    if (workspace_bytes < nb_const_bytes(N[i], P[i], n_views ? n_views[i] : 1)) return GPSA_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  // one launch pair per term (the stream orders their use of the one workspace)
  for (int i = 0; i < n_ll; ++i) {
    const int V = n_views ? n_views[i] : 1;
    const ViewRows vr = view_rows(N[i], V, view_off ? view_off[i] : nullptr);
    long long most = 0;
    for (int v = 0; v < V; ++v)
      if (vr.off[v + 1] - vr.off[v] > most) most = vr.off[v + 1] - vr.off[v];
    const NbGrid g = nb_grid(most, V, P[i]);
    double* dpart = reinterpret_cast<double*>(workspace);
    double* cpart = dpart + (long long)V * g.nrb * P[i];
    nb_const_kernel<<<dim3(g.gx, g.nrb, V), 256, 0, st>>>(Y[i], log_disp[i], P[i], vr, g.cw, skip, cpart, dpart);
    nb_const_finish_kernel<<<(unsigned)cdiv(P[i], 256), 256, 0, st>>>(cpart, dpart, V, g.nrb, g.gx, P[i],
                                                                      (w && w[i]) ? w[i] : nullptr, csum[i], dconst[i]);
  }
  GPSA_LAUNCH_CHECK();
  return 0;
}

long long gpsa_lmc_loglik_nb_workspace(long long C, int L, int P, int nparts) {
  const long long old = gpsa_lmc_loglik_workspace(C, L, P, nparts);
  if (old <= 0) return 0;
  const long long G = (old - 256) / ((long long)L * P * 4);  // the query's workgroups
  return ((old + 7) & ~7LL) + 8 * G * P;                      // ... and their [G][P] fp64 sums of u behind the dW partials
}

int gpsa_lmc_loglik_fused_nb_f32(const float* F, const float* W, const float* Y, const float* log_offset,
                                 const float* log_disp, int skip, int S, long long N, int L, int P, double* zpart,
                                 int nparts, float* dF, float* dW, double* usum, void* workspace,
                                 long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!F || !W || !Y || !log_disp || !zpart || !dF || !dW || !usum || S < 1 || N < 1 || L < 1 || P < 1 || nparts < 1)
    return GPSA_EINVAL;
  if (L > 64) return GPSA_EUNSUPPORTED;
  const long long C = (long long)S * N;
  const long long old = gpsa_lmc_loglik_workspace(C, L, P, nparts);
  if (!workspace || workspace_bytes < gpsa_lmc_loglik_nb_workspace(C, L, P, nparts)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  // gpsa_lmc_loglik_fused_f32's grid: the workspace query's workgroups, at most one per tile of 16 spots
  const int G = (int)((old - 256) / ((long long)L * P * 4));
  const long long nt = cdiv(N, 16);
  const int Gm = (int)(nt < G ? nt : G);
  float* part = (float*)workspace;
  double* upart = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + ((old + 7) & ~7LL));
  if (int rc = lmc_mfma_nb_launch(F, W, Y, log_offset, log_disp, skip, S, N, L, P, zpart, nparts, dF, part, upart, Gm, st))
    return rc;
  const long long n = (long long)L * P;
  reduce_rows_kernel<float, float><<<(unsigned)cdiv(n, 64), 256, 0, st>>>(part, Gm, n, n, dW, 1.0);
  reduce_rows_kernel<double, double><<<(unsigned)cdiv(P, 64), 256, 0, st>>>(upart, Gm, P, P, usum, 1.0);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
