// The ELBO loss closings over per-view tables: every likelihood term is a sum over its views (row ranges of the term),
// each with an fp64 weight and, over partly observed outputs, its count of observed entries.
//   gpsa_elbo_loss_weighted_fwd / _bwd   minibatch training (minibatch.py): loss = -sum_i sum_v w_iv LL_iv + kl_scale sum(kl)
//   gpsa_elbo_loss_skip_fwd / _bwd       model.skip_missing: the same over the observed entries only (a NaN in Y is a
//                                        missing observation), with or without views and weights; terms from draws apply
//                                        the select per element, fused terms arrive as partial sums of z^2 that already
//                                        left the missing entries out; the counts stand where S N P stands elsewhere
//   gpsa_elbo_loss_pois_fwd / _bwd       model.likelihood: the same tables plus a likelihood kind per term; a Poisson
//                                        term (count outputs, poisson.hip) sums y eta - exp(eta) and has the lgamma table
//                                        as its constant, a Gaussian term in the same call is closed as below
//   gpsa_elbo_loss_nb_fwd / _bwd         the same plus negative binomial terms (negbin.hip): rho per output, the tables of
//                                        gpsa_nb_const, and the gradient of rho from per-output sums
// The first two pairs are argument checks around one views_fwd_impl / views_bwd_impl: the weighted pair passes no counts and no
// fused terms.  The per-element kernels differ in their arithmetic and stay two (loglik_w_kernel counts per chunk and
// sums z^2 - 1 in the backward; loglik_skip_kernel leaves the counts to the closing).
#include "internal.hpp"

namespace gpsa {

// part[v * nb + block] = sum over the block's share of view v of  log N(Y; F, s)  (fwd)  or  z^2 - 1  (bwd, which also
// writes dF = up w_v (Y - F) / (s^2 S)); F [S, N, P], Y [N, P], grid (nb, V)
template <bool BWD>
__global__ void __launch_bounds__(256)
loglik_w_kernel(const float* __restrict__ F, const float* __restrict__ Y, const float* __restrict__ noise_u, int S,
                long long NP, int P, ViewRows vr, const double* __restrict__ w, const float* __restrict__ gloss,
                float* __restrict__ dF, double* __restrict__ part) {
  __shared__ double red[4];
  const int v = blockIdx.y, nb = gridDim.x;
  const long long lo = vr.off[v] * P, per = (vr.off[v + 1] - vr.off[v]) * P, tot = per * S;
  const double s = exp((double)noise_u[0]) + 1e-5;  // "variance" used as std
  const float inv = (float)(1.0 / s);
  const double cst = -log(s) - 0.9189385332046727;
  const float coef = BWD ? (float)(-(double)gloss[0] * w[v] / (s * s * (double)S)) : 0.f;
  double acc = 0.0;
  for (long long i0 = blockIdx.x * 256LL * 4; i0 < tot; i0 += (long long)nb * 256 * 4) {
    float acc4 = 0.f;
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long j = i0 + u * 256 + threadIdx.x;
      if (j < tot) {
        const long long sm = j / per, k = j - sm * per;
        const long long i = sm * NP + lo + k;
        const float r = Y[lo + k] - F[i];
        const float z = r * inv;
        if (BWD) {
          dF[i] = coef * r;
          acc4 += z * z - 1.f;
        } else {
          acc4 += z * z;
          ++cnt;
        }
      }
    }
    acc += BWD ? (double)acc4 : -0.5 * (double)acc4 + cst * cnt;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[(long long)v * nb + blockIdx.x] = acc;
}

// loglik_w_kernel over the observed entries: part[v * nb + block] = sum of z^2 over the block's share of view v (both
// directions; the counts join in the closings); BWD also writes dF = -gloss w_v (Y - F) / (s^2 S), exactly 0 at a missing
// entry.  w == nullptr: every view weighs 1.  F [S, N, P], Y [N, P], grid (nb, V)
template <bool BWD>
__global__ void __launch_bounds__(256)
loglik_skip_kernel(const float* __restrict__ F, const float* __restrict__ Y, const float* __restrict__ noise_u, int S,
                   long long NP, int P, ViewRows vr, const double* __restrict__ w, const float* __restrict__ gloss,
                   float* __restrict__ dF, double* __restrict__ part) {
  __shared__ double red[4];
  const int v = blockIdx.y, nb = gridDim.x;
  const long long lo = vr.off[v] * P, per = (vr.off[v + 1] - vr.off[v]) * P, tot = per * S;
  const double s = exp((double)noise_u[0]) + 1e-5;  // "variance" used as std
  const float inv = (float)(1.0 / s);
  const double wv = w != nullptr ? w[v] : 1.0;
  const float coef = BWD ? (float)(-(double)gloss[0] * wv / (s * s * (double)S)) : 0.f;
  double acc = 0.0;
  for (long long i0 = blockIdx.x * 256LL * 4; i0 < tot; i0 += (long long)nb * 256 * 4) {
    float acc4 = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long j = i0 + u * 256 + threadIdx.x;
      if (j < tot) {
        const long long sm = j / per, k = j - sm * per;
        const long long i = sm * NP + lo + k;
        const float y = Y[lo + k];
        const float r = (y == y) ? y - F[i] : 0.f;
        const float z = r * inv;
        if (BWD) dF[i] = coef * r;
        acc4 += z * z;
      }
    }
    acc += (double)acc4;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[(long long)v * nb + blockIdx.x] = acc;
}

// thread 0, views in order, fp64:  nobs == nullptr: sum_v w_v t_v with t_v = sum_b part[v * nb + b];  otherwise
// sum_v w_v (A t_v + B S nobs[v]) with w == nullptr as weights of 1, where a view without an observed entry adds exactly 0
// whatever A and B are (no 0 * log)
__device__ double view_total(const double* __restrict__ part, int V, int nb, const double* __restrict__ w,
                             const double* __restrict__ nobs, int S, double A, double B, double* red) {
  double tot = 0.0;
  for (int v = 0; v < V; ++v) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) s += part[(long long)v * nb + b];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
      if (nobs == nullptr)
        tot += w[v] * s;
      else if (nobs[v] > 0.0)
        tot += (w != nullptr ? w[v] : 1.0) * (A * s + B * (double)S * nobs[v]);
    }
    __syncthreads();
  }
  return tot;
}

struct ViewFinishArgs {
  const double* part[GPSA_MAX_MODS];   // [V][nb] partials (a fused term: V = 1, its nparts partial sums of z^2)
  const double* w[GPSA_MAX_MODS];      // [V]; with counts: or nullptr (= 1)
  const double* nobs[GPSA_MAX_MODS];   // [V] observed entries of Y per view, or nullptr: the partials are whole LL sums
  const float* noise_u[GPSA_MAX_MODS];  // (read with counts only)
  int V[GPSA_MAX_MODS], nb[GPSA_MAX_MODS], S[GPSA_MAX_MODS];
  int n_ll, n_kl;
  const double* kl;
  double kl_scale;
  double* ll;
  float* loss;
};
// ll[i] = sum_v w_v LL_{i,v} / S_i, with counts LL_{i,v} = -sum z^2 / 2 + (-log s - log(2 pi) / 2) S nobs_v;
// loss = kl_scale sum(kl) - sum_i ll[i]
__global__ void __launch_bounds__(256) elbo_views_finish_kernel(ViewFinishArgs a) {
  __shared__ double red[4];
  double lsum = 0.0;
  for (int i = 0; i < a.n_ll; ++i) {
    double B = 0.0;
    if (a.nobs[i] != nullptr) {
      const double sd = exp((double)a.noise_u[i][0]) + 1e-5;
      B = -log(sd) - 0.9189385332046727;
    }
    const double s = view_total(a.part[i], a.V[i], a.nb[i], a.w[i], a.nobs[i], a.S[i], -0.5, B, red);
    if (threadIdx.x == 0) {
      const double v = s / (double)a.S[i];
      a.ll[i] = v;
      lsum += v;
    }
  }
  double k = 0.0;
  for (int t = threadIdx.x; t < a.n_kl; t += 256) k += a.kl[t];
  k = block_sum(k, red);
  if (threadIdx.x == 0) a.loss[0] = (float)(a.kl_scale * k - lsum);
}

// dnoise_u = -gloss sum_v w_v (sum z^2 - 1)_v / s / S exp(noise_u)  (with counts: sum z^2 - S nobs_v); the first term
// also zero-fills the whole noise gradient first and writes dkl = kl_scale gloss
__global__ void __launch_bounds__(256)
loglik_views_bwd_finish_kernel(const double* __restrict__ part, int V, int nb, const double* __restrict__ w,
                               const double* __restrict__ nobs, const float* __restrict__ noise_u, int S,
                               float* __restrict__ dnoise_u, const float* __restrict__ gloss, double* __restrict__ dkl,
                               int n_kl, double kl_scale, float* __restrict__ zero_base, int zero_n) {
  __shared__ double red[4];
  if (zero_base != nullptr) {
    for (int t = threadIdx.x; t < zero_n; t += blockDim.x) zero_base[t] = 0.f;
    __syncthreads();
  }
  const double s = view_total(part, V, nb, w, nobs, S, 1.0, -1.0, red);
  if (threadIdx.x == 0) {
    const double e = exp((double)noise_u[0]), sc = e + 1e-5;
    dnoise_u[0] = (float)(-(double)gloss[0] * s / sc / (double)S * e);
  }
  if (dkl != nullptr)
    for (int t = threadIdx.x; t < n_kl; t += blockDim.x) dkl[t] = kl_scale * (double)gloss[0];
}

// blocks per view: enough for the largest view, at most 4096 partials per term in all
static inline int view_blocks(int S, const ViewRows& vr, int V, int P) {
  long long most = 0;
  for (int v = 0; v < V; ++v) {
    const long long t = (vr.off[v + 1] - vr.off[v]) * P * (long long)S;
    if (t > most) most = t;
  }
  long long b = cdiv(most, 1024);
  const long long cap = 4096 / V;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// the skip pair's tables, checked before any launch: a term is either fused (zpart[i], one view, no weights of its own:
// the fused kernels sum z^2 over all rows) or comes from its draws, with the caller's views or as one view
static int skip_args_check(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                           const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                           const int* n_views, const long long* const* view_off, const double* const* w,
                           const double* const* nobs, long long workspace_bytes) {
  if (!nobs) return GPSA_EINVAL;
  if ((n_views == nullptr) != (view_off == nullptr) || (w != nullptr && n_views == nullptr)) return GPSA_EINVAL;
  if (int rc = elbo_loss_args_check(n_ll, F, Y, noise_u, S, N, P, workspace_bytes)) return rc;
  for (int i = 0; i < n_ll; ++i) {
    if (!nobs[i] || !noise_u[i]) return GPSA_EINVAL;
    const bool fused = zpart && zpart[i];
    if (fused && (nparts < 1 || (n_views && n_views[i] != 1))) return GPSA_EINVAL;
    if (!fused && (!F[i] || !Y[i])) return GPSA_EINVAL;
    if (n_views && !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
    if (w && !w[i]) return GPSA_EINVAL;
  }
  return 0;
}
// ... and the weighted pair's: views and weights for every term
static int weighted_args_check(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                               const int* S, const long long* N, const int* P, const int* n_views,
                               const long long* const* view_off, const double* const* w, long long workspace_bytes) {
  if (int rc = elbo_loss_args_check(n_ll, F, Y, noise_u, S, N, P, workspace_bytes)) return rc;
  for (int i = 0; i < n_ll; ++i)
    if (!w[i] || !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
  return 0;
}

// Both directions take checked arguments.  nobs == nullptr: the weighted closing (loglik_w_kernel; views and weights for
// every term, no fused term); otherwise the skip closing (loglik_skip_kernel; zpart, n_views / view_off and w may each be
// nullptr).  Term i's block partials go to its own slot of the workspace; a fused term brings its partials and launches
// nothing here.
static int views_fwd_impl(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                          const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                          const int* n_views, const long long* const* view_off, const double* const* w,
                          const double* const* nobs, const double* kl, int n_kl, double kl_scale, float* loss,
                          double* ll_out, void* workspace, void* stream) {
  hipStream_t st = as_stream(stream);
  const auto kernel = nobs ? loglik_skip_kernel<false> : loglik_w_kernel<false>;
  ViewFinishArgs a = {};
  a.n_ll = n_ll;
  a.n_kl = kl ? n_kl : 0;
  a.kl = kl;
  a.kl_scale = kl_scale;
  a.ll = ll_out;
  a.loss = loss;
  for (int i = 0; i < n_ll; ++i) {
    a.w[i] = w ? w[i] : nullptr;
    a.nobs[i] = nobs ? nobs[i] : nullptr;
    a.noise_u[i] = noise_u[i];
    a.S[i] = S[i];
    if (zpart && zpart[i]) {
      a.part[i] = zpart[i];
      a.V[i] = 1;
      a.nb[i] = nparts;
      continue;
    }
    const int V = n_views ? n_views[i] : 1;
    const ViewRows vr = view_rows(N[i], V, view_off ? view_off[i] : nullptr);
    const int nb = view_blocks(S[i], vr, V, P[i]);
    double* part = reinterpret_cast<double*>(workspace) + LL_SLOT_DOUBLES * i;
    kernel<<<dim3(nb, V), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], vr, a.w[i], nullptr, nullptr,
                                        part);
    a.part[i] = part;
    a.V[i] = V;
    a.nb[i] = nb;
  }
  elbo_views_finish_kernel<<<1, 256, 0, st>>>(a);
  GPSA_LAUNCH_CHECK();
  return 0;
}

static int views_bwd_impl(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                          const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                          const int* n_views, const long long* const* view_off, const double* const* w,
                          const double* const* nobs, const float* gloss, int n_kl, double kl_scale, float* const* dF,
                          float* const* dnoise, float* dnoise_all, int n_noise, double* dkl, void* workspace,
                          void* stream) {
  hipStream_t st = as_stream(stream);
  const auto kernel = nobs ? loglik_skip_kernel<true> : loglik_w_kernel<true>;
  for (int i = 0; i < n_ll; ++i) {
    const double* wi = w ? w[i] : nullptr;
    const double* part = zpart ? zpart[i] : nullptr;
    int V = 1, nb = nparts;
    if (part == nullptr) {
      V = n_views ? n_views[i] : 1;
      const ViewRows vr = view_rows(N[i], V, view_off ? view_off[i] : nullptr);
      nb = view_blocks(S[i], vr, V, P[i]);
      double* slot = reinterpret_cast<double*>(workspace) + LL_SLOT_DOUBLES * i;
      kernel<<<dim3(nb, V), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], vr, wi, gloss, dF[i], slot);
      part = slot;
    }
    // the first term's finishing launch also zero-fills the noise gradient and writes dkl
    loglik_views_bwd_finish_kernel<<<1, 256, 0, st>>>(part, V, nb, wi, nobs ? nobs[i] : nullptr, noise_u[i], S[i],
                                                      dnoise[i], gloss, i == 0 ? dkl : nullptr, n_kl, kl_scale,
                                                      i == 0 ? dnoise_all : nullptr, n_noise);
  }
  GPSA_LAUNCH_CHECK();
  return 0;
}

// ---- the closing with Poisson terms (gpsa_elbo_loss_pois_fwd / _bwd; the per-element kernel is poisson.hip's) --------
// A Gaussian term in such a call is closed by the code above (view_total, loglik_views_bwd_finish_kernel, the two
// per-element kernels); a Poisson term's partials sum y eta - exp(eta), and its constant is the lgamma table.
struct PoisFinishArgs {
  ViewFinishArgs g;                    // every term's tables; a Poisson term's nobs / noise_u are not read
  int kind[GPSA_MAX_MODS];             // GPSA_LIK_*
  const double* lgam[GPSA_MAX_MODS];   // [V] sum of lgamma(y + 1) per view (Poisson terms)
};
// elbo_views_finish_kernel with  ll[i] = sum_v w_v (t_v / S_i - lgam_v)  for a Poisson term (t_v: its view's partials)
__global__ void __launch_bounds__(256) elbo_pois_finish_kernel(PoisFinishArgs p) {
  __shared__ double red[4];
  const ViewFinishArgs& a = p.g;
  double lsum = 0.0;
  for (int i = 0; i < a.n_ll; ++i) {
    if (p.kind[i] == GPSA_LIK_POISSON) {
      double tot = 0.0;
      for (int v = 0; v < a.V[i]; ++v) {
        double s = 0.0;
        for (int b = threadIdx.x; b < a.nb[i]; b += blockDim.x) s += a.part[i][(long long)v * a.nb[i] + b];
        s = block_sum(s, red);
        if (threadIdx.x == 0) tot += (a.w[i] != nullptr ? a.w[i][v] : 1.0) * (s / (double)a.S[i] - p.lgam[i][v]);
        __syncthreads();
      }
      if (threadIdx.x == 0) {
        a.ll[i] = tot;
        lsum += tot;
      }
      continue;
    }
    double B = 0.0;
    if (a.nobs[i] != nullptr) {
      const double sd = exp((double)a.noise_u[i][0]) + 1e-5;
      B = -log(sd) - 0.9189385332046727;
    }
    const double s = view_total(a.part[i], a.V[i], a.nb[i], a.w[i], a.nobs[i], a.S[i], -0.5, B, red);
    if (threadIdx.x == 0) {
      const double v = s / (double)a.S[i];
      a.ll[i] = v;
      lsum += v;
    }
  }
  double k = 0.0;
  for (int t = threadIdx.x; t < a.n_kl; t += 256) k += a.kl[t];
  k = block_sum(k, red);
  if (threadIdx.x == 0) a.loss[0] = (float)(a.kl_scale * k - lsum);
}
// a Poisson term's share of the backward's closing: its noise gradient is exactly 0; as the first term it also zero-fills
// the whole noise gradient and writes dkl = kl_scale gloss (what loglik_views_bwd_finish_kernel does for a Gaussian one)
__global__ void __launch_bounds__(256)
pois_bwd_finish_kernel(float* __restrict__ dnoise_u, const float* __restrict__ gloss, double* __restrict__ dkl, int n_kl,
                       double kl_scale, float* __restrict__ zero_base, int zero_n) {
  if (zero_base != nullptr) {
    for (int t = threadIdx.x; t < zero_n; t += blockDim.x) zero_base[t] = 0.f;
    __syncthreads();
  }
  if (threadIdx.x == 0) dnoise_u[0] = 0.f;
  if (dkl != nullptr)
    for (int t = threadIdx.x; t < n_kl; t += blockDim.x) dkl[t] = kl_scale * (double)gloss[0];
}

// the pair's tables, checked before any launch (the header states the rules per kind)
static int pois_args_check(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                           const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                           const int* n_views, const long long* const* view_off, const double* const* w,
                           const double* const* nobs, const int* kind, const double* const* lgam, int skip,
                           long long workspace_bytes) {
  if (!kind || !lgam) return GPSA_EINVAL;
  if ((n_views == nullptr) != (view_off == nullptr) || (w != nullptr && n_views == nullptr)) return GPSA_EINVAL;
  if (int rc = elbo_loss_args_check(n_ll, F, Y, noise_u, S, N, P, workspace_bytes)) return rc;
  for (int i = 0; i < n_ll; ++i) {
    const bool fused = zpart && zpart[i];
    if (fused && (nparts < 1 || (n_views && n_views[i] != 1))) return GPSA_EINVAL;
    if (!fused && (!F[i] || !Y[i])) return GPSA_EINVAL;
    if (n_views && !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
    if (kind[i] == GPSA_LIK_POISSON) {
      if (!lgam[i]) return GPSA_EINVAL;
    } else if (kind[i] == GPSA_LIK_GAUSSIAN) {
      if (!noise_u[i]) return GPSA_EINVAL;
      if (nobs && nobs[i]) {  // the skip closing's arithmetic
        if (!fused && !skip) return GPSA_EINVAL;
      } else {  // the weighted closing's
        if (fused || skip || !n_views || !w || !w[i]) return GPSA_EINVAL;
      }
    } else {
      return GPSA_EINVAL;
    }
  }
  return 0;
}

// term i's views, blocks and workspace slot, as views_fwd_impl / views_bwd_impl lay them out
struct PoisTerm {
  ViewRows vr;
  int V, nb;
  double* slot;
};
static PoisTerm pois_term(int i, const int* S, const long long* N, const int* P, const int* n_views,
                          const long long* const* view_off, void* workspace) {
  PoisTerm t;
  t.V = n_views ? n_views[i] : 1;
  t.vr = view_rows(N[i], t.V, view_off ? view_off[i] : nullptr);
  t.nb = view_blocks(S[i], t.vr, t.V, P[i]);
  t.slot = reinterpret_cast<double*>(workspace) + LL_SLOT_DOUBLES * i;
  return t;
}

static int pois_fwd_impl(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                         const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                         const int* n_views, const long long* const* view_off, const double* const* w,
                         const double* const* nobs, const int* kind, const double* const* lgam,
                         const float* const* log_offset, int skip, const double* kl, int n_kl, double kl_scale,
                         float* loss, double* ll_out, void* workspace, void* stream) {
  hipStream_t st = as_stream(stream);
  PoisFinishArgs p = {};
  ViewFinishArgs& a = p.g;
  a.n_ll = n_ll;
  a.n_kl = kl ? n_kl : 0;
  a.kl = kl;
  a.kl_scale = kl_scale;
  a.ll = ll_out;
  a.loss = loss;
  for (int i = 0; i < n_ll; ++i) {
    const bool pois = kind[i] == GPSA_LIK_POISSON;
    p.kind[i] = kind[i];
    p.lgam[i] = lgam[i];
    a.w[i] = w ? w[i] : nullptr;
    a.nobs[i] = (!pois && nobs) ? nobs[i] : nullptr;
    a.noise_u[i] = noise_u[i];
    a.S[i] = S[i];
    if (zpart && zpart[i]) {
      a.part[i] = zpart[i];
      a.V[i] = 1;
      a.nb[i] = nparts;
      continue;
    }
    const PoisTerm t = pois_term(i, S, N, P, n_views, view_off, workspace);
    if (pois) {
      if (int rc = pois_loglik_launch(false, F[i], Y[i], log_offset ? log_offset[i] : nullptr, S[i], N[i], P[i], t.vr,
                                      t.V, t.nb, a.w[i], nullptr, skip, nullptr, t.slot, st))
        return rc;
    } else {
      const auto kernel = a.nobs[i] ? loglik_skip_kernel<false> : loglik_w_kernel<false>;
      kernel<<<dim3(t.nb, t.V), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], t.vr, a.w[i], nullptr,
                                              nullptr, t.slot);
    }
    a.part[i] = t.slot;
    a.V[i] = t.V;
    a.nb[i] = t.nb;
  }
  elbo_pois_finish_kernel<<<1, 256, 0, st>>>(p);
  GPSA_LAUNCH_CHECK();
  return 0;
}

static int pois_bwd_impl(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                         const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                         const int* n_views, const long long* const* view_off, const double* const* w,
                         const double* const* nobs, const int* kind, const float* const* log_offset, int skip,
                         const float* gloss, int n_kl, double kl_scale, float* const* dF, float* const* dnoise,
                         float* dnoise_all, int n_noise, double* dkl, void* workspace, void* stream) {
  hipStream_t st = as_stream(stream);
  for (int i = 0; i < n_ll; ++i) {
    const bool pois = kind[i] == GPSA_LIK_POISSON;
    const double* wi = w ? w[i] : nullptr;
    const double* ni = (!pois && nobs) ? nobs[i] : nullptr;
    const double* part = zpart ? zpart[i] : nullptr;
    int V = 1, nb = nparts;
    if (part == nullptr) {
      const PoisTerm t = pois_term(i, S, N, P, n_views, view_off, workspace);
      V = t.V, nb = t.nb;
      if (pois) {
        if (int rc = pois_loglik_launch(true, F[i], Y[i], log_offset ? log_offset[i] : nullptr, S[i], N[i], P[i], t.vr,
                                        V, nb, wi, gloss, skip, dF[i], t.slot, st))
          return rc;
      } else {
        const auto kernel = ni ? loglik_skip_kernel<true> : loglik_w_kernel<true>;
        kernel<<<dim3(nb, V), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], t.vr, wi, gloss, dF[i],
                                            t.slot);
      }
      part = t.slot;
    }
    // the first term's finishing launch also zero-fills the noise gradient and writes dkl
    if (pois)
      pois_bwd_finish_kernel<<<1, 256, 0, st>>>(dnoise[i], gloss, i == 0 ? dkl : nullptr, n_kl, kl_scale,
                                                i == 0 ? dnoise_all : nullptr, n_noise);
    else
      loglik_views_bwd_finish_kernel<<<1, 256, 0, st>>>(part, V, nb, wi, ni, noise_u[i], S[i], dnoise[i], gloss,
                                                        i == 0 ? dkl : nullptr, n_kl, kl_scale,
                                                        i == 0 ? dnoise_all : nullptr, n_noise);
  }
  GPSA_LAUNCH_CHECK();
  return 0;
}

// ---- the closing with negative binomial terms (gpsa_elbo_loss_nb_fwd / _bwd; the per-element kernels are negbin.hip's) ---
// Gaussian and Poisson terms in such a call go through the very launches of the Poisson closing above; an NB term's
// partials sum t = y a - (y + r) softplus(a), its constants are gpsa_nb_const's table minus the lgamma table, and its
// backward also closes the per-output sums of u into the gradient of rho (nb_ddisp_launch).
struct NbFinishArgs {
  PoisFinishArgs p;
  const double* csum[GPSA_MAX_MODS];   // [V] sum of lgamma(y + r) - lgamma(r) per view (NB terms)
};
// elbo_pois_finish_kernel with  ll[i] = sum_v w_v (t_v / S_i + csum_v - lgam_v)  for an NB term
__global__ void __launch_bounds__(256) elbo_nb_finish_kernel(NbFinishArgs n) {
  __shared__ double red[4];
  const ViewFinishArgs& a = n.p.g;
  double lsum = 0.0;
  for (int i = 0; i < a.n_ll; ++i) {
    const int kind = n.p.kind[i];
    if (kind != GPSA_LIK_GAUSSIAN) {
      double tot = 0.0;
      for (int v = 0; v < a.V[i]; ++v) {
        double s = 0.0;
        for (int b = threadIdx.x; b < a.nb[i]; b += blockDim.x) s += a.part[i][(long long)v * a.nb[i] + b];
        s = block_sum(s, red);
        if (threadIdx.x == 0) {
          const double wv = a.w[i] != nullptr ? a.w[i][v] : 1.0;
          if (kind == GPSA_LIK_NEGBIN)
            tot += wv * (s / (double)a.S[i] + (n.csum[i][v] - n.p.lgam[i][v]));
          else
            tot += wv * (s / (double)a.S[i] - n.p.lgam[i][v]);
        }
        __syncthreads();
      }
      if (threadIdx.x == 0) {
        a.ll[i] = tot;
        lsum += tot;
      }
      continue;
    }
    double B = 0.0;
    if (a.nobs[i] != nullptr) {
      const double sd = exp((double)a.noise_u[i][0]) + 1e-5;
      B = -log(sd) - 0.9189385332046727;
    }
    const double s = view_total(a.part[i], a.V[i], a.nb[i], a.w[i], a.nobs[i], a.S[i], -0.5, B, red);
    if (threadIdx.x == 0) {
      const double v = s / (double)a.S[i];
      a.ll[i] = v;
      lsum += v;
    }
  }
  double k = 0.0;
  for (int t = threadIdx.x; t < a.n_kl; t += 256) k += a.kl[t];
  k = block_sum(k, red);
  if (threadIdx.x == 0) a.loss[0] = (float)(a.kl_scale * k - lsum);
}

// doubles of term i's [V][nrb][P] column partials of u, sized for views of up to N rows (the launch's nrb is no larger)
static long long nb_upart_doubles(int S, long long N, int P, int V) {
  return (long long)V * nb_grid((long long)S * N, V, P).nrb * P;
}
// (kind == nullptr: every term counted as negative binomial; otherwise only the NB terms have column partials)
static long long nb_loss_workspace(int n_ll, const int* S, const long long* N, const int* P, const int* n_views,
                                   const int* kind) {
  long long d = LL_SLOT_DOUBLES * n_ll;
  for (int i = 0; i < n_ll; ++i)
    if (!kind || kind[i] == GPSA_LIK_NEGBIN) d += nb_upart_doubles(S[i], N[i], P[i], n_views ? n_views[i] : 1);
  return 8 * d;
}

// the pair's tables, checked before any launch: pois_args_check's rules for the Gaussian and Poisson terms, and for an NB
// term its lgamma table, rho and the table of gpsa_nb_const that the direction reads (csum / dconst)
static int nb_args_check(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                         const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                         const int* n_views, const long long* const* view_off, const double* const* w,
                         const double* const* nobs, const int* kind, const double* const* lgam,
                         const float* const* log_disp, const double* const* nbc, int skip, long long workspace_bytes) {
  if (!kind || !lgam || !log_disp || !nbc) return GPSA_EINVAL;
  if ((n_views == nullptr) != (view_off == nullptr) || (w != nullptr && n_views == nullptr)) return GPSA_EINVAL;
  if (int rc = elbo_loss_args_check(n_ll, F, Y, noise_u, S, N, P, workspace_bytes)) return rc;
  for (int i = 0; i < n_ll; ++i) {
    const bool fused = zpart && zpart[i];
    if (fused && (nparts < 1 || (n_views && n_views[i] != 1))) return GPSA_EINVAL;
    if (!fused && (!F[i] || !Y[i])) return GPSA_EINVAL;
    if (n_views && !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
    if (kind[i] == GPSA_LIK_NEGBIN) {
      if (!lgam[i] || !log_disp[i] || !nbc[i]) return GPSA_EINVAL;
    } else if (kind[i] == GPSA_LIK_POISSON) {
      if (!lgam[i]) return GPSA_EINVAL;
    } else if (kind[i] == GPSA_LIK_GAUSSIAN) {
      if (!noise_u[i]) return GPSA_EINVAL;
      if (nobs && nobs[i]) {  // the skip closing's arithmetic
        if (!fused && !skip) return GPSA_EINVAL;
      } else {  // the weighted closing's
        if (fused || skip || !n_views || !w || !w[i]) return GPSA_EINVAL;
      }
    } else {
      return GPSA_EINVAL;
    }
  }
  if (workspace_bytes < nb_loss_workspace(n_ll, S, N, P, n_views, kind)) return GPSA_EWORKSPACE;
  return 0;
}

// an NB term's grid: the column reduction over its largest view's S * rows
static NbGrid nb_term_grid(int S, const ViewRows& vr, int V, int P) {
  long long most = 0;
  for (int v = 0; v < V; ++v)
    if (vr.off[v + 1] - vr.off[v] > most) most = vr.off[v + 1] - vr.off[v];
  return nb_grid(most * S, V, P);
}

static int nb_fwd_impl(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u, const int* S,
                       const long long* N, const int* P, const double* const* zpart, int nparts, const int* n_views,
                       const long long* const* view_off, const double* const* w, const double* const* nobs,
                       const int* kind, const double* const* lgam, const float* const* log_offset,
                       const float* const* log_disp, const double* const* csum, int skip, const double* kl, int n_kl,
                       double kl_scale, float* loss, double* ll_out, void* workspace, void* stream) {
  hipStream_t st = as_stream(stream);
  NbFinishArgs n = {};
  ViewFinishArgs& a = n.p.g;
  a.n_ll = n_ll;
  a.n_kl = kl ? n_kl : 0;
  a.kl = kl;
  a.kl_scale = kl_scale;
  a.ll = ll_out;
  a.loss = loss;
  for (int i = 0; i < n_ll; ++i) {
    const bool gauss = kind[i] == GPSA_LIK_GAUSSIAN;
    n.p.kind[i] = kind[i];
    n.p.lgam[i] = lgam[i];
    n.csum[i] = csum[i];
    a.w[i] = w ? w[i] : nullptr;
    a.nobs[i] = (gauss && nobs) ? nobs[i] : nullptr;
    a.noise_u[i] = noise_u[i];
    a.S[i] = S[i];
    if (zpart && zpart[i]) {
      a.part[i] = zpart[i];
      a.V[i] = 1;
      a.nb[i] = nparts;
      continue;
    }
    const PoisTerm t = pois_term(i, S, N, P, n_views, view_off, workspace);
    const float* off = log_offset ? log_offset[i] : nullptr;
    a.part[i] = t.slot;
    a.V[i] = t.V;
    a.nb[i] = t.nb;
    if (kind[i] == GPSA_LIK_NEGBIN) {
      const NbGrid g = nb_term_grid(S[i], t.vr, t.V, P[i]);
      if (int rc = nb_loglik_launch(false, F[i], Y[i], off, log_disp[i], S[i], N[i], P[i], t.vr, t.V, g, a.w[i], nullptr,
                                    skip, nullptr, t.slot, nullptr, st))
        return rc;
      a.nb[i] = g.nb();
    } else if (kind[i] == GPSA_LIK_POISSON) {
      if (int rc = pois_loglik_launch(false, F[i], Y[i], off, S[i], N[i], P[i], t.vr, t.V, t.nb, a.w[i], nullptr, skip,
                                      nullptr, t.slot, st))
        return rc;
    } else {
      const auto kernel = a.nobs[i] ? loglik_skip_kernel<false> : loglik_w_kernel<false>;
      kernel<<<dim3(t.nb, t.V), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], t.vr, a.w[i], nullptr,
                                              nullptr, t.slot);
    }
  }
  elbo_nb_finish_kernel<<<1, 256, 0, st>>>(n);
  GPSA_LAUNCH_CHECK();
  return 0;
}

static int nb_bwd_impl(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u, const int* S,
                       const long long* N, const int* P, const double* const* zpart, int nparts, const int* n_views,
                       const long long* const* view_off, const double* const* w, const double* const* nobs,
                       const int* kind, const float* const* log_offset, const float* const* log_disp,
                       const double* const* dconst, const double* const* usum, int skip, const float* gloss, int n_kl,
                       double kl_scale, float* const* dF, float* const* dnoise, float* dnoise_all, int n_noise,
                       double* dkl, float* const* ddisp, void* workspace, void* stream) {
  hipStream_t st = as_stream(stream);
  double* up = reinterpret_cast<double*>(workspace) + LL_SLOT_DOUBLES * n_ll;  // the terms' column partials of u, in order
  for (int i = 0; i < n_ll; ++i) {
    const bool gauss = kind[i] == GPSA_LIK_GAUSSIAN;
    const double* wi = w ? w[i] : nullptr;
    const double* ni = (gauss && nobs) ? nobs[i] : nullptr;
    const double* part = zpart ? zpart[i] : nullptr;
    const float* off = log_offset ? log_offset[i] : nullptr;
    double* upart = up;
    if (kind[i] == GPSA_LIK_NEGBIN) up += nb_upart_doubles(S[i], N[i], P[i], n_views ? n_views[i] : 1);
    int V = 1, nb = nparts;
    if (part == nullptr) {
      const PoisTerm t = pois_term(i, S, N, P, n_views, view_off, workspace);
      V = t.V, nb = t.nb;
      if (kind[i] == GPSA_LIK_NEGBIN) {
        const NbGrid g = nb_term_grid(S[i], t.vr, V, P[i]);
        if (int rc = nb_loglik_launch(true, F[i], Y[i], off, log_disp[i], S[i], N[i], P[i], t.vr, V, g, wi, gloss, skip,
                                      dF[i], nullptr, upart, st))
          return rc;
        if (int rc = nb_ddisp_launch(upart, V, g.nrb, P[i], wi, S[i], dconst[i], gloss, ddisp[i], st)) return rc;
      } else if (kind[i] == GPSA_LIK_POISSON) {
        if (int rc = pois_loglik_launch(true, F[i], Y[i], off, S[i], N[i], P[i], t.vr, V, nb, wi, gloss, skip, dF[i],
                                        t.slot, st))
          return rc;
      } else {
        const auto kernel = ni ? loglik_skip_kernel<true> : loglik_w_kernel<true>;
        kernel<<<dim3(nb, V), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], t.vr, wi, gloss, dF[i],
                                            t.slot);
      }
      part = t.slot;
    } else if (kind[i] == GPSA_LIK_NEGBIN) {
      if (int rc = nb_ddisp_launch(usum[i], 1, 1, P[i], wi, S[i], dconst[i], gloss, ddisp[i], st)) return rc;
    }
    // the first term's finishing launch also zero-fills the noise gradient and writes dkl
    if (!gauss)
      pois_bwd_finish_kernel<<<1, 256, 0, st>>>(dnoise[i], gloss, i == 0 ? dkl : nullptr, n_kl, kl_scale,
                                                i == 0 ? dnoise_all : nullptr, n_noise);
    else
      loglik_views_bwd_finish_kernel<<<1, 256, 0, st>>>(part, V, nb, wi, ni, noise_u[i], S[i], dnoise[i], gloss,
                                                        i == 0 ? dkl : nullptr, n_kl, kl_scale,
                                                        i == 0 ? dnoise_all : nullptr, n_noise);
  }
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // namespace gpsa

extern "C" {

long long gpsa_elbo_loss_nb_workspace(int n_ll, const int* S, const long long* N, const int* P, const int* n_views,
                                      const int* kind) {
  using namespace gpsa;
  if (n_ll < 1 || n_ll > GPSA_MAX_MODS || !S || !N || !P) return 0;
  for (int i = 0; i < n_ll; ++i)
    if (S[i] < 1 || N[i] < 1 || P[i] < 1 || (n_views && (n_views[i] < 1 || n_views[i] > LOSS_MAX_VIEWS))) return 0;
  return nb_loss_workspace(n_ll, S, N, P, n_views, kind);
}

int gpsa_elbo_loss_nb_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                          const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                          const int* n_views, const long long* const* view_off, const double* const* w,
                          const double* const* nobs, const int* kind, const double* const* lgam,
                          const float* const* log_offset, const float* const* log_disp, const double* const* csum,
                          int skip, const double* kl, int n_kl, double kl_scale, float* loss, double* ll_out,
                          void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!loss || !ll_out || !workspace) return GPSA_EINVAL;
  if (int rc = nb_args_check(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kind, lgam, log_disp,
                             csum, skip, workspace_bytes))
    return rc;
  return nb_fwd_impl(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kind, lgam, log_offset,
                     log_disp, csum, skip, kl, n_kl, kl_scale, loss, ll_out, workspace, stream);
}

int gpsa_elbo_loss_nb_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                          const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                          const int* n_views, const long long* const* view_off, const double* const* w,
                          const double* const* nobs, const int* kind, const double* const* lgam,
                          const float* const* log_offset, const float* const* log_disp, const double* const* dconst,
                          const double* const* usum, int skip, const float* gloss, int n_kl, double kl_scale,
                          float* const* dF, float* const* dnoise, float* dnoise_all, int n_noise, double* dkl,
                          float* const* ddisp, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!gloss || !dF || !dnoise || !ddisp || !workspace) return GPSA_EINVAL;
  if (int rc = nb_args_check(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kind, lgam, log_disp,
                             dconst, skip, workspace_bytes))
    return rc;
  for (int i = 0; i < n_ll; ++i) {
    const bool fused = zpart && zpart[i];
    if (!dnoise[i] || (!fused && !dF[i])) return GPSA_EINVAL;
    if (kind[i] == GPSA_LIK_NEGBIN && (!ddisp[i] || (fused && (!usum || !usum[i])))) return GPSA_EINVAL;
  }
  return nb_bwd_impl(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kind, log_offset, log_disp,
                     dconst, usum, skip, gloss, n_kl, kl_scale, dF, dnoise, dnoise_all, n_noise, dkl, ddisp, workspace,
                     stream);
}

int gpsa_elbo_loss_pois_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                            const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                            const int* n_views, const long long* const* view_off, const double* const* w,
                            const double* const* nobs, const int* kind, const double* const* lgam,
                            const float* const* log_offset, int skip, const double* kl, int n_kl, double kl_scale,
                            float* loss, double* ll_out, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!loss || !ll_out) return GPSA_EINVAL;
  if (int rc = pois_args_check(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kind, lgam, skip,
                               workspace_bytes))
    return rc;
  return pois_fwd_impl(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kind, lgam, log_offset,
                       skip, kl, n_kl, kl_scale, loss, ll_out, workspace, stream);
}

int gpsa_elbo_loss_pois_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                            const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                            const int* n_views, const long long* const* view_off, const double* const* w,
                            const double* const* nobs, const int* kind, const double* const* lgam,
                            const float* const* log_offset, int skip, const float* gloss, int n_kl, double kl_scale,
                            float* const* dF, float* const* dnoise, float* dnoise_all, int n_noise, double* dkl,
                            void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!gloss || !dF || !dnoise) return GPSA_EINVAL;
  if (int rc = pois_args_check(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kind, lgam, skip,
                               workspace_bytes))
    return rc;
  for (int i = 0; i < n_ll; ++i)
    if (!dnoise[i] || (!(zpart && zpart[i]) && !dF[i])) return GPSA_EINVAL;
  return pois_bwd_impl(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kind, log_offset, skip,
                       gloss, n_kl, kl_scale, dF, dnoise, dnoise_all, n_noise, dkl, workspace, stream);
}

int gpsa_elbo_loss_weighted_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                                const int* S, const long long* N, const int* P, const int* n_views,
                                const long long* const* view_off, const double* const* w, const double* kl, int n_kl,
                                double kl_scale, float* loss, double* ll_out, void* workspace,
                                long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!n_views || !view_off || !w || !loss || !ll_out) return GPSA_EINVAL;
  if (int rc = weighted_args_check(n_ll, F, Y, noise_u, S, N, P, n_views, view_off, w, workspace_bytes)) return rc;
  return views_fwd_impl(n_ll, F, Y, noise_u, S, N, P, nullptr, 0, n_views, view_off, w, nullptr, kl, n_kl, kl_scale,
                        loss, ll_out, workspace, stream);
}

int gpsa_elbo_loss_weighted_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                                const int* S, const long long* N, const int* P, const int* n_views,
                                const long long* const* view_off, const double* const* w, const float* gloss, int n_kl,
                                double kl_scale, float* const* dF, float* const* dnoise, float* dnoise_all,
                                int n_noise, double* dkl, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!n_views || !view_off || !w || !gloss || !dF || !dnoise) return GPSA_EINVAL;
  if (int rc = weighted_args_check(n_ll, F, Y, noise_u, S, N, P, n_views, view_off, w, workspace_bytes)) return rc;
  return views_bwd_impl(n_ll, F, Y, noise_u, S, N, P, nullptr, 0, n_views, view_off, w, nullptr, gloss, n_kl, kl_scale,
                        dF, dnoise, dnoise_all, n_noise, dkl, workspace, stream);
}

int gpsa_elbo_loss_skip_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                            const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                            const int* n_views, const long long* const* view_off, const double* const* w,
                            const double* const* nobs, const double* kl, int n_kl, double kl_scale, float* loss,
                            double* ll_out, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!loss || !ll_out) return GPSA_EINVAL;
  if (int rc = skip_args_check(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, workspace_bytes))
    return rc;
  return views_fwd_impl(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, kl, n_kl, kl_scale, loss,
                        ll_out, workspace, stream);
}

int gpsa_elbo_loss_skip_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                            const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                            const int* n_views, const long long* const* view_off, const double* const* w,
                            const double* const* nobs, const float* gloss, int n_kl, double kl_scale, float* const* dF,
                            float* const* dnoise, float* dnoise_all, int n_noise, double* dkl, void* workspace,
                            long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!gloss || !dF || !dnoise) return GPSA_EINVAL;
  if (int rc = skip_args_check(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, workspace_bytes))
    return rc;
  for (int i = 0; i < n_ll; ++i)
    if (!dnoise[i] || (!(zpart && zpart[i]) && !dF[i])) return GPSA_EINVAL;
  return views_bwd_impl(n_ll, F, Y, noise_u, S, N, P, zpart, nparts, n_views, view_off, w, nobs, gloss, n_kl, kl_scale,
                        dF, dnoise, dnoise_all, n_noise, dkl, workspace, stream);
}

}  // extern "C"
