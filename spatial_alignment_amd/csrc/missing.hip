// Partly observed outputs (model.skip_missing): a NaN in Y is a missing observation and is left out of the ELBO.
//   gpsa_count_observed              the observed entries of every (term, view), as device doubles
//   gpsa_elbo_loss_skip_fwd / _bwd   the ELBO loss closings over the observed entries only: terms from draws (with or
//                                    without per-view weights) apply the select per element, fused terms arrive as partial
//                                    sums of z^2 that already left the missing entries out; the counts stand where S N P
//                                    stands in the plain closings
//   gpsa_lmc_loglik_fused_skip_f32   gpsa_lmc_loglik_fused_f32 with the select in front of its products (lmc.hip)
// (the fused ELBO pass's variant is panel_elbo_skip_kernel, qf_elbo_skip.hip.)  The test is y == y: the build has no
// fast-math flag, under which the compiler would fold it away.
#include "internal.hpp"

namespace gpsa {

constexpr int SKIP_MAX_VIEWS = 64;   // views per term (as the weighted closings)
constexpr int COUNT_MAX_SEGS = 64;   // (term, view) pairs of one counting launch (a call with more loops over them)
constexpr int COUNT_BLOCKS = 64;     // block partials per pair

struct CountArgs {
  const float* Y[COUNT_MAX_SEGS];   // first entry of the pair's rows
  long long tot[COUNT_MAX_SEGS];    // its entries (rows x P)
  double* dst[COUNT_MAX_SEGS];      // nobs[i] + v
  int n_seg;
};

// part[seg * nb + block] = observed entries in the block's share of pair seg; grid (nb, n_seg)
__global__ void __launch_bounds__(256) count_observed_kernel(CountArgs a, double* __restrict__ part) {
  __shared__ double red[4];
  const int seg = blockIdx.y, nb = gridDim.x;
  const float* __restrict__ Y = a.Y[seg];
  const long long tot = a.tot[seg];
  int cnt = 0;  // (a thread's share: at most tot / 256 / nb + 1 < 2^31 for every tot the loss kernels index)
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < tot; i += (long long)nb * 256) {
    const float y = Y[i];
    cnt += (y == y) ? 1 : 0;
  }
  const double t = block_sum((double)cnt, red);
  if (threadIdx.x == 0) part[(long long)seg * nb + blockIdx.x] = t;
}
// nobs of pair seg = its block partials in block order (fp64: exact up to 2^53); one block for all pairs
__global__ void __launch_bounds__(256) count_observed_finish_kernel(CountArgs a, const double* __restrict__ part, int nb) {
  __shared__ double red[4];
  for (int seg = 0; seg < a.n_seg; ++seg) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += part[(long long)seg * nb + b];
    s = block_sum(s, red);
    if (threadIdx.x == 0) a.dst[seg][0] = s;
    __syncthreads();
  }
}

struct SkipRows {
  long long off[SKIP_MAX_VIEWS + 1];  // view v = rows off[v] .. off[v + 1]
};

// loglik_w_kernel (minibatch.hip) over the observed entries: part[v * nb + block] = sum of z^2 over the block's share of
// view v (both directions; the counts join in the closings); BWD also writes dF = -gloss w_v (Y - F) / (s^2 S), exactly 0
// at a missing entry.  w == nullptr: every view weighs 1.  F [S, N, P], Y [N, P], grid (nb, V)
template <bool BWD>
__global__ void __launch_bounds__(256)
loglik_skip_kernel(const float* __restrict__ F, const float* __restrict__ Y, const float* __restrict__ noise_u, int S,
                   long long NP, int P, SkipRows vr, const double* __restrict__ w, const float* __restrict__ gloss,
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

struct SkipFinishArgs {
  const double* part[GPSA_MAX_MODS];   // [V][nb] sums of z^2 (a fused term: V = 1, its nparts partials)
  const double* w[GPSA_MAX_MODS];      // [V] or nullptr (= 1)
  const double* nobs[GPSA_MAX_MODS];   // [V] observed entries of Y per view
  const float* noise_u[GPSA_MAX_MODS];
  int V[GPSA_MAX_MODS], nb[GPSA_MAX_MODS], S[GPSA_MAX_MODS];
  int n_ll, n_kl;
  const double* kl;
  double kl_scale;
  double* ll;
  float* loss;
};

// thread 0: sum_v w_v (A * sum_b part[v][b] + B * S * nobs[v]), views in order; a view without an observed entry adds
// exactly 0 whatever A and B are (no 0 * log)
__device__ double skip_total(const double* __restrict__ part, int V, int nb, const double* __restrict__ w,
                             const double* __restrict__ nobs, int S, double A, double B, double* red) {
  double tot = 0.0;
  for (int v = 0; v < V; ++v) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) s += part[(long long)v * nb + b];
    s = block_sum(s, red);
    if (threadIdx.x == 0 && nobs[v] > 0.0) tot += (w != nullptr ? w[v] : 1.0) * (A * s + B * (double)S * nobs[v]);
    __syncthreads();
  }
  return tot;
}

// ll[i] = sum_v w_v (-sum z^2 / 2 + (-log s - log(2 pi) / 2) S nobs_v) / S_i;  loss = kl_scale sum(kl) - sum_i ll[i]
__global__ void __launch_bounds__(256) elbo_skip_finish_kernel(SkipFinishArgs a) {
  __shared__ double red[4];
  double lsum = 0.0;
  for (int i = 0; i < a.n_ll; ++i) {
    const double sd = exp((double)a.noise_u[i][0]) + 1e-5;
    const double s = skip_total(a.part[i], a.V[i], a.nb[i], a.w[i], a.nobs[i], a.S[i], -0.5,
                                -log(sd) - 0.9189385332046727, red);
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

// dnoise_u = -gloss sum_v w_v (sum z^2 - S nobs_v) / s / S exp(noise_u); the first term also zero-fills the whole noise
// gradient first and writes dkl = kl_scale gloss
__global__ void __launch_bounds__(256)
loglik_skip_bwd_finish_kernel(const double* __restrict__ part, int V, int nb, const double* __restrict__ w,
                              const double* __restrict__ nobs, const float* __restrict__ noise_u, int S,
                              float* __restrict__ dnoise_u, const float* __restrict__ gloss, double* __restrict__ dkl,
                              int n_kl, double kl_scale, float* __restrict__ zero_base, int zero_n) {
  __shared__ double red[4];
  if (zero_base != nullptr) {
    for (int t = threadIdx.x; t < zero_n; t += blockDim.x) zero_base[t] = 0.f;
    __syncthreads();
  }
  const double s = skip_total(part, V, nb, w, nobs, S, 1.0, -1.0, red);
  if (threadIdx.x == 0) {
    const double e = exp((double)noise_u[0]), sc = e + 1e-5;
    dnoise_u[0] = (float)(-(double)gloss[0] * s / sc / (double)S * e);
  }
  if (dkl != nullptr)
    for (int t = threadIdx.x; t < n_kl; t += blockDim.x) dkl[t] = kl_scale * (double)gloss[0];
}

// blocks per view: enough for the largest view, at most 4096 partials per term in all (loglik_w_blocks)
static inline int loglik_skip_blocks(int S, const long long* off, int V, int P) {
  long long most = 0;
  for (int v = 0; v < V; ++v) {
    const long long t = (off[v + 1] - off[v]) * P * (long long)S;
    if (t > most) most = t;
  }
  long long b = cdiv(most, 1024);
  const long long cap = 4096 / V;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

static inline bool skip_views_ok(int V, const long long* off, long long N) {
  if (V < 1 || V > SKIP_MAX_VIEWS || off == nullptr || off[0] != 0 || off[V] != N) return false;
  for (int v = 0; v < V; ++v)
    if (off[v + 1] < off[v]) return false;
  return true;
}

// the tables of both directions, checked before any launch: a term is either fused (zpart[i], one view, no weights of its
// own: the fused kernels sum z^2 over all rows) or comes from its draws, with the caller's views or as one view
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
    if (n_views && !skip_views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
    if (w && !w[i]) return GPSA_EINVAL;
  }
  return 0;
}
static inline SkipRows skip_rows(int i, const long long* N, const int* n_views, const long long* const* view_off, int* V) {
  SkipRows vr;
  *V = n_views ? n_views[i] : 1;
  if (n_views) {
    for (int v = 0; v <= n_views[i]; ++v) vr.off[v] = view_off[i][v];
  } else {
    vr.off[0] = 0;
    vr.off[1] = N[i];
  }
  return vr;
}

}  // namespace gpsa

extern "C" {

long long gpsa_count_observed_workspace(void) { return 8LL * gpsa::COUNT_BLOCKS * gpsa::COUNT_MAX_SEGS; }

int gpsa_count_observed(int n_ll, const float* const* Y, const long long* N, const int* P, const int* n_views,
                        const long long* const* view_off, double* const* nobs, void* workspace,
                        long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (n_ll < 1 || n_ll > GPSA_MAX_MODS || !Y || !N || !P || !nobs || !workspace) return GPSA_EINVAL;
  if ((n_views == nullptr) != (view_off == nullptr)) return GPSA_EINVAL;
  if (workspace_bytes < gpsa_count_observed_workspace()) return GPSA_EWORKSPACE;
  for (int i = 0; i < n_ll; ++i) {
    if (!Y[i] || !nobs[i] || N[i] < 1 || P[i] < 1) return GPSA_EINVAL;
    if (n_views && !skip_views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
  }
  hipStream_t st = as_stream(stream);
  double* part = reinterpret_cast<double*>(workspace);
  CountArgs a = {};
  long long most = 0;
  int s = 0;
  // one launch pair per COUNT_MAX_SEGS pairs (one in all for any full-data fit; a minibatch over more views than that
  // takes another: the stream orders their use of the one workspace)
  auto flush = [&]() {
    a.n_seg = s;
    long long nb = cdiv(most, 4096);
    if (nb > COUNT_BLOCKS) nb = COUNT_BLOCKS;
    if (nb < 1) nb = 1;
    count_observed_kernel<<<dim3((unsigned)nb, (unsigned)s), 256, 0, st>>>(a, part);
    count_observed_finish_kernel<<<1, 256, 0, st>>>(a, part, (int)nb);
    s = 0;
    most = 0;
  };
  for (int i = 0; i < n_ll; ++i) {
    int V;
    const SkipRows vr = skip_rows(i, N, n_views, view_off, &V);
    for (int v = 0; v < V; ++v) {
      a.Y[s] = Y[i] + vr.off[v] * P[i];
      a.tot[s] = (vr.off[v + 1] - vr.off[v]) * P[i];
      a.dst[s] = nobs[i] + v;
      if (a.tot[s] > most) most = a.tot[s];
      if (++s == COUNT_MAX_SEGS) flush();
    }
  }
  if (s > 0) flush();
  GPSA_LAUNCH_CHECK();
  return 0;
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
  hipStream_t st = as_stream(stream);
  SkipFinishArgs a = {};
  a.n_ll = n_ll;
  a.n_kl = kl ? n_kl : 0;
  a.kl = kl;
  a.kl_scale = kl_scale;
  a.ll = ll_out;
  a.loss = loss;
  for (int i = 0; i < n_ll; ++i) {
    a.w[i] = w ? w[i] : nullptr;
    a.nobs[i] = nobs[i];
    a.noise_u[i] = noise_u[i];
    a.S[i] = S[i];
    if (zpart && zpart[i]) {
      a.part[i] = zpart[i];
      a.V[i] = 1;
      a.nb[i] = nparts;
      continue;
    }
    int V;
    const SkipRows vr = skip_rows(i, N, n_views, view_off, &V);
    const int nb = loglik_skip_blocks(S[i], vr.off, V, P[i]);
    double* part = reinterpret_cast<double*>(workspace) + LL_SLOT_DOUBLES * i;
    loglik_skip_kernel<false><<<dim3(nb, V), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], vr, a.w[i],
                                                           nullptr, nullptr, part);
    a.part[i] = part;
    a.V[i] = V;
    a.nb[i] = nb;
  }
  elbo_skip_finish_kernel<<<1, 256, 0, st>>>(a);
  GPSA_LAUNCH_CHECK();
  return 0;
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
  hipStream_t st = as_stream(stream);
  for (int i = 0; i < n_ll; ++i) {
    // the first term's finishing launch also zero-fills the noise gradient and writes dkl
    double* dkl_i = i == 0 ? dkl : nullptr;
    float* zero_i = i == 0 ? dnoise_all : nullptr;
    const double* wi = w ? w[i] : nullptr;
    if (zpart && zpart[i]) {
      loglik_skip_bwd_finish_kernel<<<1, 256, 0, st>>>(zpart[i], 1, nparts, wi, nobs[i], noise_u[i], S[i], dnoise[i], gloss,
                                                       dkl_i, n_kl, kl_scale, zero_i, n_noise);
      continue;
    }
    int V;
    const SkipRows vr = skip_rows(i, N, n_views, view_off, &V);
    const int nb = loglik_skip_blocks(S[i], vr.off, V, P[i]);
    double* part = reinterpret_cast<double*>(workspace) + LL_SLOT_DOUBLES * i;
    loglik_skip_kernel<true><<<dim3(nb, V), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], vr, wi, gloss,
                                                          dF[i], part);
    loglik_skip_bwd_finish_kernel<<<1, 256, 0, st>>>(part, V, nb, wi, nobs[i], noise_u[i], S[i], dnoise[i], gloss, dkl_i,
                                                     n_kl, kl_scale, zero_i, n_noise);
  }
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_lmc_loglik_fused_skip_f32(const float* F, const float* W, const float* Y, const float* noise_u, int S, long long N,
                                   int L, int P, double* zpart, int nparts, float* dF, float* dW, void* workspace,
                                   long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!F || !W || !Y || !noise_u || !zpart || !dF || !dW || S < 1 || N < 1 || L < 1 || P < 1 || nparts < 1)
    return GPSA_EINVAL;
  if (L > 64) return GPSA_EUNSUPPORTED;
  const long long C = (long long)S * N;
  const long long need = gpsa_lmc_loglik_workspace(C, L, P, nparts);
  if (workspace_bytes < need) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  // gpsa_lmc_loglik_fused_f32's grid: the workspace query's workgroups, at most one per tile of 16 spots
  const int G = (int)((need - 256) / ((long long)L * P * 4));
  const long long nt = cdiv(N, 16);
  const int Gm = (int)(nt < G ? nt : G);
  float* part = (float*)workspace;
  if (int rc = lmc_mfma_skip_launch(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, part, Gm, st)) return rc;
  const long long n = (long long)L * P;
  reduce_rows_kernel<float, float><<<(unsigned)cdiv(n, 64), 256, 0, st>>>(part, Gm, n, n, dW, 1.0);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
