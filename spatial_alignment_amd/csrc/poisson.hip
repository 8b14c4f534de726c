// Count outputs (model.likelihood = "poisson"): the per-element kernels of the Poisson likelihood term.
//   loglik_pois_kernel<BWD>   sum of y eta - exp(eta) per (view, block) / dF = gloss w_v (exp(eta) - y) / S, on the
//                             pattern of loglik_skip_kernel (loss_views.hip, where the closing pair
//                             gpsa_elbo_loss_pois_fwd / _bwd launches it through pois_loglik_launch)
//   gpsa_lgamma_sum           sum of lgamma(y + 1) per (term, view): the term's parameter-free constant, once per Y
// (the fused passes' variants are panel_elbo_pois_kernel, qf_elbo_pois.hip, and lmc_mfma_pois_kernel, lmc.hip.)
// eta = F + log_offset[row] is the log rate; exp is the exact expf (the fast __expf has an error that grows with its
// argument); Y is not validated: the formula is evaluated as written for any real y, and eta > 88 gives inf.  The NaN
// test is y == y: the build has no fast-math flag, under which the compiler would fold it away.
#include "internal.hpp"

namespace gpsa {

// F [S, N, P], Y [N, P], off [N] or nullptr, grid (nb, V); fp32 terms, four to a thread and pass, summed in fp64
template <bool BWD>
__global__ void __launch_bounds__(256)
loglik_pois_kernel(const float* __restrict__ F, const float* __restrict__ Y, const float* __restrict__ off, int S,
                   long long NP, int P, ViewRows vr, const double* __restrict__ w, const float* __restrict__ gloss,
                   int skip, float* __restrict__ dF, double* __restrict__ part) {
  __shared__ double red[4];
  const int v = blockIdx.y, nb = gridDim.x;
  const long long row0 = vr.off[v], lo = row0 * P, per = (vr.off[v + 1] - row0) * P, tot = per * S;
  const double wv = w != nullptr ? w[v] : 1.0;
  const float coef = BWD ? (float)((double)gloss[0] * wv / (double)S) : 0.f;
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
        const float eta = F[i] + (off != nullptr ? off[row0 + k / P] : 0.f);
        const float ex = expf(eta);
        const bool obs = !skip || y == y;
        if (BWD)
          dF[i] = obs ? coef * (ex - y) : 0.f;
        else
          acc4 += obs ? fmaf(y, eta, -ex) : 0.f;
      }
    }
    acc += (double)acc4;
  }
  if (!BWD) {
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[(long long)v * nb + blockIdx.x] = acc;
  }
}

int pois_loglik_launch(bool bwd, const float* F, const float* Y, const float* log_offset, int S, long long N, int P,
                       const ViewRows& vr, int V, int nb, const double* w, const float* gloss, int skip, float* dF,
                       double* part, hipStream_t st) {
  if (bwd)
    loglik_pois_kernel<true><<<dim3(nb, V), 256, 0, st>>>(F, Y, log_offset, S, N * P, P, vr, w, gloss, skip, dF, part);
  else
    loglik_pois_kernel<false><<<dim3(nb, V), 256, 0, st>>>(F, Y, log_offset, S, N * P, P, vr, w, nullptr, skip, nullptr,
                                                           part);
  GPSA_LAUNCH_CHECK();
  return 0;
}

constexpr int LGAM_MAX_SEGS = 64;   // (term, view) pairs of one launch (a call with more loops over them)
constexpr int LGAM_BLOCKS = 64;     // block partials per pair

struct LgamArgs {
  const float* Y[LGAM_MAX_SEGS];   // first entry of the pair's rows
  long long tot[LGAM_MAX_SEGS];    // its entries (rows x P)
  double* dst[LGAM_MAX_SEGS];      // out[i] + v
  int n_seg;
};

// part[seg * nb + block] = sum of lgamma(y + 1) over the block's share of pair seg, in fp64; grid (nb, n_seg)
__global__ void __launch_bounds__(256) lgamma_sum_kernel(LgamArgs a, int skip, double* __restrict__ part) {
  __shared__ double red[4];
  const int seg = blockIdx.y, nb = gridDim.x;
  const float* __restrict__ Y = a.Y[seg];
  const long long tot = a.tot[seg];
  double s = 0.0;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < tot; i += (long long)nb * 256) {
    const float y = Y[i];
    if (!skip || y == y) s += lgamma((double)y + 1.0);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[(long long)seg * nb + blockIdx.x] = s;
}
// out of pair seg = its block partials in block order; one block for all pairs
__global__ void __launch_bounds__(256) lgamma_sum_finish_kernel(LgamArgs a, const double* __restrict__ part, int nb) {
  __shared__ double red[4];
  for (int seg = 0; seg < a.n_seg; ++seg) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += part[(long long)seg * nb + b];
    s = block_sum(s, red);
    if (threadIdx.x == 0) a.dst[seg][0] = s;
    __syncthreads();
  }
}

}  // namespace gpsa

extern "C" {

long long gpsa_lgamma_sum_workspace(void) { return 8LL * gpsa::LGAM_BLOCKS * gpsa::LGAM_MAX_SEGS; }

int gpsa_lgamma_sum(int n_ll, const float* const* Y, const long long* N, const int* P, const int* n_views,
                    const long long* const* view_off, int skip, double* const* out, void* workspace,
                    long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (n_ll < 1 || n_ll > GPSA_MAX_MODS || !Y || !N || !P || !out || !workspace) return GPSA_EINVAL;
  if ((n_views == nullptr) != (view_off == nullptr)) return GPSA_EINVAL;
  if (workspace_bytes < gpsa_lgamma_sum_workspace()) return GPSA_EWORKSPACE;
  for (int i = 0; i < n_ll; ++i) {
    if (!Y[i] || !out[i] || N[i] < 1 || P[i] < 1) return GPSA_EINVAL;
    if (n_views && !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
  }
  hipStream_t st = as_stream(stream);
  double* part = reinterpret_cast<double*>(workspace);
  LgamArgs a = {};
  long long most = 0;
  int s = 0;
  // one launch pair per LGAM_MAX_SEGS pairs (the stream orders their use of the one workspace)
  auto flush = [&]() {
    a.n_seg = s;
    long long nb = cdiv(most, 4096);
    if (nb > LGAM_BLOCKS) nb = LGAM_BLOCKS;
    if (nb < 1) nb = 1;
    lgamma_sum_kernel<<<dim3((unsigned)nb, (unsigned)s), 256, 0, st>>>(a, skip, part);
    lgamma_sum_finish_kernel<<<1, 256, 0, st>>>(a, part, (int)nb);
    s = 0;
    most = 0;
  };
  for (int i = 0; i < n_ll; ++i) {
    const int V = n_views ? n_views[i] : 1;
    const ViewRows vr = view_rows(N[i], V, view_off ? view_off[i] : nullptr);
    for (int v = 0; v < V; ++v) {
      a.Y[s] = Y[i] + vr.off[v] * P[i];
      a.tot[s] = (vr.off[v + 1] - vr.off[v]) * P[i];
      a.dst[s] = out[i] + v;
      if (a.tot[s] > most) most = a.tot[s];
      if (++s == LGAM_MAX_SEGS) flush();
    }
  }
  if (s > 0) flush();
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_lmc_loglik_fused_pois_f32(const float* F, const float* W, const float* Y, const float* log_offset, int skip, int S,
                                   long long N, int L, int P, double* zpart, int nparts, float* dF, float* dW,
                                   void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!F || !W || !Y || !zpart || !dF || !dW || S < 1 || N < 1 || L < 1 || P < 1 || nparts < 1) return GPSA_EINVAL;
  if (L > 64) return GPSA_EUNSUPPORTED;
  const long long C = (long long)S * N;
  const long long need = gpsa_lmc_loglik_workspace(C, L, P, nparts);
  if (workspace_bytes < need || !workspace) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  // gpsa_lmc_loglik_fused_f32's grid: the workspace query's workgroups, at most one per tile of 16 spots
  const int G = (int)((need - 256) / ((long long)L * P * 4));
  const long long nt = cdiv(N, 16);
  const int Gm = (int)(nt < G ? nt : G);
  float* part = (float*)workspace;
  if (int rc = lmc_mfma_pois_launch(F, W, Y, log_offset, skip, S, N, L, P, zpart, nparts, dF, part, Gm, st)) return rc;
  const long long n = (long long)L * P;
  reduce_rows_kernel<float, float><<<(unsigned)cdiv(n, 64), 256, 0, st>>>(part, Gm, n, n, dW, 1.0);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
