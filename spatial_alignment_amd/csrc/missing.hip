// Partly observed outputs (model.skip_missing): a NaN in Y is a missing observation and is left out of the ELBO.
//   gpsa_count_observed              the observed entries of every (term, view), as device doubles
//   gpsa_lmc_loglik_fused_skip_f32   gpsa_lmc_loglik_fused_f32 with the select in front of its products (lmc.hip)
// (the loss closings over the observed entries, gpsa_elbo_loss_skip_fwd / _bwd, are in loss_views.hip; the fused ELBO
// pass's variant is panel_elbo_skip_kernel, qf_elbo_skip.hip.)  The test is y == y: the build has no
// fast-math flag, under which the compiler would fold it away.
#include "internal.hpp"

namespace gpsa {

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
    if (n_views && !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
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
    const int V = n_views ? n_views[i] : 1;
    const ViewRows vr = view_rows(N[i], V, view_off ? view_off[i] : nullptr);
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
