// Minibatch (stochastic variational) training: the per-step row sampler-gather and the per-view weighted Gaussian
// likelihood (include/gpsa_hip.h, "minibatch").  Both are opt-in: no full-batch path launches anything from here.
#include "common.hpp"

namespace gpsa {

// ---- keyed bijection of [0, N) ------------------------------------------------------------------------------------
// splitmix64's finaliser as the round function and key schedule; minibatch.py (feistel_perm) restates it bit for bit
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
constexpr int FEISTEL_ROUNDS = 6;
constexpr unsigned long long GOLDEN = 0x9E3779B97F4A7C15ULL;

// base key of permutation pi_{seed, m, v, e}; round r uses mix64(base ^ (r + 1) * GOLDEN)
__device__ __forceinline__ unsigned long long perm_key(unsigned long long seed, int m, int v, unsigned long long e) {
  unsigned long long h = mix64(seed);
  h = mix64(h ^ (unsigned long long)m);
  h = mix64(h ^ (unsigned long long)v);
  return mix64(h ^ e);
}

// an alternating (unbalanced) Feistel network on k = ceil(log2 N) bits, x = (A: the high a = k/2 bits, B: the low
// b = k - a bits); even rounds A ^= F(B), odd rounds B ^= F(A).  Cycle-walking (apply again while the value is >= N)
// restricts the bijection of [0, 2^k) to one of [0, N); 2^k < 2N, so fewer than two passes are expected
__device__ __forceinline__ long long feistel_perm(long long x, long long N, int k, unsigned long long base) {
  const int a = k >> 1, b = k - a;
  const unsigned long long ma = (1ULL << a) - 1ULL, mb = (1ULL << b) - 1ULL;
  unsigned long long y = (unsigned long long)x;
  do {
    unsigned long long A = y >> b, B = y & mb;
#pragma unroll
    for (int r = 0; r < FEISTEL_ROUNDS; ++r) {
      const unsigned long long kr = mix64(base ^ ((unsigned long long)(r + 1) * GOLDEN));
      if ((r & 1) == 0)
        A ^= mix64(kr ^ B) & ma;
      else
        B ^= mix64(kr ^ A) & mb;
    }
    y = (A << b) | B;
  } while (y >= (unsigned long long)N);
  return (long long)y;
}

constexpr int SAMPLE_MAX_SEGS = 64;
struct SampleArgs {
  const float* X[GPSA_MAX_MODS];
  const float* Y[GPSA_MAX_MODS];
  float* Xb[GPSA_MAX_MODS];
  float* Yb[GPSA_MAX_MODS];
  long long* rows[GPSA_MAX_MODS];
  int D[GPSA_MAX_MODS], P[GPSA_MAX_MODS];
  // segment s = one (modality, view): its rows src .. src + N of modality m, its batch block dst .. dst + B, and the
  // first global batch row g[s] (g[n_seg] = total)
  int m[SAMPLE_MAX_SEGS], v[SAMPLE_MAX_SEGS], bits[SAMPLE_MAX_SEGS];
  int N[SAMPLE_MAX_SEGS], B[SAMPLE_MAX_SEGS], src[SAMPLE_MAX_SEGS], dst[SAMPLE_MAX_SEGS];
  int g[SAMPLE_MAX_SEGS + 1];
  int n_seg;
  unsigned long long seed;
  const long long* counter;
};

// one wave per batch row: every lane forms the row's index (wave-uniform work), lane 0 stores it, the lanes copy the
// coordinates and the observations of that row
__global__ void __launch_bounds__(256) row_sample_gather_kernel(SampleArgs a) {
  const int lane = threadIdx.x & 63;
  const long long gr = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (gr >= a.g[a.n_seg]) return;
  int s = 0;
  while (s + 1 < a.n_seg && a.g[s + 1] <= gr) ++s;
  const long long j = gr - a.g[s];
  const long long N = a.N[s], B = a.B[s];
  const long long t = a.counter[0];
  const long long K = N / B;
  const long long e = t / K, kk = t - e * K;
  const long long local = feistel_perm(kk * B + j, N, a.bits[s], perm_key(a.seed, a.m[s], a.v[s], (unsigned long long)e));
  const int m = a.m[s];
  const long long idx = a.src[s] + local, out = a.dst[s] + j;
  if (lane == 0) a.rows[m][out] = idx;
  const int D = a.D[m], P = a.P[m];
  for (int d = lane; d < D; d += 64) a.Xb[m][out * D + d] = a.X[m][idx * D + d];
  const float* __restrict__ y = a.Y[m] + idx * P;
  float* __restrict__ yb = a.Yb[m] + out * P;
  for (int p = lane; p < P; p += 64) yb[p] = y[p];
}

__global__ void __launch_bounds__(64) counter_advance_kernel(long long* counter) {
  if (threadIdx.x == 0) counter[0] = counter[0] + 1;
}

// ---- per-view weighted Gaussian likelihood --------------------------------------------------------------------------
constexpr int LLW_MAX_VIEWS = 64;
struct ViewRows {
  long long off[LLW_MAX_VIEWS + 1];  // view v = rows off[v] .. off[v + 1]
};

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

// sum_v w_v sum_b part[v * nb + b]   (thread 0; views in order, fp64)
__device__ double weighted_total(const double* __restrict__ part, int V, int nb, const double* __restrict__ w,
                                 double* red) {
  double tot = 0.0;
  for (int v = 0; v < V; ++v) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) s += part[(long long)v * nb + b];
    s = block_sum(s, red);
    if (threadIdx.x == 0) tot += w[v] * s;
    __syncthreads();
  }
  return tot;
}

struct WeightedFinishArgs {
  const double* part[GPSA_MAX_MODS];
  const double* w[GPSA_MAX_MODS];
  int V[GPSA_MAX_MODS], nb[GPSA_MAX_MODS], S[GPSA_MAX_MODS];
  int n_ll, n_kl;
  const double* kl;
  double kl_scale;
  double* ll;
  float* loss;
};
// ll[i] = sum_v w_v LL_{i,v} / S_i;  loss = kl_scale sum(kl) - sum_i ll[i]
__global__ void __launch_bounds__(256) elbo_weighted_finish_kernel(WeightedFinishArgs a) {
  __shared__ double red[4];
  double lsum = 0.0;
  for (int i = 0; i < a.n_ll; ++i) {
    const double s = weighted_total(a.part[i], a.V[i], a.nb[i], a.w[i], red);
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

// dnoise_u = -gloss sum_v w_v (sum z^2 - 1)_v / s / S exp(noise_u); the first term also zero-fills the whole noise
// gradient first and writes dkl = kl_scale gloss
__global__ void __launch_bounds__(256)
loglik_w_bwd_finish_kernel(const double* __restrict__ part, int V, int nb, const double* __restrict__ w,
                           const float* __restrict__ noise_u, int S, float* __restrict__ dnoise_u,
                           const float* __restrict__ gloss, double* __restrict__ dkl, int n_kl, double kl_scale,
                           float* __restrict__ zero_base, int zero_n) {
  __shared__ double red[4];
  if (zero_base != nullptr) {
    for (int t = threadIdx.x; t < zero_n; t += blockDim.x) zero_base[t] = 0.f;
    __syncthreads();
  }
  const double s = weighted_total(part, V, nb, w, red);
  if (threadIdx.x == 0) {
    const double e = exp((double)noise_u[0]), sc = e + 1e-5;
    dnoise_u[0] = (float)(-(double)gloss[0] * s / sc / (double)S * e);
  }
  if (dkl != nullptr)
    for (int t = threadIdx.x; t < n_kl; t += blockDim.x) dkl[t] = kl_scale * (double)gloss[0];
}

// blocks per view: enough for the largest view, at most 4096 partials per term in all
static inline int loglik_w_blocks(const int S, const long long* off, int V, int P) {
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

static inline bool views_ok(int V, const long long* off, long long N) {
  if (V < 1 || V > LLW_MAX_VIEWS || off == nullptr || off[0] != 0 || off[V] != N) return false;
  for (int v = 0; v < V; ++v)
    if (off[v + 1] < off[v]) return false;
  return true;
}

}  // namespace gpsa

extern "C" {

int gpsa_row_sample_gather(int n_mods, const int* n_views, const long long* n_rows, const long long* batch,
                           unsigned long long seed, long long* counter, const float* const* X, const int* D,
                           const float* const* Y, const int* P, long long* const* rows, float* const* Xb,
                           float* const* Yb, void* stream) {
  using namespace gpsa;
  if (n_mods < 1 || n_mods > GPSA_MAX_MODS || !n_views || !n_rows || !batch || !counter || !X || !D || !Y || !P ||
      !rows || !Xb || !Yb)
    return GPSA_EINVAL;
  SampleArgs a = {};
  a.seed = seed;
  a.counter = counter;
  int s = 0;
  long long g = 0;
  for (int m = 0; m < n_mods; ++m) {
    if (n_views[m] < 1 || D[m] < 1 || P[m] < 1 || !X[m] || !Y[m] || !rows[m] || !Xb[m] || !Yb[m]) return GPSA_EINVAL;
    a.X[m] = X[m];
    a.Y[m] = Y[m];
    a.Xb[m] = Xb[m];
    a.Yb[m] = Yb[m];
    a.rows[m] = rows[m];
    a.D[m] = D[m];
    a.P[m] = P[m];
    long long src = 0, dst = 0;
    for (int v = 0; v < n_views[m]; ++v, ++s) {
      if (s >= SAMPLE_MAX_SEGS) return GPSA_EUNSUPPORTED;
      const long long N = n_rows[s], B = batch[s];
      if (N < 1 || B < 1 || B > N) return GPSA_EINVAL;
      int k = 0;
      while ((1LL << k) < N) ++k;
      a.m[s] = m;
      a.v[s] = v;
      a.bits[s] = k;
      a.N[s] = (int)N;
      a.B[s] = (int)B;
      a.src[s] = (int)src;
      a.dst[s] = (int)dst;
      a.g[s] = (int)g;
      src += N;
      dst += B;
      g += B;
      if (src > 0x7fffffffLL || g > 0x7fffffffLL) return GPSA_EUNSUPPORTED;
    }
  }
  a.n_seg = s;
  a.g[s] = (int)g;
  hipStream_t st = as_stream(stream);
  row_sample_gather_kernel<<<(unsigned)cdiv(g, 4), 256, 0, st>>>(a);
  counter_advance_kernel<<<1, 64, 0, st>>>(counter);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_elbo_loss_weighted_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                                const int* S, const long long* N, const int* P, const int* n_views,
                                const long long* const* view_off, const double* const* w, const double* kl, int n_kl,
                                double kl_scale, float* loss, double* ll_out, void* workspace,
                                long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!n_views || !view_off || !w || !loss || !ll_out) return GPSA_EINVAL;
  if (int rc = elbo_loss_args_check(n_ll, F, Y, noise_u, S, N, P, workspace_bytes)) return rc;
  for (int i = 0; i < n_ll; ++i)
    if (!w[i] || !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  WeightedFinishArgs a = {};
  a.n_ll = n_ll;
  a.n_kl = kl ? n_kl : 0;
  a.kl = kl;
  a.kl_scale = kl_scale;
  a.ll = ll_out;
  a.loss = loss;
  for (int i = 0; i < n_ll; ++i) {
    ViewRows vr;
    for (int v = 0; v <= n_views[i]; ++v) vr.off[v] = view_off[i][v];
    const int nb = loglik_w_blocks(S[i], view_off[i], n_views[i], P[i]);
    double* part = reinterpret_cast<double*>(workspace) + LL_SLOT_DOUBLES * i;
    loglik_w_kernel<false><<<dim3(nb, n_views[i]), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], vr,
                                                                 w[i], nullptr, nullptr, part);
    a.part[i] = part;
    a.w[i] = w[i];
    a.V[i] = n_views[i];
    a.nb[i] = nb;
    a.S[i] = S[i];
  }
  elbo_weighted_finish_kernel<<<1, 256, 0, st>>>(a);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_elbo_loss_weighted_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                                const int* S, const long long* N, const int* P, const int* n_views,
                                const long long* const* view_off, const double* const* w, const float* gloss, int n_kl,
                                double kl_scale, float* const* dF, float* const* dnoise, float* dnoise_all,
                                int n_noise, double* dkl, void* workspace, long long workspace_bytes, void* stream) {
  using namespace gpsa;
  if (!n_views || !view_off || !w || !gloss || !dF || !dnoise) return GPSA_EINVAL;
  if (int rc = elbo_loss_args_check(n_ll, F, Y, noise_u, S, N, P, workspace_bytes)) return rc;
  for (int i = 0; i < n_ll; ++i)
    if (!w[i] || !views_ok(n_views[i], view_off[i], N[i])) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  for (int i = 0; i < n_ll; ++i) {
    ViewRows vr;
    for (int v = 0; v <= n_views[i]; ++v) vr.off[v] = view_off[i][v];
    const int nb = loglik_w_blocks(S[i], view_off[i], n_views[i], P[i]);
    double* part = reinterpret_cast<double*>(workspace) + LL_SLOT_DOUBLES * i;
    loglik_w_kernel<true><<<dim3(nb, n_views[i]), 256, 0, st>>>(F[i], Y[i], noise_u[i], S[i], N[i] * P[i], P[i], vr,
                                                                w[i], gloss, dF[i], part);
    // the first term's finishing launch also zero-fills the noise gradient and writes dkl
    loglik_w_bwd_finish_kernel<<<1, 256, 0, st>>>(part, n_views[i], nb, w[i], noise_u[i], S[i], dnoise[i], gloss,
                                                  i == 0 ? dkl : nullptr, n_kl, kl_scale,
                                                  i == 0 ? dnoise_all : nullptr, n_noise);
  }
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
