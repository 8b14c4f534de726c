// Minibatch (stochastic variational) training: the per-step row sampler-gather (include/gpsa_hip.h, "minibatch"; the
// per-view weighted likelihood it trains with is in loss_views.hip).  Opt-in: no full-batch path launches anything from
// here.
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

}  // extern "C"
