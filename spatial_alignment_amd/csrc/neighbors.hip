// Neighbour statistics on the device: exact k nearest neighbours in fp64 and the neighbours' weighted average.
// Replaces the CPU k-nearest-neighbour library the reference's experiments step out to around the fit (gene selection,
// outlier removal, the alignment score, the prediction baselines, Moran's I) when the coordinates and the expression
// matrix already live in HBM.
//
// gpsa_knn_f64 is a brute-force scan.  One thread owns one query: its coordinates and its running top-K sit in
// registers, the references pass through LDS a tile at a time (every lane reads the same address: a broadcast), and
// the common case per pair is D subtract / fused multiply-adds and ONE compare against the list's worst key.  The list
// is sorted by the key (d2, index) - a total order - behind a template K in {1, 2, 4, 8, 16, 32} (k is rounded up, the
// spare slots are never written out); an insertion is K selects, fully unrolled, so no slot index is a run-time value
// and the list never goes to scratch.
//
// The reference axis is cut into `parts` slices scanned by separate workgroups (blockIdx.y); with more than one slice
// the lists go to the workspace ([part][slot][query]: a wave's lanes write consecutive elements) and a second kernel
// merges them by the same key.  The k smallest keys of the union of the slices' k smallest are the k smallest overall,
// and the key is a total order, so the result is the same bits for every `parts`.  No read-modify-write on memory
// anywhere: every output element has one writer.
//
// gpsa_knn_average_f32 / _f64: thread (row, p) walks the row's k neighbours in order, fp64 accumulation, reads coalesced
// along p; one kernel behind the storage type of Y and out.
#include <limits.h>
#include <math.h>

#include "toolbox.hpp"

namespace gpsa {

constexpr int KNN_TILE = 512;     // references staged in LDS at a time (D = 4: 16 KB)
constexpr int KNN_MAXK = 32;      // the largest list kept in registers
constexpr int KNN_MAXPARTS = 256;

// the sorted list of one thread.  Every loop over its slots is fully unrolled: bd / bi are registers.
template <int K>
struct KnnList {
  double bd[K];
  int bi[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      bd[s] = INFINITY;
      bi[s] = INT_MAX;  // above every row index: a real candidate at distance +inf still enters before a spare slot
    }
  }
  __device__ __forceinline__ bool takes(double d, int j) const { return key_less(d, j, bd[K - 1], bi[K - 1]); }
  // (d, j) is known to be below the worst key.  With c[s] = (d, j) < slot s (false ... false true ... true), the new
  // slot s is slot s-1 where c[s-1], else the candidate where c[s], else itself; walked from the last slot down so that
  // slot s-1 is still the old one.
  __device__ __forceinline__ void insert(double d, int j) {
    bool cs = true;
#pragma unroll
    for (int s = K - 1; s >= 1; --s) {
      const bool cp = key_less(d, j, bd[s - 1], bi[s - 1]);
      bd[s] = cp ? bd[s - 1] : (cs ? d : bd[s]);
      bi[s] = cp ? bi[s - 1] : (cs ? j : bi[s]);
      cs = cp;
    }
    bd[0] = cs ? d : bd[0];
    bi[0] = cs ? j : bi[0];
  }
};

// query i = blockIdx.x * 256 + threadIdx.x against the references [lo, hi) of slice blockIdx.y.
// DIRECT (one slice): the first k slots go to idx / d2 [nq, k];  else to the slice's lists pd / pi [parts][k][nq].
template <int K, int D, bool DIRECT>
__global__ void __launch_bounds__(256)
knn_scan_kernel(const double* __restrict__ Q, long long nq, const double* __restrict__ R, long long nr, long long chunk,
                int k, long long self0, int* __restrict__ oi, double* __restrict__ od) {
  __shared__ double rs[KNN_TILE * D];
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  const bool live = i < nq;
  const long long lo = (long long)blockIdx.y * chunk;
  const long long hi = min(nr, lo + chunk);
  double q[D];
#pragma unroll
  for (int d = 0; d < D; ++d) q[d] = live ? Q[i * D + d] : 0.0;
  const long long self = self0 >= 0 ? self0 + i : -1;  // the reference row that is this query (none: -1)
  KnnList<K> best;
  best.clear();

  for (long long r0 = lo; r0 < hi; r0 += KNN_TILE) {
    const int cnt = (int)min((long long)KNN_TILE, hi - r0);
    __syncthreads();  // the previous tile has been consumed
    for (int t = threadIdx.x; t < cnt * D; t += 256) rs[t] = R[r0 * D + t];
    __syncthreads();
    if (live) {
      for (int r = 0; r < cnt; ++r) {
        double s = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const double u = q[d] - rs[r * D + d];
          s = fma(u, u, s);
        }
        s = (s == s) ? s : (double)INFINITY;  // a NaN distance is the farthest
        const long long j = r0 + r;
        if (best.takes(s, (int)j) && j != self) best.insert(s, (int)j);
      }
    }
  }
  if (!live) return;
  if (DIRECT) {
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (s < k) {
        oi[i * k + s] = best.bi[s];
        od[i * k + s] = best.bd[s];
      }
  } else {
    const long long base = (long long)blockIdx.y * k * nq + i;
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (s < k) {
        oi[base + s * nq] = best.bi[s];
        od[base + s * nq] = best.bd[s];
      }
  }
}

// the slices' lists pd / pi [parts][k][nq] -> idx / d2 [nq, k].  A slice's list is sorted: it is left at its first key
// that does not enter.
template <int K>
__global__ void __launch_bounds__(256)
knn_merge_kernel(const double* __restrict__ pd, const int* __restrict__ pi, long long nq, int k, int parts,
                 int* __restrict__ idx, double* __restrict__ d2) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= nq) return;
  KnnList<K> best;
  best.clear();
  for (int p = 0; p < parts; ++p) {
    const long long base = (long long)p * k * nq + i;
    for (int s = 0; s < k; ++s) {
      const double d = pd[base + s * nq];
      const int j = pi[base + s * nq];
      if (!best.takes(d, j)) break;
      best.insert(d, j);
    }
  }
#pragma unroll
  for (int s = 0; s < K; ++s)
    if (s < k) {
      idx[i * k + s] = best.bi[s];
      d2[i * k + s] = best.bd[s];
    }
}

// the number of slices of the reference axis a call runs with (slice_parts): a slice's scan is cdiv(nq, 256) workgroups
static int knn_parts(long long nq, long long nr, int parts) {
  return slice_parts(cdiv(nq, 256), nr, KNN_TILE, KNN_MAXPARTS, parts);
}

static long long knn_workspace_bytes(long long nq, int k, int parts) {
  if (parts <= 1) return 0;
  const long long n = (long long)parts * k * nq;
  return n * 8 + cdiv(n * 4, 8) * 8;
}

template <int K, int D>
static int launch_knn_kd(hipStream_t st, const double* Q, long long nq, const double* R, long long nr, int k,
                         long long self0, int parts, int* idx, double* d2, void* workspace) {
  const dim3 grid((unsigned)cdiv(nq, 256), (unsigned)parts);
  if (parts == 1) {
    knn_scan_kernel<K, D, true><<<grid, 256, 0, st>>>(Q, nq, R, nr, nr, k, self0, idx, d2);
    GPSA_LAUNCH_CHECK();
    return 0;
  }
  double* pd = (double*)workspace;
  int* pi = (int*)(pd + (long long)parts * k * nq);
  knn_scan_kernel<K, D, false><<<grid, 256, 0, st>>>(Q, nq, R, nr, cdiv(nr, parts), k, self0, pi, pd);
  GPSA_LAUNCH_CHECK();
  knn_merge_kernel<K><<<(unsigned)cdiv(nq, 256), 256, 0, st>>>(pd, pi, nq, k, parts, idx, d2);
  GPSA_LAUNCH_CHECK();
  return 0;
}

template <int K>
static int launch_knn_k(int D, hipStream_t st, const double* Q, long long nq, const double* R, long long nr, int k,
                        long long self0, int parts, int* idx, double* d2, void* workspace) {
  switch (D) {
    case 1: return launch_knn_kd<K, 1>(st, Q, nq, R, nr, k, self0, parts, idx, d2, workspace);
    case 2: return launch_knn_kd<K, 2>(st, Q, nq, R, nr, k, self0, parts, idx, d2, workspace);
    case 3: return launch_knn_kd<K, 3>(st, Q, nq, R, nr, k, self0, parts, idx, d2, workspace);
    case 4: return launch_knn_kd<K, 4>(st, Q, nq, R, nr, k, self0, parts, idx, d2, workspace);
    default: return GPSA_EUNSUPPORTED;
  }
}

// thread (ty, tx) of a TY x TX workgroup: row blockIdx.x * TY + ty, output blockIdx.y * TX + tx
template <typename T, int TX, bool INVDIST>
__global__ void __launch_bounds__(256)
knn_average_kernel(const int* __restrict__ idx, const double* __restrict__ d2, long long nq, int k,
                   const T* __restrict__ Y, int P, T* __restrict__ out) {
  constexpr int TY = 256 / TX;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const long long i = (long long)blockIdx.x * TY + ty;
  const long long p = (long long)blockIdx.y * TX + tx;
  if (i >= nq || p >= P) return;
  const int* ri = idx + i * k;
  bool zero = false;  // a zero distance in the row: those neighbours alone count
  if (INVDIST) {
    const double* rd = d2 + i * k;
    for (int j = 0; j < k; ++j) zero = zero || rd[j] == 0.0;
  }
  double num = 0.0, den = 0.0;
  for (int j = 0; j < k; ++j) {
    double w = 1.0;
    if (INVDIST) {
      const double d = d2[i * k + j];
      w = zero ? (d == 0.0 ? 1.0 : 0.0) : 1.0 / sqrt(d);
    }
    const T y = Y[(long long)ri[j] * P + p];
    if (y == y) {
      num = fma(w, (double)y, num);
      den += w;
    }
  }
  out[i * P + p] = den > 0.0 ? (T)(num / den) : (T)NAN;
}

template <typename T, int TX>
static int launch_knn_average(hipStream_t st, const int* idx, const double* d2, long long nq, int k, const T* Y, int P,
                              int weights, T* out) {
  constexpr int TY = 256 / TX;
  const dim3 grid((unsigned)cdiv(nq, TY), (unsigned)cdiv(P, TX));
  if (weights)
    knn_average_kernel<T, TX, true><<<grid, 256, 0, st>>>(idx, d2, nq, k, Y, P, out);
  else
    knn_average_kernel<T, TX, false><<<grid, 256, 0, st>>>(idx, d2, nq, k, Y, P, out);
  GPSA_LAUNCH_CHECK();
  return 0;
}

// the checks and the choice of the strip's width, before any launch
template <typename T>
static int knn_average(const int* idx, const double* d2, long long nq, int k, const T* Y, long long nr, int P,
                       int weights, T* out, void* stream) {
  if (idx == nullptr || Y == nullptr || out == nullptr) return GPSA_EINVAL;
  if (nq < 1 || k < 1 || nr < 1 || P < 1) return GPSA_EINVAL;
  if (weights != 0 && weights != 1) return GPSA_EINVAL;
  if (weights == 1 && d2 == nullptr) return GPSA_EINVAL;
  if (nq > 0x7fffffffLL || P > 65535 * 256) return GPSA_EINVAL;  // the grid's x and y extents
  hipStream_t st = as_stream(stream);
  if (P <= 16) return launch_knn_average<T, 16>(st, idx, d2, nq, k, Y, P, weights, out);
  if (P <= 64) return launch_knn_average<T, 64>(st, idx, d2, nq, k, Y, P, weights, out);
  return launch_knn_average<T, 256>(st, idx, d2, nq, k, Y, P, weights, out);
}

}  // namespace gpsa

extern "C" {

long long gpsa_knn_workspace(long long nq, long long nr, int k, int parts) {
  if (nq < 1 || nr < 1 || k < 1 || parts < 0) return 0;
  return gpsa::knn_workspace_bytes(nq, k, gpsa::knn_parts(nq, nr, parts));
}

int gpsa_knn_f64(const double* Q, long long nq, const double* R, long long nr, int D, int k, int exclude_self, int parts,
                 int* idx, double* d2, void* workspace, long long workspace_bytes, void* stream) {
  if (Q == nullptr || R == nullptr || idx == nullptr || d2 == nullptr) return GPSA_EINVAL;
  if (nq < 1 || nr < 1 || D < 1 || k < 1 || parts < 0) return GPSA_EINVAL;
  if (D > gpsa::MAXD || k > gpsa::KNN_MAXK) return GPSA_EUNSUPPORTED;
  if (k > nr - (exclude_self ? 1 : 0)) return GPSA_EINVAL;
  if (nr > 0x7fffffffLL || cdiv(nq, 256) > 0x7fffffffLL) return GPSA_EINVAL;  // indices are int32
  const int np = gpsa::knn_parts(nq, nr, parts);
  const long long need = gpsa::knn_workspace_bytes(nq, k, np);
  if (workspace_bytes < need || (need > 0 && workspace == nullptr)) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  // query i is reference row self0 + i: 0 for the same array, the slice's first row where Q is a row slice of R
  long long self0 = -1;
  if (exclude_self) {
    const long long off = (const char*)Q - (const char*)R, row = 8LL * D;
    self0 = (off > 0 && off < nr * row && off % row == 0) ? off / row : 0;
  }
#define GPSA_KNN_CASE(KK) \
  if (k <= KK) return gpsa::launch_knn_k<KK>(D, st, Q, nq, R, nr, k, self0, np, idx, d2, workspace);
  GPSA_KNN_CASE(1)
  GPSA_KNN_CASE(2)
  GPSA_KNN_CASE(4)
  GPSA_KNN_CASE(8)
  GPSA_KNN_CASE(16)
  GPSA_KNN_CASE(32)
#undef GPSA_KNN_CASE
  return GPSA_EUNSUPPORTED;
}

int gpsa_knn_average_f32(const int* idx, const double* d2, long long nq, int k, const float* Y, long long nr, int P,
                         int weights, float* out, void* stream) {
  return gpsa::knn_average<float>(idx, d2, nq, k, Y, nr, P, weights, out, stream);
}

int gpsa_knn_average_f64(const int* idx, const double* d2, long long nq, int k, const double* Y, long long nr, int P,
                         int weights, double* out, void* stream) {
  return gpsa::knn_average<double>(idx, d2, nq, k, Y, nr, P, weights, out, stream);
}

}  // extern "C"
