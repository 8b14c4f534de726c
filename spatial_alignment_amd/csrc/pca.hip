// Expression PCA on the device (pca.py): the two passes over the data that a principal-component decomposition of a
// dense fp32 matrix Y [N, P] needs.  Both read the stored fp32 value and form, as the operand is staged,
//     z_ia = (double(y_ia) - mean[v(i), a]) * inv_scale[v(i), a]          (inv_scale NULL: z = y - mean)
// in fp64, with v(i) the view of row i (view_off [V + 1] on the HOST, as gpsa_column_moments_f32 takes it).  No centred
// and no fp64 copy of Y exists.  The views are walked one after the other (a launch per view: mean and inv_scale are the
// view's rows for the whole launch, so no K chunk and no row block mixes two views' means).
//
// pca_gram_kernel    G[a, b] = sum_i z_ia z_ib on v_mfma_f64_16x16x4_f64.  A workgroup owns one pair (I <= J) of column
//                    tiles of PCA_T = 64 columns and one row group; each wave a 32 x 32 quadrant (2 x 2 MFMA tiles, the
//                    lane maps of gpr.hip: A lane (row l & 15, k l >> 4), B lane (k l >> 4, col l & 15), C/D col l & 15,
//                    row (l >> 4) + 4 reg).  The rows come through LDS in chunks of PCA_KC = 32: each thread owns ONE column
//                    of the tile (its mean and scale stay in registers) and 8 rows of the chunk, and the next chunk's
//                    loads are in flight while the MFMAs of this one run.  Only pairs I <= J run; pca_gram_fold_kernel
//                    writes every element (a <= b) to both places, so G is symmetric to the bit.
//                    Row groups: a view's n rows are cut into at most Gr groups of R = ceil(ceil(n / Gr) / 32) * 32
//                    consecutive rows, Gr = pca_groups(N, P): 1 once the tile pairs alone are PCA_FILL = 256 workgroups,
//                    else min(32, ceil(256 / pairs), ceil(N / 32)) - a function of (N, P) alone, never of the device.
//                    Group g of every view adds into plane g (view 0 writes, the later views add: the launches are ordered
//                    on the stream), and the fold adds the planes in ascending g.  With Gr = 1 the plane IS the output's
//                    upper triangle and no workspace is needed.  No atomics, one writer per element per launch, the same
//                    bits on a repeated call.
// pca_project_kernel scores[i, j] = sum_a z_ia comp[j, a], comp [k, P] fp64, k <= 128.  A workgroup owns 64 rows (a wave
//                    16) and walks the columns in chunks of 32: z and the chunk of comp are staged in LDS (pitch 34
//                    doubles: the 16 x 4 operand reads are conflict-free) out of registers that were loaded while the
//                    previous chunk's MFMAs ran; each wave keeps ceil(k / 16) accumulator tiles.  A row's sum runs over
//                    the chunks in order and inside a chunk in the MFMA's k order: it does not depend on which rows are
//                    passed together.  Y is read once.  The arithmetic runs on the MFMA pipe because the vector pipe
//                    is already taken by forming z (convert, subtract, multiply per loaded value) and by the staging:
//                    2 k fp64 flops per 4 loaded bytes on top of that would make the vector pipe the limit from k of
//                    about 16 on.  On the MFMA pipe the read of Y is the limit up to k = 16 or 32 (one or two tiles per
//                    wave: at the 78.6 TF peak the MFMAs keep up with 157 / k_padded TB/s of Y, 9.8 TB/s at one tile
//                    and 4.9 at two, about what HBM delivers); beyond that the MFMAs are the limit.
#include <math.h>

#include "common.hpp"

namespace gpsa {

constexpr int PCA_T = 64;            // tile edge of the Gram kernel
constexpr int PCA_KC = 32;           // rows of a chunk of the Gram kernel
constexpr int PCA_LD = 80;           // pitch of a staged chunk: rows k, k + 1 are 32 banks apart
constexpr int PCA_MAX_GROUPS = 32;   // row groups, at most
constexpr int PCA_FILL = 256;        // tile pairs from which the row split is off
constexpr int PCA_PR = 64;           // rows of a workgroup of the projection
constexpr int PCA_PC = 32;           // columns of a chunk of the projection
constexpr int PCA_PLD = 34;          // pitch of the projection's staged chunks
constexpr int PCA_MAX_K = 128;       // components, at most
typedef double pca_acc_t __attribute__((ext_vector_type(4)));

static inline long long pca_pairs(long long P) {
  const long long nt = cdiv(P, (long long)PCA_T);
  return nt * (nt + 1) / 2;
}
static inline int pca_groups(long long N, long long P) {
  const long long pairs = pca_pairs(P);
  if (pairs >= PCA_FILL) return 1;
  long long g = cdiv((long long)PCA_FILL, pairs);
  const long long chunks = cdiv(N, (long long)PCA_KC);
  if (g > PCA_MAX_GROUPS) g = PCA_MAX_GROUPS;
  if (g > chunks) g = chunks;
  return g < 1 ? 1 : (int)g;
}

// workgroup b -> the tile pair (lo <= hi), the lower triangle row by row (gpr.hip's decode)
__device__ __forceinline__ void pca_pair(long long b, long long& lo, long long& hi) {
  long long r = (long long)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= b) ++r;
  while (r * (r + 1) / 2 > b) --r;
  hi = r;
  lo = b - r * (r + 1) / 2;
}

// the view Y [n, P] (mean / inv_scale: the view's rows); blockIdx.x: tile pair, blockIdx.y: row group of R rows
template <bool SCALED>
__global__ void __launch_bounds__(256)
pca_gram_kernel(const float* __restrict__ Y, long long n, long long P, long long R, const double* __restrict__ mean,
                const double* __restrict__ inv_scale, double* planes, int accumulate) {
  __shared__ double za[PCA_KC][PCA_LD], zb[PCA_KC][PCA_LD];
  long long I, J;
  pca_pair(blockIdx.x, I, J);
  const bool diag = I == J;
  const long long r0 = (long long)blockIdx.y * R, r1 = min(n, r0 + R);
  if (accumulate && r0 >= n) return;  // block-uniform: this view has no rows for the group
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 32, j = lane & 15, kq = lane >> 4;
  // staging: this thread's column of both tiles, rows rq, rq + 4, ... of a chunk
  const int sc = tid & 63, rq = tid >> 6;
  const long long ca = I * PCA_T + sc, cb = J * PCA_T + sc;
  const bool oka = ca < P, okb = cb < P && !diag;
  const double ma = oka ? mean[ca] : 0.0, mb = okb ? mean[cb] : 0.0;
  const double sa = (SCALED && oka) ? inv_scale[ca] : 1.0, sb = (SCALED && okb) ? inv_scale[cb] : 1.0;
  float ya[PCA_KC / 4], yb[PCA_KC / 4];
  auto load = [&](long long k0) {
#pragma unroll
    for (int q = 0; q < PCA_KC / 4; ++q) {
      const long long row = k0 + rq + 4 * q;
      ya[q] = (oka && row < r1) ? Y[row * P + ca] : 0.f;
      yb[q] = (okb && row < r1) ? Y[row * P + cb] : 0.f;
    }
  };
  pca_acc_t acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = (pca_acc_t){0.0, 0.0, 0.0, 0.0};
  const double(*zB)[PCA_LD] = diag ? za : zb;
  if (r0 < r1) load(r0);
  for (long long k0 = r0; k0 < r1; k0 += PCA_KC) {
    __syncthreads();  // the previous chunk has been read
#pragma unroll
    for (int q = 0; q < PCA_KC / 4; ++q) {
      const bool in = k0 + rq + 4 * q < r1;  // rows beyond the group and columns beyond P contribute 0
      const double ta = (double)ya[q] - ma, tb = (double)yb[q] - mb;
      za[rq + 4 * q][sc] = (in && oka) ? (SCALED ? ta * sa : ta) : 0.0;
      if (!diag) zb[rq + 4 * q][sc] = (in && okb) ? (SCALED ? tb * sb : tb) : 0.0;
    }
    __syncthreads();
    if (k0 + PCA_KC < r1) load(k0 + PCA_KC);  // in flight under the MFMAs
#pragma unroll
    for (int ks = 0; ks < PCA_KC / 4; ++ks) {
      const int kk = ks * 4 + kq;
      const double a0 = za[kk][wm + j], a1 = za[kk][wm + 16 + j];
      const double b0 = zB[kk][wn + j], b1 = zB[kk][wn + 16 + j];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
  double* plane = planes + (long long)blockIdx.y * P * P;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long row = I * PCA_T + wm + 16 * ti + kq + 4 * r, col = J * PCA_T + wn + 16 * tj + j;
        if (row < P && col < P) {
          const long long e = row * P + col;
          plane[e] = accumulate ? plane[e] + acc[ti][tj][r] : acc[ti][tj][r];
        }
      }
}

// the planes [Gr][P, P] (upper tile pairs) added in ascending group -> out [P, P], every (a <= b) to both places;
// planes may BE out (Gr = 1): a thread reads only the element it writes back
__global__ void __launch_bounds__(256)
pca_gram_fold_kernel(const double* planes, int Gr, long long P, double* out) {
  long long I, J;
  pca_pair(blockIdx.x, I, J);
  const long long PP = P * P;
  for (int e = threadIdx.x; e < PCA_T * PCA_T; e += 256) {
    const int r = e >> 6, c = e & 63;
    const long long a = I * PCA_T + r, b = J * PCA_T + c;
    if (a >= P || b >= P || (I == J && r > c)) continue;
    double s = planes[a * P + b];
    for (int g = 1; g < Gr; ++g) s += planes[g * PP + a * P + b];
    out[a * P + b] = s;
    if (a != b) out[b * P + a] = s;
  }
}

// the view Y [n, P] -> out [n, k] (fp32 rounded once, or fp64); blockIdx.x: 64 rows
template <bool SCALED, bool OUT64>
__global__ void __launch_bounds__(256)
pca_project_kernel(const float* __restrict__ Y, long long n, long long P, const double* __restrict__ mean,
                   const double* __restrict__ inv_scale, const double* __restrict__ comp, int k,
                   void* __restrict__ out) {
  __shared__ double zs[PCA_PR][PCA_PLD], cs[PCA_MAX_K][PCA_PLD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, kq = lane >> 4;
  const int sc = tid & 31, sr = tid >> 5;  // staging: one column of the chunk, rows sr, sr + 8, ...
  const long long row0 = (long long)blockIdx.x * PCA_PR;
  const int KT = (k + 15) / 16;
  pca_acc_t acc[PCA_MAX_K / 16];
#pragma unroll
  for (int tj = 0; tj < PCA_MAX_K / 16; ++tj) acc[tj] = (pca_acc_t){0.0, 0.0, 0.0, 0.0};
  // a chunk in registers: this thread's 8 values of Y, its column's mean and scale, its 2 KT values of comp
  float yv[PCA_PR / 8];
  double cv[PCA_MAX_K / 8], m = 0.0, s = 1.0;
  bool okc = false;
  auto load = [&](long long c0) {
    const long long c = c0 + sc;
    okc = c < P;
    m = okc ? mean[c] : 0.0;
    s = (SCALED && okc) ? inv_scale[c] : 1.0;
#pragma unroll
    for (int q = 0; q < PCA_PR / 8; ++q) {
      const long long row = row0 + sr + 8 * q;
      yv[q] = (okc && row < n) ? Y[row * P + c] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < PCA_MAX_K / 8; ++q) {
      const int jj = sr + 8 * q;
      if (q < 2 * KT) cv[q] = (okc && jj < k) ? comp[(long long)jj * P + c] : 0.0;
    }
  };
  load(0);
  for (long long c0 = 0; c0 < P; c0 += PCA_PC) {
    __syncthreads();  // the previous chunk has been read
#pragma unroll
    for (int q = 0; q < PCA_PR / 8; ++q) {
      const double t = (double)yv[q] - m;
      // rows beyond n and columns beyond P contribute 0
      zs[sr + 8 * q][sc] = (okc && row0 + sr + 8 * q < n) ? (SCALED ? t * s : t) : 0.0;
    }
#pragma unroll
    for (int q = 0; q < PCA_MAX_K / 8; ++q)
      if (q < 2 * KT) cs[sr + 8 * q][sc] = cv[q];
    __syncthreads();
    if (c0 + PCA_PC < P) load(c0 + PCA_PC);  // in flight under the MFMAs
#pragma unroll
    for (int ks = 0; ks < PCA_PC / 4; ++ks) {
      const int kk = ks * 4 + kq;
      const double a = zs[w * 16 + j][kk];  // A lane (row j, k kq)
#pragma unroll
      for (int tj = 0; tj < PCA_MAX_K / 16; ++tj)
        if (tj < KT) acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, cs[16 * tj + j][kk], acc[tj], 0, 0, 0);
    }
  }
#pragma unroll
  for (int tj = 0; tj < PCA_MAX_K / 16; ++tj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long row = row0 + w * 16 + kq + 4 * r;
      const int col = 16 * tj + j;
      if (tj < KT && row < n && col < k) {
        if (OUT64)
          ((double*)out)[row * k + col] = acc[tj][r];
        else
          ((float*)out)[row * k + col] = (float)acc[tj][r];
      }
    }
}

// 0 = view_off[0] < ... < view_off[V] = N
static int pca_views_check(const long long* view_off, int V, long long N) {
  if (view_off == nullptr || V < 1 || view_off[0] != 0 || view_off[V] != N) return GPSA_EINVAL;
  for (int v = 0; v < V; ++v)
    if (view_off[v + 1] <= view_off[v]) return GPSA_EINVAL;
  return 0;
}

}  // namespace gpsa

extern "C" {

int gpsa_pca_gram_groups(long long N, long long P) {
  if (N < 1 || P < 1) return 0;
  return gpsa::pca_groups(N, P);
}

long long gpsa_pca_gram_workspace(long long N, long long P, int V) {
  if (N < 1 || P < 1 || V < 1) return 0;
  const int g = gpsa::pca_groups(N, P);
  return g > 1 ? 8LL * g * P * P : 0;
}

int gpsa_pca_gram_f32(const float* Y, long long N, long long P, const double* mean, const double* inv_scale,
                      const long long* view_off, int V, double* G, void* workspace, long long workspace_bytes,
                      void* stream) {
  using namespace gpsa;
  if (Y == nullptr || mean == nullptr || G == nullptr || N < 2 || P < 1) return GPSA_EINVAL;
  if (P >= (1LL << 21) || N > 0x7fffffffLL * (long long)PCA_KC) return GPSA_EINVAL;  // the grid's extent
  if (int rc = pca_views_check(view_off, V, N)) return rc;
  const int Gr = pca_groups(N, P);
  if (Gr > 1 && (workspace == nullptr || workspace_bytes < gpsa_pca_gram_workspace(N, P, V))) return GPSA_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  double* planes = Gr > 1 ? (double*)workspace : G;
  const dim3 grid((unsigned)pca_pairs(P), (unsigned)Gr);
  for (int v = 0; v < V; ++v) {
    const long long a = view_off[v], n = view_off[v + 1] - a;
    const long long R = cdiv(cdiv(n, (long long)Gr), (long long)PCA_KC) * PCA_KC;
    if (inv_scale != nullptr)
      pca_gram_kernel<true><<<grid, 256, 0, st>>>(Y + a * P, n, P, R, mean + v * P, inv_scale + v * P, planes, v > 0);
    else
      pca_gram_kernel<false><<<grid, 256, 0, st>>>(Y + a * P, n, P, R, mean + v * P, nullptr, planes, v > 0);
    GPSA_LAUNCH_CHECK();
  }
  pca_gram_fold_kernel<<<grid.x, 256, 0, st>>>(planes, Gr, P, G);
  GPSA_LAUNCH_CHECK();
  return 0;
}

int gpsa_pca_project_f32(const float* Y, long long N, long long P, const double* mean, const double* inv_scale,
                         const long long* view_off, int V, const double* comp, int k, void* scores, int out_f64,
                         void* stream) {
  using namespace gpsa;
  if (Y == nullptr || mean == nullptr || comp == nullptr || scores == nullptr || N < 1 || P < 1) return GPSA_EINVAL;
  if (k < 1 || k > PCA_MAX_K || (out_f64 != 0 && out_f64 != 1)) return GPSA_EINVAL;
  if (P > 0x7fffffffLL || N > 0x7fffffffLL * (long long)PCA_PR) return GPSA_EINVAL;  // the grid's extent
  if (int rc = pca_views_check(view_off, V, N)) return rc;
  hipStream_t st = as_stream(stream);
  for (int v = 0; v < V; ++v) {
    const long long a = view_off[v], n = view_off[v + 1] - a;
    const unsigned blocks = (unsigned)cdiv(n, (long long)PCA_PR);
    const float* Yv = Y + a * P;
    const double *mv = mean + v * P, *sv = inv_scale ? inv_scale + v * P : nullptr;
    void* ov = out_f64 ? (void*)((double*)scores + a * k) : (void*)((float*)scores + a * k);
    if (sv != nullptr && out_f64)
      pca_project_kernel<true, true><<<blocks, 256, 0, st>>>(Yv, n, P, mv, sv, comp, k, ov);
    else if (sv != nullptr)
      pca_project_kernel<true, false><<<blocks, 256, 0, st>>>(Yv, n, P, mv, sv, comp, k, ov);
    else if (out_f64)
      pca_project_kernel<false, true><<<blocks, 256, 0, st>>>(Yv, n, P, mv, sv, comp, k, ov);
    else
      pca_project_kernel<false, false><<<blocks, 256, 0, st>>>(Yv, n, P, mv, sv, comp, k, ov);
    GPSA_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
