// The step engine: VariationalGPSA.forward (gpsa/models/vgpsa.py:212-489) with the KL terms of loss_fn
// (vgpsa.py:498-530), and their backward, each as ONE host call that enqueues the whole launch sequence.
//
// What it changes against one autograd node per layer driven from Python:
//   * no per-launch host round trip (a step was ~160 launches x ~11 us of Python / ctypes each);
//   * the warp GPs of all free views share their launches (view-blocked layout: every per-view panel is an
//     [M, Cs] block with a common column stride Cs, zero padded, problem index = blockIdx.z / .y);
//   * every parameter gradient is accumulated in fp64 along all of its paths (K_uu, K_uf, mean function,
//     KL) and rounded to the fp32 parameter once, by step_finalize_kernel;
//   * nothing is allocated here: the caller passes a ``saved`` arena (forward -> backward) and a ``scratch``
//     arena; both sizes come from a dry run of the very code that uses them (Arena::dry).
//
// Math and precision plan: as spatial_alignment_amd/engine.py documents (fp64 factorisations, fp64 warp GP,
// fp64 projection + fp32 matrix-core contractions in the data GP, fp64 gradient sums).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "internal.hpp"

namespace gpsa {

constexpr int MAXMODS = GPSA_MAX_MODS;
constexpr int KM_MAXB_STEP = 16;  // views per batched launch (kmat.hip: KM_MAXB)

// ---------------------------------------------------------------------------------------------------------
// arenas
// ---------------------------------------------------------------------------------------------------------
struct Arena {
  char* base = nullptr;
  long long off = 0, high = 0;
  long long limit = -1;  // bytes behind ``base`` (the plan's scratch_bytes; -1: a dry run, nothing behind it)
  bool dry = false;
  bool overflow = false;  // a request went past ``limit``: GPSA_RUN refuses every launch from then on (the
                          // arena is sized by a dry run; a branch that run did not walk must not write past it silently)
  template <typename T>
  T* get(long long n) {
    off = (off + 255) & ~255LL;
    T* p = dry ? nullptr : reinterpret_cast<T*>(base + off);
    off += n * (long long)sizeof(T);
    if (off > high) high = off;
    if (!dry && limit >= 0 && off > limit) overflow = true;
    return p;
  }
  long long mark() const { return off; }
  void release(long long m) { off = m; }
};

#define GPSA_CK(x)               \
  do {                           \
    int rc__ = (x);              \
    if (rc__ != 0) return rc__;  \
  } while (0)
// launches are skipped in a dry run (which only measures the arenas)
#define GPSA_RUN(x)                                   \
  do {                                                \
    if (!dry) {                                       \
      if (c.sc.overflow) return GPSA_EWORKSPACE;      \
      GPSA_CK(x);                                     \
    }                                                 \
  } while (0)

// ---------------------------------------------------------------------------------------------------------
// device tables of a plan (uploaded once at creation)
// ---------------------------------------------------------------------------------------------------------
struct ViewTab {            // device copy: how the rows of the modalities map onto the view blocks
  int V, D, S, nm, nf;
  long long Cs;             // column stride of a view block
  const long long* vstart;  // [nm][V+1] first row of view v in modality m
  const long long* colbase; // [nm][V]   offset of modality m's rows inside view v's block
  const long long* nview;   // [V]       live columns of view v (spots of all modalities)
  const long long* epsoff;  // [V]       offset of view v's draws in eps_G (floats)
  const int* bidx;          // [V]       index among the free views, -1: fixed
};

struct ModPtrs {            // per-modality pointers passed by value
  const float* X[MAXMODS];
  float* Gm[MAXMODS];
  float* Gs[MAXMODS];
  double* G64[MAXMODS];
  const float* dGm[MAXMODS];
  const float* dGs[MAXMODS];
  const double* dG64[MAXMODS];
  long long N[MAXMODS];
};

// ---------------------------------------------------------------------------------------------------------
// kernels of the engine itself
// ---------------------------------------------------------------------------------------------------------

// blocks [0, V): view v: mu_z = scale (Z slopes + intercept) (fp32, the reference's mu_z_G; scale = 100 on a
// fixed view: quirk 7, inert), resid = delta - mu_z (fp64), and the rows r = j*V + v of the KL terms'
// mean-difference matrix (quirk 2: the KL pairs row r with view r % V, coordinate r / V).
// blocks >= V: the data GP's rows: Dd[t][i] = delta_F[m][i][l] (mu = 0), one block per 256 elements.
struct PrepArgs {
  const float *Xtilde, *delta_G, *slopes, *intercepts;
  const float* delta_F[MAXMODS];
  int L[MAXMODS], Loff[MAXMODS];
  int V, D, Mx, Mg, nm;
  const int* bidx;
  float* mu_z;
  double* resid;   // [V, Mx, D]
  double* Dw;      // [V*D, Mx]
  double* Dd;      // [sum L, Mg]
  int* zinfo[4];   // int words this launch zeroes: [0..1] owner computes: the Cholesky infos of a group (the matrices
  int nzinfo[4];   // left out keep 0); [2..3] the arrival counters of the KL forward's row slices (kl.hip); else null
};

__global__ void __launch_bounds__(256) step_prep_kernel(PrepArgs a) {
  const int D = a.D;
  if (blockIdx.x == 0)
    for (int g = 0; g < 4; ++g)
      if (a.zinfo[g] != nullptr)
        for (int i = threadIdx.x; i < a.nzinfo[g]; i += 256) a.zinfo[g][i] = 0;
  if ((int)blockIdx.x < a.V) {
    const int v = blockIdx.x;
    const double scale = a.bidx[v] < 0 ? 100.0 : 1.0;
    const float* Z = a.Xtilde + (long long)v * a.Mx * D;
    const float* dl = a.delta_G + (long long)v * a.Mx * D;
    const float* A = a.slopes + (long long)v * D * D;
    const float* b = a.intercepts + (long long)v * D;
    for (int i = threadIdx.x; i < a.Mx * D; i += 256) {
      const int m = i / D, j = i - m * D;
      double mu = (double)b[j];
      for (int d = 0; d < D; ++d) mu += (double)Z[m * D + d] * (double)A[d * D + j];
      mu *= scale;
      if (a.mu_z != nullptr) a.mu_z[(long long)v * a.Mx * D + i] = (float)mu;
      const double r = (double)dl[i] - mu;
      a.resid[(long long)v * a.Mx * D + i] = r;
      if (a.Dw != nullptr) a.Dw[((long long)j * a.V + v) * a.Mx + m] = r;
    }
    return;
  }
  if (a.Dd == nullptr) return;
  long long e = ((long long)blockIdx.x - a.V) * 256 + threadIdx.x;
  for (int m = 0; m < a.nm; ++m) {
    const long long cnt = (long long)a.L[m] * a.Mg;
    if (e < cnt) {
      const int l = (int)(e / a.Mg), i = (int)(e - (long long)l * a.Mg);
      a.Dd[((long long)a.Loff[m] + l) * a.Mg + i] = (double)a.delta_F[m][(long long)i * a.L[m] + l];
      return;
    }
    e -= cnt;
  }
}

// (view block b, column c) -> modality and row: the spots of view v are the concatenation over the
// modalities of their rows of v (vgpsa.py:284-294)
__device__ __forceinline__ bool block_col_to_row(const ViewTab& t, int v, long long c, int& m, long long& r) {
  for (int mm = 0; mm < t.nm; ++mm) {
    const long long lo = t.colbase[(long long)mm * t.V + v];
    const long long cnt = t.vstart[(long long)mm * (t.V + 1) + v + 1] - t.vstart[(long long)mm * (t.V + 1) + v];
    if (c >= lo && c < lo + cnt) {
      m = mm;
      r = t.vstart[(long long)mm * (t.V + 1) + v] + (c - lo);
      return true;
    }
  }
  return false;
}

// Xv[b][c][d] = coordinates of column c of free view b (zero in the padding); grid (Cs/256, nf)
__global__ void __launch_bounds__(256)
warp_gather_kernel(ViewTab t, const int* __restrict__ free_views, ModPtrs p, float* __restrict__ Xv) {
  const int b = blockIdx.y, v = free_views[b];
  const long long c = blockIdx.x * 256LL + threadIdx.x;
  if (c >= t.Cs) return;
  int m = 0;
  long long r = 0;
  const bool live = block_col_to_row(t, v, c, m, r);
  float* dst = Xv + ((long long)b * t.Cs + c) * t.D;
  for (int d = 0; d < t.D; ++d) dst[d] = live ? p.X[m][r * t.D + d] : 0.f;
}

constexpr double TWO_JITTER_STEP = 2e-5;  // the jitter enters the variance twice (vgpsa.py:191/201 and :204)

// Output-driven sampler of ALL views of one modality (vgpsa.py:186-191, 262-273, 334-351): thread = row r.
//   fixed view:  G_means = G_samples[s] = X (exactly)
//   free view:   var = exp(var_u[v]) - q + v_j + 2e-5;  mu = X slopes_v + intercept_v + mean_j;
//                G_samples[s] = mu + var * eps (variance used as the std: quirk 1)
// also writes the fp64 copy of the draws (what the data GP's covariance is built from) and one flag per
// block: a non-positive variance.
__global__ void __launch_bounds__(256)
warp_sample_views_fwd_kernel(ViewTab t, int m, const float* __restrict__ X, const double* __restrict__ meanT,
                             const double* __restrict__ vq, const double* __restrict__ q,
                             const float* __restrict__ var_u, const float* __restrict__ slopes,
                             const float* __restrict__ intercepts, const float* __restrict__ eps, long long N,
                             float* __restrict__ Gm, float* __restrict__ Gs, double* __restrict__ G64,
                             int* __restrict__ bad) {
  const long long r = blockIdx.x * 256LL + threadIdx.x;
  const int D = t.D, S = t.S;
  int flag = 0;
  if (r < N) {
    const long long* vs = t.vstart + (long long)m * (t.V + 1);
    int lo = 0, hi = t.V;  // view of row r: vs[v] <= r < vs[v+1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (vs[mid] <= r) lo = mid; else hi = mid;
    }
    int v = lo;
    while (v + 1 < t.V && vs[v + 1] <= r) ++v;  // skip empty views at the boundary
    const int b = t.bidx[v];
    double x[MAXD];
#pragma unroll
    for (int d = 0; d < MAXD; ++d) x[d] = d < D ? (double)X[r * D + d] : 0.0;
    if (b < 0) {
      for (int j = 0; j < D; ++j) {
        const float xf = X[r * D + j];
        Gm[r * D + j] = xf;
        for (int s = 0; s < S; ++s) {
          const long long e = ((long long)s * N + r) * D + j;
          Gs[e] = xf;
          G64[e] = (double)xf;
        }
      }
    } else {
      const long long cv = t.colbase[(long long)m * t.V + v] + (r - vs[v]);  // column in the view block
      const long long nv = t.nview[v];
      const double var0 = exp((double)var_u[v]), qc = q[(long long)b * t.Cs + cv];
      const float* A = slopes + (long long)v * D * D;
      const float* e0 = eps + t.epsoff[v];
      for (int j = 0; j < D; ++j) {
        const long long o = ((long long)b * D + j) * t.Cs + cv;
        const double var = var0 - qc + vq[o] + TWO_JITTER_STEP;
        double mu = (double)intercepts[(long long)v * D + j] + meanT[o];
#pragma unroll
        for (int d = 0; d < MAXD; ++d)
          if (d < D) mu += x[d] * (double)A[d * D + j];
        if (!(var > 0.0)) flag = 1;
        Gm[r * D + j] = (float)mu;
        for (int s = 0; s < S; ++s) {
          const double gv = mu + var * (double)e0[((long long)s * nv + cv) * D + j];
          const long long e = ((long long)s * N + r) * D + j;
          Gs[e] = (float)gv;
          G64[e] = gv;
        }
      }
    }
  }
  flag = __syncthreads_or(flag);
  if (threadIdx.x == 0) bad[blockIdx.x] = flag;
}

// Column-driven backward of the sampler: thread = (free view b, column c of its block).
//   dmu = dG_means + sum_s dG_s ;  g_j = sum_s dG_s eps ;  qbar = -sum_j g_j ;  part[b][block] = sum g
// with dG_s = (fp32 gradient of the API tensor, may be absent) + (fp64 gradient from the data GP, may be
// absent).  Zeros in the padding columns.  grid (Cs/256, nf).
__global__ void __launch_bounds__(256)
warp_sample_views_bwd_kernel(ViewTab t, const int* __restrict__ free_views, ModPtrs p,
                             const float* __restrict__ eps, double* __restrict__ dmeanT,
                             double* __restrict__ g, double* __restrict__ qbar, double* __restrict__ part,
                             int* __restrict__ tick, const float* __restrict__ var_u, double* __restrict__ dvar_s) {
  __shared__ double red[4];
  __shared__ int last_s;
  const int b = blockIdx.y, v = free_views[b], D = t.D, S = t.S;
  const long long c = blockIdx.x * 256LL + threadIdx.x;
  double gtot = 0.0;
  if (c < t.Cs) {
    int m = 0;
    long long r = 0;
    const bool live = block_col_to_row(t, v, c, m, r);
    const long long nv = t.nview[v], N = live ? p.N[m] : 0;
    const float* e0 = eps + t.epsoff[v];
    for (int j = 0; j < D; ++j) {
      double dm = 0.0, gj = 0.0;
      if (live) {
        if (p.dGm[m] != nullptr) dm = (double)p.dGm[m][r * D + j];
        for (int s = 0; s < S; ++s) {
          const long long e = ((long long)s * N + r) * D + j;
          double d = 0.0;
          if (p.dGs[m] != nullptr) d += (double)p.dGs[m][e];
          if (p.dG64[m] != nullptr) d += p.dG64[m][e];
          dm += d;
          gj += d * (double)e0[((long long)s * nv + c) * D + j];
        }
      }
      const long long o = ((long long)b * D + j) * t.Cs + c;
      dmeanT[o] = dm;
      g[o] = gj;
      gtot += gj;
    }
    qbar[(long long)b * t.Cs + c] = -gtot;
  }
  const double tot = block_sum(gtot, red);
  // dvar_s[b] = exp(var_u[v]) * sum_blocks part[b][.] (the variance enters var = sigma^2 - q + v directly), closed by the
  // view's LAST block to arrive, in the fixed order the finishing launch of rounds 1 - 5 used (round 6: one launch less)
  if (threadIdx.x == 0) {
    part[(long long)b * gridDim.x + blockIdx.x] = tot;
    __threadfence();
    last_s = tick != nullptr && atomicAdd(&tick[b], 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (last_s && threadIdx.x < 64) {  // (block-uniform; the first wave)
    __threadfence();
    double s = 0.0;
    for (long long i = threadIdx.x; i < (long long)gridDim.x; i += 64)
      s += __hip_atomic_load(&part[(long long)b * gridDim.x + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s = wave_sum(s);
    if (threadIdx.x == 0) {
      dvar_s[b] = s * exp((double)var_u[v]);
      tick[b] = 0;
    }
  }
}

// dvar_s[b] = exp(var_u[v]) * sum_blocks part[b][.]   (the variance enters var = sigma^2 - q + v directly)
__global__ void __launch_bounds__(64)
warp_sample_views_bwd_finish_kernel(const double* __restrict__ part, long long nblk,
                                    const int* __restrict__ free_views, const float* __restrict__ var_u,
                                    double* __restrict__ dvar_s) {
  const int b = blockIdx.x;
  double s = 0.0;
  for (long long i = threadIdx.x; i < nblk; i += 64) s += part[(long long)b * nblk + i];
  s = wave_sum(s);
  if (threadIdx.x == 0) dvar_s[b] = s * exp((double)var_u[free_views[b]]);
}

// flag[0] = max over the Cholesky infos and the samplers' block flags (all >= 0)
__global__ void __launch_bounds__(256)
flag_reduce_kernel(const int* __restrict__ a, long long na, const int* __restrict__ b, long long nb,
                   int* __restrict__ out) {
  __shared__ int red[256];
  int w = 0;
  for (long long i = threadIdx.x; i < na; i += 256) w = max(w, abs(a[i]));
  for (long long i = threadIdx.x; i < nb; i += 256) w = max(w, abs(b[i]));
  red[threadIdx.x] = w;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// out[i] += in[i]
__global__ void __launch_bounds__(256) add_inplace_kernel(double* __restrict__ out, const double* __restrict__ in,
                                                          long long n) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i < n) out[i] += in[i];
}

__global__ void __launch_bounds__(256) add_inplace_f32_kernel(float* __restrict__ out, const float* __restrict__ in,
                                                              long long n) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i < n) out[i] += in[i];
}

template <typename TS, typename TD>
__global__ void __launch_bounds__(256) convert_kernel_step(const TS* __restrict__ src, long long n,
                                                           TD* __restrict__ dst) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i < n) dst[i] = (TD)src[i];
}

// q[c] = sum_m A[m,c] B[m,c]   ([M,C] panels; blockIdx.y = problem of a batch at stride M*C, q at stride C)
__global__ void __launch_bounds__(256)
coldot2_kernel(const double* __restrict__ A, const double* __restrict__ B, int M, long long C,
               double* __restrict__ q) {
  const long long c = blockIdx.x * 256LL + threadIdx.x;
  if (c >= C) return;
  const long long pb = (long long)blockIdx.y * M * C;
  double s0 = 0.0, s1 = 0.0;
  int m = 0;
  for (; m + 1 < M; m += 2) {
    s0 += A[pb + (long long)m * C + c] * B[pb + (long long)m * C + c];
    s1 += A[pb + (long long)(m + 1) * C + c] * B[pb + (long long)(m + 1) * C + c];
  }
  if (m < M) s0 += A[pb + (long long)m * C + c] * B[pb + (long long)m * C + c];
  q[(long long)blockIdx.y * C + c] = s0 + s1;
}

// exact inducing-point gradient: W = G + q o A (the factor of dK_uu = -W A^T) and U = W + q o A (= dK_uf), [M, C]
// fp64 panels, q [C]; U may alias G
__global__ void __launch_bounds__(256)
exact_axpy2_kernel(const double* G, const double* __restrict__ A, const double* __restrict__ q, int M, long long C,
                   double* __restrict__ W, double* U) {
  const long long c = blockIdx.x * 256LL + threadIdx.x;
  if (c >= C) return;
  const double qc = q[c];
  for (int m = blockIdx.y; m < M; m += gridDim.y) {
    const long long o = (long long)m * C + c;
    const double t = qc * A[o], w = G[o] + t;
    W[o] = w;
    U[o] = w + t;
  }
}

// Every small parameter gradient of the step from its fp64 pieces, rounded to fp32 ONCE:
//   Xtilde[v]   = dZ(K_uf) + dZ(K_uu) - scale * dresid slopes_v^T          (free views; zero for fixed)
//   delta_G[v]  = dresid                                                   (dresid = layer's share + KL's)
//   warp_ls[v]  = dls(K_uf) + dls(K_uu);  warp_var[v] = dvar(K_uf) + dvar(K_uu) + dvar(sampler)
//   Gtilde      = sum_passes dZ(K_uf) + dZ(K_uu);  data_ls / data_var likewise (+ the samplers' share)
//   delta_F[m]  = ddc (layer, fp32 [Mg, L]) + KL's dD rows ([L, Mg], transposed)
struct FinalArgs {
  int part;  // 0: everything; 1: only delta_F (the data GP's span, finished early); 2: everything but delta_F
  int V, D, Mx, Mg, nm, nf, npass;
  const int* bidx;
  const float* slopes;
  const double *dZ_wf, *dZ_wu, *dpar_wf, *dpar_wu, *dvar_ws;  // per free view b: [Mx,D], [Mx,D], [2], [2], [1]
  const double* dresid;                                        // [V, Mx, D] layer's share (free views)
  const double* dD_w;                                          // [V*D, Mx] KL's share, row j*V+v (or NULL)
  const double *dZ_df, *dpar_df;                               // per pass: [Mg, D], [2]
  const double* dvar_ds;                                       // per pass: [1] (the sampler's share, fp64: round 5)
  const double *dZ_du, *dpar_du;                               // K_uu of the data GP
  const float* ddc_F[MAXMODS];                                 // [Mg, L] or NULL (no gradient reached F)
  const double* dD_d;                                          // [sum L, Mg] or NULL
  int L[MAXMODS], Loff[MAXMODS];
  gpsa_step_param_grads out;
  const float* loss_src;  // gpsa_step_io.loss_src / loss_dst: the rank's loss into the all-reduce bucket (or NULL)
  float* loss_dst;
};

__global__ void __launch_bounds__(256) step_finalize_kernel(FinalArgs a) {
  const int D = a.D;
  const long long nX = (long long)a.V * a.Mx * D;
  long long e = blockIdx.x * 256LL + threadIdx.x;
  const long long nsmall = nX + 2LL * a.V + (long long)a.Mg * D + 2;  // everything in front of delta_F
  if (a.part == 1) e += nsmall;          // (the launch covers the delta_F entries only)
  // the loss slot rides the closing launch (part 0, or 2 in the early order: part 1 is never the last): thread 0
  if (a.part != 1 && e == 0 && a.loss_dst != nullptr) *a.loss_dst = *a.loss_src;
  if (a.part == 2 && e >= nsmall) return;
  // --- Xtilde / delta_G
  if (e < nX) {
    const int v = (int)(e / ((long long)a.Mx * D));
    const int i = (int)(e - (long long)v * a.Mx * D), m = i / D, j = i - m * D;
    const int b = a.bidx[v];
    double gx = 0.0, gd = 0.0;
    if (b >= 0) {
      const double* dr = a.dresid + (long long)v * a.Mx * D;
      gd = dr[i];
      if (a.dD_w != nullptr) gd += a.dD_w[((long long)j * a.V + v) * a.Mx + m];
      // mean function at the inducing points: resid = delta - (Z A + b)  =>  dZ = - dresid_total A^T
      double mr = 0.0;
      for (int jj = 0; jj < D; ++jj) {
        double t = dr[m * D + jj];
        if (a.dD_w != nullptr) t += a.dD_w[((long long)jj * a.V + v) * a.Mx + m];
        mr += t * (double)a.slopes[(long long)v * D * D + j * D + jj];
      }
      gx = -mr;
      if (a.dZ_wf != nullptr) gx += a.dZ_wf[(long long)b * a.Mx * D + i];
      gx += a.dZ_wu[(long long)b * a.Mx * D + i];
    }
    if (a.out.Xtilde != nullptr) a.out.Xtilde[e] = (float)gx;
    if (a.out.delta_G != nullptr) a.out.delta_G[e] = (float)gd;
    return;
  }
  e -= nX;
  // --- warp hyper-parameters
  if (e < 2LL * a.V) {
    const int v = (int)(e >> 1), which = (int)(e & 1), b = a.bidx[v];
    double gsum = 0.0;
    if (b >= 0) {
      gsum = a.dpar_wu[(long long)b * 2 + which];
      if (a.dpar_wf != nullptr) gsum += a.dpar_wf[(long long)b * 2 + which];
      if (which == 1 && a.dvar_ws != nullptr) gsum += a.dvar_ws[b];
    }
    float* dst = which == 0 ? a.out.warp_ls : a.out.warp_var;
    if (dst != nullptr) dst[v] = (float)gsum;
    return;
  }
  e -= 2LL * a.V;
  // --- Gtilde
  const long long nG = (long long)a.Mg * D;
  if (e < nG) {
    double gsum = a.dZ_du[e];
    for (int p = 0; p < a.npass; ++p) gsum += a.dZ_df[(long long)p * nG + e];
    if (a.out.Gtilde != nullptr) a.out.Gtilde[e] = (float)gsum;
    return;
  }
  e -= nG;
  if (e < 2) {
    double gsum = a.dpar_du[e];
    for (int p = 0; p < a.npass; ++p) {
      gsum += a.dpar_df[(long long)p * 2 + e];
      if (e == 1) gsum += a.dvar_ds[p];
    }
    float* dst = e == 0 ? a.out.data_ls : a.out.data_var;
    if (dst != nullptr) dst[0] = (float)gsum;
    return;
  }
  e -= 2;
  // --- delta_F[m] [Mg, L]
  for (int m = 0; m < a.nm; ++m) {
    const long long cnt = (long long)a.Mg * a.L[m];
    if (e < cnt) {
      if (a.out.delta_F[m] == nullptr) return;
      const int i = (int)(e / a.L[m]), l = (int)(e - (long long)i * a.L[m]);
      double gsum = a.ddc_F[m] != nullptr ? (double)a.ddc_F[m][e] : 0.0;
      if (a.dD_d != nullptr) gsum += a.dD_d[((long long)a.Loff[m] + l) * a.Mg + i];
      a.out.delta_F[m][e] = (float)gsum;
      return;
    }
    e -= cnt;
  }
}

// ---- fused Adam over a list of tensors --------------------------------------------------------------------
constexpr int ADAM_MAXT = 16;
struct AdamArgs {
  float* p[ADAM_MAXT];
  const float* g[ADAM_MAXT];
  float* m[ADAM_MAXT];
  float* v[ADAM_MAXT];
  long long blk0[ADAM_MAXT + 1];  // first block of tensor i (1024 elements per block)
  long long n[ADAM_MAXT];
  int nt;
  double lr, b1, b2, eps;
};

__global__ void adam_tick_kernel(float* step) { step[0] += 1.f; }

// torch.optim.Adam's update in its fp32 arithmetic (torch/optim/adam.py, single-tensor path):
//   m = lerp(m, g, 1-b1);  v = b2 v + (1-b2) g g;  p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
__global__ void __launch_bounds__(256) adam_kernel(AdamArgs a, const float* __restrict__ step) {
  int t = 0;
  while (t + 1 < a.nt && (long long)blockIdx.x >= a.blk0[t + 1]) ++t;
  // the scalars are formed in double, as Python does for torch's optimiser, then used in fp32 tensor arithmetic
  const double tt = (double)step[0];
  const float step_size = (float)(a.lr / (1.0 - pow(a.b1, tt))), rs2 = (float)sqrt(1.0 - pow(a.b2, tt));
  const float w1 = (float)(1.0 - a.b1), b2 = (float)a.b2, w2 = (float)(1.0 - a.b2), eps = (float)a.eps;
  const long long base = ((long long)blockIdx.x - a.blk0[t]) * 1024;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long i = base + u * 256 + threadIdx.x;
    if (i < a.n[t]) {
      const float g = a.g[t][i];
      float m = a.m[t][i], v = a.v[t][i];
      m = m + w1 * (g - m);
      v = b2 * v + w2 * g * g;
      a.m[t][i] = m;
      a.v[t][i] = v;
      const float denom = sqrtf(v) / rs2 + eps;
      a.p[t][i] = a.p[t][i] - step_size * (m / denom);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------------
struct Group {  // matrices of one size, factorised together: the priors first, then the variational ones
  int M = 0, n_prior = 0, n_omega = 0, kl_off = 0;
  // offsets into the saved arena (bytes)
  long long o_mats = 0, o_inv = 0, o_logdet = 0, o_info = 0, o_D = 0, o_KD = 0;
  // device index tables of the grouped KL kernels
  int *om_idx = nullptr, *pr_idx = nullptr, *pr_list = nullptr, *grp_off = nullptr, *order = nullptr;
  // owner computes (gpsa_step_desc.kl_own_lo / _hi): the terms own_lo <= t < own_hi of this group are this plan's; the
  // others are listed as absent in the tables above and their covariances are never factorised
  int own_lo = 0, own_hi = 0;
  bool own_all() const { return own_lo == 0 && own_hi == n_omega; }
  int nb() const { return n_prior + n_omega; }
};

struct Run { int v0, b0, cnt; };

struct Pass {  // one evaluation of the data GP: a modality's own spots, or its G_test
  int m = 0;
  bool test = false;
  long long C = 0;          // columns = S * rows
  long long o_alpha = 0, o_sigma = 0;
  long long o_keep = -1;  // [L][Mg][C] fp32 products Omega_l alpha kept for the backward (-1: not kept)
  long long o_alpha64 = -1;  // [Mg][C] the projection unrounded (exact_inducing_grad; -1: not kept)
  // fused ELBO (gpsa_quadform_elbo_f32): g_ext [L+1][C], dmeanT [L][C], abar [Mg][C] live from the forward to the
  // backward (-1: this pass cannot run fused: a test pass, LMC, more than 13 row tiles)
  long long o_fuse = -1;
  bool x3 = false;   // the fused ELBO pass runs panel_elbo_x3_kernel (gpsa_step_desc.contraction = 1)
  bool gx3 = false;  // the data GP's Gram runs gram_x3_kernel (the same)
  bool fused(const gpsa_step_io& io) const { return io.fuse_elbo != 0 && o_fuse >= 0 && io.Y[m] != nullptr; }
};

struct Plan {
  gpsa_step_desc d;
  std::vector<int> fixed;
  std::vector<long long> rows;  // [nm*V]
  int V, D, S, Mx, Mg, nm, nf;
  std::vector<int> free_views, bidx;
  std::vector<long long> nview, epsoff;
  long long Cs = 0, eps_total = 0;
  std::vector<Run> runs;
  bool merged = false;
  int ng = 0;
  Group grp[2];
  int Loff[MAXMODS], Ltot = 0;
  std::vector<Pass> passes;
  // saved arena
  long long o_klcache = 0;  // the KL terms of the forward that filled this arena (io.reuse_mm hands them out again)
  long long o_resid = 0, o_Xv = 0, o_alpha_w = 0, o_Wk = 0, o_G64[MAXMODS], o_bad = 0, saved_bytes = 0;
  long long saved_bytes_nokeep = 0;   // arena without the kept products (they sit at its end)
  long long o_apk_w = 0, o_apk_d = 0;  // packed inverses of the projection kernel: forward packs, backward reuses
  long long nbad = 0;
  long long scratch_bytes = 0;
  long long bwd_acc_bytes = 0;  // accumulator of a microbatched step's slices (step_backward: io.bwd_acc)
  // device tables
  char* dev = nullptr;
  ViewTab tab;
  int* d_free = nullptr;
  // optional HIP-event timing of the three contraction launches of the first data-GP pass (bench.py's
  // roofline figures): slot = step index modulo the ring, 2 events per kernel
  std::vector<hipEvent_t> tev;
  bool skip_seen = false;  // the last fused ELBO launch left the NaN entries of Y out (gpsa_step_io.skip_missing)
  // gpsa_step_likelihood: the likelihood of modality m's fused ELBO pass and, for a Poisson one, its rows' log offsets
  int lik[GPSA_MAX_MODS] = {};
  const float* log_offset[GPSA_MAX_MODS] = {};
  // gpsa_step_dispersion: a negative binomial modality's rho [L], its per-element u [L, C] and their per-output sums [L]
  const float* log_disp[GPSA_MAX_MODS] = {};
  float* u_elems[GPSA_MAX_MODS] = {};
  double* usum[GPSA_MAX_MODS] = {};
  int tslots = 0, tfwd = 0, tbwd = 0;
  void tick(int kernel, int edge, bool fwd, hipStream_t st) {
    if (tslots == 0) return;
    const int slot = (fwd ? tfwd : tbwd) % tslots;
    (void)hipEventRecord(tev[(size_t)(slot * 3 + kernel) * 2 + edge], st);
  }

  // hipGraph cache of the plan's launch sequences (round 5; see graph_call below)
  struct GraphKey {  // raw bytes (a member-wise copy of the structs need not carry their padding: memcmp would differ)
    static constexpr size_t O_IO = sizeof(gpsa_step_params), O_OG = O_IO + sizeof(gpsa_step_io),
                            O_PG = O_OG + sizeof(gpsa_step_out_grads), O_PTR = O_PG + sizeof(gpsa_step_param_grads),
                            BYTES = O_PTR + 3 * sizeof(void*) + 2 * sizeof(int);
    unsigned char b[BYTES];
    int stages() const { int v; memcpy(&v, b + O_PTR + 3 * sizeof(void*), sizeof(int)); return v; }
    int bwd() const { int v; memcpy(&v, b + O_PTR + 3 * sizeof(void*) + sizeof(int), sizeof(int)); return v; }
    void set(const gpsa_step_params* prm, const gpsa_step_io* io, const gpsa_step_out_grads* og,
             const gpsa_step_param_grads* pg, const void* saved, const void* scratch, const void* stream, int stages_,
             int bwd_) {
      memset(b, 0, BYTES);
      memcpy(b, prm, sizeof(*prm));
      memcpy(b + O_IO, io, sizeof(*io));
      if (og) memcpy(b + O_OG, og, sizeof(*og));
      if (pg) memcpy(b + O_PG, pg, sizeof(*pg));
      const void* ptrs[3] = {saved, scratch, stream};
      memcpy(b + O_PTR, ptrs, sizeof(ptrs));
      const int tail[2] = {stages_, bwd_};
      memcpy(b + O_PTR + sizeof(ptrs), tail, sizeof(tail));
    }
  };
  struct GraphEntry {
    GraphKey key;
    hipGraphExec_t exec;
    unsigned long long used;
    hipStream_t last;  // the stream of its most recent launch (the key holds the stream, so this is the key's - kept
                       // explicitly: the eviction below retires a graph behind ITS stream, not the current call's)
  };
  std::vector<GraphEntry> graphs;
  // executable graphs dropped from the cache while a launch of theirs may still be queued on the caller's stream: each
  // waits here behind an event recorded on that stream and is destroyed once the event has fired
  struct Retired {
    hipGraphExec_t exec;
    hipEvent_t ev;
  };
  std::vector<Retired> retired;
  std::vector<GraphKey> seen;   // argument sets met once (a second meeting captures)
  hipStream_t gstream = nullptr;  // captures run on a stream of the plan's own (the caller's may be the null stream,
                                  // which cannot be captured); the graph is then launched into the caller's
  unsigned long long gtick = 0;
  long long g_hits = 0, g_eager = 0, g_captures = 0, g_idle_captures = 0;
  int g_enabled = -1;           // -1: GPSA_STEP_GRAPH decides (default off)
  long long n_early = 0;        // backwards that took the early order (gpsa_step_io.f_event)

  Group& gw() { return grp[0]; }
  Group& gd() { return merged ? grp[0] : grp[1]; }
  int pos_Kw(int b) const { return b; }
  int pos_KF() const { return merged ? nf : 0; }
  int pos_OmG(int r) const { return grp[0].n_prior + r; }
  int pos_OmF(int m, int l) const { return merged ? grp[0].n_prior + V * D + Loff[m] + l : 1 + Loff[m] + l; }
};

static long long align256(long long x) { return (x + 255) & ~255LL; }

static void free_plan(Plan* p) {
  if (p == nullptr) return;
  if (p->dev != nullptr) (void)hipFree(p->dev);
  for (hipEvent_t e : p->tev) (void)hipEventDestroy(e);
  if (!p->graphs.empty() || !p->retired.empty()) (void)hipDeviceSynchronize();  // nothing of theirs is in flight any more
  for (auto& ge : p->graphs)
    if (ge.exec != nullptr) (void)hipGraphExecDestroy(ge.exec);
  for (auto& r : p->retired) {
    (void)hipGraphExecDestroy(r.exec);
    (void)hipEventDestroy(r.ev);
  }
  if (p->gstream != nullptr) (void)hipStreamDestroy(p->gstream);
  delete p;
}

static Plan* make_plan(const gpsa_step_desc* dsc, bool host_only = false) {
  if (dsc == nullptr) return nullptr;
  const int V = dsc->n_views, D = dsc->n_dims, nm = dsc->n_mods, S = dsc->n_samples;
  if (V < 1 || D < 1 || D > MAXD || nm < 1 || nm > MAXMODS || S < 0 || dsc->m_x < 1 || dsc->m_g < 1)
    return nullptr;
  if (dsc->view_fixed == nullptr || dsc->view_rows == nullptr) return nullptr;
  if (dsc->contraction != 0 && dsc->contraction != 1) return nullptr;
  Plan* p = new (std::nothrow) Plan();
  if (p == nullptr) return nullptr;
  p->d = *dsc;
  p->fixed.assign(dsc->view_fixed, dsc->view_fixed + V);
  p->rows.assign(dsc->view_rows, dsc->view_rows + (long long)nm * V);
  p->d.view_fixed = nullptr;
  p->d.view_rows = nullptr;
  p->V = V; p->D = D; p->S = S; p->Mx = dsc->m_x; p->Mg = dsc->m_g; p->nm = nm;
  p->bidx.assign(V, -1);
  p->nview.assign(V, 0);
  p->epsoff.assign(V, 0);
  for (int m = 0; m < nm; ++m) {
    long long tot = 0;
    for (int v = 0; v < V; ++v) {
      if (p->rows[(long long)m * V + v] < 0) { free_plan(p); return nullptr; }
      tot += p->rows[(long long)m * V + v];
    }
    if (tot != dsc->n_rows[m] || dsc->n_latent[m] < 1 || dsc->n_out[m] < 1) { free_plan(p); return nullptr; }
    if (!dsc->has_lmc[m] && dsc->n_latent[m] != dsc->n_out[m]) { free_plan(p); return nullptr; }
  }
  long long maxn = 0;
  for (int v = 0; v < V; ++v) {
    for (int m = 0; m < nm; ++m) p->nview[v] += p->rows[(long long)m * V + v];
    if (!p->fixed[v]) {
      p->bidx[v] = (int)p->free_views.size();
      p->free_views.push_back(v);
      p->epsoff[v] = p->eps_total;
      p->eps_total += (long long)S * p->nview[v] * D;
      if (p->nview[v] > maxn) maxn = p->nview[v];
    }
  }
  p->nf = (int)p->free_views.size();
  p->Cs = (maxn + 63) / 64 * 64;
  // maximal runs of consecutive free views (uniform strides in the per-view parameter arrays), <= 16 each
  for (int b = 0; b < p->nf;) {
    int e = b + 1;
    while (e < p->nf && p->free_views[e] == p->free_views[e - 1] + 1 && e - b < KM_MAXB_STEP) ++e;
    p->runs.push_back(Run{p->free_views[b], b, e - b});
    b = e;
  }
  p->Ltot = 0;
  for (int m = 0; m < nm; ++m) {
    p->Loff[m] = p->Ltot;
    p->Ltot += dsc->n_latent[m];
  }
  for (int m = nm; m < MAXMODS; ++m) p->Loff[m] = p->Ltot;
  p->merged = p->Mx == p->Mg;
  if (p->merged) {
    p->ng = 1;
    p->grp[0].M = p->Mx;
    p->grp[0].n_prior = p->nf + 1;
    p->grp[0].n_omega = V * D + p->Ltot;
    p->grp[0].kl_off = 0;
  } else {
    p->ng = 2;
    p->grp[0].M = p->Mx; p->grp[0].n_prior = p->nf; p->grp[0].n_omega = V * D; p->grp[0].kl_off = 0;
    p->grp[1].M = p->Mg; p->grp[1].n_prior = 1; p->grp[1].n_omega = p->Ltot; p->grp[1].kl_off = V * D;
  }
  for (int g = 0; g < p->ng; ++g) {
    Group& G = p->grp[g];
    G.own_lo = 0;
    G.own_hi = G.n_omega;
    if (dsc->kl_own_hi > 0) {  // this plan's range of the global term list, cut to the group's terms
      const int lo = dsc->kl_own_lo - G.kl_off, hi = dsc->kl_own_hi - G.kl_off;
      G.own_lo = lo < 0 ? 0 : (lo > G.n_omega ? G.n_omega : lo);
      G.own_hi = hi < G.own_lo ? G.own_lo : (hi > G.n_omega ? G.n_omega : hi);
    }
  }
  // data-GP passes
  for (int m = 0; m < nm; ++m)
    if (dsc->n_rows[m] > 0 && S > 0) {
      Pass q; q.m = m; q.test = false; q.C = (long long)S * dsc->n_rows[m];
      p->passes.push_back(q);
    }
  if (dsc->s_test > 0)
    for (int m = 0; m < nm; ++m)
      if (dsc->n_test[m] > 0) {
        Pass q; q.m = m; q.test = true; q.C = (long long)dsc->s_test * dsc->n_test[m];
        p->passes.push_back(q);
      }
  // ---- saved arena layout
  long long o = 0;
  auto take = [&](long long bytes) { long long r = o; o = align256(o + bytes); return r; };
  for (int g = 0; g < p->ng; ++g) {
    Group& G = p->grp[g];
    const long long mm = (long long)G.M * G.M;
    G.o_mats = take(G.nb() * mm * 8);
    G.o_inv = take(G.nb() * mm * 8);
    G.o_logdet = take(G.nb() * 8LL);
    G.o_info = take(G.nb() * 4LL);
    G.o_D = take((long long)G.n_omega * G.M * 8);
    G.o_KD = take((long long)G.n_omega * G.M * 8);
  }
  p->o_klcache = take(((long long)V * D + p->Ltot) * 8);
  p->o_resid = take((long long)V * p->Mx * D * 8);
  p->o_Xv = take((long long)p->nf * p->Cs * D * 4);
  p->o_alpha_w = take((long long)p->nf * p->Mx * p->Cs * 8);
  p->o_Wk = take((long long)p->nf * D * p->Mx * p->Cs * 8);
  for (int m = 0; m < nm; ++m) p->o_G64[m] = take((long long)S * dsc->n_rows[m] * D * 8);
  p->nbad = 0;
  for (int m = 0; m < nm; ++m) p->nbad += (dsc->n_rows[m] + 255) / 256;
  p->o_bad = take((p->nbad + 1) * 4);
  for (auto& q : p->passes) {
    q.o_alpha = take((long long)p->Mg * q.C * 4);
    q.o_sigma = take((long long)dsc->n_latent[q.m] * q.C * 4);
    if (dsc->exact_inducing_grad) q.o_alpha64 = take((long long)p->Mg * q.C * 8);
    const int Lq = dsc->n_latent[q.m];
    if (!q.test && !dsc->has_lmc[q.m] && gpsa_quadform_elbo_f32_workspace(p->Mg, q.C, Lq) > 0) {
      q.o_fuse = take((2LL * Lq + 1 + p->Mg) * q.C * 4);
      q.x3 = dsc->contraction == 1 && gpsa_quadform_elbo_x3_f32_workspace(p->Mg, q.C, Lq) > 0;
    }
    q.gx3 = !q.test && dsc->contraction == 1 && gpsa_quadform_bwd_omega_x3_workspace(p->Mg, q.C, Lq) > 0;
  }
  p->o_apk_w = take(gpsa_whiten_workspace(p->Mx) * (long long)(p->nf > 0 ? p->nf : 1));
  p->o_apk_d = take(gpsa_whiten_workspace(p->Mg));
  p->saved_bytes_nokeep = o + 256;
  // The data GPs' products Omega_l alpha, kept by a training forward so that the backward streams them instead
  // of recomputing L M x M x C products.  At the END of the arena (a forward without a backward allocates only
  // the part before them); only while they stay within GPSA_KEEP_GB (default 48) GiB in total.
  {
    static const double keep_gb = [] { const char* e = getenv("GPSA_KEEP_GB"); return e ? atof(e) : 48.0; }();
    double budget = keep_gb * 1073741824.0;
    if (dsc->keep_budget_bytes > 0) {
      budget = (double)dsc->keep_budget_bytes;  // the caller has looked at its allocator (step_engine.get_plan)
    } else if (dsc->keep_budget_bytes < 0) {
      budget = -1.0;
    } else if (!host_only) {  // no figure from the caller: never plan beyond what the device has free right now
      size_t fr = 0, total = 0;
      if (hipMemGetInfo(&fr, &total) == hipSuccess && 0.6 * (double)fr < budget) budget = 0.6 * (double)fr;
    }
    long long tot = 0;
    bool ok = true;
    for (auto& q : p->passes) {
      const long long b = gpsa_quadform_keep_f32_bytes(p->Mg, q.C, dsc->n_latent[q.m]);
      if (b == 0) ok = false;
      tot += b;
    }
    if (ok && (double)tot <= budget)
      for (auto& q : p->passes) q.o_keep = take(gpsa_quadform_keep_f32_bytes(p->Mg, q.C, dsc->n_latent[q.m]));
  }
  p->saved_bytes = o + 256;
  // ---- device tables
  const long long n_ll = (long long)nm * (V + 1) + (long long)nm * V + V + V;  // vstart, colbase, nview, epsoff
  long long n_int = V /*bidx*/ + p->nf /*free*/;
  for (int g = 0; g < p->ng; ++g) {
    const Group& G = p->grp[g];
    n_int += 2 * G.n_omega + G.n_prior + (G.n_prior + 2) + G.n_omega;
  }
  const long long bytes = n_ll * 8 + n_int * 4 + 64;
  std::vector<char> host((size_t)bytes, 0);
  long long* hl = reinterpret_cast<long long*>(host.data());
  int* hi = reinterpret_cast<int*>(host.data() + n_ll * 8);
  // host_only (gpsa_step_describe): the tables are built but never uploaded; the pointers into them are only
  // ever handed to launches, which a dry run skips
  if (!host_only && hipMalloc(reinterpret_cast<void**>(&p->dev), (size_t)bytes) != hipSuccess) { p->dev = nullptr; free_plan(p); return nullptr; }
  long long* dl = reinterpret_cast<long long*>(p->dev);
  int* di = reinterpret_cast<int*>(p->dev + n_ll * 8);
  long long lo = 0, io = 0;
  // vstart [nm][V+1], colbase [nm][V]
  p->tab.vstart = dl + lo;
  for (int m = 0; m < nm; ++m) {
    long long acc = 0;
    for (int v = 0; v <= V; ++v) {
      hl[lo++] = acc;
      if (v < V) acc += p->rows[(long long)m * V + v];
    }
  }
  p->tab.colbase = dl + lo;
  for (int m = 0; m < nm; ++m)
    for (int v = 0; v < V; ++v) {
      long long acc = 0;
      for (int mm = 0; mm < m; ++mm) acc += p->rows[(long long)mm * V + v];
      hl[lo++] = acc;
    }
  p->tab.nview = dl + lo;
  for (int v = 0; v < V; ++v) hl[lo++] = p->nview[v];
  p->tab.epsoff = dl + lo;
  for (int v = 0; v < V; ++v) hl[lo++] = p->epsoff[v];
  p->tab.bidx = di + io;
  for (int v = 0; v < V; ++v) hi[io++] = p->bidx[v];
  p->d_free = di + io;
  for (int b = 0; b < p->nf; ++b) hi[io++] = p->free_views[b];
  for (int g = 0; g < p->ng; ++g) {
    Group& G = p->grp[g];
    // prior of term t of this group (position among the group's priors), -1: absent (fixed view)
    std::vector<int> prior(G.n_omega, -1);
    for (int t = 0; t < G.n_omega; ++t) {
      if (g == 0 && t < V * D) prior[t] = p->bidx[t % V];  // quirk 2: row r pairs with view r % V
      else prior[t] = p->merged ? p->nf : 0;
      if (t < G.own_lo || t >= G.own_hi) prior[t] = -1;  // another rank's term (owner computes)
    }
    G.om_idx = di + io;
    for (int t = 0; t < G.n_omega; ++t) hi[io++] = G.n_prior + t;
    G.pr_idx = di + io;
    for (int t = 0; t < G.n_omega; ++t) hi[io++] = prior[t];
    G.pr_list = di + io;
    for (int q = 0; q < G.n_prior; ++q) hi[io++] = q;
    std::vector<int> order, off(1, 0);
    for (int q = 0; q <= G.n_prior; ++q) {
      const int want = q < G.n_prior ? q : -1;
      for (int t = 0; t < G.n_omega; ++t)
        if (prior[t] == want) order.push_back(t);
      off.push_back((int)order.size());
    }
    G.grp_off = di + io;
    for (int q = 0; q < G.n_prior + 2; ++q) hi[io++] = off[q];
    G.order = di + io;
    for (int t = 0; t < G.n_omega; ++t) hi[io++] = order[t];
  }
  if (!host_only && hipMemcpy(p->dev, host.data(), (size_t)bytes, hipMemcpyHostToDevice) != hipSuccess) { free_plan(p); return nullptr; }
  p->tab.V = V; p->tab.D = D; p->tab.S = S; p->tab.nm = nm; p->tab.nf = p->nf; p->tab.Cs = p->Cs;
  return p;
}

// ---------------------------------------------------------------------------------------------------------
// sequencing helpers
// ---------------------------------------------------------------------------------------------------------
static inline int splitk_for(long long k, int m, int n) {  // ops.HipOps.pick_splitk
  const long long tiles = cdiv(m, 64) * cdiv(n, 64);
  long long s = cdiv(512, tiles > 0 ? tiles : 1);
  if (s > 256) s = 256;
  if (s > k / 64) s = k / 64;
  if (s < 1) s = 1;
  return (int)s;
}
static inline int splitk_small(long long k, int m, int n, int batch) {  // ops.HipOps.gemm's latency rule
  if (batch == 1 && k >= 128 && k <= 1024 && cdiv(m, 64) * cdiv(n, 64) <= 32) {
    int s = (int)(k / 48);
    return s > 4 ? 4 : (s < 1 ? 1 : s);
  }
  return 1;
}

// the same rule for the handful of priors' products of the KL backward (0.5 K^-1 S K^-1: two dependent M x M x M
// products, batch = the number of priors): 48 workgroups with a 13-step K loop each were 21.5 us apiece at M = 200
static inline int splitk_few(long long k, int m, int n, int batch) {
  if (batch <= 4 && k >= 128 && k <= 1024 && cdiv(m, 64) * cdiv(n, 64) * batch <= 64) {
    int s = (int)(k / 48);
    return s > 4 ? 4 : (s < 1 ? 1 : s);
  }
  return splitk_small(k, m, n, batch);
}

struct Ctx {
  Plan& P;
  const gpsa_step_params& prm;
  const gpsa_step_io& io;
  char* saved;
  Arena& sc;
  hipStream_t st;
  bool dry;
  bool apk_d = false;  // the data GP's packed inverse has been written in this call
  bool quiet = false;  // a materialising re-run of a pass: not one of the step's timed launches
  void* stv() const { return (void*)st; }
  template <typename T> T* sv(long long off) const { return reinterpret_cast<T*>(saved + off); }
  double* mats(const Group& G, int pos) const { return sv<double>(G.o_mats) + (long long)pos * G.M * G.M; }
  double* inv(const Group& G, int pos) const { return sv<double>(G.o_inv) + (long long)pos * G.M * G.M; }
};

// fp64 product through gemm_launch<double> with workspace from the scratch arena
static int gemm64(Ctx& c, int ta, int tb, int m, int n, long long k, double alpha, const double* A, long long lda,
                  long long sA, const double* B, long long ldb, long long sB, double beta, double* C,
                  long long ldc, long long sC, int batch, int splitk) {
  const bool dry = c.dry;
  const long long mk = c.sc.mark();
  void* ws = nullptr;
  long long wsb = 0;
  if (splitk > 1) {
    wsb = (long long)batch * splitk * m * n * 8;
    ws = c.sc.get<char>(wsb);
  }
  GPSA_RUN(gemm_launch<double>(ta, tb, m, n, k, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc, sC, batch, splitk,
                               ws, wsb, c.st));
  c.sc.release(mk);
  return 0;
}
static int gemm32(Ctx& c, int ta, int tb, int m, int n, long long k, double alpha, const float* A, long long lda,
                  long long sA, const float* B, long long ldb, long long sB, double beta, float* C,
                  long long ldc, long long sC, int batch, int splitk) {
  const bool dry = c.dry;
  const long long mk = c.sc.mark();
  void* ws = nullptr;
  long long wsb = 0;
  if (splitk > 1) {
    wsb = (long long)batch * splitk * m * n * 4;
    ws = c.sc.get<char>(wsb);
  }
  GPSA_RUN(gemm_launch<float>(ta, tb, m, n, k, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc, sC, batch, splitk,
                              ws, wsb, c.st));
  c.sc.release(mk);
  return 0;
}
// out[M,C] += A[M,L] B[L,C]: the one-pass kernel where it takes the shape, the tiled product otherwise
static int thin_update(Ctx& c, const float* A, int M, int L, const float* B, long long C, float* out) {
  if (!c.dry) {
    if (c.sc.overflow) return GPSA_EWORKSPACE;
    const int rc = gpsa_thin_update_f32(A, M, L, B, C, out, c.stv());
    if (rc != GPSA_EUNSUPPORTED) return rc;
  }
  return gemm32(c, 0, 0, M, (int)C, L, 1.0, A, L, 0, B, C, 0, 1.0, out, C, 0, 1, 1);
}
template <typename TIA, typename TIB, typename TO>
static int gemmx(Ctx& c, int ta, int tb, int m, int n, long long k, double alpha, const TIA* A, long long lda,
                 long long sA, const TIB* B, long long ldb, long long sB, double beta, TO* C, long long ldc,
                 long long sC, int batch, int splitk) {
  const bool dry = c.dry;
  const long long mk = c.sc.mark();
  void* ws = nullptr;
  long long wsb = 0;
  if (splitk > 1) {
    wsb = (long long)batch * splitk * m * n * 8;
    ws = c.sc.get<char>(wsb);
  }
  GPSA_RUN((gemm64_launch<TIA, TIB, TO>(ta, tb, m, n, k, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc, sC, batch,
                                        splitk, ws, wsb, c.st)));
  c.sc.release(mk);
  return 0;
}

// long-K fp64 products through gpsa_longk_f64 (csrc/longk64.hip); rc == GPSA_EUNSUPPORTED: the shape is not covered and
// the caller keeps its generic path.  The dry run reserves the workspace either way.
static int longk(Ctx& c, int nprob, const double* const* G, const double* const* Bm, const void* const* d, int d_dtype,
                 int M, long long K, long long ld, int sym, const double* alpha, const double* beta, double* const* out) {
  const long long wsb = gpsa_longk_f64_workspace(M, K, nprob);
  if (wsb == 0 || (ld & 1)) return GPSA_EUNSUPPORTED;
  const long long mk = c.sc.mark();
  void* ws = c.sc.get<char>(wsb);
  int rc = 0;
  if (!c.dry) rc = gpsa_longk_f64(nprob, G, Bm, d, d_dtype, M, K, ld, sym, alpha, beta, out, ws, wsb, c.stv());
  c.sc.release(mk);
  return rc;
}

// ---- M x M stage: every prior covariance and variational covariance of the step, factorised together ------
static int mm_stage_fwd(Ctx& c) {
  Plan& P = c.P;
  const bool dry = c.dry;
  const int V = P.V, D = P.D, Mx = P.Mx, Mg = P.Mg;
  Group& GW = P.gw();
  Group& GD = P.gd();
  const bool kl = P.d.want_kl != 0;
  // the KL forward deals a term's rows to several workgroups: their partial sums and arrival counters (zeroed by the
  // launch below) live in the scratch arena for the length of this call
  double* klpart[2] = {nullptr, nullptr};
  int* klcnt[2] = {nullptr, nullptr};
  if (kl && !c.io.reuse_mm)
    for (int g = 0; g < P.ng; ++g)
      if (P.grp[g].n_omega > 0) {
        klpart[g] = c.sc.get<double>((long long)P.grp[g].n_omega * mvn_kl_grouped_fwd_slices(P.grp[g].M));
        klcnt[g] = c.sc.get<int>(P.grp[g].n_omega);
      }
  // mean function at the inducing points, residuals, the KL terms' mean differences
  {
    PrepArgs a;
    memset(&a, 0, sizeof(a));
    a.Xtilde = c.prm.Xtilde; a.delta_G = c.prm.delta_G; a.slopes = c.prm.slopes; a.intercepts = c.prm.intercepts;
    for (int m = 0; m < P.nm; ++m) { a.delta_F[m] = c.prm.delta_F[m]; a.L[m] = P.d.n_latent[m]; a.Loff[m] = P.Loff[m]; }
    a.V = V; a.D = D; a.Mx = Mx; a.Mg = Mg; a.nm = P.nm;
    a.bidx = P.tab.bidx;
    a.mu_z = c.io.mu_z;
    a.resid = c.sv<double>(P.o_resid);
    a.Dw = kl ? c.sv<double>(GW.o_D) : nullptr;
    a.Dd = kl ? c.sv<double>(GD.o_D) + (P.merged ? (long long)V * D * Mx : 0) : nullptr;
    for (int g = 0; g < P.ng; ++g)
      if (kl && !P.grp[g].own_all() && !c.io.reuse_mm) {
        a.zinfo[g] = c.sv<int>(P.grp[g].o_info);
        a.nzinfo[g] = P.grp[g].nb();
      }
    for (int g = 0; g < P.ng; ++g)
      if (klcnt[g] != nullptr) {
        a.zinfo[2 + g] = klcnt[g];
        a.nzinfo[2 + g] = P.grp[g].n_omega;
      }
    const long long nd = kl ? cdiv((long long)P.Ltot * Mg, 256) : 0;
    if (!dry) {
      step_prep_kernel<<<(unsigned)(V + nd), 256, 0, c.st>>>(a);
      GPSA_LAUNCH_CHECK();
    }
  }
  if (c.io.reuse_mm) {  // same parameters, same arena: everything below is still there
    if (kl && !dry)
      GPSA_CK(copy_async(c.io.kl, c.sv<double>(P.o_klcache), (size_t)((long long)V * D + P.Ltot) * 8, c.st));
    return 0;
  }
  // prior covariances K_uu + 1e-5 I of the free views (batched over runs) and of the data GP
  for (const Run& r : P.runs)
    GPSA_RUN(gpsa_kmat_batched(P.d.kind_warp, c.prm.Xtilde + (long long)r.v0 * Mx * D, (long long)Mx * D, Mx,
                               c.prm.Xtilde + (long long)r.v0 * Mx * D, (long long)Mx * D, Mx, D,
                               c.prm.warp_ls + r.v0, c.prm.warp_var + r.v0, 1, nullptr, r.cnt, 1e-5,
                               c.mats(GW, P.pos_Kw(r.b0)), (long long)Mx * Mx, c.stv()));
  GPSA_RUN(gpsa_kmat_batched(P.d.kind_data, c.prm.Gtilde, 0, Mg, c.prm.Gtilde, 0, Mg, D, c.prm.data_ls,
                             c.prm.data_var, 0, nullptr, 1, 1e-5, c.mats(GD, P.pos_KF()), 0, c.stv()));
  // variational covariances Omega = A A^T + 1e-5 I straight from the fp32 parameters
  // (the warp GPs' factors and the first modality's in one launch when the sizes agree)
  const int m_first = (Mx == Mg && P.nm > 0) ? 1 : 0;
  if (m_first)
    GPSA_RUN(gpsa_omega_fwd2(c.prm.Omega_sqt_G, V * D, c.mats(GW, P.pos_OmG(0)), c.prm.Omega_sqt_F[0], P.d.n_latent[0],
                             c.mats(GD, P.pos_OmF(0, 0)), Mx, 1e-5, c.stv()));
  else
    GPSA_RUN(gpsa_omega_fwd(c.prm.Omega_sqt_G, Mx, V * D, 1e-5, c.mats(GW, P.pos_OmG(0)), c.stv()));
  for (int m = m_first; m < P.nm; ++m)
    GPSA_RUN(gpsa_omega_fwd(c.prm.Omega_sqt_F[m], Mg, P.d.n_latent[m], 1e-5, c.mats(GD, P.pos_OmF(m, 0)), c.stv()));
  // factorise: the priors always; the variational covariances only when the KL terms are wanted (the
  // layers use Omega itself, never its factor)
  for (int g = 0; g < P.ng; ++g) {
    Group& G = P.grp[g];
    const long long mm = (long long)G.M * G.M;
    double* logdet = c.sv<double>(G.o_logdet);
    int* info = c.sv<int>(G.o_info);
    const int np = G.n_prior, n_own = G.own_hi - G.own_lo;
    // owner computes: only the priors and this plan's own variational covariances (batch positions np + own_lo ..
    // np + own_hi) are factorised and inverted - in ONE launch all the same (a second one would cost a second matrix's
    // latency); the entries of the others in Linv / inv / logdet stay unwritten and nobody reads them (their terms are
    // listed as absent), their infos were zeroed by step_prep_kernel
    const bool sel = kl && !G.own_all();
    const int nb_main = kl ? G.nb() : np;
    // K^-1 = L^-T L^-1 for ``cnt`` matrices in one product
    // (the triangle mode contracts k >= max(i, j) only and mirrors; it needs split-K 1: a large batch)
    auto inverse_product = [&](const double* Lin, double* out, int cnt) -> int {
      if (cnt <= 0) return 0;
      if (splitk_small(G.M, G.M, G.M, cnt) == 1)
        GPSA_RUN(gemm_launch_tri<double>(1, 0, G.M, G.M, G.M, 1.0, Lin, G.M, mm, Lin, G.M, mm, 0.0, out, G.M, mm, cnt, 1,
                                         nullptr, 0, c.st, GEMM_TRI_LTL));
      else
        GPSA_CK(gemm64(c, 1, 0, G.M, G.M, G.M, 1.0, Lin, G.M, mm, Lin, G.M, mm, 0.0, out, G.M, mm, cnt,
                       splitk_small(G.M, G.M, G.M, cnt)));
      return 0;
    };
    if (nb_main > 0) {
      const long long mk = c.sc.mark();
      double* Linv = c.sc.get<double>(nb_main * mm);
      if (G.M > 256) {
        const long long wsb = gpsa_chol_inv_blocked_workspace(G.M, nb_main);
        void* ws = c.sc.get<char>(wsb);
        if (!sel) {
          GPSA_RUN(gpsa_chol_inv_blocked_f64(c.mats(G, 0), Linv, G.M, nb_main, logdet, info, ws, wsb, c.stv()));
        } else {  // (beyond the single-launch kernels the factorisation is a launch sequence anyway: two of them)
          if (np > 0)
            GPSA_RUN(gpsa_chol_inv_blocked_f64(c.mats(G, 0), Linv, G.M, np, logdet, info, ws, wsb, c.stv()));
          if (n_own > 0)
            GPSA_RUN(gpsa_chol_inv_blocked_f64(c.mats(G, np + G.own_lo), Linv + (long long)(np + G.own_lo) * mm, G.M,
                                               n_own, logdet + np + G.own_lo, info + np + G.own_lo, ws, wsb, c.stv()));
        }
      } else if (!sel) {
        GPSA_RUN(gpsa_chol_inv_f64(c.mats(G, 0), Linv, G.M, nb_main, logdet, info, c.stv()));
      } else {
        GPSA_RUN(gpsa_chol_inv_sel_f64(c.mats(G, 0), Linv, G.M, nb_main, np, np + G.own_lo, np + G.own_hi, logdet, info,
                                       c.stv()));
      }
      if (!sel) {
        GPSA_CK(inverse_product(Linv, c.inv(G, 0), nb_main));
      } else if (G.own_lo == 0) {  // the priors and the owned covariances are neighbours in the batch
        GPSA_CK(inverse_product(Linv, c.inv(G, 0), np + n_own));
      } else {
        GPSA_CK(inverse_product(Linv, c.inv(G, 0), np));
        GPSA_CK(inverse_product(Linv + (long long)(np + G.own_lo) * mm, c.inv(G, np + G.own_lo), n_own));
      }
      c.sc.release(mk);
    }
  }
  if (kl)
    for (int g = 0; g < P.ng; ++g) {
      Group& G = P.grp[g];
      // (the terms also go to the arena's cache, for passes that reuse this stage: same launch, no copy)
      if (G.n_omega > 0)
        GPSA_RUN(mvn_kl_grouped_fwd_copy(c.mats(G, 0), c.inv(G, 0), c.sv<double>(G.o_logdet), G.om_idx, G.pr_idx,
                                         c.sv<double>(G.o_D), G.M, G.n_omega, c.io.kl + G.kl_off,
                                         c.sv<double>(G.o_KD), c.sv<double>(P.o_klcache) + G.kl_off, klpart[g], klcnt[g],
                                         c.st));
    }
  return 0;
}

// ---- warp GPs of all free views ---------------------------------------------------------------------------
static ModPtrs mod_ptrs(Ctx& c, const gpsa_step_out_grads* og, const double* const* dG64) {
  ModPtrs p;
  memset(&p, 0, sizeof(p));
  for (int m = 0; m < c.P.nm; ++m) {
    p.X[m] = c.io.X[m];
    p.Gm[m] = c.io.G_means[m];
    p.Gs[m] = c.io.G_samples[m];
    p.G64[m] = c.sv<double>(c.P.o_G64[m]);
    p.N[m] = c.P.d.n_rows[m];
    if (og != nullptr) {
      p.dGm[m] = og->dG_means[m];
      p.dGs[m] = og->dG_samples[m];
    }
    if (dG64 != nullptr) p.dG64[m] = dG64[m];
  }
  return p;
}

// alpha = K^-1 K_uf and q = k^T alpha for ``cnt`` fp64 panels (projection kernel, or plain products beyond
// its size)
static int project_views(Ctx& c, const double* Kinv, const double* Kuf, int M, long long Cs, double* alpha,
                         double* q, int cnt, int b0, bool packed) {
  // packed: the saved arena already holds these views' packed inverses (the forward's call): no second packing
  const bool dry = c.dry;
  const long long wsb1 = gpsa_whiten_workspace(M);
  if (wsb1 > 0) {
    void* ws = c.sv<char>(c.P.o_apk_w) + wsb1 * b0;
    GPSA_RUN(gpsa_whiten_batched_f64(packed ? nullptr : Kinv, (long long)M * M, Kuf, M, Cs, (long long)M * Cs, alpha, q,
                                     cnt, ws, wsb1 * cnt, c.stv()));
    return 0;
  }
  GPSA_CK(gemm64(c, 0, 0, M, (int)Cs, M, 1.0, Kinv, M, (long long)M * M, Kuf, Cs, (long long)M * Cs, 0.0, alpha,
                 Cs, (long long)M * Cs, cnt, 1));
  if (q != nullptr && !dry) {
    dim3 grid((unsigned)cdiv(Cs, 256), (unsigned)cnt);
    coldot2_kernel<<<grid, 256, 0, c.st>>>(Kuf, alpha, M, Cs, q);
    GPSA_LAUNCH_CHECK();
  }
  return 0;
}

static int warp_stage_fwd(Ctx& c) {
  Plan& P = c.P;
  const bool dry = c.dry;
  const int V = P.V, D = P.D, Mx = P.Mx, nf = P.nf;
  const long long Cs = P.Cs;
  Group& GW = P.gw();
  (void)V;
  const long long mk = c.sc.mark();
  double* meanT = nullptr;
  double* vq = nullptr;
  double* q = nullptr;
  if (nf > 0 && Cs > 0) {
    float* Xv = c.sv<float>(P.o_Xv);
    double* alpha = c.sv<double>(P.o_alpha_w);
    double* Wk = c.sv<double>(P.o_Wk);
    meanT = c.sc.get<double>((long long)nf * D * Cs);
    vq = c.sc.get<double>((long long)nf * D * Cs);
    q = c.sc.get<double>((long long)nf * Cs);
    double* Kuf = c.sc.get<double>((long long)nf * Mx * Cs);
    if (!dry) {
      dim3 grid((unsigned)cdiv(Cs, 256), (unsigned)nf);
      warp_gather_kernel<<<grid, 256, 0, c.st>>>(P.tab, P.d_free, mod_ptrs(c, nullptr, nullptr), Xv);
      GPSA_LAUNCH_CHECK();
    }
    for (const Run& r : P.runs) {
      long long nlive[KM_MAXB_STEP];
      for (int i = 0; i < r.cnt; ++i) nlive[i] = P.nview[r.v0 + i];
      GPSA_RUN(gpsa_kmat_batched(P.d.kind_warp, c.prm.Xtilde + (long long)r.v0 * Mx * D, (long long)Mx * D, Mx,
                                 Xv + (long long)r.b0 * Cs * D, Cs * D, Cs, D, c.prm.warp_ls + r.v0,
                                 c.prm.warp_var + r.v0, 1, nlive, r.cnt, 0.0, Kuf + (long long)r.b0 * Mx * Cs,
                                 (long long)Mx * Cs, c.stv()));
      GPSA_CK(project_views(c, c.inv(GW, P.pos_Kw(r.b0)), Kuf + (long long)r.b0 * Mx * Cs, Mx, Cs,
                            alpha + (long long)r.b0 * Mx * Cs, q + (long long)r.b0 * Cs, r.cnt, r.b0, false));
      // quirk 2: the forward of view v reads the Omega rows v*D + j
      GPSA_RUN(gpsa_quadform_fwd_keep_batched_f64(
          alpha + (long long)r.b0 * Mx * Cs, c.mats(GW, P.pos_OmG(r.v0 * D)), Mx, Cs, D,
          vq + (long long)r.b0 * D * Cs, Wk + (long long)r.b0 * D * Mx * Cs,
          c.sv<double>(P.o_resid) + (long long)r.v0 * Mx * D, meanT + (long long)r.b0 * D * Cs, r.cnt, c.stv()));
    }
  }
  // draws of every modality's rows (fixed views pass their coordinates through)
  int* bad = c.sv<int>(P.o_bad);
  long long boff = 0;
  for (int m = 0; m < P.nm; ++m) {
    const long long N = P.d.n_rows[m];
    if (N == 0) continue;
    const long long nb = cdiv(N, 256);
    if (!dry) {
      warp_sample_views_fwd_kernel<<<(unsigned)nb, 256, 0, c.st>>>(
          P.tab, m, c.io.X[m], meanT, vq, q, c.prm.warp_var, c.prm.slopes, c.prm.intercepts, c.io.eps_G, N,
          c.io.G_means[m], c.io.G_samples[m], c.sv<double>(P.o_G64[m]), bad + boff);
      GPSA_LAUNCH_CHECK();
    }
    boff += nb;
  }
  c.sc.release(mk);
  // one word for the host: Cholesky infos and variance flags
  if (c.io.flag != nullptr && !dry) {
    Group& G0 = P.grp[0];
    // infos of the two groups are not contiguous: reduce group 0 + flags, then fold group 1 in
    const int n0 = P.d.want_kl ? G0.nb() : G0.n_prior;
    flag_reduce_kernel<<<1, 256, 0, c.st>>>(c.sv<int>(G0.o_info), n0, bad, P.nbad, c.io.flag);
    GPSA_LAUNCH_CHECK();
    if (P.ng == 2) {
      Group& G1 = P.grp[1];
      const int n1 = P.d.want_kl ? G1.nb() : G1.n_prior;
      flag_reduce_kernel<<<1, 256, 0, c.st>>>(c.sv<int>(G1.o_info), n1, c.io.flag, 1, c.io.flag);
      GPSA_LAUNCH_CHECK();
    }
  }
  return 0;
}

// ---- data GP ----------------------------------------------------------------------------------------------
static int data_pass_fwd(Ctx& c, const Pass& ps) {
  Plan& P = c.P;
  const bool dry = c.dry;
  const int m = ps.m, Mg = P.Mg, D = P.D, L = P.d.n_latent[m], Pm = P.d.n_out[m];
  const long long C = ps.C;
  Group& GD = P.gd();
  const double* Kinv = c.inv(GD, P.pos_KF());
  const double* Om = c.mats(GD, P.pos_OmF(m, 0));
  float* alpha = c.sv<float>(ps.o_alpha);
  float* Sigma = c.sv<float>(ps.o_sigma);
  const float* eps = ps.test ? c.io.eps_F_test[m] : c.io.eps_F[m];
  float* F = ps.test ? c.io.F_latent_test[m] : c.io.F_latent[m];
  float* Fo = ps.test ? c.io.F_obs_test[m] : c.io.F_obs[m];
  const long long mk = c.sc.mark();
  double* q = c.sc.get<double>(C);
  {
    const long long mk2 = c.sc.mark();
    double* Kuf = c.sc.get<double>((long long)Mg * C);
    const long long wsb = gpsa_whiten_workspace(Mg);
    const bool exact = ps.o_alpha64 >= 0;  // the unrounded projection stays for the backward
    // long panels of the training pass: K_uf formed inside the projection kernel, never in memory (the scratch above
    // stays reserved: the plan's dry run cannot know whether the shape is taken)
    bool fused = false;
    if (!ps.test && exact && wsb > 0 && !dry) {
      if (c.sc.overflow) return GPSA_EWORKSPACE;
      const int rc = gpsa_whiten_gen_f64_dual(c.apk_d ? nullptr : Kinv, P.d.kind_data, c.prm.Gtilde,
                                              c.sv<double>(P.o_G64[m]), D, c.prm.data_ls, c.prm.data_var, Mg, C,
                                              c.sv<double>(ps.o_alpha64), alpha, q, c.sv<char>(P.o_apk_d), wsb, c.stv());
      if (rc == 0) fused = true, c.apk_d = true;
      else if (rc != GPSA_EUNSUPPORTED) return rc;
    }
    if (!fused) {
      // covariance on the warp GP's UNROUNDED draws (fp64), fp32 parameters as stored; G_test is the caller's fp32
      if (ps.test)
        GPSA_RUN(gpsa_kmat(GPSA_F64, GPSA_F32, P.d.kind_data, c.prm.Gtilde, Mg, c.io.G_test[m], C, D, c.prm.data_ls,
                           c.prm.data_var, 0.0, Kuf, c.stv()));
      else
        GPSA_RUN(gpsa_kmat(GPSA_F64, GPSA_F32_X64, P.d.kind_data, c.prm.Gtilde, Mg, c.sv<double>(P.o_G64[m]), C, D,
                           c.prm.data_ls, c.prm.data_var, 0.0, Kuf, c.stv()));
      if (wsb > 0 && !exact) {  // the packed inverse stays in the saved arena: later passes and the backward reuse it
        void* ws = c.sv<char>(P.o_apk_d);
        GPSA_RUN(gpsa_whiten_f64(c.apk_d ? nullptr : Kinv, GPSA_F64, Kuf, Mg, C, GPSA_F32, alpha, q, ws, wsb,
                                 c.stv()));
        c.apk_d = true;
      } else if (wsb > 0) {
        void* ws = c.sv<char>(P.o_apk_d);
        double* a64 = c.sv<double>(ps.o_alpha64);
        GPSA_RUN(gpsa_whiten_f64_dual(c.apk_d ? nullptr : Kinv, Kuf, Mg, C, a64, alpha, q, ws, wsb, c.stv()));
        c.apk_d = true;
      } else {  // beyond the projection kernel: alpha (fp64) = K^-1 K_uf, q from it, then rounded
        double* a64 = exact ? c.sv<double>(ps.o_alpha64) : c.sc.get<double>((long long)Mg * C);
        GPSA_CK(gemm64(c, 0, 0, Mg, (int)C, Mg, 1.0, Kinv, Mg, 0, Kuf, C, 0, 0.0, a64, C, 0, 1, 1));
        if (!dry) {
          coldot2_kernel<<<dim3((unsigned)cdiv(C, 256), 1), 256, 0, c.st>>>(Kuf, a64, Mg, C, q);
          GPSA_LAUNCH_CHECK();
          convert_kernel_step<double, float><<<(unsigned)cdiv((long long)Mg * C, 256), 256, 0, c.st>>>(
              a64, (long long)Mg * C, alpha);
          GPSA_LAUNCH_CHECK();
        }
      }
    }
    c.sc.release(mk2);
  }
  float* meanT = c.sc.get<float>((long long)L * C);
  float* v = c.sc.get<float>((long long)L * C);
  // mean[l,c] = sum_m delta_F[m,l] alpha[m,c]   (mu_z = 0 for the data GP) - unless the fused kernel forms it itself: with
  // delta_l^T packed into the first padding row of Omega_l, the product's row M IS the mean (MFMAs the padding runs anyway)
  const bool mean_in_product = ps.fused(c.io) && gpsa_quadform_elbo_takes_delta(Mg) != 0;
  if (!mean_in_product)
    GPSA_CK(gemm32(c, 1, 0, L, (int)C, Mg, 1.0, c.prm.delta_F[m], L, 0, alpha, C, 0, 0.0, meanT, C, 0, 1, 1));
  if (ps.fused(c.io)) {
    // variance, draw, likelihood and the backward's abar in one pass over the products: F and Sigma are never written
    if (c.io.noise_u[m] == nullptr || c.io.ll_part[m] == nullptr) return GPSA_EINVAL;
    float* g_ext = c.sv<float>(ps.o_fuse);
    float* dmeanT = g_ext + (long long)(L + 1) * C;
    float* abar = dmeanT + (long long)L * C;
    // io.skip_missing: the fp32 skip kernels (panel_elbo_skip_kernel), also in a bf16x3 plan - there is no x3 skip closing
    // (gpsa_step_contraction then reports the pass as fp32); such a plan's scratch holds the larger of the two workspaces
    // P.lik[m] == GPSA_LIK_POISSON (gpsa_step_likelihood): the fp32 Poisson kernels (panel_elbo_pois_kernel), with the same
    // rule for a bf16x3 plan
    // P.lik[m] == GPSA_LIK_NEGBIN (gpsa_step_dispersion): the fp32 NB kernels (panel_elbo_nb_kernel), the same rule again;
    // the kind without its tensors is refused here, before any launch of the pass
    const bool pois = P.lik[m] == GPSA_LIK_POISSON, nb = P.lik[m] == GPSA_LIK_NEGBIN;
    if (nb && (P.log_disp[m] == nullptr || P.u_elems[m] == nullptr || P.usum[m] == nullptr)) return GPSA_EINVAL;
    const bool skip = c.io.skip_missing != 0, x3 = ps.x3 && !skip && !pois && !nb;
    const long long ws32 = gpsa_quadform_elbo_f32_workspace(Mg, C, L);
    const long long wsx3 = ps.x3 ? gpsa_quadform_elbo_x3_f32_workspace(Mg, C, L) : 0;
    const long long wsb = x3 ? wsx3 : ws32;
    void* ws = c.sc.get<char>(ps.x3 && ws32 > wsx3 ? ws32 : (ps.x3 ? wsx3 : ws32));
    const bool timed = !dry && !c.quiet && &ps == &P.passes[0];
    if (timed) P.tick(0, 0, true, c.st);
    if (!dry) P.skip_seen = skip;
    if (nb && mean_in_product)
      GPSA_RUN(gpsa_quadform_elbo_delta_nb_f32(GPSA_F64, alpha, Om, Mg, C, L, c.prm.delta_F[m], q, c.prm.data_var, eps,
                                               c.io.Y[m], (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar,
                                               c.io.ll_part[m], c.io.F_fused_T[m], P.log_offset[m], P.log_disp[m],
                                               P.u_elems[m], P.usum[m], skip ? 1 : 0, ws, wsb, c.stv()));
    else if (nb)
      GPSA_RUN(gpsa_quadform_elbo_nb_f32(GPSA_F64, alpha, Om, Mg, C, L, meanT, q, c.prm.data_var, eps, c.io.Y[m],
                                         (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar, c.io.ll_part[m],
                                         c.io.F_fused_T[m], P.log_offset[m], P.log_disp[m], P.u_elems[m], P.usum[m],
                                         skip ? 1 : 0, ws, wsb, c.stv()));
    else if (pois && mean_in_product)
      GPSA_RUN(gpsa_quadform_elbo_delta_pois_f32(GPSA_F64, alpha, Om, Mg, C, L, c.prm.delta_F[m], q, c.prm.data_var, eps,
                                                 c.io.Y[m], (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar,
                                                 c.io.ll_part[m], c.io.F_fused_T[m], P.log_offset[m], skip ? 1 : 0, ws,
                                                 wsb, c.stv()));
    else if (pois)
      GPSA_RUN(gpsa_quadform_elbo_pois_f32(GPSA_F64, alpha, Om, Mg, C, L, meanT, q, c.prm.data_var, eps, c.io.Y[m],
                                           (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar,
                                           c.io.ll_part[m], c.io.F_fused_T[m], P.log_offset[m], skip ? 1 : 0, ws, wsb,
                                           c.stv()));
    else if (skip && mean_in_product)
      GPSA_RUN(gpsa_quadform_elbo_delta_skip_f32(GPSA_F64, alpha, Om, Mg, C, L, c.prm.delta_F[m], q, c.prm.data_var, eps,
                                                 c.io.Y[m], (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar,
                                                 c.io.ll_part[m], c.io.F_fused_T[m], ws, wsb, c.stv()));
    else if (skip)
      GPSA_RUN(gpsa_quadform_elbo_skip_f32(GPSA_F64, alpha, Om, Mg, C, L, meanT, q, c.prm.data_var, eps, c.io.Y[m],
                                           (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar,
                                           c.io.ll_part[m], c.io.F_fused_T[m], ws, wsb, c.stv()));
    else if (x3 && mean_in_product)
      GPSA_RUN(gpsa_quadform_elbo_delta_x3_f32(GPSA_F64, alpha, Om, Mg, C, L, c.prm.delta_F[m], q, c.prm.data_var, eps,
                                               c.io.Y[m], (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar,
                                               c.io.ll_part[m], c.io.F_fused_T[m], ws, wsb, c.stv()));
    else if (x3)
      GPSA_RUN(gpsa_quadform_elbo_x3_f32(GPSA_F64, alpha, Om, Mg, C, L, meanT, q, c.prm.data_var, eps, c.io.Y[m],
                                         (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar, c.io.ll_part[m],
                                         c.io.F_fused_T[m], ws, wsb, c.stv()));
    else if (mean_in_product)
      GPSA_RUN(gpsa_quadform_elbo_delta_f32(GPSA_F64, alpha, Om, Mg, C, L, c.prm.delta_F[m], q, c.prm.data_var, eps,
                                            c.io.Y[m], (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar,
                                            c.io.ll_part[m], c.io.F_fused_T[m], ws, wsb, c.stv()));
    else
      GPSA_RUN(gpsa_quadform_elbo_f32(GPSA_F64, alpha, Om, Mg, C, L, meanT, q, c.prm.data_var, eps, c.io.Y[m],
                                      (long long)(C / P.S), P.S, c.io.noise_u[m], g_ext, dmeanT, abar, c.io.ll_part[m],
                                      c.io.F_fused_T[m], ws, wsb, c.stv()));
    if (timed) { P.tick(0, 1, true, c.st); ++P.tfwd; }
    c.sc.release(mk);
    return 0;
  }
  {
    const long long wsb = gpsa_quadform_workspace(GPSA_F32, Mg, C, L);
    void* ws = c.sc.get<char>(wsb);
    const bool timed = !dry && !c.quiet && &ps == &P.passes[0];
    if (timed) P.tick(0, 0, true, c.st);
    if (c.io.keep_products && ps.o_keep >= 0)  // training: the full product, kept for the backward
      GPSA_RUN(gpsa_quadform_fwd_keep_f32(GPSA_F64, alpha, Om, Mg, C, L, v, c.sv<float>(ps.o_keep), ws, wsb, c.stv()));
    else
      GPSA_RUN(gpsa_quadform_fwd(GPSA_F32, GPSA_F64, alpha, Om, Mg, C, L, v, ws, wsb, c.stv()));
    if (timed) { P.tick(0, 1, true, c.st); ++P.tfwd; }
  }
  GPSA_RUN(gpsa_data_sample_fwd(meanT, v, q, c.prm.data_var, eps, C, L, F, Sigma, c.stv()));
  if (P.d.has_lmc[m] && Fo != nullptr)
    GPSA_CK(gemm32(c, 0, 0, (int)C, Pm, L, 1.0, F, L, 0, c.prm.W[m], Pm, 0, 0.0, Fo, Pm, 0, 1, 1));
  c.sc.release(mk);
  return 0;
}

static int step_forward(Plan& P, const gpsa_step_params& prm, const gpsa_step_io& io, char* saved, Arena& sc,
                        hipStream_t st, int stages) {
  Ctx c{P, prm, io, saved, sc, st, sc.dry};
  if (stages & 1) {
    GPSA_CK(mm_stage_fwd(c));
    GPSA_CK(warp_stage_fwd(c));
  }
  if (stages & 2) {
    // bits 8..: only the training passes of these modalities (0: every pass): a training forward leaves the
    // modalities whose likelihood can ride in the data GP's pass for loss_fn, which knows the observations; bit 2:
    // a re-run that materialises such a modality's draws after the fact (not one of the step's timed launches)
    const int mask = (stages >> 8) & ((1 << MAXMODS) - 1);
    c.quiet = (stages & 4) != 0;
    for (const Pass& ps : P.passes) {
      if (mask != 0 && (ps.test || ((mask >> ps.m) & 1) == 0)) continue;
      GPSA_CK(data_pass_fwd(c, ps));
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------
struct BwdBufs {          // fp64 pieces of the parameter gradients (scratch, alive for the whole backward)
  double* dstack[2];      // gradient wrt every matrix of the groups' batches
  double *dZ_wf, *dZ_wu, *dpar_wf, *dpar_wu, *dvar_ws, *dresid;
  double *dZ_df, *dpar_df, *dZ_du, *dpar_du;
  double* dvar_ds;
  float* ddc_F[MAXMODS];
  double* dG64[MAXMODS];
  double* dD[2];
  bool have_dG[MAXMODS];
  bool have_ddc[MAXMODS];
  int* tick;              // [BWD_TICKS] arrival counters of the kernels that close their own block partials (zero at entry)
};
constexpr int BWD_TICKS = 64;  // [0 .. 31] the sampler backward's free views; [32 ..] the data GP passes' fused post

static int data_pass_bwd(Ctx& c, const Pass& ps, int pass_idx, const float* dFl_in, const float* dFo_in,
                         BwdBufs& B, const gpsa_step_param_grads& out, bool first_for_mod, const float* gloss) {
  Plan& P = c.P;
  const bool dry = c.dry;
  const int m = ps.m, Mg = P.Mg, D = P.D, L = P.d.n_latent[m], Pm = P.d.n_out[m];
  const long long C = ps.C, mm = (long long)Mg * Mg;
  Group& GD = P.gd();
  const double* Kinv = c.inv(GD, P.pos_KF());
  const double* Om = c.mats(GD, P.pos_OmF(m, 0));
  double* dOm = B.dstack[P.merged ? 0 : 1] + (long long)P.pos_OmF(m, 0) * mm;
  double* dKuu = B.dstack[P.merged ? 0 : 1] + (long long)P.pos_KF() * mm;
  const float* alpha = c.sv<float>(ps.o_alpha);
  const float* Sigma = c.sv<float>(ps.o_sigma);
  const float* eps = ps.test ? c.io.eps_F_test[m] : c.io.eps_F[m];
  const float* F = ps.test ? c.io.F_latent_test[m] : c.io.F_latent[m];
  const long long mk = c.sc.mark();
  // gradient wrt the latent draws: the caller's own plus the LMC's F_obs = F W (vgpsa.py:428-432)
  const float* dFl = dFl_in;
  if (P.d.has_lmc[m] && dFo_in != nullptr) {
    float* buf = c.sc.get<float>(C * L);
    if (dFl_in != nullptr) GPSA_RUN(copy_async(buf, dFl_in, (size_t)(C * L * 4), c.st));
    GPSA_CK(gemm32(c, 0, 1, (int)C, L, Pm, 1.0, dFo_in, Pm, 0, c.prm.W[m], Pm, 0, dFl_in != nullptr ? 1.0 : 0.0, buf, L,
                   0, 1, 1));
    if (out.W[m] != nullptr)  // dW = F^T dF_obs
      GPSA_CK(gemm32(c, 1, 0, L, Pm, C, 1.0, F, L, 0, dFo_in, Pm, 0, first_for_mod ? 0.0 : 1.0, out.W[m], Pm, 0, 1,
                     splitk_for(C, L, Pm)));
    dFl = buf;
  } else if (!P.d.has_lmc[m] && dFo_in != nullptr && dFl_in != nullptr && dFo_in != dFl_in) {
    return GPSA_EINVAL;  // without LMC F_obs IS F_latent: one gradient
  } else if (dFl == nullptr) {
    dFl = dFo_in;
  }
  const bool fusedp = ps.fused(c.io);
  float* g_ext = fusedp ? c.sv<float>(ps.o_fuse) : c.sc.get<float>((long long)(L + 1) * C);
  float* dmeanT = fusedp ? g_ext + (long long)(L + 1) * C : c.sc.get<float>((long long)L * C);
  float* qbar = g_ext + (long long)L * C;
  if (!fusedp) {
    const long long wsb = 8 * (C / 32 + 2);
    void* ws = c.sc.get<char>(wsb);
    GPSA_RUN(gpsa_data_sample_bwd(dFl, eps, Sigma, c.prm.data_var, C, L, g_ext, dmeanT, qbar, GPSA_F64,
                                  B.dvar_ds + pass_idx, ws, wsb, c.stv()));
  }
  // abar = delta_F dmean + 2 sum_l g_l Omega_l alpha
  float* abar = fusedp ? dmeanT + (long long)L * C : c.sc.get<float>((long long)Mg * C);
  if (fusedp) {
    // the forward left g, dmean and 2 sum_l g_l Omega_l alpha (at upstream gradient 1) in the saved arena
    if (gloss == nullptr) return GPSA_EINVAL;
    const long long wsb = 8 * (C / 256 + 2);
    void* ws = c.sc.get<char>(wsb);
    const bool timed = !dry && !c.quiet && &ps == &P.passes[0];
    if (timed) P.tick(1, 0, false, c.st);  // (slot 1: what is left of the alpha-gradient - the mean term's share)
    if (pass_idx < BWD_TICKS - 32)  // (a ticket per pass: the post kernel's last block closes dvar itself)
      GPSA_RUN(elbo_fused_post_ticket(g_ext, dmeanT, abar, Mg, C, L, gloss, c.prm.data_var, B.dvar_ds + pass_idx,
                                      (double*)ws, B.tick + 32 + pass_idx, c.st));
    else
      GPSA_RUN(gpsa_elbo_fused_post(g_ext, dmeanT, abar, Mg, C, L, gloss, c.prm.data_var, GPSA_F64,
                                    B.dvar_ds + pass_idx, ws, wsb, c.stv()));
    GPSA_CK(thin_update(c, c.prm.delta_F[m], Mg, L, dmeanT, C, abar));
    if (timed) P.tick(1, 1, false, c.st);
  } else {
    const long long wsb = gpsa_quadform_workspace(GPSA_F32, Mg, C, L);
    const long long mk2 = c.sc.mark();
    void* ws = c.sc.get<char>(wsb);
    const bool timed = !dry && !c.quiet && &ps == &P.passes[0];
    if (timed) P.tick(1, 0, false, c.st);
    const bool kept = c.io.keep_products && ps.o_keep >= 0;
    if (kept)  // one streaming pass over the products the forward kept, the mean term's share in the same pass
      GPSA_RUN(gpsa_quadform_bwd_alpha_kept_f32(c.sv<float>(ps.o_keep), g_ext, Mg, C, L, c.prm.delta_F[m], dmeanT, abar,
                                                c.stv()));
    else
      GPSA_RUN(gpsa_quadform_bwd_alpha(GPSA_F32, GPSA_F64, alpha, Om, g_ext, Mg, C, L, abar, ws, wsb, c.stv()));
    if (timed) P.tick(1, 1, false, c.st);
    c.sc.release(mk2);
    if (!kept) GPSA_CK(thin_update(c, c.prm.delta_F[m], Mg, L, dmeanT, C, abar));
  }
  // d delta_F = alpha dmean^T - as a C-long product here, unless the Gram kernel below can carry it in the first padding
  // row of its last tile row (gpsa_quadform_bwd_omega_delta_f32)
  const bool ddelta_in_gram = gpsa_quadform_bwd_omega_takes_delta(Mg, C) != 0;
  if (!ddelta_in_gram)
    GPSA_CK(gemm32(c, 0, 1, Mg, L, C, 1.0, alpha, C, 0, dmeanT, C, 0, first_for_mod ? 0.0 : 1.0, B.ddc_F[m], L, 0, 1,
                   splitk_for(C, Mg, L)));
  B.have_ddc[m] = true;
  // exact_inducing_grad: gamma = K^-1 abar STORED in fp64, W = gamma + qbar alpha64, dK_uu = -W alpha64^T as one
  // C-long fp64 product, dK_uf = W + qbar alpha64 handed to the covariance backward as an fp64 panel
  const bool exact = ps.o_alpha64 >= 0;
  double* gamma64 = nullptr;
  if (exact) {
    const double* a64 = c.sv<double>(ps.o_alpha64);
    gamma64 = c.sc.get<double>((long long)Mg * C);
    const long long wsb = gpsa_whiten_workspace(Mg);
    if (wsb > 0) {
      GPSA_RUN(gpsa_whiten_f64(nullptr, GPSA_F32, abar, Mg, C, GPSA_F64, gamma64, nullptr, c.sv<char>(P.o_apk_d), wsb,
                               c.stv()));
    } else {
      const long long mk2 = c.sc.mark();
      double* abar64 = c.sc.get<double>((long long)Mg * C);
      if (!dry) {
        convert_kernel_step<float, double><<<(unsigned)cdiv((long long)Mg * C, 256), 256, 0, c.st>>>(
            abar, (long long)Mg * C, abar64);
        GPSA_LAUNCH_CHECK();
      }
      GPSA_CK(gemm64(c, 0, 0, Mg, (int)C, Mg, 1.0, Kinv, Mg, 0, abar64, C, 0, 0.0, gamma64, C, 0, 1, 1));
      c.sc.release(mk2);
    }
    // dK_uu = -(gamma + qbar o alpha64) alpha64^T as ONE C-long fp64 product whose left operand is formed while it is
    // staged, and dK_uf = gamma + 2 qbar o alpha64 formed inside the covariance backward as it reads its two panels
    // (round 5: a pass of its own read both panels and wrote W and dK_uf out - 640 MB at the headline size)
    {
      const double* Gs[1] = {gamma64};
      const double* Bs[1] = {a64};
      const void* ds[1] = {qbar};
      const double al[1] = {-1.0}, be[1] = {1.0};
      double* os[1] = {dKuu};
      int rc = longk(c, 1, Gs, Bs, ds, GPSA_F32, Mg, C, C, 0, al, be, os);
      // (the dry run walks the fallback as well: a launch-time refusal - operand alignment - must find its workspace)
      if (rc == GPSA_EUNSUPPORTED || (dry && rc == 0)) {  // (M > 256, an odd or short C, an unaligned panel: the generic product)
        const long long wsb2 = gpsa_exact_dkuu_workspace(Mg, C);
        const long long mk2 = c.sc.mark();
        void* ws2 = c.sc.get<char>(wsb2);
        GPSA_RUN(gpsa_exact_dkuu_f64(gamma64, a64, qbar, Mg, C, dKuu, ws2, wsb2, c.stv()));
        c.sc.release(mk2);
      } else if (rc != 0) {
        return rc;
      }
    }
    if (ps.test) {  // a test pass's covariance backward is the plain entry point: it takes dK_uf written out
      const long long mk2 = c.sc.mark();
      double* qbar64 = c.sc.get<double>(C);
      double* W64 = c.sc.get<double>((long long)Mg * C);
      if (!dry) {
        convert_kernel_step<float, double><<<(unsigned)cdiv(C, 256), 256, 0, c.st>>>(qbar, C, qbar64);
        GPSA_LAUNCH_CHECK();
        dim3 grid((unsigned)cdiv(C, 256), (unsigned)((Mg < 64) ? Mg : 64));
        exact_axpy2_kernel<<<grid, 256, 0, c.st>>>(gamma64, a64, qbar64, Mg, C, W64, gamma64);
        GPSA_LAUNCH_CHECK();
      }
      c.sc.release(mk2);
    }
  }
  // exact training pass: the covariance backward HERE, straight behind the C-long product that has just read the same
  // two fp64 panels (gamma, alpha: 320 MB at the headline size - what of them the memory-side cache still holds is
  // not fetched again; behind the Gram kernel, where it stood until round 6, nothing of them was left).
  const bool cov_early = exact && !ps.test;
  if (cov_early) {
    const long long mk2 = c.sc.mark();
    const long long wsb = gpsa_kmat_bwd_workspace(GPSA_F64, Mg, C, D);
    void* ws = c.sc.get<char>(wsb);
    GPSA_RUN(gpsa_kmat_bwd_x64_f64_axpy(P.d.kind_data, c.prm.Gtilde, Mg, c.sv<double>(P.o_G64[m]), C, D, c.prm.data_ls,
                                        c.prm.data_var, gamma64, c.sv<double>(ps.o_alpha64), qbar, 2.0,
                                        B.dZ_df + (long long)pass_idx * Mg * D, B.dG64[m],
                                        B.dpar_df + (long long)pass_idx * 2, ws, wsb, c.stv()));
    B.have_dG[m] = true;
    c.sc.release(mk2);
  }
  // gamma = K^-1 abar (fp64 product on the fp32 panel).  With many columns dK_uu comes from the identity below
  // and only dK_uf = gamma + 2 qbar a is needed: the column-scaled update rides in the covariance backward
  float* gamma = exact ? nullptr : c.sc.get<float>((long long)Mg * C);
  const bool identity = !exact && C >= 4LL * L * Mg;
  bool axpy_in_cov = false;
  if (!exact) {
    const long long wsb = gpsa_whiten_workspace(Mg);
    if (wsb > 0) {
      const long long mk2 = c.sc.mark();
      void* ws = c.sv<char>(P.o_apk_d);  // packed by the forward
      // (the column-scaled update is NOT fused into this solve's store - gpsa_whiten_axpy_f32: measured with bench.py,
      // A/B in one run, twice, the fused store made the step 37 us SLOWER (8.939 vs 8.901 ms): its row-strided reads
      // of alpha in the projection kernel's epilogue cost more than the separate streaming pass saves)
      GPSA_RUN(gpsa_whiten_f64(nullptr, GPSA_F32, abar, Mg, C, GPSA_F32, gamma, nullptr, ws, wsb, c.stv()));
      c.sc.release(mk2);
    } else {
      GPSA_CK((gemmx<double, float, float>(c, 0, 0, Mg, (int)C, Mg, 1.0, Kinv, Mg, 0, abar, C, 0, 0.0, gamma, C, 0, 1, 1)));
    }
  }
  // dOmega_l = sum_c g_l alpha alpha^T (fp32 matrix cores, fp64 result)
  {
    const long long mk2 = c.sc.mark();
    long long wsb = gpsa_quadform_workspace(GPSA_F32, Mg, C, L);
    if (ps.gx3 && gpsa_quadform_bwd_omega_x3_workspace(Mg, C, L) > wsb) wsb = gpsa_quadform_bwd_omega_x3_workspace(Mg, C, L);
    void* ws = c.sc.get<char>(wsb);
    double* dst = first_for_mod ? dOm : c.sc.get<double>((long long)L * mm);
    const bool timed = !dry && !c.quiet && &ps == &P.passes[0];
    if (timed) P.tick(2, 0, false, c.st);
    int rc = 0;
    if (dry) {  // what a launch-time refusal of either call below would need: the C-long product's split-K partials
      const long long mk3 = c.sc.mark();  // and the fp32 staging copy of the generic Gram path
      if (ddelta_in_gram)
        GPSA_CK(gemm32(c, 0, 1, Mg, L, C, 1.0, alpha, C, 0, dmeanT, C, 0, 0.0, B.ddc_F[m], L, 0, 1, splitk_for(C, Mg, L)));
      c.sc.get<float>((long long)L * mm);
      c.sc.release(mk3);
    }
    if (!dry && ddelta_in_gram) {
      rc = ps.gx3 ? gpsa_quadform_bwd_omega_delta_x3(GPSA_F64, alpha, g_ext, dmeanT, Mg, C, L, dst, B.ddc_F[m],
                                                     first_for_mod ? 0.0 : 1.0, ws, wsb, c.stv())
                  : gpsa_quadform_bwd_omega_delta_f32(GPSA_F64, alpha, g_ext, dmeanT, Mg, C, L, dst, B.ddc_F[m],
                                                      first_for_mod ? 0.0 : 1.0, ws, wsb, c.stv());
      if (rc == GPSA_EUNSUPPORTED) {  // (operand alignment): the product after all, then the plain call
        GPSA_CK(gemm32(c, 0, 1, Mg, L, C, 1.0, alpha, C, 0, dmeanT, C, 0, first_for_mod ? 0.0 : 1.0, B.ddc_F[m], L, 0, 1,
                       splitk_for(C, Mg, L)));
        rc = ps.gx3 ? gpsa_quadform_bwd_omega_x3(GPSA_F32, GPSA_F64, alpha, g_ext, Mg, C, L, dst, ws, wsb, c.stv())
                    : gpsa_quadform_bwd_omega(GPSA_F32, GPSA_F64, alpha, g_ext, Mg, C, L, dst, ws, wsb, c.stv());
      }
    } else if (!dry) {
      rc = ps.gx3 ? gpsa_quadform_bwd_omega_x3(GPSA_F32, GPSA_F64, alpha, g_ext, Mg, C, L, dst, ws, wsb, c.stv())
                  : gpsa_quadform_bwd_omega(GPSA_F32, GPSA_F64, alpha, g_ext, Mg, C, L, dst, ws, wsb, c.stv());
    }
    if (rc == GPSA_EUNSUPPORTED) {  // generic path stores in the compute type: convert
      float* tmp = c.sc.get<float>((long long)L * mm);
      GPSA_RUN(gpsa_quadform_bwd_omega(GPSA_F32, GPSA_F32, alpha, g_ext, Mg, C, L, tmp, ws, wsb, c.stv()));
      if (!dry) {
        convert_kernel_step<float, double><<<(unsigned)cdiv((long long)L * mm, 256), 256, 0, c.st>>>(
            tmp, (long long)L * mm, dst);
        GPSA_LAUNCH_CHECK();
      }
    } else if (rc != 0) {
      return rc;
    }
    if (timed) { P.tick(2, 1, false, c.st); ++P.tbwd; }
    if (dry) (void)c.sc.get<float>((long long)L * mm);
    if (!first_for_mod && !dry) {
      add_inplace_kernel<<<(unsigned)cdiv((long long)L * mm, 256), 256, 0, c.st>>>(dOm, dst, (long long)L * mm);
      GPSA_LAUNCH_CHECK();
    }
    // dK_uu
    if (identity) {
      // dK_uu = -(gamma + qbar a) a^T without a second C-long product (engine.py:_layer_backward):
      //   gamma a^T = K^-1 (abar a^T),  abar a^T = dc ddc^T + 2 sum_l Omega_l dOmega_l,  (qbar a) a^T = -sum_l dOmega_l
      // on THIS pass's dOmega (dst) and ddc
      double* Pm_ = c.sc.get<double>(mm);
      float* ddc_p = B.ddc_F[m];
      if (!first_for_mod) {  // this pass's own ddc (the accumulated one holds earlier passes too)
        ddc_p = c.sc.get<float>((long long)Mg * L);
        GPSA_CK(gemm32(c, 0, 1, Mg, L, C, 1.0, alpha, C, 0, dmeanT, C, 0, 0.0, ddc_p, L, 0, 1, splitk_for(C, Mg, L)));
      }
      GPSA_CK(gemm64(c, 1, 0, Mg, Mg, (long long)L * Mg, 2.0, Om, Mg, 0, dst, Mg, 0, 0.0, Pm_, Mg, 0, 1,
                     splitk_for((long long)L * Mg, Mg, Mg)));
      GPSA_CK((gemmx<float, float, double>(c, 0, 1, Mg, Mg, L, 1.0, c.prm.delta_F[m], L, 0, ddc_p, L, 0, 1.0, Pm_, Mg, 0,
                                           1, 1)));
      double* sumOm = c.sc.get<double>(mm);
      if (!dry) {
        reduce_rows_kernel<double, double><<<(unsigned)cdiv(mm, 64), 256, 0, c.st>>>(dst, L, mm, mm, sumOm, 1.0);
        GPSA_LAUNCH_CHECK();
      }
      GPSA_CK(gemm64(c, 0, 0, Mg, Mg, Mg, -1.0, Kinv, Mg, 0, Pm_, Mg, 0, 1.0, sumOm, Mg, 0, 1, splitk_small(Mg, Mg, Mg, 1)));
      if (!dry) {  // the gradient buffer starts at zero: every pass adds its share
        add_inplace_kernel<<<(unsigned)cdiv(mm, 256), 256, 0, c.st>>>(dKuu, sumOm, mm);
        GPSA_LAUNCH_CHECK();
      }
      // dK_uf = gamma + 2 qbar a: formed inside the covariance backward as it reads the panel (no pass that
      // writes it out) - except for test passes, whose covariance backward is the plain entry point
      if (ps.test)
        GPSA_RUN(gpsa_col_axpy(GPSA_F32, gamma, alpha, qbar, 2.0, Mg, C, gamma, c.stv()));
      else
        axpy_in_cov = true;
    } else if (!exact) {
      // few columns: W = gamma + qbar a;  dK_uu = -W a^T ADDED in fp64;  dK_uf = W + qbar a
      GPSA_RUN(gpsa_col_axpy(GPSA_F32, gamma, alpha, qbar, 1.0, Mg, C, gamma, c.stv()));
      GPSA_CK((gemmx<float, float, double>(c, 0, 1, Mg, Mg, C, -1.0, gamma, C, 0, alpha, C, 0, 1.0, dKuu, Mg, 0, 1,
                                           splitk_for(C, Mg, Mg))));
      GPSA_RUN(gpsa_col_axpy(GPSA_F32, gamma, alpha, qbar, 1.0, Mg, C, gamma, c.stv()));
    }
    c.sc.release(mk2);
  }
  // covariance backward: fp32 panel, fp64 arithmetic and results; the coordinates' gradient goes back to
  // the warp GPs in fp64
  if (!cov_early) {
    const long long wsb = gpsa_kmat_bwd_workspace(GPSA_F64, Mg, C, D);
    void* ws = c.sc.get<char>(wsb);
    double* dZ = B.dZ_df + (long long)pass_idx * Mg * D;
    double* dpar = B.dpar_df + (long long)pass_idx * 2;
    if (exact && ps.test) {
      GPSA_RUN(gpsa_kmat_bwd(GPSA_F64, GPSA_F32_OUT64, P.d.kind_data, c.prm.Gtilde, Mg, c.io.G_test[m], C, D,
                             c.prm.data_ls, c.prm.data_var, gamma64, 0, dZ, nullptr, dpar, ws, wsb, c.stv()));
    } else if (exact) {
      GPSA_RUN(gpsa_kmat_bwd_x64_f64_axpy(P.d.kind_data, c.prm.Gtilde, Mg, c.sv<double>(P.o_G64[m]), C, D, c.prm.data_ls,
                                          c.prm.data_var, gamma64, c.sv<double>(ps.o_alpha64), qbar, 2.0, dZ, B.dG64[m],
                                          dpar, ws, wsb, c.stv()));
      B.have_dG[m] = true;
    } else if (ps.test) {
      GPSA_RUN(gpsa_kmat_bwd(GPSA_F64, GPSA_F32_ACC64, P.d.kind_data, c.prm.Gtilde, Mg, c.io.G_test[m], C, D,
                             c.prm.data_ls, c.prm.data_var, gamma, 0, dZ, nullptr, dpar, ws, wsb, c.stv()));
    } else {
      GPSA_RUN(gpsa_kmat_bwd_x64_axpy(P.d.kind_data, c.prm.Gtilde, Mg, c.sv<double>(P.o_G64[m]), C, D, c.prm.data_ls,
                                      c.prm.data_var, gamma, axpy_in_cov ? alpha : nullptr, axpy_in_cov ? qbar : nullptr,
                                      2.0, dZ, B.dG64[m], dpar, ws, wsb, c.stv()));
      B.have_dG[m] = true;
    }
  }
  c.sc.release(mk);
  return 0;
}

// acc: the products are ADDED to what the gradient batch already holds (the early order: the KL backward ran first)
static int warp_stage_bwd(Ctx& c, const gpsa_step_out_grads& og, BwdBufs& B, bool acc) {
  Plan& P = c.P;
  const bool dry = c.dry;
  const int D = P.D, Mx = P.Mx, nf = P.nf;
  const long long Cs = P.Cs, mm = (long long)Mx * Mx;
  Group& GW = P.gw();
  if (nf == 0 || Cs == 0) return 0;
  const long long mk = c.sc.mark();
  const float* Xv = c.sv<float>(P.o_Xv);
  const double* alpha = c.sv<double>(P.o_alpha_w);
  const double* Wk = c.sv<double>(P.o_Wk);
  double* dmeanT = c.sc.get<double>((long long)nf * D * Cs);
  double* g = c.sc.get<double>((long long)nf * D * Cs);
  double* qbar = c.sc.get<double>((long long)nf * Cs);
  const long long nblk = cdiv(Cs, 256);
  double* part = c.sc.get<double>((long long)nf * nblk);
  if (!dry) {
    const double* dG64[MAXMODS];
    for (int m = 0; m < MAXMODS; ++m) dG64[m] = (m < P.nm && B.have_dG[m]) ? B.dG64[m] : nullptr;
    dim3 grid((unsigned)nblk, (unsigned)nf);
    const bool closes = nf <= 32;  // (a ticket per free view)
    warp_sample_views_bwd_kernel<<<grid, 256, 0, c.st>>>(P.tab, P.d_free, mod_ptrs(c, &og, dG64), c.io.eps_G, dmeanT,
                                                         g, qbar, part, closes ? B.tick : nullptr, c.prm.warp_var,
                                                         B.dvar_ws);
    GPSA_LAUNCH_CHECK();
    if (!closes) {
      warp_sample_views_bwd_finish_kernel<<<nf, 64, 0, c.st>>>(part, nblk, P.d_free, c.prm.warp_var, B.dvar_ws);
      GPSA_LAUNCH_CHECK();
    }
  }
  double* abar = c.sc.get<double>((long long)nf * Mx * Cs);   // abar, then gamma's right-hand side
  double* gamma = c.sc.get<double>((long long)nf * Mx * Cs);
  for (const Run& r : P.runs) {
    const long long oMC = (long long)r.b0 * Mx * Cs, oDC = (long long)r.b0 * D * Cs;
    const double* resid = c.sv<double>(P.o_resid) + (long long)r.v0 * Mx * D;
    // abar = 2 sum_j g_j o W_j + dc dmean
    GPSA_RUN(gpsa_quadform_bwd_alpha_kept_batched_f64(Wk + (long long)r.b0 * D * Mx * Cs, g + oDC, Mx, Cs, D, resid,
                                                      dmeanT + oDC, abar + oMC, r.cnt, c.stv()));
    // d resid = alpha dmean^T  (the layer's share; the KL's is added by the finalize kernel)
    GPSA_CK(gemm64(c, 0, 1, Mx, D, Cs, 1.0, alpha + oMC, Cs, (long long)Mx * Cs, dmeanT + oDC, Cs, (long long)D * Cs,
                   0.0, B.dresid + (long long)r.v0 * Mx * D, D, (long long)Mx * D, r.cnt, splitk_for(Cs, Mx, D)));
    // gamma = K^-1 abar
    GPSA_CK(project_views(c, c.inv(GW, P.pos_Kw(r.b0)), abar + oMC, Mx, Cs, gamma + oMC, nullptr, r.cnt, r.b0, true));
    // dOmega rows v*D + j (quirk 2) = sum_c g_j alpha alpha^T, and  W = gamma + qbar a;  dK_uu = -W a^T;
    // dK_uf = W + qbar a.  Round 5: all cnt (D + 1) long-K products of the run in two launches of the LDS-DMA fp64
    // kernel (csrc/longk64.hip), the scaled / summed left operands formed in registers - no alpha o g_j copies, one
    // column update (gamma + 2 qbar a) instead of two
    bool done = false;
    // (both launches or neither: whether a shape is covered depends on the number of products too)
    if (r.cnt * D <= 48 && gpsa_longk_f64_workspace(Mx, Cs, r.cnt * D) > 0 && gpsa_longk_f64_workspace(Mx, Cs, r.cnt) > 0) {
      const double *Gs[48], *Bs[48];
      const void* ds[48];
      double al[48], be[48];
      double* os[48];
      int n = 0;
      for (int i = 0; i < r.cnt; ++i)
        for (int jj = 0; jj < D; ++jj, ++n) {
          Gs[n] = nullptr;
          Bs[n] = alpha + oMC + (long long)i * Mx * Cs;
          ds[n] = g + oDC + ((long long)i * D + jj) * Cs;
          al[n] = 1.0;
          be[n] = acc ? 1.0 : 0.0;
          os[n] = B.dstack[0] + ((long long)P.pos_OmG((r.v0 + i) * D + jj)) * mm;
        }
      int rc = longk(c, n, nullptr, Bs, ds, GPSA_F64, Mx, Cs, Cs, 1, al, be, os);
      if (rc == 0) {
        for (int i = 0; i < r.cnt; ++i) {
          Gs[i] = gamma + oMC + (long long)i * Mx * Cs;
          Bs[i] = alpha + oMC + (long long)i * Mx * Cs;
          ds[i] = qbar + (long long)(r.b0 + i) * Cs;
          al[i] = -1.0;
          be[i] = acc ? 1.0 : 0.0;
          os[i] = B.dstack[0] + (long long)P.pos_Kw(r.b0 + i) * mm;
        }
        rc = longk(c, r.cnt, Gs, Bs, ds, GPSA_F64, Mx, Cs, Cs, 0, al, be, os);
        if (rc != 0) return rc == GPSA_EUNSUPPORTED ? GPSA_EINVAL : rc;  // (same shape as the first launch)
        GPSA_RUN(gpsa_col_axpy_batched_f64(gamma + oMC, alpha + oMC, qbar + (long long)r.b0 * Cs, 2.0, Mx, Cs,
                                           gamma + oMC, r.cnt, c.stv()));
        done = true;
      } else if (rc != GPSA_EUNSUPPORTED) {
        return rc;
      }
    }
    if (!done || dry) {  // (the dry run sizes the arena for this path too)
      if (acc && !dry) return GPSA_EINVAL;  // (the early order is only taken when every run is covered: warp_runs_longk)
      {
        const long long mk2 = c.sc.mark();
        const long long wsb = gpsa_gram_batched_workspace(Mx, Cs, D, r.cnt);
        void* ws = c.sc.get<char>(wsb);
        GPSA_RUN(gpsa_gram_batched_f64(alpha + oMC, g + oDC, Mx, Cs, D, B.dstack[0] + (long long)P.pos_OmG(r.v0 * D) * mm,
                                       r.cnt, ws, wsb, c.stv()));
        c.sc.release(mk2);
      }
      GPSA_RUN(gpsa_col_axpy_batched_f64(gamma + oMC, alpha + oMC, qbar + (long long)r.b0 * Cs, 1.0, Mx, Cs, gamma + oMC,
                                         r.cnt, c.stv()));
      GPSA_CK(gemm64(c, 0, 1, Mx, Mx, Cs, -1.0, gamma + oMC, Cs, (long long)Mx * Cs, alpha + oMC, Cs, (long long)Mx * Cs,
                     0.0, B.dstack[0] + (long long)P.pos_Kw(r.b0) * mm, Mx, mm, r.cnt, splitk_for(Cs, Mx, Mx)));
      GPSA_RUN(gpsa_col_axpy_batched_f64(gamma + oMC, alpha + oMC, qbar + (long long)r.b0 * Cs, 1.0, Mx, Cs, gamma + oMC,
                                         r.cnt, c.stv()));
    }
    // covariance backward of K_uf
    {
      const long long mk2 = c.sc.mark();
      long long nlive[KM_MAXB_STEP];
      for (int i = 0; i < r.cnt; ++i) nlive[i] = P.nview[r.v0 + i];
      const long long wsb = gpsa_kmat_bwd_batched_workspace(Mx, Cs, D, r.cnt);
      void* ws = c.sc.get<char>(wsb);
      GPSA_RUN(gpsa_kmat_bwd_batched(P.d.kind_warp, c.prm.Xtilde + (long long)r.v0 * Mx * D, (long long)Mx * D, Mx,
                                     Xv + (long long)r.b0 * Cs * D, Cs * D, Cs, D, c.prm.warp_ls + r.v0,
                                     c.prm.warp_var + r.v0, 1, nlive, r.cnt, gamma + oMC, (long long)Mx * Cs, 0,
                                     B.dZ_wf + (long long)r.b0 * Mx * D, (long long)Mx * D,
                                     B.dpar_wf + (long long)r.b0 * 2, ws, wsb, c.stv()));
      c.sc.release(mk2);
    }
  }
  c.sc.release(mk);
  return 0;
}

// every run of free views takes the long-K kernel for its backward products (the early order needs their beta)
static bool warp_runs_longk(const Plan& P) {
  for (const Run& r : P.runs)
    if (!(r.cnt * P.D <= 48 && gpsa_longk_f64_workspace(P.Mx, P.Cs, r.cnt * P.D) > 0 &&
          gpsa_longk_f64_workspace(P.Mx, P.Cs, r.cnt) > 0))
      return false;
  return true;
}

static int step_backward(Plan& P, const gpsa_step_params& prm, const gpsa_step_io& io,
                         const gpsa_step_out_grads& og, char* saved, Arena& sc, const gpsa_step_param_grads& out,
                         hipStream_t st) {
  Ctx c{P, prm, io, saved, sc, st, sc.dry};
  const bool dry = c.dry;
  const int V = P.V, D = P.D, Mx = P.Mx, Mg = P.Mg, nf = P.nf, npass = (int)P.passes.size();
  BwdBufs B;
  memset(&B, 0, sizeof(B));
  const bool kl = P.d.want_kl != 0 && og.dkl != nullptr;
  for (int g = 0; g < P.ng; ++g) {
    Group& G = P.grp[g];
    B.dD[g] = sc.get<double>((long long)G.n_omega * G.M);
  }
  // everything that must start at zero sits in ONE contiguous region: one fill
  const long long z0 = (sc.off + 255) & ~255LL;
  for (int g = 0; g < P.ng; ++g) {
    Group& G = P.grp[g];
    B.dstack[g] = sc.get<double>((long long)G.nb() * G.M * G.M);
  }
  const long long nwz = (long long)(nf > 0 ? nf : 1) * Mx * D;
  B.dZ_wf = sc.get<double>(nwz);
  B.dpar_wf = sc.get<double>(2LL * (nf > 0 ? nf : 1));
  B.dvar_ws = sc.get<double>(nf > 0 ? nf : 1);
  B.dresid = sc.get<double>((long long)V * Mx * D);
  B.dZ_df = sc.get<double>((long long)(npass > 0 ? npass : 1) * Mg * D);
  B.dpar_df = sc.get<double>(2LL * (npass > 0 ? npass : 1));
  B.dvar_ds = sc.get<double>(npass > 0 ? npass : 1);
  B.tick = sc.get<int>(BWD_TICKS);
  const long long zf = sc.off;  // the region is all doubles (the samplers' scalars were fp32 until round 5)
  sc.get<char>(256);  // (round the region up to the arena's 256-byte granule: the runtime fills an unaligned tail
  const long long z1 = (sc.off + 255) & ~255LL;  //  with a second launch)
  if (!dry) GPSA_CK(zero_fill_async(sc.base + z0, (size_t)(z1 - z0), st));
  if (dry) {
    long long ab = z1 - z0;
    for (int m = 0; m < P.nm; ++m) ab += ((long long)Mg * P.d.n_latent[m] * 4 + 255) & ~255LL;
    for (int m = 0; m < P.nm; ++m)  // dW [L, P] of the LMC modalities (written per slice, straight into out.W)
      if (P.d.has_lmc[m]) ab += ((long long)P.d.n_latent[m] * P.d.n_out[m] * 4 + 255) & ~255LL;
    P.bwd_acc_bytes = ab + 256;
  }
  B.dZ_wu = sc.get<double>(nwz);
  B.dpar_wu = sc.get<double>(2LL * (nf > 0 ? nf : 1));
  B.dZ_du = sc.get<double>((long long)Mg * D); B.dpar_du = sc.get<double>(2);
  for (int m = 0; m < P.nm; ++m) {
    B.ddc_F[m] = sc.get<float>((long long)Mg * P.d.n_latent[m]);
    B.dG64[m] = sc.get<double>((long long)P.S * P.d.n_rows[m] * D);
  }
  // ---- data GP passes
  bool seen[MAXMODS] = {false, false, false, false};
  for (int pi = 0; pi < npass; ++pi) {
    const Pass& ps = P.passes[pi];
    const float* dFl = ps.test ? og.dF_latent_test[ps.m] : og.dF_latent[ps.m];
    const float* dFo = ps.test ? og.dF_obs_test[ps.m] : og.dF_obs[ps.m];
    if (dFl == nullptr && dFo == nullptr && !ps.fused(io)) continue;  // no gradient reached this pass's draws
    // pi selects this pass's slot of the per-pass pieces; the first pass of a modality writes its shared
    // pieces (dOmega rows, d delta_F, dW), later ones add to them
    GPSA_CK(data_pass_bwd(c, ps, pi, dFl, dFo, B, out, !seen[ps.m], og.gloss));
    seen[ps.m] = true;
  }
  // ---- order of the rest.  Ordinary: warp GPs' backward, KL backward, priors' covariance backward, dOmega -> dA,
  //      finalisation.  EARLY (io.f_event: a data-parallel caller wants to start reducing the data GP's span of the
  //      gradients - Omega_sqt_F, delta_F, W: 97 % of the bytes - while the rest still runs): KL backward first, then
  //      dOmega -> dA and the finalisation of the data GP's parameters, the event, and only then the warp GPs' backward
  //      (its products ADDED to the KL shares already in the batch), the priors' backward and everything else.
  const bool early = io.f_event != nullptr && !dry && (io.bwd_acc == nullptr || io.bwd_acc_mode == 0) &&
                     warp_runs_longk(P);
  if (!early) GPSA_CK(warp_stage_bwd(c, og, B, false));
  // ---- one optimiser step as several passes over row slices (train.Microbatches): everything N-scaled of this
  //      slice is in the region [z0, z1) (fp64 pieces, then the samplers' fp32 scalars) and in ddc_F.  A slice that is not
  //      the last adds it to the caller's accumulator and is done; the last one adds the accumulator to its own and
  //      closes ONCE for all of them - KL backward, prior covariances' backward, dOmega -> dA (36 ms at BASELINE config 5),
  //      the fp64 -> fp32 finalisation - instead of once per slice
  if (io.bwd_acc_mode != 0 && io.bwd_acc != nullptr && !dry) {
    char* accb = reinterpret_cast<char*>(io.bwd_acc);
    const long long nD = (zf - z0) / 8;
    double* rD = reinterpret_cast<double*>(sc.base + z0);
    double* aD = reinterpret_cast<double*>(accb);  // (the accumulator mirrors the region byte for byte)
    long long aoff = z1 - z0;
    if (io.bwd_acc_mode == 1) {
      GPSA_CK(copy_async(aD, rD, (size_t)(nD * 8), st));
    } else {
      double* dst = io.bwd_acc_mode == 2 ? aD : rD;
      const double* src = io.bwd_acc_mode == 2 ? rD : aD;
      add_inplace_kernel<<<(unsigned)cdiv(nD, 256), 256, 0, st>>>(dst, src, nD);
      GPSA_LAUNCH_CHECK();
    }
    for (int m = 0; m < P.nm; ++m) {
      const long long n = (long long)Mg * P.d.n_latent[m];
      float* a = reinterpret_cast<float*>(accb + aoff);
      aoff += (n * 4 + 255) & ~255LL;
      if (!B.have_ddc[m]) {  // no gradient reached this modality's draws in this slice
        if (io.bwd_acc_mode == 1) GPSA_CK(zero_fill_async(a, (size_t)(n * 4), st));
        continue;
      }
      if (io.bwd_acc_mode == 1) {
        GPSA_CK(copy_async(a, B.ddc_F[m], (size_t)(n * 4), st));
      } else {
        add_inplace_f32_kernel<<<(unsigned)cdiv(n, 256), 256, 0, st>>>(io.bwd_acc_mode == 2 ? a : B.ddc_F[m],
                                                                        io.bwd_acc_mode == 2 ? B.ddc_F[m] : a, n);
        GPSA_LAUNCH_CHECK();
      }
    }
    // dW = F^T dF_obs of an LMC modality goes straight into the caller's gradient (data_pass_bwd; the host zeroes it
    // when no gradient reached F_obs): a slice that does not close hands autograd nothing, so its share travels here
    for (int m = 0; m < P.nm; ++m) {
      if (!P.d.has_lmc[m]) continue;
      const long long n = (long long)P.d.n_latent[m] * P.d.n_out[m];
      float* a = reinterpret_cast<float*>(accb + aoff);
      aoff += (n * 4 + 255) & ~255LL;
      if (out.W[m] == nullptr) continue;
      if (io.bwd_acc_mode == 1) {
        GPSA_CK(copy_async(a, out.W[m], (size_t)(n * 4), st));
      } else {
        add_inplace_f32_kernel<<<(unsigned)cdiv(n, 256), 256, 0, st>>>(io.bwd_acc_mode == 2 ? a : out.W[m],
                                                                        io.bwd_acc_mode == 2 ? out.W[m] : a, n);
        GPSA_LAUNCH_CHECK();
      }
    }
    if (io.bwd_acc_mode != 3) return 0;
  }
  auto kl_backward = [&]() -> int {
  // ---- KL terms: dOmega, dK_p = 0.5 K_p^-1 S_p K_p^-1, dD, accumulated in place
    for (int g = 0; g < P.ng && kl; ++g) {
      Group& G = P.grp[g];
      if (G.n_omega == 0 || G.n_prior == 0) continue;
      const long long mm = (long long)G.M * G.M;
      const long long mk = sc.mark();
      double* S = sc.get<double>((long long)G.n_prior * mm);
      double* T1 = sc.get<double>((long long)G.n_prior * mm);
      GPSA_RUN(gpsa_mvn_kl_grouped_bwd_acc(c.mats(G, 0), c.inv(G, 0), G.om_idx, G.pr_list, G.grp_off, G.order,
                                           c.sv<double>(G.o_D), c.sv<double>(G.o_KD), og.dkl + G.kl_off, G.M, G.n_omega,
                                           G.n_prior, B.dstack[g] + (long long)G.n_prior * mm, B.dD[g], S, 1, c.stv()));
      GPSA_CK(gemm64(c, 0, 0, G.M, G.M, G.M, 1.0, c.inv(G, 0), G.M, mm, S, G.M, mm, 0.0, T1, G.M, mm, G.n_prior,
                     splitk_few(G.M, G.M, G.M, G.n_prior)));
      GPSA_CK(gemm64(c, 0, 0, G.M, G.M, G.M, 0.5, T1, G.M, mm, c.inv(G, 0), G.M, mm, 1.0, B.dstack[g], G.M, mm, G.n_prior,
                     splitk_few(G.M, G.M, G.M, G.n_prior)));
      sc.release(mk);
    }
    return 0;
  };
  auto priors_backward = [&]() -> int {
  // ---- prior covariances: K_uu of the free views and of the data GP
    {
      for (const Run& r : P.runs) {
        const long long mk = sc.mark();
        const long long wsb = gpsa_kmat_bwd_batched_workspace(Mx, Mx, D, r.cnt);
        void* ws = sc.get<char>(wsb);
        GPSA_RUN(gpsa_kmat_bwd_batched(P.d.kind_warp, prm.Xtilde + (long long)r.v0 * Mx * D, (long long)Mx * D, Mx,
                                       prm.Xtilde + (long long)r.v0 * Mx * D, (long long)Mx * D, Mx, D, prm.warp_ls + r.v0,
                                       prm.warp_var + r.v0, 1, nullptr, r.cnt,
                                       B.dstack[0] + (long long)P.pos_Kw(r.b0) * Mx * Mx, (long long)Mx * Mx, 1,
                                       B.dZ_wu + (long long)r.b0 * Mx * D, (long long)Mx * D, B.dpar_wu + (long long)r.b0 * 2,
                                       ws, wsb, c.stv()));
        sc.release(mk);
      }
      {
        const long long mk = sc.mark();
        const long long wsb = gpsa_kmat_bwd_batched_workspace(Mg, Mg, D, 1);
        void* ws = sc.get<char>(wsb);
        GPSA_RUN(gpsa_kmat_bwd_batched(P.d.kind_data, prm.Gtilde, 0, Mg, prm.Gtilde, 0, Mg, D, prm.data_ls, prm.data_var, 0,
                                       nullptr, 1, B.dstack[P.merged ? 0 : 1] + (long long)P.pos_KF() * Mg * Mg, 0, 1,
                                       B.dZ_du, 0, B.dpar_du, ws, wsb, c.stv()));
        sc.release(mk);
      }
    }
    return 0;
  };
  // variational covariances: d Omega_sqt = (G + G^T) A = 2 G A (every gradient that reaches Omega is symmetric);
  // which: 1 = the warp GPs' factors, 2 = the modalities', 3 = both (one launch with the first modality's when the
  // sizes agree)
  auto omega_backward = [&](int which) -> int {
    int m_first = 0;
    if ((which & 1) && out.Omega_sqt_G != nullptr) {
      if ((which & 2) && Mx == Mg && P.nm > 0 && out.Omega_sqt_F[0] != nullptr) {
        m_first = 1;
        GPSA_RUN(gpsa_omega_bwd2(B.dstack[0] + (long long)P.pos_OmG(0) * Mx * Mx, prm.Omega_sqt_G, out.Omega_sqt_G, V * D,
                                 B.dstack[P.merged ? 0 : 1] + (long long)P.pos_OmF(0, 0) * Mg * Mg, prm.Omega_sqt_F[0],
                                 out.Omega_sqt_F[0], P.d.n_latent[0], Mx, 1, c.stv()));
      } else {
        GPSA_RUN(gpsa_omega_bwd(B.dstack[0] + (long long)P.pos_OmG(0) * Mx * Mx, prm.Omega_sqt_G, Mx, V * D, 1,
                                out.Omega_sqt_G, c.stv()));
      }
    }
    if (which & 2)
      for (int m = m_first; m < P.nm; ++m)
        if (out.Omega_sqt_F[m] != nullptr)
          GPSA_RUN(gpsa_omega_bwd(B.dstack[P.merged ? 0 : 1] + (long long)P.pos_OmF(m, 0) * Mg * Mg, prm.Omega_sqt_F[m], Mg,
                                  P.d.n_latent[m], 1, out.Omega_sqt_F[m], c.stv()));
    return 0;
  };
  auto finalize = [&](int part) -> int {
    FinalArgs a;
    memset(&a, 0, sizeof(a));
    a.part = part;
    a.V = V; a.D = D; a.Mx = Mx; a.Mg = Mg; a.nm = P.nm; a.nf = nf; a.npass = npass;
    a.bidx = P.tab.bidx;
    a.slopes = prm.slopes;
    a.dZ_wf = B.dZ_wf; a.dZ_wu = B.dZ_wu; a.dpar_wf = B.dpar_wf; a.dpar_wu = B.dpar_wu; a.dvar_ws = B.dvar_ws;
    a.dresid = B.dresid;
    a.dD_w = kl ? B.dD[0] : nullptr;
    a.dZ_df = B.dZ_df; a.dpar_df = B.dpar_df; a.dvar_ds = B.dvar_ds; a.dZ_du = B.dZ_du; a.dpar_du = B.dpar_du;
    a.dD_d = kl ? (P.merged ? B.dD[0] + (long long)V * D * Mx : B.dD[1]) : nullptr;
    const long long nsmall = (long long)V * Mx * D + 2LL * V + (long long)Mg * D + 2;
    long long nF = 0;
    for (int m = 0; m < P.nm; ++m) {
      a.ddc_F[m] = B.have_ddc[m] ? B.ddc_F[m] : nullptr;
      a.L[m] = P.d.n_latent[m];
      a.Loff[m] = P.Loff[m];
      nF += (long long)Mg * P.d.n_latent[m];
    }
    a.out = out;
    if (part != 1 && io.loss_src != nullptr && io.loss_dst != nullptr) {
      a.loss_src = io.loss_src;
      a.loss_dst = io.loss_dst;
    }
    const long long tot = part == 1 ? nF : (part == 2 ? nsmall : nsmall + nF);
    if (!dry && tot > 0) {
      step_finalize_kernel<<<(unsigned)cdiv(tot, 256), 256, 0, st>>>(a);
      GPSA_LAUNCH_CHECK();
    }
    return 0;
  };
  if (early) {
    ++P.n_early;
    GPSA_CK(kl_backward());
    GPSA_CK(omega_backward(2));
    GPSA_CK(finalize(1));
    GPSA_CK((int)hipEventRecord(reinterpret_cast<hipEvent_t>(io.f_event), st));
    GPSA_CK(warp_stage_bwd(c, og, B, true));
    GPSA_CK(priors_backward());
    GPSA_CK(omega_backward(1));
    GPSA_CK(finalize(2));
  } else {
    GPSA_CK(kl_backward());
    GPSA_CK(priors_backward());
    GPSA_CK(omega_backward(3));
    GPSA_CK(finalize(0));
    if (io.f_event != nullptr && !dry) GPSA_CK((int)hipEventRecord(reinterpret_cast<hipEvent_t>(io.f_event), st));
  }
  return 0;
}

}  // namespace gpsa

/* ---- hipGraph cache of the engine's launch sequences (round 5; EXPERIMENTAL, off by default) -------------------------
 * A call of gpsa_step_forward / _backward enqueues 20 - 45 launches; on a launch-bound problem (BASELINE config 1's size,
 * a 1/8 row shard of the headline one, S = 1) the host time per launch is a visible part of the step.  The launch
 * sequence is a pure function of (plan, the four pointer structs, the two arenas, stages, stream): when a call arrives
 * with an argument set that has been seen before - the caching allocator of a fresh training loop hands out the same
 * blocks every other step - its sequence is captured once and replayed as ONE hipGraphLaunch from then on.  The capture
 * runs on a stream of the plan's own (the caller's is usually PyTorch's null stream, which cannot be captured); the
 * graph is launched into the caller's stream.  A first sighting runs eagerly; <= 32 graphs per plan
 * (GPSA_STEP_GRAPH_MAX), least recently used out - retired behind an event, never destroyed under a queued launch; after 8 captures in a row that were never replayed the plan stops capturing.  Never used inside somebody
 * else's capture (train.GraphedTrainStep) or with the kernel timing on.
 * Measured (tools/graph_probe.py, BASELINE config 1's size, the reference's loop, runs alternating in one process):
 *   * a fresh process replays 3879 of 3903 calls from 6 graphs (three call kinds x the allocator's two alternating block
 *     sets); a model built after others have come and gone in the same process meets a longer-period allocation
 *     pattern: 9 captures, no replay, the plan gives up;
 *   * ms/step with the cache on / off: 0.541 / 0.676, 0.590 / 0.723, 0.543 / 0.542 (FusedAdam) and 0.623 / 0.697,
 *     0.725 / 0.727 (torch.optim.Adam + loss.item()), while the SAME configuration drifts between 0.52 and 0.87 ms from
 *     run to run on these boxes - Python, not the launches, is most of the host's share, and the gain is not separable
 *     from the drift;
 *   * OPEN: in one sequence of runs the third model with the cache on raised the forward's numerics error (a
 *     non-positive-definite covariance) some hundred steps in; twelve runs with the cache off never did.  Not
 *     reproduced since (36 model runs of tools/graph_probe.py with the eviction of that day and with the current one;
 *     tools/graph_stress.py and tests/test_step_engine.py train models twice from one seed, cache off / on, and
 *     compare the loss trajectories bit for bit).  One real hazard of that day's code is closed: an evicted graph
 *     was destroyed at once, possibly under a launch of its own still queued behind the host - it now retires behind
 *     an event.  A second one was found at the end of round 6 (LAB_NOTES): a hipMemsetAsync captured into a graph - the
 *     backward's zero fill was one - can land BEHIND the kernel node that follows it; the library zero-fills with a
 *     kernel of its own since.  Whether that was the error of round 5 is not known: it never reproduced.
 * Hence OFF unless asked for (GPSA_STEP_GRAPH=1, gpsa_step_graph(plan, 1, ...)).  End of round 6, with the memset
 * hazard closed: 18 more model runs clean (profiles/r06_graph_cache_stress_final.txt), the whole GPU suite green with the
 * cache forced on (500 tests), and again with it on for launch-bound plans only (a default that was built and taken
 * back: BASELINE config 1 gained 0 - 90 % with FusedAdam and 0 - 35 % in the verbatim loop depending on the box and
 * the run - 1017 / 1380 against 1016 steps/s on a slow host, 1590 - 1740 on a fast one - which does not buy back one
 * open question in the last round).  bench.py reports config 1 with the cache on as an extra key.  The model's route
 * to one launch per step stays the whole-step graph, train.GraphedTrainStep / fit(graphed=True). */
namespace gpsa {

static bool graph_usable(Plan& P, hipStream_t st) {
  if (P.g_enabled < 0) {
    const char* e = getenv("GPSA_STEP_GRAPH");
    P.g_enabled = (e && e[0] == '1') ? 1 : 0;
  }
  if (!P.g_enabled || P.tslots != 0 || P.g_idle_captures > 8) return false;
  for (int m = 0; m < P.nm; ++m)  // (gpsa_step_likelihood's state is not part of the key: such a plan runs eagerly)
    if (P.lik[m] != GPSA_LIK_GAUSSIAN) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
  return true;
}

template <typename F>
static int graph_call(Plan& P, const Plan::GraphKey& key, hipStream_t st, F&& enqueue) {
  ++P.gtick;
  for (size_t i = 0; i < P.retired.size();) {  // dropped graphs whose last launch has completed
    if (hipEventQuery(P.retired[i].ev) == hipSuccess) {
      (void)hipGraphExecDestroy(P.retired[i].exec);
      (void)hipEventDestroy(P.retired[i].ev);
      P.retired.erase(P.retired.begin() + (long)i);
    } else {
      (void)hipGetLastError();  // hipErrorNotReady
      ++i;
    }
  }
  for (auto& ge : P.graphs)
    if (memcmp(ge.key.b, key.b, Plan::GraphKey::BYTES) == 0) {
      if (ge.used == 0) P.g_idle_captures = 0;
      ge.used = P.gtick;
      ge.last = st;
      ++P.g_hits;
      return (int)hipGraphLaunch(ge.exec, st);
    }
  bool met = false;
  for (auto& k : P.seen)
    if (memcmp(k.b, key.b, Plan::GraphKey::BYTES) == 0) { met = true; break; }
  if (!met) {
    static const bool dbg = [] { const char* e = getenv("GPSA_STEP_GRAPH_DEBUG"); return e && e[0] == '1'; }();
    if (dbg) {  // which 8-byte words differ from the most recent call of the same kind
      for (size_t q = P.seen.size(); q-- > 0;) {
        const Plan::GraphKey& o = P.seen[q];
        if (o.bwd() != key.bwd() || o.stages() != key.stages()) continue;
        fprintf(stderr, "[step graph] %s stages %d differs from its last sighting at bytes:", key.bwd() ? "bwd" : "fwd",
                key.stages());
        for (size_t i = 0; i < Plan::GraphKey::BYTES; i += 8)
          if (memcmp(o.b + i, key.b + i, 8) != 0) fprintf(stderr, " %zu", i);
        fprintf(stderr, "  [io at %zu, og at %zu, pg at %zu, arenas at %zu]\n", Plan::GraphKey::O_IO, Plan::GraphKey::O_OG,
                Plan::GraphKey::O_PG, Plan::GraphKey::O_PTR);
        break;
      }
    }
    if (P.seen.size() >= 96) P.seen.erase(P.seen.begin());
    P.seen.push_back(key);
    ++P.g_eager;
    return enqueue(st);
  }
  // second sighting: capture (on the plan's own stream), instantiate, replay into the caller's stream
  if (P.gstream == nullptr && hipStreamCreateWithFlags(&P.gstream, hipStreamNonBlocking) != hipSuccess) {
    P.gstream = nullptr;
    (void)hipGetLastError();
    P.g_enabled = 0;
    ++P.g_eager;
    return enqueue(st);
  }
  if (hipStreamBeginCapture(P.gstream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    P.g_enabled = 0;
    ++P.g_eager;
    return enqueue(st);
  }
  const int rc = enqueue(P.gstream);
  hipGraph_t g = nullptr;
  const hipError_t ec = hipStreamEndCapture(P.gstream, &g);
  if (rc != 0 || ec != hipSuccess || g == nullptr) {
    if (g != nullptr) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    if (rc != 0) return rc;  // the sequence itself failed: nothing has run, the caller sees its error
    P.g_enabled = 0;         // capture is not available here: eager from now on
    ++P.g_eager;
    return enqueue(st);
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ei != hipSuccess || exec == nullptr) {
    (void)hipGetLastError();
    P.g_enabled = 0;
    ++P.g_eager;
    return enqueue(st);
  }
  static const size_t gmax = [] {
    const char* e = getenv("GPSA_STEP_GRAPH_MAX");
    const int v = e ? atoi(e) : 32;
    return (size_t)(v < 1 ? 1 : v);
  }();
  if (P.graphs.size() >= gmax) {
    size_t lru = 0;
    for (size_t i = 1; i < P.graphs.size(); ++i)
      if (P.graphs[i].used < P.graphs[lru].used) lru = i;
    // The dropped graph's latest launch may still be queued (the host runs steps ahead of the device): destroying it
    // now pulls the kernel arguments from under that launch (round 5's unexplained numerics errors "with the cache
    // on, in models built after others" - the models whose allocation pattern has more than 16 distinct argument sets
    // and therefore evicts).  It retires behind an event on the stream it was launched into instead.
    hipEvent_t ev = nullptr;
    // (the victim may have been launched into ANOTHER stream than this call's - the key includes the stream)
    hipStream_t vst = P.graphs[lru].last;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, vst) == hipSuccess) {
      P.retired.push_back(Plan::Retired{P.graphs[lru].exec, ev});
    } else {
      if (ev != nullptr) (void)hipEventDestroy(ev);
      (void)hipStreamSynchronize(vst);
      (void)hipGraphExecDestroy(P.graphs[lru].exec);
    }
    P.graphs.erase(P.graphs.begin() + (long)lru);
  }
  P.graphs.push_back(Plan::GraphEntry{key, exec, 0, st});  // used == 0: captured, not replayed yet
  ++P.g_captures;
  ++P.g_idle_captures;
  return (int)hipGraphLaunch(exec, st);
}

}  // namespace gpsa

extern "C" {

static gpsa::Plan* plan_with_sizes(const gpsa_step_desc* desc, bool host_only);

void* gpsa_step_create(const gpsa_step_desc* desc) { return plan_with_sizes(desc, false); }

/* host-only description of a plan (no device needed): out[0..5] = saved bytes, scratch bytes, KL terms, floats
 * of eps_G, batched runs of free views, column stride of the view blocks.  0, or GPSA_EINVAL for a description
 * gpsa_step_create would refuse. */
int gpsa_step_describe(const gpsa_step_desc* desc, long long* out) {
  if (!out) return GPSA_EINVAL;
  gpsa::Plan* p = plan_with_sizes(desc, true);
  if (p == nullptr) return GPSA_EINVAL;
  out[0] = p->saved_bytes;
  out[1] = p->scratch_bytes;
  out[2] = (long long)p->V * p->D + p->Ltot;
  out[3] = p->eps_total;
  out[4] = (long long)p->runs.size();
  out[5] = p->Cs;
  out[6] = p->saved_bytes_nokeep;
  gpsa::free_plan(p);
  return 0;
}

static gpsa::Plan* plan_with_sizes(const gpsa_step_desc* desc, bool host_only) {
  using namespace gpsa;
  Plan* p = make_plan(desc, host_only);
  if (p == nullptr) return nullptr;
  // scratch requirement = high-water mark of a dry run of the forward and of the backward
  Arena a;
  a.dry = true;
  gpsa_step_params prm;
  gpsa_step_io io;
  gpsa_step_out_grads og;
  gpsa_step_param_grads pg;
  memset(&prm, 0, sizeof(prm)); memset(&io, 0, sizeof(io)); memset(&og, 0, sizeof(og)); memset(&pg, 0, sizeof(pg));
  // pretend every gradient is present so that the dry run walks every branch
  static const float dummy = 0.f;
  static const double dummyd = 0.0;
  for (int m = 0; m < p->nm; ++m) {
    og.dF_latent[m] = &dummy;
    if (p->d.has_lmc[m]) og.dF_obs[m] = &dummy;
    og.dF_latent_test[m] = &dummy;
    if (p->d.has_lmc[m]) og.dF_obs_test[m] = &dummy;
    pg.W[m] = const_cast<float*>(&dummy);
    io.F_obs[m] = const_cast<float*>(&dummy);
    io.F_obs_test[m] = const_cast<float*>(&dummy);
  }
  og.dkl = &dummyd;
  if (step_forward(*p, prm, io, nullptr, a, nullptr, 3) != 0) { free_plan(p); return nullptr; }
  a.off = 0;
  if (step_backward(*p, prm, io, og, nullptr, a, pg, nullptr) != 0) { free_plan(p); return nullptr; }
  // ... and the fused-ELBO variant of the same step (its kernel's workspace holds the partial-tile slabs)
  io.fuse_elbo = 1;
  og.gloss = &dummy;
  for (int m = 0; m < p->nm; ++m) {
    io.Y[m] = io.noise_u[m] = &dummy;
    io.ll_part[m] = const_cast<double*>(&dummyd);
  }
  a.off = 0;
  if (step_forward(*p, prm, io, nullptr, a, nullptr, 3) != 0) { free_plan(p); return nullptr; }
  a.off = 0;
  if (step_backward(*p, prm, io, og, nullptr, a, pg, nullptr) != 0) { free_plan(p); return nullptr; }
  p->scratch_bytes = a.high + 4096;
  return p;
}

void gpsa_step_destroy(void* plan) { gpsa::free_plan(reinterpret_cast<gpsa::Plan*>(plan)); }
long long gpsa_step_saved_bytes(const void* plan) { return plan ? reinterpret_cast<const gpsa::Plan*>(plan)->saved_bytes : -1; }
long long gpsa_step_saved_bytes_nokeep(const void* plan) {
  return plan ? reinterpret_cast<const gpsa::Plan*>(plan)->saved_bytes_nokeep : -1;
}
int gpsa_step_fused(const void* plan, int m) {
  if (!plan) return 0;
  for (const gpsa::Pass& q : reinterpret_cast<const gpsa::Plan*>(plan)->passes)
    if (q.m == m && !q.test) return q.o_fuse >= 0 ? 1 : 0;
  return 0;
}
int gpsa_step_contraction(const void* plan, int m) {
  if (!plan) return 0;
  for (const gpsa::Pass& q : reinterpret_cast<const gpsa::Plan*>(plan)->passes)
    if (q.m == m && !q.test) {  // (skip_seen: the plan's last fused pass took the fp32 skip kernel, gpsa_step_io.skip_missing;
      const gpsa::Plan* p = reinterpret_cast<const gpsa::Plan*>(plan);  //  a Poisson modality's takes the fp32 Poisson kernel)
      return ((q.o_fuse >= 0 && q.x3 && !p->skip_seen && p->lik[m] == GPSA_LIK_GAUSSIAN) ? 1 : 0) | (q.gx3 ? 2 : 0);
    }
  return 0;
}
int gpsa_step_likelihood(void* plan, int m, int kind, const float* log_offset) {
  if (!plan) return GPSA_EINVAL;
  gpsa::Plan* p = reinterpret_cast<gpsa::Plan*>(plan);
  if (m < 0 || m >= p->nm || (kind != GPSA_LIK_GAUSSIAN && kind != GPSA_LIK_POISSON)) return GPSA_EINVAL;
  if (kind == GPSA_LIK_GAUSSIAN && log_offset != nullptr) return GPSA_EINVAL;
  p->lik[m] = kind;
  p->log_offset[m] = log_offset;
  p->log_disp[m] = nullptr;  // (a modality that was negative binomial is so no longer)
  p->u_elems[m] = nullptr;
  p->usum[m] = nullptr;
  return 0;
}
int gpsa_step_dispersion(void* plan, int m, const float* log_disp, float* u_elems, double* usum, const float* log_offset) {
  if (!plan) return GPSA_EINVAL;
  gpsa::Plan* p = reinterpret_cast<gpsa::Plan*>(plan);
  if (m < 0 || m >= p->nm || !log_disp || !u_elems || !usum) return GPSA_EINVAL;
  p->lik[m] = GPSA_LIK_NEGBIN;
  p->log_offset[m] = log_offset;
  p->log_disp[m] = log_disp;
  p->u_elems[m] = u_elems;
  p->usum[m] = usum;
  return 0;
}
long long gpsa_step_bwd_acc_bytes(const void* plan) { return plan ? reinterpret_cast<const gpsa::Plan*>(plan)->bwd_acc_bytes : -1; }
long long gpsa_step_scratch_bytes(const void* plan) { return plan ? reinterpret_cast<const gpsa::Plan*>(plan)->scratch_bytes : -1; }
int gpsa_step_n_kl(const void* plan) {
  if (!plan) return -1;
  const gpsa::Plan* p = reinterpret_cast<const gpsa::Plan*>(plan);
  return p->V * p->D + p->Ltot;
}
int gpsa_step_n_factorised(const void* plan) {
  if (!plan) return -1;
  const gpsa::Plan* p = reinterpret_cast<const gpsa::Plan*>(plan);
  int n = 0;
  for (int g = 0; g < p->ng; ++g) n += p->grp[g].n_prior + (p->grp[g].own_hi - p->grp[g].own_lo);
  return n;
}
long long gpsa_step_eps_g_numel(const void* plan) { return plan ? reinterpret_cast<const gpsa::Plan*>(plan)->eps_total : -1; }
long long gpsa_step_early_backwards(const void* plan) {
  return plan ? reinterpret_cast<const gpsa::Plan*>(plan)->n_early : -1;
}
int gpsa_step_batch_layout(const void* plan, long long* out) {
  if (!plan || !out) return GPSA_EINVAL;
  const gpsa::Plan* p = reinterpret_cast<const gpsa::Plan*>(plan);
  out[0] = p->ng;
  for (int g = 0; g < p->ng; ++g) {
    out[1 + 4 * g] = p->grp[g].M;
    out[2 + 4 * g] = p->grp[g].n_prior;
    out[3 + 4 * g] = p->grp[g].n_omega;
    out[4 + 4 * g] = p->grp[g].o_mats;
  }
  return 0;
}

/* timing of the contraction kernels (diagnostic; bench.py): events around gpsa_quadform_fwd / _bwd_alpha /
 * _bwd_omega of the first data-GP pass for the next ``slots`` steps (a ring); 0 switches it off */
/* id of the stream capture ``stream`` is part of, 0 when it is not capturing (hipStreamGetCaptureInfo): a host that
 * caches device scratch per stream must not hand a block it allocated INSIDE one capture - it lives in that graph's
 * private pool - to a later capture */
unsigned long long gpsa_stream_capture_id(void* stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo(as_stream(stream), &cs, &id) != hipSuccess) return 0;
  return cs == hipStreamCaptureStatusActive ? (id ? id : ~0ULL) : 0;
}

int gpsa_step_timing(void* plan, int slots) {
  using namespace gpsa;
  if (!plan || slots < 0) return GPSA_EINVAL;
  Plan& P = *reinterpret_cast<Plan*>(plan);
  for (hipEvent_t e : P.tev) (void)hipEventDestroy(e);
  P.tev.clear();
  P.tslots = 0;
  P.tfwd = P.tbwd = 0;
  // timing-only events: no system-scope fence (cache write-back and invalidation) at the record - the reader
  // synchronises the stream itself.  (Measured: no difference in the bench loop either way; GPSA_TIMING_FENCE=1: plain events)
  static const bool fence = [] { const char* e = getenv("GPSA_TIMING_FENCE"); return e && e[0] == '1'; }();
  for (int i = 0; i < slots * 6; ++i) {
    hipEvent_t e;
    if ((fence ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableSystemFence)) != hipSuccess)
      return GPSA_EINVAL;
    P.tev.push_back(e);
  }
  P.tslots = slots;
  return 0;
}

/* ms[3 * n]: per recorded step (oldest first, n = min(steps since gpsa_step_timing, slots)) the duration of
 * the three kernels; the caller has synchronised the stream.  Returns n or a negative error. */
int gpsa_step_timing_read(void* plan, float* ms, int max_steps) {
  using namespace gpsa;
  if (!plan || !ms) return GPSA_EINVAL;
  Plan& P = *reinterpret_cast<Plan*>(plan);
  if (P.tslots == 0) return 0;
  int n = P.tfwd < P.tbwd ? P.tfwd : P.tbwd;
  if (n > P.tslots) n = P.tslots;
  if (n > max_steps) n = max_steps;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      const int stepno = (k == 0 ? P.tfwd : P.tbwd) - n + i;
      const int slot = stepno % P.tslots;
      float t = 0.f;
      if (hipEventElapsedTime(&t, P.tev[(size_t)(slot * 3 + k) * 2], P.tev[(size_t)(slot * 3 + k) * 2 + 1]) != hipSuccess)
        return GPSA_EINVAL;
      ms[i * 3 + k] = t;
    }
  return n;
}

int gpsa_step_forward(void* plan, const gpsa_step_params* params, const gpsa_step_io* io, void* saved, void* scratch,
                      int stages, void* stream) {
  using namespace gpsa;
  if (!plan || !params || !io || !saved || !scratch) return GPSA_EINVAL;
  Plan& P = *reinterpret_cast<Plan*>(plan);
  if (P.d.want_kl && io->kl == nullptr) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  auto enqueue = [&](hipStream_t s) {
    Arena a;
    a.base = reinterpret_cast<char*>(scratch);
    a.limit = reinterpret_cast<gpsa::Plan*>(plan)->scratch_bytes;
    return step_forward(P, *params, *io, reinterpret_cast<char*>(saved), a, s, stages);
  };
  if (!graph_usable(P, st)) return enqueue(st);
  Plan::GraphKey key;
  key.set(params, io, nullptr, nullptr, saved, scratch, stream, stages, 0);
  return graph_call(P, key, st, enqueue);
}

int gpsa_step_backward(void* plan, const gpsa_step_params* params, const gpsa_step_io* io,
                       const gpsa_step_out_grads* og, void* saved, void* scratch, const gpsa_step_param_grads* grads,
                       void* stream) {
  using namespace gpsa;
  if (!plan || !params || !io || !og || !saved || !scratch || !grads) return GPSA_EINVAL;
  Plan& P = *reinterpret_cast<Plan*>(plan);
  hipStream_t st = as_stream(stream);
  auto enqueue = [&](hipStream_t s) {
    Arena a;
    a.base = reinterpret_cast<char*>(scratch);
    a.limit = reinterpret_cast<gpsa::Plan*>(plan)->scratch_bytes;
    return step_backward(P, *params, *io, *og, reinterpret_cast<char*>(saved), a, *grads, s);
  };
  // (a backward that records the caller's event - the overlapped reducer's f_event - stays eager: an event record
  //  captured into a cached graph and waited for from outside it is a combination nobody has tested)
  if (io->f_event != nullptr || !graph_usable(P, st)) return enqueue(st);
  Plan::GraphKey key;
  key.set(params, io, og, grads, saved, scratch, stream, 0, 1);
  return graph_call(P, key, st, enqueue);
}

/* the cache's switch and counters: enable != 0 / 0 (-1: leave as it is); out[0..3] = replays, eager calls, captures,
 * graphs held (out may be NULL) */
int gpsa_step_graph(void* plan, int enable, long long* out) {
  using namespace gpsa;
  if (!plan) return GPSA_EINVAL;
  Plan& P = *reinterpret_cast<Plan*>(plan);
  if (enable >= 0) {
    P.g_enabled = enable ? 1 : 0;
    P.g_idle_captures = 0;
  }
  if (out) {
    out[0] = P.g_hits; out[1] = P.g_eager; out[2] = P.g_captures; out[3] = (long long)P.graphs.size();
  }
  return 0;
}

int gpsa_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const long long* numel, double lr, double beta1, double beta2, double eps,
                   float* step, void* stream) {
  using namespace gpsa;
  if (n < 1 || !params || !grads || !exp_avg || !exp_avg_sq || !numel || !step) return GPSA_EINVAL;
  hipStream_t st = as_stream(stream);
  adam_tick_kernel<<<1, 1, 0, st>>>(step);
  GPSA_LAUNCH_CHECK();
  for (int i0 = 0; i0 < n; i0 += ADAM_MAXT) {
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    a.nt = n - i0 < ADAM_MAXT ? n - i0 : ADAM_MAXT;
    long long blk = 0;
    for (int t = 0; t < a.nt; ++t) {
      a.p[t] = params[i0 + t]; a.g[t] = grads[i0 + t]; a.m[t] = exp_avg[i0 + t]; a.v[t] = exp_avg_sq[i0 + t];
      a.n[t] = numel[i0 + t];
      a.blk0[t] = blk;
      blk += cdiv(numel[i0 + t], 1024);
    }
    a.blk0[a.nt] = blk;
    a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps;
    if (blk > 0) {
      adam_kernel<<<(unsigned)blk, 256, 0, st>>>(a, step);
      GPSA_LAUNCH_CHECK();
    }
  }
  return 0;
}

}  // extern "C"
