// Launchers shared between the translation units of libgpsa_hip (defined where their kernels live).
#pragma once
#include "common.hpp"

namespace gpsa {

// gemm.hip: C[b] = alpha op(A[b]) op(B[b]) + beta C[b], row-major, strided batch, deterministic split-K
template <typename T>
int gemm_launch(int transA, int transB, int m, int n, long long k, double alpha, const T* A, long long lda,
                long long sA, const T* B, long long ldb, long long sB, double beta, T* C, long long ldc,
                long long sC, int batch, int splitk, void* ws, long long ws_bytes, hipStream_t st);
// triangle modes of the MFMA product (gemm.hip documents them at the kernel)
enum { GEMM_TRI_NONE = 0, GEMM_TRI_UPPER_A = 1, GEMM_TRI_LOWER_C = 2, GEMM_TRI_LTL = 3 };
template <typename T>
int gemm_launch_tri(int transA, int transB, int m, int n, long long k, double alpha, const T* A, long long lda,
                    long long sA, const T* B, long long ldb, long long sB, double beta, T* C, long long ldc,
                    long long sC, int batch, int splitk, void* ws, long long ws_bytes, hipStream_t st, int tri);
// the same accumulated in fp64 from operands / into results of either precision (instantiated for
// (double,float,float), (float,float,double), (double,double,float))
template <typename TIA, typename TIB, typename TO>
int gemm64_launch(int transA, int transB, int m, int n, long long k, double alpha, const TIA* A, long long lda,
                  long long sA, const TIB* B, long long ldb, long long sB, double beta, TO* C, long long ldc,
                  long long sC, int batch, int splitk, void* ws, long long ws_bytes, hipStream_t st);

// quadform.hip: Omega = A A^T + jitter I with LDS-DMA staging (GPSA_EUNSUPPORTED: shape / alignment not covered)
int omega_fwd_dma_launch(const float* A0, int n0, double* O0, const float* A1, int n1, double* O1, int M, double jitter,
                         hipStream_t st);

// quadform.hip: dA = 2 G A for symmetric G with the same staging
int omega_bwd_dma_launch(const double* G0, const float* A0, float* D0, int n0, const double* G1, const float* A1,
                         float* D1, int n1, int M, hipStream_t st);

// kl.hip: gpsa_mvn_kl_grouped_fwd that also writes the terms to kl_copy (may be NULL)
int mvn_kl_grouped_fwd_slices(int M);  // row slices per term (sizes the partial sums: [T][slices] doubles)
int mvn_kl_grouped_fwd_copy(const double* mats, const double* inv, const double* logdet, const int* om_idx,
                            const int* pr_idx, const double* D, int M, int T, double* kl, double* KD,
                            double* kl_copy, double* part, int* cnt, hipStream_t st);

// lmc.hip: the LMC likelihood, its gradient and the two LMC gradient products on the matrix cores, G workgroups
// (zpart [nparts >= G], dWpart [G][L][P]); GPSA_EUNSUPPORTED beyond 64 latent outputs
int lmc_mfma_launch(const float* F, const float* W, const float* Y, const float* noise_u, int S, long long N, int L,
                    int P, double* zpart, int nparts, float* dF, float* dWpart, int G, hipStream_t st);
// ... with the NaN entries of Y left out of all of it (lmc_mfma_skip_kernel)
int lmc_mfma_skip_launch(const float* F, const float* W, const float* Y, const float* noise_u, int S, long long N, int L,
                         int P, double* zpart, int nparts, float* dF, float* dWpart, int G, hipStream_t st);

// loss_views.hip: the per-view row table of a likelihood term (the weighted and the skip loss closings, and the counting
// of missing.hip): at most LOSS_MAX_VIEWS views, view v = rows off[v] .. off[v + 1]
constexpr int LOSS_MAX_VIEWS = 64;
struct ViewRows {
  long long off[LOSS_MAX_VIEWS + 1];
};
static inline bool views_ok(int V, const long long* off, long long N) {
  if (V < 1 || V > LOSS_MAX_VIEWS || off == nullptr || off[0] != 0 || off[V] != N) return false;
  for (int v = 0; v < V; ++v)
    if (off[v + 1] < off[v]) return false;
  return true;
}
// the caller's V views (checked by views_ok), or with off == nullptr one view of all N rows
static inline ViewRows view_rows(long long N, int V, const long long* off) {
  ViewRows vr;
  if (off != nullptr) {
    for (int v = 0; v <= V; ++v) vr.off[v] = off[v];
  } else {
    vr.off[0] = 0;
    vr.off[1] = N;
  }
  return vr;
}

// poisson.hip: the Poisson term's per-element kernel (loglik_pois_kernel<bwd>), grid (nb, V) over the term's views:
// forward: part[v * nb + block] = sum of y eta - exp(eta) over the block's share of view v; backward: dF = gloss w_v
// (exp(eta) - y) / S, part untouched.  eta = F + log_offset[row] (nullptr: 0); w == nullptr: every view weighs 1; skip:
// a NaN in Y is left out (dF exactly 0)
int pois_loglik_launch(bool bwd, const float* F, const float* Y, const float* log_offset, int S, long long N, int P,
                       const ViewRows& vr, int V, int nb, const double* w, const float* gloss, int skip, float* dF,
                       double* part, hipStream_t st);
// lmc.hip: lmc_mfma_launch for a Poisson modality (lmc_mfma_pois_kernel)
int lmc_mfma_pois_launch(const float* F, const float* W, const float* Y, const float* log_offset, int skip, int S,
                         long long N, int L, int P, double* zpart, int nparts, float* dF, float* dWpart, int G,
                         hipStream_t st);

// lmc.hip: lmc_mfma_launch for a negative binomial modality (lmc_mfma_nb_kernel): upart [G][P] fp64, the workgroups'
// per-output sums of u
int lmc_mfma_nb_launch(const float* F, const float* W, const float* Y, const float* log_offset, const float* log_disp,
                       int skip, int S, long long N, int L, int P, double* zpart, int nparts, float* dF, float* dWpart,
                       double* upart, int G, hipStream_t st);

// negbin.hip: the negative binomial term's per-element kernel (loglik_nb_kernel<bwd>) as a column reduction: threads
// along p, the S * rows_v rows of view v in g.nrb row blocks, grid (g.gx, g.nrb, V).  forward: part[v * g.nb() + block]
// = the block's sum of t; backward: dF = gloss w_v ((y + r) sigma(a) - y) / S and upart[(v * g.nrb + row block) * P + p]
// = the row block's sum of u in column p.  nb_grid sizes both (at most 4096 block partials per term).
struct NbGrid {
  int gx, nrb, cw;  // column blocks, row blocks per view, columns per pass of a block (a power of two <= 64)
  int nb() const { return gx * nrb; }
};
NbGrid nb_grid(long long rows, int V, int P);
int nb_loglik_launch(bool bwd, const float* F, const float* Y, const float* log_offset, const float* log_disp, int S,
                     long long N, int P, const ViewRows& vr, int V, const NbGrid& g, const double* w, const float* gloss,
                     int skip, float* dF, double* part, double* upart, hipStream_t st);
// ddisp[p] = -gloss ( sum_v w_v sum_b upart[(v nrb + b) P + p] / S + dconst[p] )  (w == nullptr: weights of 1; a term
// that came as partial sums: V = nrb = 1, upart = its [P] sums of u)
int nb_ddisp_launch(const double* upart, int V, int nrb, int P, const double* w, int S, const double* dconst,
                    const float* gloss, float* ddisp, hipStream_t st);

// proj64.hip: alpha = Kinv X (fp64 matrix cores) as a persistent output-stationary kernel over pack_whiten_kernel's
// packed inverse(s); proj64_ok says which shapes it takes; q is closed by atomic adds onto
// zero: q_zeroed says an earlier launch on the stream has cleared it (else a memset node goes in front)
bool proj64_ok(int MB, long long C, int batch);
template <typename TI>
int proj64_launch(int MB, const double* Apk, const TI* X, int M, long long C, double* alpha, float* out32, double* q,
                  int batch, long long sX, hipStream_t st, bool q_zeroed);
// zero fill as a kernel of this library, not a runtime memset (elementwise.hip: a memset NODE of a replayed graph was
// seen to land behind the kernel that follows it); returns 0 or a hipError_t
int zero_fill_async(void* ptr, size_t bytes, hipStream_t st);
int copy_async(void* dst, const void* src, size_t bytes, hipStream_t st);  // device to device, as a kernel
// gpsa_elbo_fused_post as one launch (elementwise.hip): tick = a device word that is zero at entry
int elbo_fused_post_ticket(float* g_ext, float* dmeanT, float* abar, int M, long long C, int L, const float* gloss,
                           const float* var_u, double* dvar_u, double* part, int* tick, hipStream_t st);
// the same with the right-hand side K_uf[m, c] = k(Z_m, x_c) formed inside the kernel (round 6)
int proj64_gen_launch(int MB, const double* Apk, int kind, const float* Z, const double* X64, int D, const float* ls_u,
                      const float* var_u, int M, long long C, double* alpha, float* out32, double* q, hipStream_t st,
                      bool q_zeroed);

}  // namespace gpsa
