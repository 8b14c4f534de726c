/* gpsa_hip.h — C ABI of libgpsa_hip.so: hand-written HIP (gfx950 / MI355X) kernels for the
 * GPSA variational deep-GP forward / ELBO / backward hot path.
 *
 * Boundary contract
 *   - plain C: device pointers + sizes + a hipStream_t passed as void*; no torch types.
 *   - every entry point returns 0 on success or a (positive) hipError_t / negative GPSA_E* code;
 *     nothing allocates, frees or synchronises (safe for stream capture into a hipGraph);
 *     scratch memory is passed in by the caller (size from the matching *_workspace() query).
 *   - all matrices are dense row-major.  dtype: GPSA_F32 (float) or GPSA_F64 (double).
 *   - scalar kernel hyper-parameters are passed as DEVICE pointers (unconstrained = log values,
 *     as the reference stores them) so that no host<->device sync is ever needed.
 *
 * Each entry point cites the reference code (python, /root/reference) it replaces.  The reference
 * has no FFI of its own (pure PyTorch); the binding a maintainer would add is the ctypes stub shown
 * in INTEGRATION.md and implemented in spatial_alignment_amd/_lib.py.
 */
#ifndef GPSA_HIP_H
#define GPSA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

enum {
  GPSA_F32 = 0,
  GPSA_F64 = 1,
  GPSA_F32_X64 = 2,   /* gpsa_kmat in_dtype only: fp32 Z / hyper-parameters, fp64 X */
  GPSA_F32_OUT64 = 3, /* gpsa_kmat_bwd in_dtype only: fp32 inputs, fp64 gradients (with dtype = GPSA_F64) */
  GPSA_F32_ACC64 = 4  /* gpsa_kmat_bwd in_dtype only: fp32 inputs AND an fp32 Kbar, fp64 arithmetic / partial
                         sums / gradients (with dtype = GPSA_F64) */
};
enum { GPSA_K_RBF = 0, GPSA_K_MATERN12 = 1, GPSA_K_MATERN32 = 2 };
enum { GPSA_EINVAL = -1, GPSA_EWORKSPACE = -2, GPSA_EUNSUPPORTED = -3 };

/* library / build info */
int gpsa_version(void);               /* 100*major + minor */
const char* gpsa_build_arch(void);    /* "gfx950" */
const char* gpsa_source_hash(void);   /* "GPSA_SOURCE_HASH=<sha256 of csrc/ + this header at build time>": the host
                                         side refuses a library that was not built from the sources next to it */

/* ---- covariance ("kernel") matrices ---------------------------------------------------------
 * K[m,c] = k(Z[m,:], X[c,:]) (+ jitter on the diagonal m==c, used for K_uu).
 * replaces gpsa/util/util.py:8-23 (rbf_kernel), :33-47 (matern12_kernel), :50-66 (matern32_kernel)
 * as called from gpsa/models/vgpsa.py:314-318, 390-392, 409.
 * Z [M,D], X [C,D], K [M,C]; ls_u / var_u: device scalars (log lengthscale, log variance). D <= 4.
 * dtype = type K is computed and stored in; in_dtype = storage type of Z, X, ls_u, var_u (the fp32
 * parameters are read as they are).  Supported (dtype, in_dtype): (F32,F32), (F64,F64), (F64,F32) and
 * (F64, F32_X64): fp32 Z / hyper-parameters with an fp64 X - the data GP's k(Gtilde, G_samples) on the warp
 * GP's unrounded draws. */
int gpsa_kmat(int dtype, int in_dtype, int kind, const void* Z, int M, const void* X, long long C,
              int D, const void* ls_u, const void* var_u, double jitter, void* K, void* stream);

/* Backward of gpsa_kmat: given Kbar = dLoss/dK [M,C] (dtype) produce, in in_dtype,
 *   dZ [M,D], dX [C,D] (may be NULL), dparams[2] = {dLoss/d ls_u, dLoss/d var_u}.
 * same != 0: Z and X are the same points (K_uu, C == M): the X-side sums are added into dZ and dX is
 * not written.  (autograd of util.py:8-66 in the reference).  Deterministic: per-workgroup partial sums
 * (in dtype) in the workspace, then ONE second launch that adds them in a fixed order.
 * in_dtype = GPSA_F32_OUT64 (dtype GPSA_F64): fp32 inputs, dZ / dX / dparams stored as fp64 - the data GP's
 * backward, whose sigma^2 and coordinate gradients are differences of large terms; GPSA_F32_ACC64: the
 * same with Kbar itself stored as fp32 (the data GP's gradient panel). */
long long gpsa_kmat_bwd_workspace(int dtype, int M, long long C, int D);
int gpsa_kmat_bwd(int dtype, int in_dtype, int kind, const void* Z, int M, const void* X, long long C,
                  int D, const void* ls_u, const void* var_u, const void* Kbar, int same, void* dZ,
                  void* dX, void* dparams, void* workspace, long long workspace_bytes, void* stream);

/* ---- dense products ---------------------------------------------------------------------------
 * C[b] = alpha * op(A[b]) * op(B[b]) + beta * C[b];  op(A): m x k, op(B): k x n, row-major, strided batch.
 * splitk > 1 splits the k loop over workgroups (deterministic: partials in workspace, then summed).
 * replaces the torch.matmul / torch.mm calls of vgpsa.py:179-196, 207-210, 227, 302, 430. */
long long gpsa_gemm_workspace(int dtype, int m, int n, int batch, int splitk);
int gpsa_gemm(int dtype, int transA, int transB, int m, int n, long long k, double alpha,
              const void* A, long long lda, long long strideA, const void* B, long long ldb,
              long long strideB, double beta, void* C, long long ldc, long long strideC, int batch,
              int splitk, void* workspace, long long workspace_bytes, void* stream);

/* out[M,C] += A[M,L] B[L,C] (fp32, row-major, contiguous): a thin inner dimension under a long panel, in ONE pass
 * over the panel - the mean term's share of the data GP's projection gradient, autograd of vgpsa.py:192
 * (abar += delta_F dmean^T: M = 200, L = 50, C = 100k at the headline size).  GPSA_EUNSUPPORTED outside M <= 256,
 * L <= 64, C >= 4096 a multiple of 4, out 16-byte aligned: use gpsa_gemm with beta = 1. */
int gpsa_thin_update_f32(const float* A, int M, int L, const float* B, long long C, float* out, void* stream);

/* ---- variational covariances (vgpsa.py:206-210): Omega[b] = A[b] A[b]^T + jitter I ---------------
 * A [batch,M,M] is the fp32 parameter (Omega_sqt_*), read as stored; Omega [batch,M,M] fp64 (matrix
 * cores).  gpsa_omega_bwd is its adjoint: dA[b] = (G[b] + G[b]^T) A[b] with G = dLoss/dOmega (fp64);
 * symmetric != 0 promises G = G^T and computes 2 G A (no strided reads of G^T). */
int gpsa_omega_fwd(const float* A, int M, int batch, double jitter, double* Omega, void* stream);
int gpsa_omega_bwd(const double* G, const float* A, int M, int batch, int symmetric, float* dA,
                   void* stream);
/* The same over TWO parameter tensors in one launch (the warp GPs' Omega_sqt_G_list, vgpsa.py:131-143, and a
 * modality's Omega_sqt_F_dict entry, :145-153, which share M when m_X_per_view == m_G): segment 0 has n0
 * matrices, segment 1 n1 (0: absent). */
int gpsa_omega_fwd2(const float* A0, int n0, double* Omega0, const float* A1, int n1, double* Omega1, int M,
                    double jitter, void* stream);
int gpsa_omega_bwd2(const double* G0, const float* A0, float* dA0, int n0, const double* G1, const float* A1,
                    float* dA1, int n1, int M, int symmetric, void* stream);

/* ---- inducing-point factorisations (fp64, batched, one workgroup per matrix) -----------------
 * gpsa_chol_f64: in-place lower Cholesky of A[b] (upper triangle zeroed); logdet[b] = 2*sum(log diag);
 *   info[b] = 0 or (1 + index of the first non-positive pivot) — the reference raises
 *   torch.linalg.LinAlgError there (vgpsa.py:257, 320, 394, 412 torch.cholesky).
 * gpsa_tri_inv_f64: Linv[b] = inverse of the lower-triangular L[b] (replaces the triangular solves
 *   inside torch.cholesky_solve, vgpsa.py:177). */
int gpsa_chol_f64(void* A, int M, int batch, void* logdet, int* info, void* stream);
int gpsa_tri_inv_f64(const void* L, void* Linv, int M, int batch, void* stream);
/* gpsa_chol_inv_f64: Linv[b] = chol(A[b])^-1 with logdet / info as gpsa_chol_f64, in one register-
 *   resident sweep (A is not modified; M <= 256, GPSA_EUNSUPPORTED above: chain the two calls above).
 *   Same reference lines as the pair it fuses. */
int gpsa_chol_inv_f64(const void* A, void* Linv, int M, int batch, void* logdet, int* info,
                      void* stream);
/* gpsa_chol_inv_sel_f64: the same for a SELECTION of a batch in one launch (M <= 256): the matrices
 *   b < n_always and keep_lo <= b < keep_hi of A [batch,M,M]; results land at their own index b in Linv,
 *   logdet and info, the other entries are not touched.  A data-parallel rank that owns only a range of the
 *   KL terms of vgpsa.py:498-530 factorises the priors and ITS variational covariances (owner computes; the
 *   gradient all-reduce sums the shares) - still one launch, i.e. one matrix's latency. */
int gpsa_chol_inv_sel_f64(const void* A, void* Linv, int M, int batch, int n_always, int keep_lo, int keep_hi,
                          void* logdet, int* info, void* stream);
/* gpsa_chol_inv_blocked_f64: the same result for any M: right-looking over diagonal blocks of <= 256
 *   columns (register-resident kernel per block, fp64-MFMA products for the panel, the trailing update and
 *   the rows of the inverse).  workspace >= gpsa_chol_inv_blocked_workspace(M, batch) bytes. */
long long gpsa_chol_inv_blocked_workspace(int M, int batch);
int gpsa_chol_inv_blocked_f64(const void* A, void* Linv, int M, int batch, void* logdet, int* info,
                              void* workspace, long long workspace_bytes, void* stream);

/* ---- EXPERIMENT (not on the product path, never the timed step; csrc/split_bf16.hip) ------------------------------
 * The contraction W_l = Omega_l alpha of vgpsa.py:192-196 with every fp32 operand written as a sum of bf16 pieces and
 * the product as bf16 matrix instructions accumulated in fp32 (fp32 MFMA is 1/16 of the bf16 rate on gfx950):
 *   nprod 6: three pieces, the six products a_i b_j with i + j <= 4;  4: two pieces, four products;  3: two pieces
 *   without a2 b2;  1: plain bf16 operands;  0: the fp32 instruction on the same tiling (comparison).
 * Omega [L,M,M], alpha [M,C], W [L,M,C] fp32.  A plain kernel (operands from global memory): numerics, not speed.
 * gpsa_experiment_split_bf16_rate: the MFMA + LDS-fragment-read loop of the fused ELBO kernel's tile (13 x 2
 * accumulators, ``outputs`` outputs per workgroup, 256 workgroups) in fp32 (nprod 0) or split form (6 / 4 / 3); the
 * caller times it; out >= 65536 floats. */
int gpsa_experiment_split_bf16_product(const float* Omega, const float* alpha, int M, long long C, int L, int nprod,
                                       float* W, void* stream);
int gpsa_experiment_split_bf16_rate(int nprod, int outputs, float* out, void* stream);

/* ---- the dominant contraction: variational variance term --------------------------------------
 * v[l,c] = alpha[:,c]^T Omega[l] alpha[:,c]            (vgpsa.py:192-196 a_t_Omega_tril, square, sum;
 *                                                        Omega_tril Omega_tril^T == Omega exactly)
 * alpha [M,C], Omega [L,M,M] symmetric, v [L,C].  Never materialises the [S,L,N,M] tensor.
 * fp32 + M <= 256 runs on the MFMA (v_mfma_f32_16x16x4_f32) path; otherwise a tiled generic path.
 * omega_dtype: storage type of Omega (the fp64 Omega = A A^T + 1e-5 I is read as stored and rounded
 * to the compute type while it is packed for the matrix cores). */
long long gpsa_quadform_workspace(int dtype, int M, long long C, int L);
int gpsa_quadform_fwd(int dtype, int omega_dtype, const void* alpha, const void* Omega, int M,
                      long long C, int L, void* v, void* workspace, long long workspace_bytes,
                      void* stream);
/* dalpha[:,c] = 2 * sum_l g[l,c] * Omega[l] alpha[:,c]      (autograd of the above wrt alpha) */
int gpsa_quadform_bwd_alpha(int dtype, int omega_dtype, const void* alpha, const void* Omega,
                            const void* g, int M, long long C, int L, void* dalpha, void* workspace,
                            long long workspace_bytes, void* stream);
/* The same form for a layer with few outputs (the warp GP: L = D <= 3), keeping the products
 * W[l] = Omega[l] alpha ([L,M,C], dtype) it is made of, so that its backward is one streaming pass
 *   dalpha[:,c] = 2 * sum_l g[l,c] * W[l][:,c]
 * instead of L more M x M x C products.  Omega in dtype.  (vgpsa.py:192-196 and its autograd.)
 * dcT [M,L] / meanT [L,C] (both or neither NULL): the layer's mean term meanT[l,c] = sum_m dcT[m,l] alpha[m,c]
 * (vgpsa.py:182-184) in the same pass over alpha that closes the form. */
int gpsa_quadform_fwd_keep(int dtype, const void* alpha, const void* Omega, int M, long long C, int L,
                           void* v, void* W, const void* dcT, void* meanT, void* stream);
/* dcT [M,L] / dmeanT [L,C] (both or neither NULL): adds the mean term's share dcT dmeanT to dalpha. */
int gpsa_quadform_bwd_alpha_kept(int dtype, const void* W, const void* g, int M, long long C, int L,
                                 const void* dcT, const void* dmeanT, void* dalpha, void* stream);
/* The data GP's form (many outputs, fp32 matrix cores, M <= 256) with its products kept: v as gpsa_quadform_fwd
 * and, in the same pass, the products Omega[l] alpha themselves into W - an opaque buffer of
 * gpsa_quadform_keep_f32_bytes(M, C, L) bytes (about L M C 4) in the kernel's own accumulator order, so that each
 * wave stores 1 KiB contiguous.  Training's backward is then gpsa_quadform_bwd_alpha_kept_f32:
 *     dalpha[:,c] = 2 sum_l g[l,c] (Omega[l] alpha)[:,c]  ( + dcT dmeanT: the mean term's share, dcT [M,L] and
 *     dmeanT [L,C] both or neither NULL, as in gpsa_quadform_bwd_alpha_kept )
 * as ONE streaming read of W instead of the L M x M x C products of gpsa_quadform_bwd_alpha (vgpsa.py:192-196
 * and its autograd; the forward alone loses the symmetric half-price form: without a backward use
 * gpsa_quadform_fwd).  Omega [L,M,M] stored as omega_dtype.  workspace >= gpsa_quadform_keep_f32_workspace(M, L).
 * M <= 256: the register-resident full-product kernel; beyond (configs 4 / 5): one tiled product per output into
 * a row-major [L][M][C] buffer, streamed back by a row-blocked kernel - the same entry points, the same sizes
 * queries. */
long long gpsa_quadform_keep_f32_workspace(int M, int L);
long long gpsa_quadform_keep_f32_bytes(int M, long long C, int L);
int gpsa_quadform_fwd_keep_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                               float* v, float* W, void* workspace, long long workspace_bytes, void* stream);
int gpsa_quadform_bwd_alpha_kept_f32(const float* W, const float* g, int M, long long C, int L, const float* dcT,
                                     const float* dmeanT, float* dalpha, void* stream);
/* The data GP's forward, its Gaussian log-likelihood and the backward's abar in ONE pass over the products
 * Omega_l alpha (training with the engine's own ELBO: replaces gpsa_quadform_fwd_keep_f32 + gpsa_data_sample_fwd +
 * gpsa_loglik_fwd/_bwd + gpsa_data_sample_bwd + gpsa_quadform_bwd_alpha_kept_f32; reference vgpsa.py:186-204,
 * 334-351, 532-538 and their autograd adjoints).  Per (l, c), c = s*N + n:
 *   var = (exp(var_u) - q[c]) + alpha_c^T Omega_l alpha_c + 2e-5;  F = meanT[l,c] + sqrt(var) eps[c,l]
 *   z = (Y[n,l] - F) / s,  s = exp(noise_u) + 1e-5;   part[] sums z^2  (LL = -z^2/2 - log s - log(2 pi)/2 per element)
 *   dmeanT[l,c] = dLoss/dF = -(Y - F) / (s^2 S);   g[l,c] = dLoss/dvar = dmeanT * eps / (2 sqrt(var))
 *   abar[:,c]   = 2 sum_l g[l,c] Omega_l alpha_c                (the mean term's share is NOT included)
 * all at upstream gradient dLoss = 1 (linear in it).  part: gpsa_quadform_elbo_parts() doubles (unused tail zeroed).
 * FT (optional, NULL = not wanted): [L][C], the draws themselves, F[s][n][l] at FT[l][s N + n] - for a caller that
 * looks at them afterwards; nothing on the path reads them.
 * M <= 256 (16 row tiles; round 3: 208) only: GPSA_EUNSUPPORTED beyond. */
int gpsa_quadform_elbo_parts(void);
long long gpsa_quadform_elbo_f32_workspace(int M, long long C, int L);
int gpsa_quadform_elbo_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                           const float* meanT, const double* q, const float* var_u, const float* eps, const float* Y,
                           long long N, int S, const float* noise_u, float* g, float* dmeanT, float* abar, double* part,
                           float* FT, void* workspace, long long workspace_bytes, void* stream);
/* The same with the mean formed by the kernel itself: delta [M][L] (delta_F of vgpsa.py:194-196: mean = K_fu K_uu^-1
 * delta = delta^T alpha) is packed into the first padding row of every Omega_l, so that row M of the product
 * Omega_l alpha - MFMAs the padding of the last row tile executes anyway - is delta_l^T alpha_c; no [L,C] mean is read
 * and the caller's [L,M] x [M,C] product goes away.  Only when M is not a multiple of 16 and row M lies in the kernel's
 * last row tile (gpsa_quadform_elbo_takes_delta(M) != 0; M = 200: yes); GPSA_EUNSUPPORTED otherwise. */
int gpsa_quadform_elbo_takes_delta(int M);
int gpsa_quadform_elbo_delta_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                                 const float* delta, const double* q, const float* var_u, const float* eps,
                                 const float* Y, long long N, int S, const float* noise_u, float* g, float* dmeanT,
                                 float* abar, double* part, float* FT, void* workspace, long long workspace_bytes,
                                 void* stream);
/* The same two passes with the contraction Omega_l alpha on the bf16 matrix instructions: every fp32 operand split
 * into three bf16 pieces, the six products a_i b_j with i + j <= 4 accumulated in fp32 (as accurate as the fp32
 * instruction on the headline operands; the opt-in mode gpsa_step_desc.contraction = 1).  Same arguments, same
 * outputs, same GPSA_EUNSUPPORTED cases; their own workspace. */
long long gpsa_quadform_elbo_x3_f32_workspace(int M, long long C, int L);
int gpsa_quadform_elbo_x3_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                              const float* meanT, const double* q, const float* var_u, const float* eps, const float* Y,
                              long long N, int S, const float* noise_u, float* g, float* dmeanT, float* abar, double* part,
                              float* FT, void* workspace, long long workspace_bytes, void* stream);
int gpsa_quadform_elbo_delta_x3_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                                    const float* delta, const double* q, const float* var_u, const float* eps,
                                    const float* Y, long long N, int S, const float* noise_u, float* g, float* dmeanT,
                                    float* abar, double* part, float* FT, void* workspace, long long workspace_bytes,
                                    void* stream);
/* gpsa_quadform_elbo_f32 / _delta_f32 over partly observed outputs: Y[n,l] != Y[n,l] (a NaN) marks a missing entry,
 * which is left out - z = 0, dmeanT = 0 and g = 0 exactly there, nothing of it in abar or part (the count of observed
 * entries the loss needs: gpsa_count_observed).  fp32 contraction only; same arguments, sizes, workspace query
 * (gpsa_quadform_elbo_f32_workspace) and GPSA_EUNSUPPORTED cases.  Without a NaN in Y they compute what the plain entries
 * compute (their own kernels, panel_elbo_skip_kernel: equal to rounding, not necessarily bitwise). */
int gpsa_quadform_elbo_skip_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                                const float* meanT, const double* q, const float* var_u, const float* eps, const float* Y,
                                long long N, int S, const float* noise_u, float* g, float* dmeanT, float* abar,
                                double* part, float* FT, void* workspace, long long workspace_bytes, void* stream);
int gpsa_quadform_elbo_delta_skip_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                                      const float* delta, const double* q, const float* var_u, const float* eps,
                                      const float* Y, long long N, int S, const float* noise_u, float* g, float* dmeanT,
                                      float* abar, double* part, float* FT, void* workspace, long long workspace_bytes,
                                      void* stream);
/* dOmega[l] = sum_c g[l,c] * alpha[:,c] alpha[:,c]^T  (full symmetric [L,M,M]), stored as out_dtype
 * (out_dtype != dtype only on the fp32 MFMA path, whose partial sums are widened while they are added:
 * GPSA_EUNSUPPORTED otherwise, and the caller converts) */
int gpsa_quadform_bwd_omega(int dtype, int out_dtype, const void* alpha, const void* g, int M, long long C,
                            int L, void* dOmega, void* workspace, long long workspace_bytes, void* stream);
/* The same (fp32 operands, fp32 matrix cores) with the mean term's gradient riding along:
 *   ddelta[m,l] = dbeta * ddelta[m,l] + sum_c alpha[m,c] dmeanT[l,c]      (d delta_F of mean = delta^T alpha, [M][L])
 * comes out of row M of the padded dOmega_l tiles - the first padding row of the kernel's last row tile takes dmeanT[l,c]
 * as its scaled row fragment - so the caller's C-long [M,C] x [C,L] product goes away.  Workspace as
 * gpsa_quadform_workspace(GPSA_F32, M, C, L).  Only where gpsa_quadform_bwd_omega_takes_delta(M, C) != 0 (M not a
 * multiple of 16 and in the kernel's last row tile, M <= 256, C a multiple of 4, 16-byte aligned operands);
 * GPSA_EUNSUPPORTED otherwise. */
int gpsa_quadform_bwd_omega_takes_delta(int M, long long C);
int gpsa_quadform_bwd_omega_delta_f32(int out_dtype, const float* alpha, const float* g, const float* dmeanT, int M,
                                      long long C, int L, void* dOmega, float* ddelta, double dbeta, void* workspace,
                                      long long workspace_bytes, void* stream);
/* The two Gram calls above with the contraction on the bf16 matrix instructions: alpha split into three bf16 pieces
 * (an image written once per call), the g-scaled row fragment split in registers, six products a_i b_j with i + j <= 4
 * accumulated in fp32 (the opt-in mode gpsa_step_desc.contraction = 1).  M <= 256 and dtype GPSA_F32 only
 * (GPSA_EUNSUPPORTED otherwise: gpsa_quadform_bwd_omega_x3_workspace returns 0 there); the delta form where row M is a
 * padding row of the last tile row.  Deterministic: partials added in a fixed order. */
long long gpsa_quadform_bwd_omega_x3_workspace(int M, long long C, int L);
int gpsa_quadform_bwd_omega_x3(int dtype, int out_dtype, const void* alpha, const void* g, int M, long long C, int L,
                               void* dOmega, void* workspace, long long workspace_bytes, void* stream);
int gpsa_quadform_bwd_omega_delta_x3(int out_dtype, const float* alpha, const float* g, const float* dmeanT, int M,
                                     long long C, int L, void* dOmega, float* ddelta, double dbeta, void* workspace,
                                     long long workspace_bytes, void* stream);

/* alpha = Kinv Kuf on the fp64 matrix cores, with Kinv [M,M] = K_uu^-1 (fp64, from gpsa_chol_inv_f64 +
 * L^-T L^-1) and Kuf [M,C] stored as in_dtype (widened on the fly); alpha [M,C] is stored as alpha_dtype
 * (GPSA_F32 / GPSA_F64); q[c] = sum_m Kuf[m,c] alpha[m,c] (fp64, may be NULL).  These are the
 * K_fu K_uu^-1 factors of the conditional mean and covariance of both GP layers,
 * gpsa/models/vgpsa.py:179-183 and 194-196, and - applied to a gradient panel - the K_uu^-1 solve of
 * their backward.  M <= 256; GPSA_EUNSUPPORTED above (callers then chain gpsa_panel_mm).  workspace >=
 * gpsa_whiten_workspace(M) bytes; the call leaves the matrix-core layout of Kinv in it, and a later call with
 * Kinv == NULL on the same workspace reuses it (the backward's solve against the forward's inverse; the same
 * holds for gpsa_whiten_axpy_f32 and, per problem, gpsa_whiten_batched_f64). */
long long gpsa_whiten_workspace(int M);
int gpsa_whiten_f64(const double* Kinv, int in_dtype, const void* Kuf, int M, long long C,
                    int alpha_dtype, void* alpha, double* q, void* workspace, long long workspace_bytes,
                    void* stream);

/* Y = op(P) X with P [M,M] (stored as p_dtype, op = transpose when transP), X [M,C] and Y in dtype
 * (+ optional colsq[c] = sum_m Y[m,c]^2, may be NULL).
 * The whitening products beta = L^-1 K_uf, alpha = L^-T beta of vgpsa.py:177-180 and their adjoints.
 * workspace: fp32 with M <= 256 (the matrix-core kernel; MP = M rounded up to 32, 64, 112, 208 or 256 rows) takes
 * 4 MP (MP + 64) bytes - the packed operand and four 16-column chunks of slack that its staging ring requests and never
 * multiplies - and returns GPSA_EWORKSPACE below that; every other case takes a copy of P in dtype (M M elements,
 * rounded up to 256 bytes) when p_dtype != dtype and nothing else. */
int gpsa_panel_mm(int dtype, int p_dtype, int transP, const void* P, const void* X, int M, long long C,
                  void* Y, void* colsq, void* workspace, long long workspace_bytes, void* stream);

/* out[m,c] = Y[m,c] + s * d[c] * X[m,c]   (X, Y, out [M,C]; d [C]; out may alias Y).
 * Column-scaled update used by the whitening backward (autograd of vgpsa.py:177-180). */
int gpsa_col_axpy(int dtype, const void* Y, const void* X, const void* d, double s, int M,
                  long long C, void* out, void* stream);

/* ---- reparameterised sampling -----------------------------------------------------------------
 * data GP (vgpsa.py:197-204, 423-426):  var = (exp(var_u) - q[c])_fp64 + v[l,c] + 2e-5 ;
 *   F[c,l] = meanT[l,c] + sqrt(var) * eps[c,l] ;  Sigma[l,c] = var (kept for backward). */
int gpsa_data_sample_fwd(const float* meanT, const float* v, const double* q, const float* var_u,
                         const float* eps, long long C, int L, float* F, float* Sigma, void* stream);
/* given dF [C,L]:  g[l,c] = dF*eps/(2 sqrt(Sigma)),  dmeanT[l,c] = dF[c,l],  qbar[c] = -sum_l g,
 *   dvar_u (device scalar of type dvar_dtype - GPSA_F32 or GPSA_F64 -, overwritten) = exp(var_u) * sum g: the step
 *   engine takes it in fp64 - this share of the data kernel variance's gradient cancels against the covariance
 *   shares to ~1e-3 of its size near a stationary point, and its fp32 rounding alone then shows at 1e-4 of the sum
 *   (round 5).   workspace >= 8*(C/32+2) bytes */
int gpsa_data_sample_bwd(const float* dF, const float* eps, const float* Sigma, const float* var_u,
                         long long C, int L, float* g, float* dmeanT, float* qbar, int dvar_dtype, void* dvar_u,
                         void* workspace, long long workspace_bytes, void* stream);
/* warp GP (vgpsa.py:186-191, 334-351; variance used as the std), fp64 inside, with the
 * linear mean function of the view (vgpsa.py:283-289 mean_slopes / mean_intercepts) evaluated in place:
 *   var = exp(var_u) - q[c] + v[j,c] + 2e-5 ; Gmean[c,j] = (X[c,:] slopes)[j] + intercept[j] + meanT[j,c] ;
 *   Gs[s,c,j] = Gmean[c,j] + var * eps[s,c,j].
 * X [n,D], slopes [D,D], intercept [D], var_u: fp32 as stored.  bad[ceil(n/256)]: per-block flags, 1 if
 * any var <= 0 or NaN (the reference's Normal(...) argument validation raises ValueError there).
 * Gs64 [S,n,D] (may be NULL): the same draws before they are rounded to the fp32 API tensor; the data GP's
 * covariance k(Gtilde, G) (vgpsa.py:409) is evaluated on these, as the reference's fp64 run does. */
int gpsa_warp_sample_fwd(const double* meanT, const double* v, const double* q, const float* var_u,
                         const float* X, const float* slopes, const float* intercept,
                         const float* eps, long long n, int D, int S, float* Gmean, float* Gs,
                         double* Gs64, int* bad, void* stream);
/* given dGmean [n,D] (may be NULL) and dGs [S,n,D] as the sum of an fp32 part dGs and an fp64 part dGs64
 * (either may be NULL: the gradient wrt the fp32 API tensor and wrt its unrounded copy Gs64):
 *   dmeanT[j,c], g[j,c] = sum_s dGs*eps, qbar[c],
 *   dvar_u, dslopes [D,D], dintercept [D] (overwritten).  workspace >= 8*21*ceil(n/256) bytes */
int gpsa_warp_sample_bwd(const float* dGmean, const float* dGs, const double* dGs64, const float* eps,
                         const float* var_u, const float* X, long long n, int D, int S, double* dmeanT, double* g,
                         double* qbar, float* dvar_u, float* dslopes, float* dintercept,
                         void* workspace, long long workspace_bytes, void* stream);

/* linear mean function at the inducing points and the variational residual (vgpsa.py:283-289, 296):
 *   mu_z = scale * (Z slopes + intercept)  [M,D] fp32 ;  resid = delta - mu_z  [M,D] fp64
 * (scale = 100 reproduces the reference's inert x100 on a fixed view) and its adjoint:
 * given dresid: ddelta = dresid, dZ, dslopes, dintercept (all overwritten, fp32). */
int gpsa_mean_resid_fwd(const float* Z, const float* slopes, const float* intercept,
                        const float* delta, int M, int D, double scale, float* mu_z, double* resid,
                        void* stream);
int gpsa_mean_resid_bwd(const double* dresid, const float* Z, const float* slopes, int M, int D,
                        double scale, float* ddelta, float* dZ, float* dslopes, float* dintercept,
                        void* stream);

/* ---- Gaussian likelihood (vgpsa.py:532-538; "variance" used as std) -----------
 * scale = exp(noise_u[0]) + 1e-5 ;  out[0] = sum_{s,n,p} log N(Y[n,p]; F[s,n,p], scale) / S.
 * workspace >= 8*(blocks+2) bytes with blocks = min(4096, ceil(S*N*P/1024)). */
int gpsa_loglik_fwd(const float* F, const float* Y, const float* noise_u, int S, long long N, int P,
                    double* out, void* workspace, long long workspace_bytes, void* stream);
/* dF = gout[0] * dLL/dF ; dnoise_u[0] = gout[0] * dLL/d noise_u  (gout: device scalar, double) */
int gpsa_loglik_bwd(const float* F, const float* Y, const float* noise_u, const double* gout, int S,
                    long long N, int P, float* dF, float* dnoise_u, void* workspace,
                    long long workspace_bytes, void* stream);

/* ---- small helpers used by the KL terms (vgpsa.py:498-530) -------------------------------------
 * out[b] = sum_i A[b,i]*B[b,i] (strideA/strideB in elements; 0 broadcasts) */
int gpsa_bdot(int dtype, const void* A, long long strideA, const void* B, long long strideB,
              long long n, int batch, void* out, void* workspace, long long workspace_bytes,
              void* stream);  /* workspace >= 8*min(32, ceil(n/2048))*batch bytes (GPSA_EWORKSPACE below that;
                                 8*32*batch is enough for every n) */
/* A[b] += s * I  (A [batch,M,M]) */
int gpsa_add_diag(int dtype, void* A, int M, int batch, double s, void* stream);

/* ---- KL terms (vgpsa.py:498-530: kl_divergence(MVN(delta_l, Omega_tril_l), MVN(mu_l, Kuu_chol))), fp64 --------
 * kl[l] = 0.5 (logdet K - logdet Omega_l + <K^-1, Omega_l> + d_l^T KD_l - M),  d = delta - mu  [M,L],
 * KD = K^-1 d [M,L] (from gpsa_gemm).  omega_stride / logdet_stride: elements between consecutive l. */
int gpsa_mvn_kl_fwd(const double* Kinv, const double* logdetK, const double* Omega,
                    long long omega_stride, const double* logdetO, long long logdet_stride,
                    const double* Dm, const double* KD, int M, int L, double* kl, void* stream);
/* backward for upstream g[l]:  dOmega[l] = 0.5 g_l (K^-1 - Omega_l^-1) [L,M,M];  dDm = KD diag(g) [M,L];
 * Sp = (sum g) K - sum_l g_l (Omega_l + d_l d_l^T)  [M,M], so that dLoss/dK = 0.5 K^-1 Sp K^-1. */
int gpsa_mvn_kl_bwd(const double* Kuu, const double* Kinv, const double* Omega, long long omega_stride,
                    const double* Oinv, long long oinv_stride, const double* Dm, const double* KD,
                    const double* g, int M, int L, double* dOmega, double* dDm, double* Sp,
                    void* stream);

/* Grouped form: all T KL terms of a step in one launch each way.  The step's matrices live in ONE
 * batch mats [B,M,M] with inverses inv [B,M,M] and logdet [B] (gpsa_chol_inv_f64 + L^-T L^-1): term t
 * pairs the variational covariance mats[om_idx[t]] with the prior mats[pr_idx[t]] (pr_idx[t] < 0: the
 * term is absent - a fixed view - and contributes kl = 0 and zero gradients); D [T,M] holds d_t.
 * fwd: kl [T], KD [T,M] = K_p^-1 d_t (kept for the backward).
 * bwd: the terms are listed per prior: order[grp_off[pg] .. grp_off[pg+1]) are the terms of prior
 *   pr_list[pg], pg < P; group P lists the absent terms.  Writes dOmega [T,M,M], dD [T,M] and
 *   S [P,M,M] with dLoss/dK_p = 0.5 K_p^-1 S_p K_p^-1 (two batched gpsa_gemm calls by the caller). */
int gpsa_mvn_kl_grouped_fwd(const double* mats, const double* inv, const double* logdet,
                            const int* om_idx, const int* pr_idx, const double* D, int M, int T,
                            double* kl, double* KD, void* stream);
int gpsa_mvn_kl_grouped_bwd(const double* mats, const double* inv, const int* om_idx,
                            const int* pr_list, const int* grp_off, const int* order, const double* D,
                            const double* KD, const double* g, int M, int T, int P, double* dOmega,
                            double* dD, double* S, void* stream);

/* ---- ELBO scalar glue (vgpsa.py:540): loss = -(sum_i ll[i]) + kl_scale * sum_t kl[t] ---------------
 * ll [n_ll], kl [n_kl] fp64 device arrays (the per-modality log-likelihoods and the per-term KLs),
 * loss [1] fp32; gpsa_elbo_bwd is the adjoint: dll[i] = -gloss, dkl[t] = kl_scale * gloss. */
int gpsa_elbo_fwd(const double* ll, int n_ll, const double* kl, int n_kl, double kl_scale, float* loss,
                  void* stream);
int gpsa_elbo_bwd(const float* gloss, int n_ll, int n_kl, double kl_scale, double* dll, double* dkl,
                  void* stream);

/* ---- inducing-point initialisation: Lloyd's k-means on the device ----------
 * replaces sklearn.cluster.KMeans at gpsa/models/vgpsa.py:74-76, 90-92.  X [N,D] fp32, centres [K,D].
 * gpsa_kmeans_assign: assign[n] = nearest centre (ties -> lowest index), d2[n] (may be NULL) its
 *   squared distance.   gpsa_kmeans_update: centres[k] = mean of its points (empty cluster: unchanged),
 *   counts[k] (may be NULL).  Deterministic (no atomics). */
long long gpsa_kmeans_workspace(long long N, int D, int K);
int gpsa_kmeans_assign(const float* X, long long N, int D, const float* centres, int K, int* assign,
                       float* d2, void* stream);
int gpsa_kmeans_update(const float* X, const int* assign, long long N, int D, int K, float* centres,
                       int* counts, void* workspace, long long workspace_bytes, void* stream);


/* ---- batched forms: the warp GPs of several views in one launch each way -------------------------------
 * View-blocked layout: the per-view panels of a batch are [M, C] blocks back to back (C = the batch's
 * column stride, >= every view's spot count); problem b has n_live[b] live columns, the rest are zero
 * padding written by the forward (everything computed from a zero column is zero).  fp32 inputs as stored
 * (inducing points, hyper-parameters, coordinates), fp64 arithmetic and results.
 * gpsa_kmat_batched: K[b] = k(Z + b strideZ, X + b strideX) (+ jitter on the diagonal), ls_u / var_u + b
 *   stride_par; n_live (HOST array of batch entries) may be NULL (all C columns live).  batch <= 16.
 * gpsa_kmat_bwd_batched: its adjoint: dZ + b stride_dZ [M,D] and dparams + 2 b (fp64); same != 0: X are the
 *   inducing points themselves (K_uu), the X-side sums are folded into dZ.
 * References as gpsa_kmat / gpsa_kmat_bwd (util.py:8-66 called from vgpsa.py:314-318 for every view). */
int gpsa_kmat_batched(int kind, const float* Z, long long strideZ, int M, const float* X, long long strideX,
                      long long C, int D, const float* ls_u, const float* var_u, int stride_par,
                      const long long* n_live, int batch, double jitter, double* K, long long strideK,
                      void* stream);
long long gpsa_kmat_bwd_batched_workspace(int M, long long C, int D, int batch);
int gpsa_kmat_bwd_batched(int kind, const float* Z, long long strideZ, int M, const float* X, long long strideX,
                          long long C, int D, const float* ls_u, const float* var_u, int stride_par,
                          const long long* n_live, int batch, const double* Kbar, long long strideK, int same,
                          double* dZ, long long stride_dZ, double* dparams, void* workspace,
                          long long workspace_bytes, void* stream);
/* The data GP's covariance backward (autograd of vgpsa.py:409): fp32 Z / hyper-parameters, X = the warp
 * GP's unrounded fp64 draws, an fp32 gradient panel Kbar [M,C]; fp64 arithmetic, partial sums and results
 * (dZ [M,D], dX [C,D] or NULL, dparams[2]).  workspace >= gpsa_kmat_bwd_workspace(GPSA_F64, M, C, D). */
int gpsa_kmat_bwd_x64(int kind, const float* Z, int M, const double* X, long long C, int D, const float* ls_u,
                      const float* var_u, const float* Kbar, double* dZ, double* dX, double* dparams,
                      void* workspace, long long workspace_bytes, void* stream);
/* ... with an fp64 gradient panel (the exact inducing-point gradient of the data GP: gpsa_step_desc.exact_inducing_grad) */
int gpsa_kmat_bwd_x64_f64(int kind, const float* Z, int M, const double* X, long long C, int D, const float* ls_u,
                          const float* var_u, const double* Kbar, double* dZ, double* dX, double* dparams,
                          void* workspace, long long workspace_bytes, void* stream);
/* ... the fp64 panel in two pieces, Kbar[m,c] + s * d[c] * X2[m,c] (X2 [M,C] fp64, d [C] fp32; both NULL: Kbar
 * alone): the exact mode's dK_uf = K^-1 abar + 2 qbar o alpha on the unrounded projection, formed as it is read */
int gpsa_kmat_bwd_x64_f64_axpy(int kind, const float* Z, int M, const double* X, long long C, int D, const float* ls_u,
                               const float* var_u, const double* Kbar, const double* X2, const float* d, double s,
                               double* dZ, double* dX, double* dparams, void* workspace, long long workspace_bytes,
                               void* stream);
/* C += -(G + d o A) A^T: the exact mode's dK_uu = -(K^-1 abar + qbar o alpha) alpha^T (autograd of vgpsa.py:177-180
 * through K_uu) as ONE C-long fp64 product whose left operand is formed from its two panels as it is staged.
 * G, A [M, C] fp64, d [C] fp32, dK [M, M] fp64 (added to); workspace >= gpsa_exact_dkuu_workspace(M, C) bytes. */
long long gpsa_exact_dkuu_workspace(int M, long long C);
int gpsa_exact_dkuu_f64(const double* G, const double* A, const float* d, int M, long long C, double* dK,
                        void* workspace, long long workspace_bytes, void* stream);
/* Long-K fp64 products with a small square result, nprob of them in one launch (csrc/longk64.hip):
 *     out[p] [M, M] = beta[p] out[p] + alpha[p] * sum_k (G[p][:, k] + d[p][k] B[p][:, k]) B[p][:, k]^T
 * G[p], B[p]: [M, K] row-major fp64 panels with leading dimension ld (G == NULL: the left operand is d o B alone);
 * d[p]: [K] of type d_dtype (GPSA_F32 / GPSA_F64; d == NULL: the left operand is G alone); sym != 0: the caller
 * guarantees a symmetric result (the lower triangle is computed and mirrored).  The step's products of this shape:
 * the warp GPs' dOmega_j = sum_c g_j alpha alpha^T and dK_uu = -(gamma + qbar o alpha) alpha^T, and the exact
 * inducing-point gradient's dK_uu of the data GP (autograd of vgpsa.py:177-196 through K_uu and Omega).  alpha, beta,
 * and the pointer arrays are HOST arrays of nprob entries.  gpsa_longk_f64_workspace == 0 / GPSA_EUNSUPPORTED: the
 * shape is not covered (M > 256, odd or short K, unaligned panels) - use gpsa_gemm. */
long long gpsa_longk_f64_workspace(int M, long long K, int nprob);
int gpsa_longk_f64(int nprob, const double* const* G, const double* const* B, const void* const* d, int d_dtype,
                   int M, long long K, long long ld, int sym, const double* alpha, const double* beta,
                   double* const* out, void* workspace, long long workspace_bytes, void* stream);
/* ... with the gradient panel in two pieces, Kbar[m,c] + s * d[c] * X2[m,c] (X2 [M,C], d [C] fp32; both NULL: Kbar
 * alone): the data GP's dK_uf = K^-1 abar + 2 qbar o alpha (autograd of vgpsa.py:177-196) formed as it is read */
int gpsa_kmat_bwd_x64_axpy(int kind, const float* Z, int M, const double* X, long long C, int D, const float* ls_u,
                           const float* var_u, const float* Kbar, const float* X2, const float* d, double s,
                           double* dZ, double* dX, double* dparams, void* workspace, long long workspace_bytes,
                           void* stream);
/* gpsa_whiten_f64 on an fp64 panel with the result stored twice from the same accumulators: unrounded (alpha64) and
 * rounded to fp32 (alpha32: what the matrix-core contractions read) - the exact inducing-point gradient of the data
 * GP keeps both (gpsa_step_desc.exact_inducing_grad; autograd of vgpsa.py:177-180, 409) */
int gpsa_whiten_f64_dual(const double* Kinv, const double* Kuf, int M, long long C, double* alpha64, float* alpha32,
                         double* q, void* workspace, long long workspace_bytes, void* stream);

/* gpsa_whiten_f64_dual with K_uf[m, c] = k(Z_m, x_c) formed inside the projection kernel (Z [M,D] fp32, X64 [C,D]
 * fp64, log-parameters fp32: what gpsa_kmat(GPSA_F64, GPSA_F32_X64, ...) evaluates) - vgpsa.py:171-189 in one pass,
 * no K_uf in memory.  GPSA_EUNSUPPORTED for shapes the persistent kernel does not take (the caller then runs
 * gpsa_kmat + gpsa_whiten_f64_dual). */
int gpsa_whiten_gen_f64_dual(const double* Kinv, int kind, const float* Z, const double* X64, int D, const float* ls_u,
                             const float* var_u, int M, long long C, double* alpha64, float* alpha32, double* q,
                             void* workspace, long long workspace_bytes, void* stream);
/* gpsa_whiten_f64 on an fp32 panel with gpsa_col_axpy fused into its store:
 *   out[m,c] = (Kinv X)[m,c] + s * d[c] * X2[m,c]      (X, X2, out [M,C] fp32; d [C] fp32; fp64 arithmetic)
 * the data GP's dK_uf = K^-1 abar + 2 qbar o alpha (autograd of vgpsa.py:177-196) in one pass. */
int gpsa_whiten_axpy_f32(const double* Kinv, const float* X, int M, long long C, const float* X2, const float* d,
                         double s, float* out, void* workspace, long long workspace_bytes, void* stream);
/* gpsa_whiten_f64 for a batch of fp64 panels with one inverse each: problem b reads Kinv + b strideKinv and
 * Kuf + b strideX, writes alpha + b strideX and q + b C (q may be NULL).
 * workspace >= batch * gpsa_whiten_workspace(M). */
int gpsa_whiten_batched_f64(const double* Kinv, long long strideKinv, const double* Kuf, int M, long long C,
                            long long strideX, double* alpha, double* q, int batch, void* workspace,
                            long long workspace_bytes, void* stream);
/* gpsa_quadform_fwd_keep / _bwd_alpha_kept / gpsa_col_axpy (fp64) for ``batch`` layers with contiguous
 * operands: alpha [batch][M,C], Omega [batch][L,M,M], W [batch][L,M,C], v / meanT / g / dmeanT [batch][L,C],
 * dcT [batch][M,L], d [batch][C]. */
int gpsa_quadform_fwd_keep_batched_f64(const double* alpha, const double* Omega, int M, long long C, int L,
                                       double* v, double* W, const double* dcT, double* meanT, int batch,
                                       void* stream);
int gpsa_quadform_bwd_alpha_kept_batched_f64(const double* W, const double* g, int M, long long C, int L,
                                             const double* dcT, const double* dmeanT, double* dalpha,
                                             int batch, void* stream);
int gpsa_col_axpy_batched_f64(const double* Y, const double* X, const double* d, double s, int M, long long C,
                              double* out, int batch, void* stream);
/* dOmega[b][l] = sum_c g[b][l,c] alpha[b][:,c] alpha[b][:,c]^T (fp64, ``batch`` layers with contiguous
 * operands; gpsa_quadform_bwd_omega for the views' warp GPs in one launch sequence). */
long long gpsa_gram_batched_workspace(int M, long long C, int L, int batch);
int gpsa_gram_batched_f64(const double* alpha, const double* g, int M, long long C, int L, double* dOmega,
                          int batch, void* workspace, long long workspace_bytes, void* stream);
/* gpsa_mvn_kl_grouped_bwd with accumulate != 0: dOmega += ... (it already holds the layers' share). */
int gpsa_mvn_kl_grouped_bwd_acc(const double* mats, const double* inv, const int* om_idx,
                                const int* pr_list, const int* grp_off, const int* order, const double* D,
                                const double* KD, const double* g, int M, int T, int P, double* dOmega,
                                double* dD, double* S, int accumulate, void* stream);
/* gpsa_mvn_kl_grouped_fwd as the step launches it: a term's rows dealt to gpsa_mvn_kl_grouped_fwd_slices(M)
 * workgroups (1 up to M = 64, then ceil(M / 64), at most 8) whose partial sums the last one to arrive adds in a
 * fixed order.  part [T][slices] doubles (any contents), cnt [T] ints ZEROED by the caller and zero again afterwards;
 * both NULL (or either): one workgroup per term.  kl_copy [T] or NULL: a second copy of kl.  GPSA_EINVAL on a NULL
 * among the other pointers. */
int gpsa_mvn_kl_grouped_fwd_slices(int M);
int gpsa_mvn_kl_grouped_fwd_sliced(const double* mats, const double* inv, const double* logdet, const int* om_idx,
                                   const int* pr_idx, const double* D, int M, int T, double* kl, double* KD,
                                   double* kl_copy, double* part, int* cnt, void* stream);

/* ==== the step engine: forward(S) and its backward as ONE host call each =================================
 * Replaces the body of VariationalGPSA.forward (gpsa/models/vgpsa.py:212-489) plus the KL terms of loss_fn
 * (vgpsa.py:498-530), and what autograd derives from them, for the built-in covariance functions: the host
 * enqueues the whole launch sequence of a step from C++ (no per-launch Python / ctypes round trip), the
 * warp GPs of all free views run batched in the same launches, every parameter gradient is accumulated in
 * fp64 along all of its paths and rounded to the fp32 parameter once.
 *
 * A plan (gpsa_step_create) fixes the problem's shape; it owns only host tables and a few hundred bytes of
 * device index tables (allocated at creation - the ONLY allocation of the library; the hot entry points
 * below allocate nothing, never synchronise, and are safe to capture into a hipGraph).  The caller passes
 * two arenas per call: ``saved`` (gpsa_step_saved_bytes: what the backward needs from the forward; one per
 * live forward) and ``scratch`` (gpsa_step_scratch_bytes: transient, reusable by the next call on the same
 * stream).
 *
 * Views are consecutive row blocks of each modality (what GPSA.create_view_idx_dict produces,
 * gpsa/models/gpsa.py:155-183); spots of all modalities of a view share that view's warp GP
 * (vgpsa.py:284-294).  All parameters are the fp32 tensors of the reference's state_dict. */
#define GPSA_MAX_MODS 4

typedef struct gpsa_step_desc {
  int n_views, n_dims, n_mods, n_samples;   /* V, D (<= 4), modalities (<= GPSA_MAX_MODS), S */
  int m_x, m_g;                             /* inducing points per view / of the data GP */
  int kind_warp, kind_data;                 /* GPSA_K_* */
  int n_latent[GPSA_MAX_MODS];              /* L_m: latent outputs of the data GP (= P_m without LMC) */
  int n_out[GPSA_MAX_MODS];                 /* P_m */
  int has_lmc[GPSA_MAX_MODS];               /* F_obs = F_latent W (vgpsa.py:428-432) */
  long long n_rows[GPSA_MAX_MODS];          /* N_m */
  int s_test;                               /* leading dim of G_test, 0: no test pass (vgpsa.py:437-477) */
  long long n_test[GPSA_MAX_MODS];          /* rows of G_test[m] */
  int want_kl;                              /* factorise the variational covariances and evaluate the KL terms */
  const int* view_fixed;                    /* HOST [V]: 1 = fixed view (vgpsa.py:262-273) */
  const long long* view_rows;               /* HOST [n_mods * V]: rows of view v in modality m, [m * V + v] */
  long long keep_budget_bytes;              /* HBM a training forward may spend on the data GPs' kept products
                                               Omega_l alpha (L_m m_g C floats per pass): > 0 that many bytes; < 0
                                               never keep; 0: GPSA_KEEP_GB (default 48) GiB, and no more than 60 % of
                                               the device memory free at gpsa_step_create */
  int exact_inducing_grad;                  /* 1: the data GP's gradient wrt its inducing points Gtilde from the UNROUNDED
                                               projection: alpha = K^-1 K_uf kept in fp64 for the backward, gamma =
                                               K^-1 abar stored in fp64, dK_uu = -(gamma + qbar alpha) alpha^T as one
                                               C-long fp64 product.  The K_uu and K_uf shares of that gradient cancel to
                                               1e-4 .. 1e-5 of their size, so fp32 roundings of alpha / gamma are 1e-3 of
                                               the result at M >= 200.  +8 M C bytes, one M x M x C fp64 product */
  int kl_own_lo, kl_own_hi;                 /* data-parallel ranks, OWNER COMPUTES: this plan evaluates only the KL terms
                                               kl_own_lo <= t < kl_own_hi of the V*D + sum L_m terms (order: Omega_G rows
                                               r = j*V+v, then every modality's outputs; vgpsa.py:498-530) - the other
                                               terms come out as 0 with zero gradients and their variational covariances
                                               are neither factorised nor inverted.  kl_own_hi <= 0: every term (one
                                               process, or the 1/world weighting).  Summed over ranks whose ranges
                                               partition the terms, loss and gradients are the full ELBO's. */
  int contraction;                          /* the data GPs' fused ELBO pass: 0 = fp32 matrix instructions; 1 = bf16x3
                                               (gpsa_quadform_elbo_x3_f32: every operand in three bf16 pieces); any
                                               other value is refused.  LMC modalities, M > 256 and every other kernel
                                               are unaffected: gpsa_step_contraction says what runs */
} gpsa_step_desc;

typedef struct gpsa_step_params {           /* device pointers, fp32, the reference's parameter layout */
  const float* Xtilde;                      /* [V, m_x, D] */
  const float* delta_G;                     /* [V, m_x, D] */
  const float* Omega_sqt_G;                 /* [V*D, m_x, m_x], row j*V+v (vgpsa.py:131-143) */
  const float* warp_ls;                     /* [V] log lengthscales */
  const float* warp_var;                    /* [V] log variances */
  const float* slopes;                      /* [V, D, D] */
  const float* intercepts;                  /* [V, D] */
  const float* Gtilde;                      /* [m_g, D] */
  const float* data_ls;                     /* [1] */
  const float* data_var;                    /* [1] */
  const float* Omega_sqt_F[GPSA_MAX_MODS];  /* [L_m, m_g, m_g] */
  const float* delta_F[GPSA_MAX_MODS];      /* [m_g, L_m] */
  const float* W[GPSA_MAX_MODS];            /* [L_m, P_m] or NULL */
} gpsa_step_params;

typedef struct gpsa_step_param_grads {      /* fp32 outputs, overwritten; NULL = not wanted */
  float *Xtilde, *delta_G, *Omega_sqt_G, *warp_ls, *warp_var, *Gtilde, *data_ls, *data_var;
  float* Omega_sqt_F[GPSA_MAX_MODS];
  float* delta_F[GPSA_MAX_MODS];
  float* W[GPSA_MAX_MODS];
} gpsa_step_param_grads;

typedef struct gpsa_step_io {
  const float* X[GPSA_MAX_MODS];            /* in  [N_m, D] spatial coordinates */
  const float* eps_G;                       /* in  standard-normal draws of the free, non-empty views back to
                                                   back, each [S, n_v, D] (order of vgpsa.py:346-348) */
  const float* eps_F[GPSA_MAX_MODS];        /* in  [S, N_m, L_m] (vgpsa.py:423) */
  const float* G_test[GPSA_MAX_MODS];       /* in  [s_test, n_test_m, D] or NULL */
  const float* eps_F_test[GPSA_MAX_MODS];   /* in  [s_test, n_test_m, L_m] */
  float* G_means[GPSA_MAX_MODS];            /* out [N_m, D] */
  float* G_samples[GPSA_MAX_MODS];          /* out [S, N_m, D] */
  float* F_latent[GPSA_MAX_MODS];           /* out [S, N_m, L_m] */
  float* F_obs[GPSA_MAX_MODS];              /* out [S, N_m, P_m] with LMC, else NULL (F_obs is F_latent) */
  float* F_latent_test[GPSA_MAX_MODS];      /* out [s_test, n_test_m, L_m] */
  float* F_obs_test[GPSA_MAX_MODS];
  float* mu_z;                              /* out [V, m_x, D]: prior means at the inducing points (mu_z_G) */
  double* kl;                               /* out [gpsa_step_n_kl] per-term KL (order: Omega_G rows r = j*V+v,
                                                   then every modality's outputs), NULL with want_kl = 0 */
  int* flag;                                /* out [1]: nonzero = a covariance was not positive definite or a
                                                   warp variance not positive (the reference raises there) */
  int keep_products;                        /* in  nonzero (training): the data GPs' forward keeps its products
                                                   Omega_l alpha in the saved arena (gpsa_quadform_fwd_keep_f32)
                                                   and gpsa_step_backward streams them back; needs the arena of
                                                   gpsa_step_saved_bytes.  0 (no backward to follow): the cheaper
                                                   forward, gpsa_step_saved_bytes_nokeep suffices, and a backward
                                                   recomputes the products.  Pass the same value to both calls. */
  int reuse_mm;                             /* in  nonzero: the saved arena still holds the M x M stage (prior and
                                                   variational covariances, their factorisations and inverses, KL terms)
                                                   of an earlier gpsa_step_forward on the SAME parameters - skip it.
                                                   For the slices of one microbatched step (train.Microbatches) */
  /* Fused ELBO (training through the engine's own loss, Gaussian likelihood on F_latent, no LMC): with fuse_elbo
   * nonzero and Y[m] / noise_u[m] given, modality m's data GP runs gpsa_quadform_elbo_f32 - F_latent[m] is not
   * written (the draws leave only through the optional F_fused_T[m]), ll_part[m] receives the partial sums of z^2 for
   * gpsa_elbo_loss_fused_fwd / _bwd, and gpsa_step_backward takes the loss's upstream gradient from
   * gpsa_step_out_grads.gloss instead of dF_latent[m].  Modalities the fused kernel does not cover (LMC, more than
   * 256 inducing points: gpsa_step_fused(plan, m) == 0) run unfused and must be given F_latent[m] as usual. */
  int fuse_elbo;
  const float* Y[GPSA_MAX_MODS];            /* in  [N_m, L_m] observations */
  const float* noise_u[GPSA_MAX_MODS];      /* in  [1] the likelihood's log "variance" of modality m */
  double* ll_part[GPSA_MAX_MODS];           /* out [gpsa_quadform_elbo_parts()] */
  float* F_fused_T[GPSA_MAX_MODS];          /* out, optional: [L_m][S N_m] the draws of a fused modality, F[s][n][l] at
                                                   [l][s N_m + n] (gpsa_quadform_elbo_f32's FT) */
  /* One optimiser step as several forward / backward passes over row slices (train.Microbatches) that CLOSE once:
   * bwd_acc = gpsa_step_bwd_acc_bytes(plan) bytes the caller keeps across the slices' gpsa_step_backward calls;
   * bwd_acc_mode 1: first slice (its N-scaled gradient pieces are stored there, nothing else is done: ``grads`` is not
   * written), 2: a middle slice (added), 3: the last slice (the accumulator is added to its own pieces, then the M x M
   * closing - KL backward, prior covariances' backward, dOmega -> dA, finalisation - runs once and ``grads`` is written),
   * 0: an ordinary backward.  The KL terms' gradient og->dkl belongs to the LAST slice's call. */
  double* bwd_acc;
  int bwd_acc_mode;
  /* Data-parallel overlap (round 5; parallel.GradAllReducer(overlap=True)): with f_event (a hipEvent_t) given,
   * gpsa_step_backward finishes the DATA GP's span of the gradients first - Omega_sqt_F, delta_F, W: 97 % of the bytes
   * at the headline configuration - and records the event on the caller's stream behind it, so that the caller can
   * start reducing that span on another stream while the warp GPs' backward, the priors' covariance backward and the
   * rest run.  The KL backward then runs in front of the warp GPs' backward, whose products are added to its shares
   * instead of overwriting them: the fp64 sums meet in another order (results equal to rounding, not bitwise).  The
   * event is recorded at the very end when the early order is not available (a microbatched step, the side stream, a
   * shape the long-K kernel does not cover).  NULL: the ordinary order. */
  void* f_event;
  /* Data-parallel loss slot (parallel.GradAllReducer(with_loss=True)): with both given, the backward's closing kernel
   * (the finalisation of the small gradients) copies the fp32 scalar *loss_src to *loss_dst - a float in the spare room
   * behind the caller's gradients, so that the gradient all-reduce sums the ranks' partial losses with no launch and no
   * collective of its own.  *loss_src must be final when gpsa_step_backward is enqueued (the loss is written by the
   * ELBO launches in front of it on the same stream).  Either NULL: nothing is written.  Only a backward that closes
   * (bwd_acc_mode 0 or 3) writes it. */
  const float* loss_src;
  float* loss_dst;
  /* Partly observed outputs (model.skip_missing): nonzero = a NaN in Y[m] is a missing observation, and the fused ELBO
   * pass runs gpsa_quadform_elbo_skip_f32 / _delta_skip_f32 (ll_part then goes to gpsa_elbo_loss_skip_fwd / _bwd with the
   * counts of gpsa_count_observed).  Also in a bf16x3 plan: there is no x3 skip closing, the pass runs the fp32 skip
   * kernel (the Gram stays on x3) and gpsa_step_contraction reports it.  0 (a zero-initialised io): today's kernels. */
  int skip_missing;
} gpsa_step_io;

typedef struct gpsa_step_out_grads {        /* gradients of the caller's scalar wrt the forward's outputs */
  const float* dG_means[GPSA_MAX_MODS];     /* each may be NULL (= zero) */
  const float* dG_samples[GPSA_MAX_MODS];
  const float* dF_latent[GPSA_MAX_MODS];
  const float* dF_obs[GPSA_MAX_MODS];
  const float* dF_latent_test[GPSA_MAX_MODS];
  const float* dF_obs_test[GPSA_MAX_MODS];
  const double* dkl;                        /* [n_kl] or NULL */
  const float* gloss;                       /* [1] device scalar: upstream gradient of the loss (io.fuse_elbo) */
} gpsa_step_out_grads;

void* gpsa_step_create(const gpsa_step_desc* desc);   /* NULL: invalid / unsupported description */
/* the same plan described on the host only (no device): out[7] = saved bytes, scratch bytes, KL terms, floats of
 * eps_G, batched runs of free views, column stride of the view blocks, saved bytes without the kept products */
int gpsa_step_describe(const gpsa_step_desc* desc, long long* out);
void gpsa_step_destroy(void* plan);
long long gpsa_step_saved_bytes(const void* plan);
long long gpsa_step_saved_bytes_nokeep(const void* plan);  /* arena of a forward with io.keep_products == 0 */
int gpsa_step_fused(const void* plan, int m);         /* 1: modality m's training pass can run the fused ELBO kernel */
int gpsa_step_contraction(const void* plan, int m);   /* bit mask of modality m's bf16x3 kernels in a training step: 1 =
                                                         the fused ELBO pass (when gpsa_step_io.fuse_elbo is set: the
                                                         unfused path runs the fp32 kernels; cleared once a fused pass
                                                         of the plan has run with gpsa_step_io.skip_missing, set again
                                                         by one without; clear while gpsa_step_likelihood has
                                                         made m a Poisson modality), 2 = the data GP's Gram */
long long gpsa_step_scratch_bytes(const void* plan);
long long gpsa_step_bwd_acc_bytes(const void* plan);  /* gpsa_step_io.bwd_acc */
int gpsa_step_n_kl(const void* plan);                 /* V*D + sum_m L_m */
int gpsa_step_n_factorised(const void* plan);         /* matrices a forward with want_kl factorises: the priors + the
                                                         variational covariances of the plan's own KL terms
                                                         (gpsa_step_desc.kl_own_lo / _hi; all of them by default) */
long long gpsa_step_eps_g_numel(const void* plan);    /* floats in gpsa_step_io.eps_G */
/* EXPERIMENTAL, off by default: gpsa_step_forward / _backward can replay a cached hipGraph of their launch sequence
 * when they meet an argument set (pointer structs, arenas, stages, stream) for the second time, instead of enqueueing
 * 20 - 45 launches one by one (csrc/step.hip: "hipGraph cache" has the measurements and an open issue).  For callers
 * that own fixed buffers; GPSA_STEP_GRAPH=1 turns it on for the process.  This is the cache's switch and its counters:
 * enable != 0 / 0 (-1: leave as it is); out[0..3] = replays, eager calls, captures, graphs held (out may be NULL). */
int gpsa_step_graph(void* plan, int enable, long long* out);
/* backwards of this plan that took the early order of gpsa_step_io.f_event (the data GP's gradients finished first) */
long long gpsa_step_early_backwards(const void* plan);
/* Where the step's factorisation batch sits in the ``saved`` arena, for the reference's forward -> loss_fn hand-off
 * attributes Kuu_chol_list / curr_Omega_tril_list / Kuu_chol_F / curr_Omega_tril_F (vgpsa.py:237, 257, 321, 394, 412):
 * the engine keeps the matrices (K_uu + 1e-5 I, Omega = A A^T + 1e-5 I; fp64, [B, M, M] per group) and their inverses,
 * not the Cholesky factors, so the attributes are formed from these on access.  out[0] = number of groups (1: m_x ==
 * m_g, one batch; 2: the warp GPs' group, then the data GP's); per group g at out[1 + 4 g]: M, priors, variational
 * covariances, byte offset of the batch.  Order within a group: the priors (free views in order; the data GP's last /
 * alone), then Omega_G rows 0 .. V*D-1 (group 0), then every modality's Omega_F rows. */
int gpsa_step_batch_layout(const void* plan, long long* out);
/* stages: bit 0 = the M x M factorisations, the KL terms and the warp GPs (everything ``flag`` depends on),
 * bit 1 = the data GPs.  3 = the whole forward; a caller that wants to look at ``flag`` while the data GPs
 * run enqueues the two stages with two calls and its flag copy in between.
 * bits 8 .. 8 + GPSA_MAX_MODS - 1 (with bit 1): run the data GP of these modalities' training rows only (0: every
 * pass), on the ``saved`` arena stage 1 filled.  This is how the reference's two calls map onto the fused ELBO:
 * forward() enqueues stage 1 (+ the modalities that cannot fuse), loss_fn(), which is where the observations arrive
 * (vgpsa.py:491, 532-538), sets io.Y[m] and enqueues modality m's pass.  A caller that wants modality m's draws after
 * all passes Y[m] = NULL and F_latent[m] instead (the unfused kernels; the same io then goes to gpsa_step_backward).
 * bit 2: such a pass is an extra (re-)run, not one of the step's launches gpsa_step_timing records. */
int gpsa_step_forward(void* plan, const gpsa_step_params* params, const gpsa_step_io* io, void* saved,
                      void* scratch, int stages, void* stream);
/* diagnostic (bench.py's roofline figures): HIP events around the three contraction launches (the variance
 * form, its alpha-gradient, its Omega-gradient) of the first data-GP pass, on the stream they are launched on,
 * for a ring of ``slots`` steps; gpsa_step_timing_read returns the recorded steps' durations [n][3] in ms
 * (after the caller synchronised).  slots = 0 switches the events off. */
/* id of the stream capture ``stream`` belongs to (0: not capturing).  For hosts that cache scratch per stream: a block
 * allocated inside a capture lives in that graph's private pool and must not be reused by another capture. */
unsigned long long gpsa_stream_capture_id(void* stream);
int gpsa_step_timing(void* plan, int slots);
int gpsa_step_timing_read(void* plan, float* ms, int max_steps);
/* backward of the forward that filled ``saved`` (same params / io pointers and contents) */
int gpsa_step_backward(void* plan, const gpsa_step_params* params, const gpsa_step_io* io,
                       const gpsa_step_out_grads* og, void* saved, void* scratch,
                       const gpsa_step_param_grads* grads, void* stream);

/* ---- Gaussian likelihood + ELBO in one call each way (vgpsa.py:532-540) ------------------------------------
 * loss[0] = -(sum_i LL_i) + kl_scale * sum_t kl[t],  LL_i = sum log N(Y_i; F_i, exp(noise_u[i]) + 1e-5) / S_i
 * (n_ll likelihood terms: one per modality; F_i [S, N_i, P_i], Y_i [N_i, P_i]; kl [n_kl] fp64 or NULL).
 * backward: dF_i (overwritten), dnoise[i] (overwritten), dkl[t] = kl_scale * gloss; dnoise_all [n_noise] or NULL:
 * the whole noise-gradient vector the dnoise[i] point into, zero-filled first (the reference's noise_variance
 * holds entries no likelihood term reads, vgpsa.py:217 / :534).
 * workspace >= 8 * 4100 * n_ll bytes. */
int gpsa_elbo_loss_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                       const int* S, const long long* N, const int* P, const double* kl, int n_kl,
                       double kl_scale, float* loss, double* ll_out, void* workspace,
                       long long workspace_bytes, void* stream);
int gpsa_elbo_loss_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                       const int* S, const long long* N, const int* P, const float* gloss, int n_kl,
                       double kl_scale, float* const* dF, float* const* dnoise, float* dnoise_all, int n_noise,
                       double* dkl, void* workspace, long long workspace_bytes, void* stream);

/* gpsa_elbo_loss_fwd / _bwd with some likelihood terms fused into the step (gpsa_step_io.fuse_elbo): zpart[i] non-null =
 * term i's partial sums of z^2 (nparts doubles: gpsa_step_io.ll_part[m]); F[i] / dF[i] are then ignored.  One
 * implementation serves both pairs: the plain pair above is this one without a zpart table (every term from its draws),
 * and a table of NULLs here issues exactly the plain pair's launches. */
int gpsa_elbo_loss_fused_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                             const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                             const double* kl, int n_kl, double kl_scale, float* loss, double* ll_out, void* workspace,
                             long long workspace_bytes, void* stream);
int gpsa_elbo_loss_fused_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                             const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                             const float* gloss, int n_kl, double kl_scale, float* const* dF, float* const* dnoise,
                             float* dnoise_all, int n_noise, double* dkl, void* workspace, long long workspace_bytes,
                             void* stream);
/* ---- LMC likelihood without F_obs (round 4; replaces, for an LMC modality in training, the product
 * F_obs = F_latent W of vgpsa.py:428-432, the Gaussian likelihood over [S, N, P] of vgpsa.py:532-538 and autograd's
 * dF_latent = dF_obs W^T, dW = F_latent^T dF_obs): one pass that forms, at upstream gradient 1 of loss = -LL,
 *   zpart[]  block partials of sum ((Y[n,p] - F_obs[s,n,p]) / s)^2  (nparts doubles, tail zeroed: the ``zpart`` of
 *            gpsa_elbo_loss_fused_fwd / _bwd, which finish LL and the noise gradient from it),
 *   dF [S N, L] = dLoss/dF_latent,   dW [L, P] = dLoss/dW,        with s = exp(noise_u) + 1e-5, dF_obs = -(Y - F_obs)/(s^2 S).
 * F [S N, L] (F_latent, sample-major as the API tensor), W [L, P], Y [N, P].  L <= 64 (GPSA_EUNSUPPORTED beyond); since
 * round 5 the three products run on the matrix cores (csrc/lmc.hip; GPSA_LMC_MFMA=0: the vector-pipe kernel, L <= 32). */
long long gpsa_lmc_loglik_workspace(long long C, int L, int P, int nparts);
int gpsa_lmc_loglik_fused_f32(const float* F, const float* W, const float* Y, const float* noise_u, int S, long long N,
                              int L, int P, double* zpart, int nparts, float* dF, float* dW, void* workspace,
                              long long workspace_bytes, void* stream);
/* the fused forward's outputs (formed at upstream gradient 1) as the backward wants them: g, dmeanT, abar scaled by the
 * loss's upstream gradient (untouched when it is 1), g_ext row L = qbar = -sum_l g, dvar_u = exp(var_u) sum g */
int gpsa_elbo_fused_post(float* g_ext, float* dmeanT, float* abar, int M, long long C, int L, const float* gloss,
                         const float* var_u, int dvar_dtype, void* dvar_u, void* workspace, long long workspace_bytes,
                         void* stream);

/* ---- fused Adam over a list of tensors (torch.optim.Adam, no weight decay / amsgrad; the optimiser step of
 * the reference loop, examples/grid_example.py:59-78), ONE launch: for every element
 *   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * with t = ++step[0] kept on the device (capturable).  ptrs: HOST arrays of n device pointers. */
int gpsa_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const long long* numel, double lr, double beta1, double beta2,
                   double eps, float* step, void* stream);

/* ---- minibatch (stochastic variational) training (csrc/minibatch.hip, csrc/loss_views.hip; opt-in) ----------------
 * gpsa_row_sample_gather: draw step t's batch of every (modality m, view v) and gather it, in one launch plus a one-wave
 * launch that advances the step counter (counter[0] += 1 on the device: a replayed graph draws the next batch).
 * n_views[m] views per modality; n_rows / batch: N_{m,v} and B_{m,v} (1 <= B <= N) flattened over (m, v) in order
 * (at most 64 pairs); the views of modality m are consecutive row blocks of X[m] [sum_v N, D[m]] / Y[m] [sum_v N, P[m]].
 * With K = N div B, e = t div K, k = t mod K, row j < B of the batch of (m, v) is
 *     view start + pi_{seed,m,v,e}(k B + j),
 * pi a keyed bijection of [0, N) (a 6-round alternating Feistel network on ceil(log2 N) bits with cycle-walking; the
 * package's minibatch.feistel_perm restates it).  Outputs (views one after the other, batch order):
 * rows[m] [sum_v B] int64 (row numbers of X[m]), Xb[m] [sum_v B, D[m]], Yb[m] [sum_v B, P[m]] (bit-exact copies). */
int gpsa_row_sample_gather(int n_mods, const int* n_views, const long long* n_rows, const long long* batch,
                           unsigned long long seed, long long* counter, const float* const* X, const int* D,
                           const float* const* Y, const int* P, long long* const* rows, float* const* Xb,
                           float* const* Yb, void* stream);
/* gpsa_elbo_loss_fwd / _bwd with per-view weights:
 *   loss[0] = -(sum_i LL_i) + kl_scale * sum_t kl[t],  LL_i = sum_v w_i[v] sum_{rows of v} log N(Y_i; F_i, s_i) / S_i
 * view v of term i = rows view_off[i][v] .. view_off[i][v + 1] (host array of n_views[i] + 1 offsets, 0 .. N_i;
 * n_views[i] <= 64); w[i]: DEVICE array of n_views[i] doubles.  ll_out[i] = the weighted LL_i.  The backward's dF_i rows
 * carry their view's weight, dnoise[i] sums the views' parts with their weights; otherwise as gpsa_elbo_loss_bwd.
 * workspace >= 8 * 4100 * n_ll bytes. */
int gpsa_elbo_loss_weighted_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                                const int* S, const long long* N, const int* P, const int* n_views,
                                const long long* const* view_off, const double* const* w, const double* kl, int n_kl,
                                double kl_scale, float* loss, double* ll_out, void* workspace,
                                long long workspace_bytes, void* stream);
int gpsa_elbo_loss_weighted_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                                const int* S, const long long* N, const int* P, const int* n_views,
                                const long long* const* view_off, const double* const* w, const float* gloss, int n_kl,
                                double kl_scale, float* const* dF, float* const* dnoise, float* dnoise_all,
                                int n_noise, double* dkl, void* workspace, long long workspace_bytes, void* stream);

/* ---- partly observed outputs (csrc/missing.hip, csrc/loss_views.hip; opt-in: model.skip_missing) ----------------------
 * A NaN in Y is a missing observation; the ELBO is the one of the observed entries:
 *   LL_i = sum_v w_i[v] sum_{(n,p) observed in view v} log N(Y_i[n,p]; F_i[s,n,p], s_i) / S_i,   KL terms whole.
 * gpsa_count_observed: nobs[i][v] = number of non-NaN entries of Y_i [N_i, P_i] in the rows of view v (view_off as in
 * gpsa_elbo_loss_weighted_fwd; n_views == view_off == NULL: one view per term, all rows), written as DEVICE doubles by a
 * counting launch over all (term, view) pairs (64 to a launch; a call with more pairs loops over them) and a fixed-order
 * fp64 closing - no atomics, no host read: a captured step counts the batch it is replayed on.
 * workspace >= gpsa_count_observed_workspace() bytes. */
long long gpsa_count_observed_workspace(void);
int gpsa_count_observed(int n_ll, const float* const* Y, const long long* N, const int* P, const int* n_views,
                        const long long* const* view_off, double* const* nobs, void* workspace,
                        long long workspace_bytes, void* stream);
/* gpsa_elbo_loss_fwd / _bwd over the observed entries.  zpart (NULL, or per term NULL / nparts partial sums of z^2 from
 * gpsa_quadform_elbo_skip_f32, gpsa_lmc_loglik_fused_skip_f32: F[i] / dF[i] ignored; such a term has one view);
 * n_views / view_off / w: per-view weights as gpsa_elbo_loss_weighted_fwd (all NULL: one view of weight 1 per term; w
 * alone NULL: the views weigh 1); nobs[i]: DEVICE array of the term's views' counts (gpsa_count_observed with the same
 * views), which stand where S N P stands in the plain closings (the constant term, dnoise).  A term from draws applies
 * the select per element: dF = 0 exactly at a missing entry.  A view or term without an observed entry adds exactly 0 to
 * the loss and to dnoise.  workspace >= 8 * 4100 * n_ll bytes. */
int gpsa_elbo_loss_skip_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                            const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                            const int* n_views, const long long* const* view_off, const double* const* w,
                            const double* const* nobs, const double* kl, int n_kl, double kl_scale, float* loss,
                            double* ll_out, void* workspace, long long workspace_bytes, void* stream);
int gpsa_elbo_loss_skip_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                            const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                            const int* n_views, const long long* const* view_off, const double* const* w,
                            const double* const* nobs, const float* gloss, int n_kl, double kl_scale, float* const* dF,
                            float* const* dnoise, float* dnoise_all, int n_noise, double* dkl, void* workspace,
                            long long workspace_bytes, void* stream);
/* gpsa_lmc_loglik_fused_f32 over the observed entries: a missing (n, p) has dF_obs = 0 BEFORE the dF_latent and dW
 * products and z = 0.  Matrix-core kernel only (L <= 64); workspace: gpsa_lmc_loglik_workspace. */
int gpsa_lmc_loglik_fused_skip_f32(const float* F, const float* W, const float* Y, const float* noise_u, int S, long long N,
                                   int L, int P, double* zpart, int nparts, float* dF, float* dW, void* workspace,
                                   long long workspace_bytes, void* stream);

/* ---- count outputs: the Poisson likelihood (csrc/poisson.hip, csrc/loss_views.hip, csrc/qf_elbo_pois.hip, csrc/lmc.hip;
 * opt-in: model.likelihood) ---------------------------------------------------------------------------------------------
 * For a term of kind GPSA_LIK_POISSON the draws are log rates: with eta[s,n,p] = F[s,n,p] + log_offset[n] (log_offset
 * [N] fp32 or NULL = 0: per-row log size factors),
 *   LL = sum_v w[v] ( sum_{s, (n,p) in view v} (y eta - exp(eta)) / S  -  sum_{(n,p) in view v} lgamma(y + 1) ),
 *   dLoss/dF = gloss w[v] (exp(eta) - y) / S,
 * the same Monte-Carlo estimator as the Gaussian term's over the same draws.  Y is fp32 and is NOT validated: the formula
 * is evaluated as written for any real y; exp is the exact expf, and eta > 88 gives inf.  The term's noise_u entry does not
 * enter; its gradient is written as exactly 0.  skip != 0: a NaN in Y is a missing observation - its dF is exactly 0 and it
 * adds nothing to either sum (no count table: the term has no per-entry constant that depends on a parameter); skip == 0:
 * a NaN propagates to the loss.
 * gpsa_lgamma_sum: out[i][v] = sum of lgamma(Y_i[n,p] + 1) over the rows of view v (views as gpsa_count_observed's; NaN
 * entries left out when skip != 0), DEVICE doubles from an fp64 partial-sum launch and a fixed-order closing - no atomics,
 * no host read.  It depends on no parameter: once per Y tensor.  workspace >= gpsa_lgamma_sum_workspace() bytes. */
#define GPSA_LIK_GAUSSIAN 0
#define GPSA_LIK_POISSON 1
long long gpsa_lgamma_sum_workspace(void);
int gpsa_lgamma_sum(int n_ll, const float* const* Y, const long long* N, const int* P, const int* n_views,
                    const long long* const* view_off, int skip, double* const* out, void* workspace,
                    long long workspace_bytes, void* stream);
/* The ELBO loss closing for a model with at least one Poisson term: the tables of gpsa_elbo_loss_skip_fwd / _bwd (zpart,
 * n_views / view_off / w, nobs, each nullable as there) plus, per term, kind[i] (GPSA_LIK_*), lgam[i] (gpsa_lgamma_sum
 * with the same views and skip flag; read for Poisson terms) and log_offset[i] (Poisson terms; NULL entry or NULL table =
 * 0), and the skip flag.
 *   Poisson term: from its draws (loglik_pois_kernel) or, zpart[i] non-null, from nparts partial sums of y eta - exp(eta)
 *     (gpsa_quadform_elbo_pois_f32, gpsa_lmc_loglik_fused_pois_f32; one view); nobs[i] and noise_u[i] are not read.
 *   Gaussian term: exactly what the other closings do.  nobs[i] non-null: the skip closing's arithmetic over counts (from
 *     draws only with skip != 0; from partial sums of z^2 also with skip == 0, the caller then passing N_i P_i as the
 *     count); nobs[i] NULL (or no nobs table): the weighted closing's, which needs views and w[i] (skip == 0, from draws).
 * Every check runs before the first launch (GPSA_EINVAL / GPSA_EWORKSPACE).  workspace >= 8 * 4100 * n_ll bytes. */
int gpsa_elbo_loss_pois_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                            const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                            const int* n_views, const long long* const* view_off, const double* const* w,
                            const double* const* nobs, const int* kind, const double* const* lgam,
                            const float* const* log_offset, int skip, const double* kl, int n_kl, double kl_scale,
                            float* loss, double* ll_out, void* workspace, long long workspace_bytes, void* stream);
int gpsa_elbo_loss_pois_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                            const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                            const int* n_views, const long long* const* view_off, const double* const* w,
                            const double* const* nobs, const int* kind, const double* const* lgam,
                            const float* const* log_offset, int skip, const float* gloss, int n_kl, double kl_scale,
                            float* const* dF, float* const* dnoise, float* dnoise_all, int n_noise, double* dkl,
                            void* workspace, long long workspace_bytes, void* stream);
/* gpsa_quadform_elbo_skip_f32 / _delta_skip_f32 with the Poisson term in the closing (panel_elbo_pois_kernel): per (l, c),
 * c = s N + n, eta = F + log_offset[n];  dmeanT = dLoss/dF = (exp(eta) - Y[n,l]) / S;  g as there;  part[] sums
 * y eta - exp(eta).  noise_u is not read (may be NULL); log_offset [N] or NULL; skip as above.  fp32 contraction only; same
 * sizes, workspace query (gpsa_quadform_elbo_f32_workspace) and GPSA_EUNSUPPORTED cases. */
int gpsa_quadform_elbo_pois_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                                const float* meanT, const double* q, const float* var_u, const float* eps, const float* Y,
                                long long N, int S, const float* noise_u, float* g, float* dmeanT, float* abar,
                                double* part, float* FT, const float* log_offset, int skip, void* workspace,
                                long long workspace_bytes, void* stream);
int gpsa_quadform_elbo_delta_pois_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                                      const float* delta, const double* q, const float* var_u, const float* eps,
                                      const float* Y, long long N, int S, const float* noise_u, float* g, float* dmeanT,
                                      float* abar, double* part, float* FT, const float* log_offset, int skip,
                                      void* workspace, long long workspace_bytes, void* stream);
/* gpsa_lmc_loglik_fused_skip_f32 for a Poisson LMC modality (lmc_mfma_pois_kernel): F_obs = F W is the log rate,
 * dF_obs = (exp(eta) - y) / S in front of the unchanged dF_latent and dW products, zpart sums y eta - exp(eta).
 * Matrix-core kernel only (L <= 64); workspace: gpsa_lmc_loglik_workspace. */
int gpsa_lmc_loglik_fused_pois_f32(const float* F, const float* W, const float* Y, const float* log_offset, int skip, int S,
                                   long long N, int L, int P, double* zpart, int nparts, float* dF, float* dW,
                                   void* workspace, long long workspace_bytes, void* stream);
/* The likelihood of modality m's fused ELBO pass in the step engine (gpsa_step_io carries no field for it): kind
 * GPSA_LIK_POISSON makes stage 2 of gpsa_step_forward run gpsa_quadform_elbo_pois_f32 / _delta_pois_f32 for m with
 * log_offset ([N_m] or NULL; must stay valid while the plan may run) and gpsa_step_io.skip_missing as the skip flag;
 * ll_part[m] then goes to gpsa_elbo_loss_pois_fwd / _bwd.  Also in a bf16x3 plan: there is no x3 Poisson closing, the
 * pass runs the fp32 kernel (the Gram stays on x3) and gpsa_step_contraction reports it for as long as the kind is
 * set.  GPSA_LIK_GAUSSIAN (a new plan's state; log_offset must be NULL) goes back.  Set it before enqueuing m's pass. */
int gpsa_step_likelihood(void* plan, int m, int kind, const float* log_offset);

/* ---- count outputs: the negative binomial likelihood with a dispersion per output (csrc/negbin.hip,
 * csrc/loss_views.hip; opt-in: model.likelihood = "negative_binomial") -------------------------------------------------------------
 * For a term of kind GPSA_LIK_NEGBIN the draws are log means.  log_disp [P] fp32 is rho, r_p = exp(rho_p) the "size";
 * with eta[s,n,p] = F[s,n,p] + log_offset[n] and a = eta - rho_p,
 *   log NB(y; mu, r) = [lgamma(y + r) - lgamma(r) - lgamma(y + 1)] + y a - (y + r) softplus(a),
 *   softplus(a) = max(a, 0) + log1p(exp(-|a|)),  sigma(a) = 1 / (1 + exp(-a)),
 *   LL = sum_v w[v] ( sum_{s, (n,p) in v} t / S + sum_{(n,p) in v} c ),  t = y a - (y + r) softplus(a),
 *                                                                      c = lgamma(y + r) - lgamma(r) - lgamma(y + 1),
 *   dLoss/dF = gloss w[v] ((y + r) sigma(a) - y) / S,
 *   dLL/drho_p = sum_v w[v] ( sum_{s,n} u / S + sum_n r (psi(y + r) - psi(r)) ),  u = -r softplus(a) + (y + r) sigma(a) - y.
 * No exp(eta) appears: the term stays finite where the Poisson term overflows (eta = 136 gives t = -136, dF = 1 in fp32).
 * expf / log1pf are the exact ones; the per-element terms are fp32, every sum is fp64 in a fixed order (no atomics).  Y is
 * NOT validated; skip != 0: a NaN in Y is a missing observation (dF exactly 0, nothing added to any sum, rho's included);
 * skip == 0: a NaN propagates.  The term's noise_u entry does not enter; its gradient is written as exactly 0.
 * gpsa_nb_const: the draw-independent pieces, once per step (they depend on rho), in fp64 per term:
 *   csum[i][v]   = sum over the rows of view v of lgamma(y + r) - lgamma(r)      (unweighted, like gpsa_lgamma_sum's table)
 *   dconst[i][p] = sum_v w_i[v] sum_{n in v} r_p (psi(y + r_p) - psi(r_p))       (w NULL or w[i] NULL: weights of 1)
 * psi: the recurrence up to x >= 8, then the asymptotic series through x^-14; y + r <= 0 gives NaN there.  A column
 * reduction over Y [N, P]: threads along p, row blocks into fp64 partials, a fixed-order finish.  The lgamma(y + 1) table
 * stays gpsa_lgamma_sum's.  workspace >= the largest gpsa_nb_const_workspace(N_i, P_i, n_views_i) bytes of the call. */
#define GPSA_LIK_NEGBIN 2
long long gpsa_nb_const_workspace(long long N, int P, int n_views);
int gpsa_nb_const(int n_ll, const float* const* Y, const long long* N, const int* P, const float* const* log_disp,
                  const int* n_views, const long long* const* view_off, const double* const* w, int skip,
                  double* const* csum, double* const* dconst, void* workspace, long long workspace_bytes, void* stream);
/* The ELBO loss closing for a model with at least one negative binomial term: the tables of gpsa_elbo_loss_pois_fwd /
 * _bwd plus, per term, log_disp[i] ([P_i] fp32; NB terms), csum[i] / dconst[i] (gpsa_nb_const with the same views, weights
 * and skip flag) and lgam[i] (gpsa_lgamma_sum; Poisson AND NB terms).  _bwd writes ddisp[i] ([P_i] fp32; NB terms): the
 * gradient of the loss with respect to rho, gloss included.  An NB term from its draws runs loglik_nb_kernel; one that
 * arrives as nparts partial sums of t (zpart[i]; one view) brings usum[i], the [P_i] fp64 per-output sums of u over (s, n).
 * Gaussian and Poisson terms in the same call are closed exactly as gpsa_elbo_loss_pois_* closes them.  Every check runs
 * before the first launch.  workspace >= gpsa_elbo_loss_nb_workspace(n_ll, S, N, P, n_views, kind) bytes (n_views NULL:
 * one view per term; kind: the call's table - only its NB terms have column partials - or NULL: every term counted as NB). */
/* gpsa_quadform_elbo_pois_f32 / _delta_pois_f32 with the negative binomial term in the closing (panel_elbo_nb_kernel): per
 * (l, c), c = s N + n, a = F + log_offset[n] - log_disp[l];  dmeanT = dLoss/dF = ((y + r) sigma(a) - y) / S;  g as there;
 * part[] sums t.  u_elems [L, C] fp32 receives u per element at the index of g and dmeanT (exact 0 for a missing entry;
 * columns the kernel does not own are not written: C is covered exactly), and usum [L] fp64 its per-output sums over C
 * from a fixed-order row reduction - gpsa_elbo_loss_nb_bwd's usum[i].  noise_u is not read (may be NULL); log_offset [N] or
 * NULL; skip as above.  fp32 contraction only; same sizes, workspace query (gpsa_quadform_elbo_f32_workspace) and
 * GPSA_EUNSUPPORTED cases. */
int gpsa_quadform_elbo_nb_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                              const float* meanT, const double* q, const float* var_u, const float* eps, const float* Y,
                              long long N, int S, const float* noise_u, float* g, float* dmeanT, float* abar, double* part,
                              float* FT, const float* log_offset, const float* log_disp, float* u_elems, double* usum,
                              int skip, void* workspace, long long workspace_bytes, void* stream);
int gpsa_quadform_elbo_delta_nb_f32(int omega_dtype, const float* alpha, const void* Omega, int M, long long C, int L,
                                    const float* delta, const double* q, const float* var_u, const float* eps,
                                    const float* Y, long long N, int S, const float* noise_u, float* g, float* dmeanT,
                                    float* abar, double* part, float* FT, const float* log_offset, const float* log_disp,
                                    float* u_elems, double* usum, int skip, void* workspace, long long workspace_bytes,
                                    void* stream);
/* The step engine's setter for a negative binomial modality m: stage 2 of gpsa_step_forward then runs
 * gpsa_quadform_elbo_nb_f32 / _delta_nb_f32 for m with log_disp [L_m], u_elems [L_m, S N_m] fp32, usum [L_m] fp64 and
 * log_offset ([N_m] or NULL), all of which must stay valid while the plan may run; gpsa_step_io.skip_missing is the skip
 * flag and ll_part[m] goes to gpsa_elbo_loss_nb_fwd / _bwd with usum as usum[i].  It is the ONLY way to that kind:
 * gpsa_step_likelihood keeps refusing every kind but GPSA_LIK_GAUSSIAN and GPSA_LIK_POISSON, and either of those goes back
 * (and forgets the tensors).  A NULL log_disp, u_elems or usum is GPSA_EINVAL; a pass enqueued for a modality of this kind
 * without them is GPSA_EINVAL before any launch.  In a bf16x3 plan the pass runs the fp32 NB kernel (there is no x3 NB
 * closing; the Gram stays on x3) and gpsa_step_contraction reports it for as long as the kind is set. */
int gpsa_step_dispersion(void* plan, int m, const float* log_disp, float* u_elems, double* usum, const float* log_offset);
/* gpsa_lmc_loglik_fused_pois_f32 for a negative binomial LMC modality (lmc_mfma_nb_kernel): F_obs = F W is the log mean,
 * dF_obs = ((y + r) sigma(a) - y) / S in front of the unchanged dF_latent and dW products, zpart sums t, and usum [P] fp64
 * receives the per-output sums of u over (s, n) - per-workgroup [P] partials next to the dW partials, reduced in a fixed
 * order - which gpsa_elbo_loss_nb_bwd takes as usum[i].  Matrix-core kernel only (L <= 64, else GPSA_EUNSUPPORTED);
 * workspace >= gpsa_lmc_loglik_nb_workspace (gpsa_lmc_loglik_workspace plus the new partials). */
long long gpsa_lmc_loglik_nb_workspace(long long C, int L, int P, int nparts);
int gpsa_lmc_loglik_fused_nb_f32(const float* F, const float* W, const float* Y, const float* log_offset,
                                 const float* log_disp, int skip, int S, long long N, int L, int P, double* zpart,
                                 int nparts, float* dF, float* dW, double* usum, void* workspace,
                                 long long workspace_bytes, void* stream);
long long gpsa_elbo_loss_nb_workspace(int n_ll, const int* S, const long long* N, const int* P, const int* n_views,
                                      const int* kind);
int gpsa_elbo_loss_nb_fwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                          const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                          const int* n_views, const long long* const* view_off, const double* const* w,
                          const double* const* nobs, const int* kind, const double* const* lgam,
                          const float* const* log_offset, const float* const* log_disp, const double* const* csum,
                          int skip, const double* kl, int n_kl, double kl_scale, float* loss, double* ll_out,
                          void* workspace, long long workspace_bytes, void* stream);
int gpsa_elbo_loss_nb_bwd(int n_ll, const float* const* F, const float* const* Y, const float* const* noise_u,
                          const int* S, const long long* N, const int* P, const double* const* zpart, int nparts,
                          const int* n_views, const long long* const* view_off, const double* const* w,
                          const double* const* nobs, const int* kind, const double* const* lgam,
                          const float* const* log_offset, const float* const* log_disp, const double* const* dconst,
                          const double* const* usum, int skip, const float* gloss, int n_kl, double kl_scale,
                          float* const* dF, float* const* dnoise, float* dnoise_all, int n_noise, double* dkl,
                          float* const* ddisp, void* workspace, long long workspace_bytes, void* stream);

/* ---- prediction: closed-form moments of the data GP (csrc/predict.hip) ----------------------------------------------
 * The counterpart of gpsa_data_sample_fwd: from a chunk of c rows evaluated at S warp samples - meanT, v [L, S*c] fp32
 * (column s*c + r), q [S*c] fp64, var_u as there - it forms per sample the conditional of vgpsa.py:174-204,
 *   mu_s[r,l] = meanT[l, s c + r],  sigma2_s[r,l] = (exp(var_u) - q[s c + r])_fp64 + v[l, s c + r] + 2e-5,
 * mixes it with W [L,P] (LMC, vgpsa.py:428-432; W = NULL: P == L, no mix) per sample,
 *   m_s = mu_s W,  u_s = sigma2_s (W o W),
 * and reduces the S samples inside the kernel (law of total variance; fp64 arithmetic, centred sums):
 *   F_mean[r,p] = mean_s m_s,  F_var[r,p] = mean_s u_s + mean_s (m_s - F_mean)^2  (+ tau^2 when include_noise),
 *   tau = exp(noise_u[0]) + 1e-5 used as a standard deviation (vgpsa.py:217, 532-538).
 * Y [c,P] (may be NULL, then lpd must be NULL too): lpd[r] = sum_p log( mean_s N(Y[r,p]; m_s, u_s + tau^2) ) in fp64,
 * always with the noise, NaN entries of Y skipped, the mixture through a running maximum.
 * Fl_mean / Fl_var [c,L] (both or neither): the same moments of the latent outputs (no mix, no noise).
 * It stands for the draw-and-average idiom of the reference's prediction scripts
 * (experiments/expression/slideseq/slideseq_prediction.py:360-368: forward(prediction_mode=True, S) + mean over draws).
 * Nothing of size S*c*L or S*c*P is written; no workspace.  Any c, S, L, P >= 1; with W: L <= 64
 * (GPSA_EUNSUPPORTED beyond), GPSA_EINVAL on W == NULL with P != L or a missing noise_u. */
int gpsa_predict_moments_f32(const float* meanT, const float* v, const double* q, const float* var_u, long long c,
                             int S, int L, int P, const float* W, const float* noise_u, int include_noise,
                             const float* Y, float* F_mean, float* F_var, float* Fl_mean, float* Fl_var, double* lpd,
                             void* stream);

/* ---- prediction of counts: the same layer closed under a Poisson likelihood (csrc/predict_counts.hip) -----------------
 * Inputs, layout and the per-sample m_s, u_s exactly as gpsa_predict_moments_f32 forms them (mix with W per sample,
 * + 2e-5, never tau).  The log rate of row r, output p under sample s is eta ~ Normal(mu, u), mu = m_s[r,p] +
 * log_offset[r] (log_offset [c] fp32 or NULL = 0), u = u_s[r,p]; with lam_s = exp(mu + u/2)
 *   Y_mean[r,p] = mean_s lam_s,   Y_var[r,p] = Y_mean + mean_s[lam_s^2 expm1(u)] + var_s(lam_s)
 * (fp64, the between-sample term from sums centred on the first sample).  Y [c,P] fp32 (may be NULL, then lpd must be
 * NULL too, and neither a mode nor a quadrature is computed):
 *   lpd[r] = sum_p log( mean_s Int Poisson(Y[r,p]; e^eta) Normal(eta; mu, u) d eta )   in fp64, NaN entries skipped,
 * each integral by 20-node Gauss-Hermite quadrature centred on the mode of y eta - e^eta - (eta - mu)^2 / (2u) (8 Newton
 * iterations from min(mu + u y, max(mu, log y))), the samples mixed through a running maximum.  Y is not validated: the
 * formula is taken as written for any real y > -1 (lgamma(y + 1) by Stirling's series for a positive argument; y <= -1
 * gives NaN, where the library's lgamma would give its value at a non-positive argument).  Accuracy of one integral against brute force: 1.9e-10 (u <= 0.5), 2.0e-8
 * (u <= 1), 1.8e-6 (u <= 2), 4.6e-5 (u <= 4) as |error| / max(1, |log density|); nothing is measured beyond u = 4.
 * Y_mean / Y_var [c,P] fp32 are required.  No workspace.  Any c, S, L, P >= 1; with W: L <= 64 (GPSA_EUNSUPPORTED beyond),
 * GPSA_EINVAL on W == NULL with P != L, a missing array, or Y and lpd not both given / both NULL. */
int gpsa_predict_counts_f32(const float* meanT, const float* v, const double* q, const float* var_u, long long c, int S,
                            int L, int P, const float* W, const float* log_offset, const float* Y, float* Y_mean,
                            float* Y_var, double* lpd, void* stream);

/* ---- the learned warp as a function of the point (csrc/warp_field.hip): mean, Jacobian, determinant, inverse ----------
 * A non-fixed view's warp mean is closed form in x (vgpsa.py:174-204, mean only):
 *   g(x) = x A + b + k(x, Z) beta,   J[j, d] = d g_j / d x_d = A[d, j] + sum_m beta[m, j] cd(x, z_m) (x[d] - z_m[d])
 * Z, beta [M, D] (beta = K_uu^-1 (delta_G - (Z A + b)), formed by the caller), A [D, D], b [D], ls_u / var_u: device
 * scalars, unconstrained, as gpsa_kmat takes them; kind: GPSA_K_*.  Everything fp64; k(X, Z) is never formed in memory.
 * gpsa_warp_field_f64: X [n, D] -> G [n, D] and, where non-NULL, J [n, D, D] and det [n] = det J.
 * gpsa_warp_invert_f64: exactly `iters` undamped Newton updates x <- x - J(x)^-1 (g(x) - target) from x0 [n, D] in one
 *   launch (no early exit), then residual [n] = |g(X) - target|_2 evaluated at the returned X [n, D].  A zero or non-finite
 *   pivot of the D x D solve (partial pivoting) or a non-finite iterate fails the row: X = NaN, residual = +inf.
 * A row's result depends on its own inputs and M alone (not on n or its neighbours), the same bits from run to run.
 * GPSA_EINVAL: a NULL pointer (J / det excepted), n, M, D < 1, an unknown kind, iters < 0;  GPSA_EUNSUPPORTED: D > 4. */
int gpsa_warp_field_f64(int kind, const double* Z, const double* beta, const double* A, const double* b,
                        const double* ls_u, const double* var_u, const double* X, long long n, int M, int D, double* G,
                        double* J, double* det, void* stream);
int gpsa_warp_invert_f64(int kind, const double* Z, const double* beta, const double* A, const double* b,
                         const double* ls_u, const double* var_u, const double* target, const double* x0, int iters,
                         long long n, int M, int D, double* X, double* residual, void* stream);

/* ---- neighbour statistics (csrc/neighbors.hip): exact k nearest neighbours and the neighbours' weighted average ---------
 * gpsa_knn_f64: for every row of Q [nq, D] the k rows of R [nr, D] with the smallest key (d2, index), ascending in that
 *   key: d2 = sum_d (q_d - r_d)^2 in fp64 in difference form, ties in d2 to the lower index (a total order, so the result
 *   is the same bits for every `parts`).  idx [nq, k] int32, d2 [nq, k] fp64.  exclude_self != 0 skips reference j == i
 *   for query i (leave-one-out: the caller passes the same array as Q and R; where Q points at a later row of R's array,
 *   a row slice for a chunked call, the row skipped is the query's own row of R).  A distance that is NaN counts as +inf.
 *   parts: slices of the reference axis scanned by separate workgroups and merged by a second kernel by the same key;
 *   0 = auto (enough workgroups in flight when nq is small).  No atomics.  workspace >= gpsa_knn_workspace(nq, nr, k,
 *   parts) bytes (0 when the call resolves to one slice).
 *   GPSA_EINVAL: a NULL pointer, nq, nr, D, k < 1, parts < 0, k > nr - (exclude_self ? 1 : 0);  GPSA_EUNSUPPORTED: D > 4,
 *   k > 32;  GPSA_EWORKSPACE.  Every check runs before the first launch.
 * gpsa_knn_average_f32: out[i, p] = sum_j w_ij Y[idx[i, j], p] / sum_j w_ij over the neighbours j whose Y entry is not
 *   NaN (none: NaN), accumulated in fp64 in the order j = 0 .. k-1.  idx [nq, k], Y [nr, P] fp32, out [nq, P] fp32.
 *   weights 0: uniform (d2 may be NULL);  1: inverse distance, w = 1 / sqrt(d2), and in a row where some d2 == 0 exactly
 *   the zero-distance neighbours get weight 1 and the others 0.  No workspace.  Indices are not validated.
 *   GPSA_EINVAL: a NULL pointer (d2 with weights 0 excepted), nq, k, nr, P < 1, an unknown `weights`.
 * gpsa_knn_average_f64: the same kernel with Y and out in fp64 (Moran's I needs the lag of a centred column to fp64
 *   rounding; an fp32 result carries 6e-8). */
long long gpsa_knn_workspace(long long nq, long long nr, int k, int parts);
int gpsa_knn_f64(const double* Q, long long nq, const double* R, long long nr, int D, int k, int exclude_self, int parts,
                 int* idx, double* d2, void* workspace, long long workspace_bytes, void* stream);
int gpsa_knn_average_f32(const int* idx, const double* d2, long long nq, int k, const float* Y, long long nr, int P,
                         int weights, float* out, void* stream);
int gpsa_knn_average_f64(const int* idx, const double* d2, long long nq, int k, const double* Y, long long nr, int P,
                         int weights, double* out, void* stream);

/* ---- count preprocessing (csrc/counts.hip): margins, Poisson deviance, residual transforms, per-view z-score -------------
 * Y [N, P] fp32, row-major, counts held as floats.  Every sum is fp64 in a fixed order, no atomics, nothing of N * P
 * elements is allocated.  The three reductions take workspace >= gpsa_count_workspace(N, P) bytes (a pure host query:
 * the column partials of at most 1024 row groups while a group stays <= 512 rows, about 16 * 1024 * P bytes).
 * Common refusals, all before the first launch: GPSA_EINVAL for a NULL pointer, N < 1, P < 1, P >= 2^31, N > 16 (2^31 - 1)
 * (the grids' extents);
 * GPSA_EWORKSPACE for a NULL or short workspace.
 * gpsa_count_margins_f32: ONE read of Y -> row_sum [N] fp64, col_sum [P] fp64, row_nnz [N] and col_nnz [P] int64 (entries
 *   > 0), n_invalid (one int64 on the device): the entries that are NaN, +-inf or < 0.
 * gpsa_count_deviance_f32: log_sz [N] fp64 -> ll_sat[g] = sum_i y log y - y log_sz_i and abs_sat[g] = sum_i |y log y| +
 *   |y log_sz_i| (terms of y = 0 are 0), both [P] fp64.  The deviance 2 (ll_sat - col_sum log(col_sum / sum_i sz_i)) is
 *   closed by the caller.
 * gpsa_count_transform_f32: elementwise, fp64 arithmetic, rounded once to fp32; out [N, P] may be Y.  With
 *   mu = row_sum_i col_sum_g / total (an entry with mu = 0 gives 0):
 *     mode 0, Pearson:  z = (y - mu) / sqrt(mu + mu^2 / theta), clipped to +-clip when clip > 0   (theta = inf: Poisson)
 *     mode 1, NB deviance residual: sign(y - mu) sqrt(max(0, 2 (y log(y / mu) - (y + theta) log((y + theta) / (mu + theta)))))
 *     mode 2, Poisson deviance residual: sign(y - mu) sqrt(max(0, 2 (y log(y / mu) - (y - mu))))
 *     mode 3: log1p(y target / row_sum_i), 0 in a row with row_sum = 0 (col_sum may be NULL)
 *   Each mode reads only its own scalars.  GPSA_EINVAL also for an unknown mode, total or target not in (0, inf),
 *   theta <= 0 or NaN (modes 0, 1), theta = inf in mode 1, clip < 0.
 * gpsa_standardize_views_f32: out = (y - mean) / std per (view, column) over the consecutive row ranges
 *   view_off [V + 1] (a HOST array, 0 = view_off[0] < ... < view_off[V] = N); std is the population value (ddof 0), the
 *   moments are Welford updates joined by Chan's formula.  A column that is constant within a view is written as 0 and
 *   counted in n_constant [V] (int64, device).  out may be Y.  GPSA_EINVAL also for V < 1, offsets that do not
 *   partition [0, N) or an empty view. */
long long gpsa_count_workspace(long long N, long long P);
int gpsa_count_margins_f32(const float* Y, long long N, long long P, double* row_sum, double* col_sum, long long* row_nnz,
                           long long* col_nnz, long long* n_invalid, void* workspace, long long workspace_bytes,
                           void* stream);
int gpsa_count_deviance_f32(const float* Y, long long N, long long P, const double* log_sz, double* ll_sat, double* abs_sat,
                            void* workspace, long long workspace_bytes, void* stream);
int gpsa_count_transform_f32(int mode, const float* Y, long long N, long long P, const double* row_sum,
                             const double* col_sum, double total, double theta, double clip, double target, float* out,
                             void* stream);
int gpsa_standardize_views_f32(const float* Y, long long N, long long P, const long long* view_off, int V, float* out,
                               long long* n_constant, void* workspace, long long workspace_bytes, void* stream);

/* ---- count preprocessing from a sparse matrix (csrc/counts_sparse.hip): check, margins, deviance, gather ----------------
 * The matrix is CSR on the device: crow [N + 1] int64, col [nnz] int32, val [nnz] fp32 (all device pointers; col and val
 * may be NULL when nnz == 0).  The same rules as above: fp64 sums in a fixed order, no atomics, one writer per output
 * element, the same bits on a repeated call.  Integer counts give the dense entries' results bit for bit; other values
 * agree to rounding.  keep [N] uint8 (device) or NULL: a row with keep == 0 is skipped by the two reductions as if absent.
 * gpsa_csr_check and the two reductions take workspace >= gpsa_count_csr_workspace(N, P) bytes (a pure host query, 0 for
 * N < 1 or P < 1: the column partials of at most 32 row groups, the row partials of the P / 512 column tiles; it does
 * not depend on nnz).
 * Refusals, all before the first launch and with nothing written: GPSA_EINVAL for a NULL pointer (keep excepted), N < 1,
 * P < 1, N or P >= 2^31, nnz < 0, nnz > N * P, nnz > 0 with a NULL col or val, n_rows < 1, G < 1 or G > P;
 * GPSA_EWORKSPACE for a NULL or short workspace.
 * gpsa_csr_check: out [4] int64 on the device = the number of crow violations (crow[0] != 0, a decrease, crow[N] != nnz);
 *   of column indices outside [0, P); of places inside a row where the column index does not strictly increase (unsorted
 *   rows and duplicates); of stored values equal to 0 (information, not an error).  Every read is bounded by
 *   construction: crow over [0, N], col and val flat over [0, nnz), the per-row pass over row bounds clamped to [0, nnz].
 * gpsa_count_margins_csr_f32: ONE read of the matrix -> row_sum [N], col_sum [P] fp64, row_nnz [N], col_nnz [P] int64 (the
 *   stored entries > 0: a stored 0 does not count), n_invalid (one int64): the stored values that are NaN, +-inf or < 0.
 *   A row masked out has row_sum = 0, row_nnz = 0 and contributes to no column.
 * gpsa_count_deviance_csr_f32: log_sz [N] fp64 indexed by the original row -> ll_sat, abs_sat [P] as defined for
 *   gpsa_count_deviance_f32; the caller closes the deviance.
 * gpsa_csr_gather_dense_f32: out [n_rows, G] fp32 row-major, out[j, slot[g]] = the value stored at (rows[j], g) for every
 *   gene g with slot[g] in [0, G) (slot [P] int32, -1: dropped; rows [n_rows] int64), 0 where nothing is stored.  A row is
 *   assembled in LDS and stored coalesced: each element of out is written exactly once.
 * Defence in depth: the three compute entries do not rely on the check.  They clamp every row range to [0, nnz] and skip
 * a column index outside [0, P), a slot outside [0, G) and a row outside [0, N) (written as zeros), so a malformed matrix
 * gives wrong sums but is never followed outside its buffers. */
long long gpsa_count_csr_workspace(long long N, long long P);
int gpsa_csr_check(const long long* crow, const int* col, const float* val, long long N, long long P, long long nnz,
                   long long* out, void* workspace, long long workspace_bytes, void* stream);
int gpsa_count_margins_csr_f32(const long long* crow, const int* col, const float* val, const unsigned char* keep,
                               long long N, long long P, long long nnz, double* row_sum, double* col_sum,
                               long long* row_nnz, long long* col_nnz, long long* n_invalid, void* workspace,
                               long long workspace_bytes, void* stream);
int gpsa_count_deviance_csr_f32(const long long* crow, const int* col, const float* val, const unsigned char* keep,
                                long long N, long long P, long long nnz, const double* log_sz, double* ll_sat,
                                double* abs_sat, void* workspace, long long workspace_bytes, void* stream);
int gpsa_csr_gather_dense_f32(const long long* crow, const int* col, const float* val, long long N, long long P,
                              long long nnz, const long long* rows, long long n_rows, const int* slot, long long G,
                              float* out, void* stream);

/* ---- per-view column moments (csrc/moments.hip): what dispersion-based gene selection and a variance filter reduce to ----
 * For every view v (the consecutive rows view_off[v] .. view_off[v + 1] - 1; view_off [V + 1] is a HOST array, 0 =
 * view_off[0] < ... < view_off[V] = N, as gpsa_standardize_views_f32 takes it) and every column c:
 *   s1[v, c] = sum t, s2[v, c] = sum t^2, abs1[v, c] = sum |t| over the view's rows, all [V, P] fp64 row-major, and
 *   n_nonfinite (one int64 on the device): the number of t that are NaN or +-inf.
 * t is formed in fp64 from the stored fp32 value y:
 *   mode 0: t = y (negative values allowed: the variance filter on transformed data; abs1 is the error scale of s1);
 *   mode 1: t = expm1(y) (the matrix is log1p of the normalised counts);
 *   mode 2: t = y scale_i, scale [N] fp64 on the device (target / row_sum_i, 0 for an empty row): the moments of the
 *           normalised counts straight from the raw counts.  scale is read in mode 2 only and may be NULL otherwise.
 * The caller closes mean and variance.  The rules of the count entries hold: fp64 sums in a fixed order, no atomics, one
 * writer per output element, the same bits on a repeated call, nothing of N * P elements allocated; a row group never
 * mixes two views (the views are walked one after the other).  Integer values in mode 0 give the same s1 bit for bit
 * from both entries.
 * gpsa_column_moments_f32: Y [N, P] fp32 row-major.  workspace >= gpsa_column_moments_workspace(N, P, V) bytes (a pure
 *   host query, 0 for N, P or V < 1: three column planes of at most 512 row groups, 24 * 512 * P bytes and change).
 * gpsa_column_moments_csr_f32: the matrix in CSR as in the section above, keep [N] uint8 or NULL: a row with keep == 0
 *   contributes to nothing.  Unstored entries contribute exactly 0 in all three modes (expm1(0) = 0): the sums and
 *   n_nonfinite run over the stored entries.  scale is indexed by the row of the whole matrix.  workspace >=
 *   gpsa_column_moments_csr_workspace(N, P, V) bytes (three column planes of at most 16 row groups; not a function of
 *   nnz).  Every row range is clamped to [0, nnz] and every column index is checked inside the kernel: a malformed matrix
 *   gives wrong sums but is never followed outside its buffers.
 * Refusals, all before the first launch and with nothing written: GPSA_EINVAL for a NULL pointer (keep, and scale
 * outside mode 2, excepted), an unknown mode, N < 1, P < 1, P >= 2^31, N > 16 (2^31 - 1) (dense) or N >= 2^31 (CSR),
 * nnz < 0, nnz > N * P, nnz > 0 with a NULL col or val, V < 1, offsets that do not partition [0, N) or an empty view;
 * GPSA_EWORKSPACE for a NULL or short workspace. */
long long gpsa_column_moments_workspace(long long N, long long P, int V);
long long gpsa_column_moments_csr_workspace(long long N, long long P, int V);
int gpsa_column_moments_f32(int mode, const float* Y, long long N, long long P, const double* scale,
                            const long long* view_off, int V, double* s1, double* s2, double* abs1,
                            long long* n_nonfinite, void* workspace, long long workspace_bytes, void* stream);
int gpsa_column_moments_csr_f32(int mode, const long long* crow, const int* col, const float* val,
                                const unsigned char* keep, long long N, long long P, long long nnz, const double* scale,
                                const long long* view_off, int V, double* s1, double* s2, double* abs1,
                                long long* n_nonfinite, void* workspace, long long workspace_bytes, void* stream);

/* ---- exact GP regression (csrc/gpr.hip): sklearn's GaussianProcessRegressor with [C *] k + WhiteKernel ------------------
 * What the reference's experiments fit on the CPU around GPSA: the prediction baselines
 * (experiments/simulations/two_dimensional_prediction.py:126-155, 238, one_dimensional_prediction.py:128-139,
 * expression/st/st_prediction.py:142-156, 251) and the data kernel's starting length scale (two_dimensional.py:84-91).
 * All fp64.  K(theta) = a k(X, X; l) + (tau2 + jitter) I with theta = (log a, log l, log tau2), three doubles on the
 * DEVICE; a = 1 (theta[0] is not read for it) unless amplitude != 0, sklearn's ConstantKernel() * k.  kind: GPSA_K_*, in
 * sklearn's forms: rbf exp(-d^2 / (2 l^2)); matern32 (1 + r) exp(-r), r = sqrt(3) d / l; matern12 exp(-d / l).  D <= 4.
 * gpsa_gpr_cov_f64: K [na, nb] = a k(XA, XB)  (kernel(X) / kernel(X*, X) of GaussianProcessRegressor.fit / .predict).
 *   same != 0 (XA and XB are the same array, na == nb): the diagonal gets (a + tau2) + jitter, every off-diagonal 64 x 64
 *   tile is computed once and written to both places - K is symmetric to the bit.
 * gpsa_gpr_lml_grad_f64: out[0..2] = dLML / d(log a, log l, log tau2) = 1/2 sum_ij W_ij dK_ij / dtheta, W = alpha alpha^T -
 *   P Kinv  (log_marginal_likelihood(theta, eval_gradient=True)'s einsum over the K_gradient cube).  X [N, D], alpha =
 *   K^-1 Y [N, P], Kinv [N, N].  Per tile (I, J <= I) of the pair grid alpha_I alpha_J^T runs on v_mfma_f64_16x16x4_f64
 *   (P zero-padded to a multiple of 4 in registers), k and dk / dlog l come from X_I, X_J on the fly, off-diagonal tiles
 *   count twice; the tau2 entry is 1/2 tau2 (sum_i |alpha_i|^2 - P tr Kinv) from the diagonal tiles.  out[0] is written
 *   with a = 1 when amplitude == 0.  Nothing of N x N is written; no atomics: per-workgroup partials in the workspace
 *   (>= gpsa_gpr_lml_grad_workspace(N, P) bytes, a pure host query) are added in a fixed order by a second launch, so
 *   a repeated call gives the same bits.
 * gpsa_gpr_mean_f64: out [ns, P] = a k(XS, X) alpha  (GaussianProcessRegressor.predict's K_trans @ alpha_).  The kernel
 *   tile is generated straight into the MFMA's A operand: no [ns, N] matrix exists.  The sum over the training rows runs
 *   in one fixed order that does not depend on which rows of XS are passed together.
 * GPSA_EINVAL: a NULL pointer, a size < 1, an unknown kind, jitter < 0 or NaN, same != 0 with XA != XB or na != nb;
 * GPSA_EUNSUPPORTED: D > 4, a grid extent (N > 65535 * 64 rows in gpsa_gpr_lml_grad_f64 / gpsa_gpr_cov_f64's na);
 * GPSA_EWORKSPACE.  Every check runs before the first launch. */
int gpsa_gpr_cov_f64(int kind, const double* XA, long long na, const double* XB, long long nb, int D, const double* theta,
                     int amplitude, int same, double jitter, double* K, void* stream);
long long gpsa_gpr_lml_grad_workspace(long long N, int P);
int gpsa_gpr_lml_grad_f64(int kind, const double* X, long long N, int D, const double* theta, int amplitude,
                          const double* alpha, int P, const double* Kinv, double* out, void* workspace,
                          long long workspace_bytes, void* stream);
int gpsa_gpr_mean_f64(int kind, const double* XS, long long ns, const double* X, long long N, int D, const double* theta,
                      int amplitude, const double* alpha, int P, double* out, void* stream);

/* ---- optimal-transport slice alignment (csrc/ot.hip): entropic fused Gromov-Wasserstein between two slices --------------
 * The pieces of a projected-gradient solve (Peyre, Cuturi and Solomon 2016) whose outer step is
 *   cost = (1 - alpha) M + 2 alpha (cA 1^T + 1 cB^T - 2 C1 T C2),   T <- argmin <cost, T> + e KL(T || a x b)
 * next to gpsa_gemm, which forms P log Q^T and C1 T C2.  All fp64, row-major; expression is read as fp32.  Every sum runs
 * in a fixed order without atomics (a repeated call gives the same bits); nothing of n m elements is allocated; every
 * *_workspace is a pure host query.
 *
 * gpsa_ot_dist_f64: Cm [n, n] = |x_i - x_k| (Euclidean, not squared) from X [n, D]; difference form, symmetric to the
 *   bit, the diagonal exactly 0.
 * gpsa_ot_sqmatvec_f64: out [n] = sum_k Cm_ik^2 v_k for Cm [n, ncol]  (cA = (C1 o C1) a).
 * gpsa_ot_expr_rows_f32: Y [n, P] fp32 ->
 *   mode 0 ("kl"):        Pm = (y + 0.01) / row sum, Lg = log Pm, term [n] = sum_p Pm Lg; n_invalid (one int64 on the
 *                         device) counts the entries that are negative, NaN or inf;
 *   mode 1 ("euclidean"): Pm = y, term = sum_p y^2 (Lg may be NULL); n_invalid counts the NaN or inf entries.
 * gpsa_ot_expr_cost_f64: in place over G [n, m]: mode 0  M = ra_i - G_ij  (G = P log Q^T);
 *   mode 1  M = max(0, ra_i + rb_j - 2 G_ij)  (G = A B^T: the SQUARED Euclidean distance of expression rows).
 * gpsa_ot_cost_f64: in place over G = C1 T C2 [n, m]: the cost above; the same pass writes sums[0..2] = sum |cost|,
 *   <M, T>, <cAt 1^T + 1 cBt^T - 2 G, T>  (cAt, cBt: (C o C) times T's own marginals; alpha in [0, 1]).
 * gpsa_ot_sinkhorn_f64: `iters` log-domain sweeps on the stream, f and g read and updated in place:
 *   f_i = -e LSE_j((g_j - cost_ij) / e + log b_j), then g_j = -e LSE_i((f_i - cost_ij) / e + log a_i); e = *eps, a DEVICE
 *   double.  A row is never split over workgroups; the column pass keeps a (max, sum) partial per (row group, column) in
 *   the workspace and merges the groups in order.  Running maxima are subtracted before every exp.
 * gpsa_ot_plan_f64: T_ij = a_i b_j exp((f_i + g_j - cost_ij) / e) written over T (the previous plan); rowsum [n] = T 1,
 *   colsum [m] = T^T 1, sums[0..2] = |T 1 - a|_1, |T^T 1 - b|_1, |T - T_old|_1.
 *
 * GPSA_EINVAL: a NULL pointer (Lg in mode 1, rb in mode 0 excepted), a size < 1, an unknown mode, alpha outside [0, 1],
 * iters < 0;  GPSA_EUNSUPPORTED: D > 4, n or m >= 2^31, n > 65535 * 64 in gpsa_ot_dist_f64;  GPSA_EWORKSPACE.  Every check
 * runs before the first launch. */
int gpsa_ot_dist_f64(const double* X, long long n, int D, double* Cm, void* stream);
int gpsa_ot_sqmatvec_f64(const double* Cm, long long n, long long ncol, const double* v, double* out, void* stream);
long long gpsa_ot_expr_rows_workspace(long long n);
int gpsa_ot_expr_rows_f32(int mode, const float* Y, long long n, long long P, double* Pm, double* Lg, double* term,
                          long long* n_invalid, void* workspace, long long workspace_bytes, void* stream);
int gpsa_ot_expr_cost_f64(int mode, double* G, long long n, long long m, const double* ra, const double* rb,
                          void* stream);
long long gpsa_ot_cost_workspace(long long n, long long m);
int gpsa_ot_cost_f64(double* G, const double* M, const double* T, const double* cA, const double* cB, const double* cAt,
                     const double* cBt, double alpha, long long n, long long m, double* sums, void* workspace,
                     long long workspace_bytes, void* stream);
long long gpsa_ot_sinkhorn_workspace(long long n, long long m);
int gpsa_ot_sinkhorn_f64(const double* cost, long long n, long long m, const double* loga, const double* logb,
                         const double* eps, double* f, double* g, int iters, void* workspace,
                         long long workspace_bytes, void* stream);
long long gpsa_ot_plan_workspace(long long n, long long m);
int gpsa_ot_plan_f64(const double* cost, long long n, long long m, const double* f, const double* g, const double* a,
                     const double* b, const double* eps, double* T, double* rowsum, double* colsum, double* sums,
                     void* workspace, long long workspace_bytes, void* stream);

/* ---- histology images (csrc/image.hip): the pixel modality out of an image, and an image read at any coordinates -------
 * img is [H, W, C] row-major, C in 1..4; a uint8 value u is (float)u / 255.0f (one fp32 division), an fp32 value is taken
 * as is.  No atomics, every sum in a fixed order, one writer per output element, the same bits on a repeated call;
 * nothing of H W elements is allocated; gpsa_image_select_workspace is a pure host query (0 for sizes an entry refuses).
 *
 * select: `bin` = b in 1..64 reduces the image to H' = H div b, W' = W div b output pixels, each the mean of its full
 *   b x b block per channel (fp64 sum in row-major order within the block, / b^2 in fp64, rounded to fp32 once; partial
 *   blocks at the right and bottom edges are dropped).  Output pixel (r, c) lies at x = c b + (b - 1) / 2,
 *   y = r b + (b - 1) / 2 and is
 *     background  when every channel has rintf(v * 10.0f) == rintf(bg * 10.0f)  (fp32 product, round-half-even: numpy's
 *                 round(v, 1) == bg on fp32; a NaN channel is never background; has_bg = 0: the rule is off);
 *     outside     when it is not background and fails xmin < x < xmax && ymin < y < ymax, strict, in fp64, with
 *                 bbox = {xmin, xmax, ymin, ymax}, a HOST array (has_bbox = 0: the rule is off, bbox may be NULL);
 *     kept        otherwise.
 *   gpsa_image_select_count_*: per-tile class counts into the workspace, scanned in tile order into tile offsets; the
 *     totals (kept, background, outside) are left as three int64 at the head of the workspace, on the device.
 *   gpsa_image_select_write_*: the same arguments and the SAME workspace after a count; recomputes the class and writes
 *     the kept pixels in the row-major order of the output pixels (a stable compaction): coords [n, 2] fp32 = (x, y),
 *     pixels [n, C] fp32.  It reads the kept total back from the workspace (8 bytes, the stream is synchronised); with
 *     capacity (the rows of coords / pixels) below it nothing is written: GPSA_EINVAL.  A kept total of 0 launches nothing.
 * sample: out [n, C] fp32 and valid [n] uint8 at xy [n, 2] fp64 = (x, y) in pixel coordinates, x the column.  A row is
 *   valid when 0 <= x <= W - 1 && 0 <= y <= H - 1 (NaN and +-inf are not); an invalid row reads nothing and is `fill` in
 *   every channel.  order 1: bilinear in fp64 on the cell x0 = min(floor(x), W - 2) (0 when W = 1), fx = x - x0, likewise
 *   y: top = I[y0,x0] (1 - fx) + I[y0,x1] fx, bot the same on y1, out = top (1 - fy) + bot fy, rounded to fp32 once, so
 *   x = W - 1 never reads column W.  order 0: the pixel at floor(x + 0.5), clamped into the image.  A row's result does
 *   not depend on the other rows or on n.
 *
 * GPSA_EINVAL: a NULL pointer, H or W < 1, C outside 1..4, bin outside 1..64 or larger than H or W, H' W' >= 2^31, a bbox
 * with a NaN, capacity < 1 or below the kept total, n < 1 or >= 2^31, an order other than 0 and 1;  GPSA_EWORKSPACE: a
 * workspace that is NULL or shorter than gpsa_image_select_workspace(H, W, bin).  Every check runs before the first
 * launch. */
long long gpsa_image_select_workspace(long long H, long long W, int bin);
int gpsa_image_select_count_u8(const unsigned char* img, long long H, long long W, int C, int bin, int has_bg, float bg,
                               int has_bbox, const double* bbox, void* workspace, long long workspace_bytes,
                               void* stream);
int gpsa_image_select_count_f32(const float* img, long long H, long long W, int C, int bin, int has_bg, float bg,
                                int has_bbox, const double* bbox, void* workspace, long long workspace_bytes,
                                void* stream);
int gpsa_image_select_write_u8(const unsigned char* img, long long H, long long W, int C, int bin, int has_bg, float bg,
                               int has_bbox, const double* bbox, void* workspace, long long workspace_bytes,
                               float* coords, float* pixels, long long capacity, void* stream);
int gpsa_image_select_write_f32(const float* img, long long H, long long W, int C, int bin, int has_bg, float bg,
                                int has_bbox, const double* bbox, void* workspace, long long workspace_bytes,
                                float* coords, float* pixels, long long capacity, void* stream);
int gpsa_image_sample_u8(const unsigned char* img, long long H, long long W, int C, const double* xy, long long n,
                         int order, float fill, float* out, unsigned char* valid, void* stream);
int gpsa_image_sample_f32(const float* img, long long H, long long W, int C, const double* xy, long long n, int order,
                          float fill, float* out, unsigned char* valid, void* stream);

/* ---- spatial autocorrelation (csrc/autocorr.hip): the weight graph, its sums, the permuted Moran / Geary numerators ------
 * The graph is CSR on the device: crow [n + 1] int64, col [nnz] int32 ascending within a row, w [nnz] fp64 (col and w may
 * be NULL when nnz == 0).  No atomics, every sum fp64 in a fixed order, one writer per output element, the same bits on
 * a repeated call; nothing of n x n is allocated; the *_workspace queries are pure host functions (0 for sizes an entry
 * refuses).
 *
 * gpsa_graph_merge_count / _write: the graph out of kNN lists.  out [n, k] int32: every row's k neighbours ASCENDING by
 *   index (the caller sorts the kNN lists), no self entry; in_src [n k] int32 / in_ptr [n + 1] int64: the rows that list
 *   row i are in_src[in_ptr[i] .. in_ptr[i + 1]), ascending (a stable sort of the flattened lists by target).  kind 0: the
 *   row is its out-list (in_ptr / in_src may be NULL); 1: the union of the two lists; 2: their intersection (a row may be
 *   empty).  _count writes crow [n + 1] (row lengths, then one workgroup's prefix sum); the caller reads nnz = crow[n] and
 *   _write fills col (ascending) and w = 1, or 1 / (row length) when row_standardize != 0.  One thread merges one row.
 * gpsa_graph_check_f64: out [5] int64 on the device = the number of crow violations (crow[0] != 0, a decrease, crow[n] !=
 *   nnz); of columns outside [0, n); of places inside a row where the column does not strictly increase; of self edges;
 *   of weights that are NaN, infinite or < 0.  Every read is bounded: row ranges are clamped to [0, nnz].
 * gpsa_graph_sums_f64: out [3] fp64 on the device = S0 = sum w;  S1 = 1/2 sum_ij (w_ij + w_ji)^2, per stored edge
 *   1/2 (w_ij + w_ji)^2 where the reverse edge is stored (binary search in row j) and w_ij^2 where it is not;  S2 =
 *   sum_i (w_i. + w_.i)^2, the column sum over the transposed structure: tperm [nnz] int64 = the positions of the entries
 *   in the order of a stable sort by column, tptr [n + 1] int64 = where each column starts in it.  A thread per row, the
 *   rows of a workgroup (256) added in row order, the workgroups in order.  Indices outside their arrays are skipped.
 * gpsa_graph_check_f64 and gpsa_graph_sums_f64 take workspace >= gpsa_graph_workspace(n) bytes.
 *
 * gpsa_autocorr_perm_f64: Z [n, P] fp64 row-major (a column-centred matrix), perms [R, n] int32, mode 0 | 1 ->
 *   mode 0 (Moran):  num[r, p] = sum_i Z[pi_r(i), p] * sum_{j in row i} w_ij Z[pi_r(j), p]
 *   mode 1 (Geary):  num[r, p] = sum_i sum_{j in row i} w_ij (Z[pi_r(i), p] - Z[pi_r(j), p])^2
 *   num [R, P] fp64.  The permuted matrix never exists: rows of Z are gathered through perms, a wave's lanes run over 64
 *   consecutive genes (a gathered row is one coalesced read), it carries 4 permutations (4 rows in flight per neighbour
 *   position) and a workgroup 16, which share one read of the rows' crow / col / w.  Within a row j runs in CSR order
 *   (explicit fma), the rows ascend within a row group, the row groups - ceil(n / max(32, ceil(n / 32))) of them, a
 *   function of n alone - are added in ascending order by a second kernel: num[r, p] is the same bits whatever R, P
 *   or the other rows of perms are, so an identity row anywhere equals the observed statistic exactly.  A row longer
 *   than a wave is walked 64 positions at a time; an empty row contributes nothing.
 *   No read outside Z: an entry of perms or col outside [0, n) is not followed (a bad pi_r(i) drops row i of permutation
 *   r, a bad col or pi_r(j) drops that edge) and *n_bad (one int64 on the device) is the number of such entries of perms
 *   and col, each counted once.  Row ranges are clamped to [0, nnz].  perms is not checked to hold permutations.
 *   workspace >= gpsa_autocorr_perm_workspace(n, P, R) bytes: the groups' partials, 8 G R P, and 2 KiB.
 *
 * GPSA_EINVAL: a NULL pointer (in_ptr / in_src with kind 0, col / w with nnz == 0 excepted), n, k, P or R < 1, nnz < 0,
 * an unknown kind or mode;  GPSA_EUNSUPPORTED: n or P >= 2^31, R > 16 * 65535;  GPSA_EWORKSPACE: a workspace that is NULL
 * or short.  Every check runs before the first launch. */
long long gpsa_graph_workspace(long long n);
int gpsa_graph_merge_count(const int* out, const long long* in_ptr, const int* in_src, long long n, int k, int kind,
                           long long* crow, void* stream);
int gpsa_graph_merge_write(const int* out, const long long* in_ptr, const int* in_src, long long n, int k, int kind,
                           int row_standardize, const long long* crow, long long nnz, int* col, double* w,
                           void* stream);
int gpsa_graph_check_f64(const long long* crow, const int* col, const double* w, long long n, long long nnz,
                         long long* out, void* workspace, long long workspace_bytes, void* stream);
int gpsa_graph_sums_f64(const long long* crow, const int* col, const double* w, const long long* tptr,
                        const long long* tperm, long long n, long long nnz, double* out, void* workspace,
                        long long workspace_bytes, void* stream);
long long gpsa_autocorr_perm_workspace(long long n, long long P, long long R);
int gpsa_autocorr_perm_f64(const double* Z, long long n, long long P, const long long* crow, const int* col,
                           const double* w, long long nnz, const int* perms, long long R, int mode, double* num,
                           long long* n_bad, void* workspace, long long workspace_bytes, void* stream);

/* ---- rigid pre-registration (csrc/register.hip): the score of K candidate transforms of slice B against slice A ---------
 * gpsa_rigid_scores_f64, D = 2: XA [m, 2] fp64 and YA [m, P] fp32 (slice A), XB [n, 2] fp64 and YB [n, P] fp32 (slice B),
 *   T [K, 6] fp64 (per candidate R row-major, then t), all row-major.  For candidate k and row i of B
 *     q_d = fma(R_d0, x0, fma(R_d1, x1, t_d)),   d2(j) = fma(u1, u1, fma(u0, u0, 0)) with u = q - XA[j] (gpsa_knn_f64's
 *   accumulation), a NaN d2 counted as +inf, and nn[k, i] = the row j of A with the smallest key (d2, j): ties in d2 to
 *   the lower index, a total order (a row of B with a NaN coordinate gets nn = 0, d2 = +inf).  Row i is MATCHED iff
 *   d2[k, i] <= max_d2, and
 *     sse[k] = sum_{i matched} sum_p (double(YB[i, p]) - double(YA[nn[k, i], p]))^2     fp64 [K]
 *     d2_sum[k] = sum_{i matched} d2[k, i]                                             fp64 [K]
 *     n_matched[k]                                                                     int64 [K]
 *   nn [K, n] int32 and d2 [K, n] fp64 are optional outputs (both or neither NULL; without them the tables live in the
 *   workspace).  One thread scans 8 candidates for one row of B per pass over A (A through LDS in tiles of 1024 rows,
 *   read as a broadcast); parts: slices of the A axis scanned by separate workgroups and merged by the same key, 0 = auto.
 *   The sums are fp64 in a fixed order: a workgroup per (candidate, row group), the row groups - ceil(n / max(32,
 *   ceil(n / 32))) of them, a function of n alone - added in ascending order.  No atomics, one writer per output element:
 *   candidate k's outputs depend on T[k] and (n, P) alone - the same bits whatever K, `parts`, the other rows of T or
 *   the call's repeat.  workspace >= gpsa_rigid_scores_workspace(n, m, K, P, parts, tables) bytes, tables != 0 when the
 *   caller passes nn / d2: 24 K G for the partials, 12 K n for the tables otherwise, 12 parts K n with parts > 1.
 *   GPSA_EINVAL: a NULL pointer (nn / d2 together excepted), n, m, K, P < 1, parts < 0, max_d2 negative, NaN or infinite;
 *   GPSA_EUNSUPPORTED: n or m >= 2^31, K > 65535, K n > 2^38;  GPSA_EWORKSPACE.  Every check runs before the first launch. */
long long gpsa_rigid_scores_workspace(long long n, long long m, long long K, int P, int parts, int tables);
int gpsa_rigid_scores_f64(const double* XA, const float* YA, long long m, const double* XB, const float* YB,
                          long long n, int P, const double* T, long long K, double max_d2, int parts, double* sse,
                          long long* n_matched, double* d2_sum, int* nn, double* d2, void* workspace,
                          long long workspace_bytes, void* stream);

/* ---- expression PCA (csrc/pca.hip): the covariance's Gram and the projection on the components ------------------------
 * What scanpy's sc.tl.pca / sklearn's PCA compute on the host before an alignment on a few components (the reference's
 * ST scripts select n_top_genes = 3000 and standardise per slice, experiments/expression/st/st_prediction.py); the
 * solver on top is built from gpsa_gemm and gpsa_chol_inv_f64 (pca.py).  Y [N, P] fp32 row-major; mean [V, P] and
 * inv_scale [V, P] fp64 on the device (inv_scale NULL: no scaling); view_off [V + 1] is a HOST array, 0 = view_off[0] <
 * ... < view_off[V] = N, as gpsa_column_moments_f32 takes it.  Both entries form
 *   z_ia = (double(y_ia) - mean[v(i), a]) * inv_scale[v(i), a]
 * in fp64 from the stored fp32 value as the operand is staged: no centred and no fp64 copy of Y exists.  The views are
 * walked one after the other (a launch per view), so no K chunk and no row block mixes two views' means.  fp64 sums in
 * a fixed order, no atomics, one writer per output element per launch, the same bits on a repeated call.
 * gpsa_pca_gram_f32: G [P, P] fp64 = sum_i z_ia z_ib on v_mfma_f64_16x16x4_f64, tiles of 64 x 64 columns, rows in chunks
 *   of 32.  Only tile pairs with column tile >= row tile are computed and every element (a <= b) is written to both
 *   places: G is symmetric to the bit.  A view's rows are cut into at most Gr = gpsa_pca_gram_groups(N, P) groups of
 *   ceil(ceil(n / Gr) / 32) * 32 rows whose partials are added in ascending order (views inside a group in view order);
 *   Gr = 1 once the ceil(P / 64) (ceil(P / 64) + 1) / 2 tile pairs are 256 or more, else min(32, ceil(256 / pairs),
 *   ceil(N / 32)): a function of (N, P) alone, not of the device.  workspace >= gpsa_pca_gram_workspace(N, P, V) bytes, a
 *   pure host query (0 for N, P or V < 1): 8 Gr P^2 for Gr > 1, and 0 for Gr = 1 (the partial is G itself; workspace may
 *   be NULL then).
 * gpsa_pca_project_f32: scores [N, k] = sum_a z_ia comp[j, a] with comp [k, P] fp64, k <= 128; fp64 accumulation on the
 *   MFMA pipe (the vector pipe forms z), Y read once; stored as fp32 rounded once (out_f64 = 0) or as fp64 (1).  A
 *   row's sum runs over the columns in one fixed order: the same bits whatever rows are passed together.
 * Refusals, all before the first launch and with nothing written: GPSA_EINVAL for a NULL pointer (inv_scale, and the
 * workspace when the query is 0, excepted), N < 2 (Gram) or N < 1 (projection), P < 1, P >= 2^21 (Gram) or 2^31, k outside
 * 1..128, out_f64 outside {0, 1}, V < 1, offsets that do not partition [0, N) or an empty view; GPSA_EWORKSPACE for a NULL
 * or short workspace when the query is not 0. */
int gpsa_pca_gram_groups(long long N, long long P);
long long gpsa_pca_gram_workspace(long long N, long long P, int V);
int gpsa_pca_gram_f32(const float* Y, long long N, long long P, const double* mean, const double* inv_scale,
                      const long long* view_off, int V, double* G, void* workspace, long long workspace_bytes,
                      void* stream);
int gpsa_pca_project_f32(const float* Y, long long N, long long P, const double* mean, const double* inv_scale,
                         const long long* view_off, int V, const double* comp, int k, void* scores, int out_f64,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPSA_HIP_H */
