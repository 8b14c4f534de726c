// LMC likelihood without F_obs on the matrix cores (round 5; vgpsa.py:428-432 F_obs = F_latent W, :532-538 the Gaussian
// likelihood; the VALU kernel of round 4 stays in elementwise.hip as the fallback).
//
// For an LMC modality the reference forms F_obs[s,n,:] = F_latent[s,n,:] W ([S,N,L] x [L,P]) and the likelihood, its
// gradient and the two LMC gradient products each stream that [S,N,P] tensor again (400 MB each way at BASELINE config
// 3).  One pass over (F_latent, W, Y) does all of it - per tile of 16 spots, sample s and 16 outputs p:
//     fobs = F W                (MFMA: rows c = the tile's spots, columns p, contraction over the L latent outputs)
//     r = Y - fobs;  z^2 += (r / sigma)^2;  dfo = -r / (sigma^2 S)                (on the accumulator registers)
//     dW[l, p] += sum_c F[c, l] dfo[c, p]   (MFMA: the dfo registers ARE the B operand - its K slot kq stands for spot
//                                            4 kq + step, which is how the accumulator holds them; accumulators live
//                                            across all tiles of the workgroup)
//     dF[c, l]  = sum_p dfo[c, p] W[l, p]   (MFMA: contraction over p, which runs across lanes in the accumulator
//                                            layout - the 16 x 16 dfo tile is transposed through a wave-private LDS
//                                            tile: 4 writes + 4 reads per lane, no barrier)
// Round 4's kernel did the three products on the vector pipe: 0.42 of config 3's 5.3 ms.  Here 12 NLT MFMAs per
// (16 spots, 16 outputs); the observations Y of a spot tile are read ONCE and reused for all S samples (the VALU kernel
// walked the S N columns and fetched Y[c mod N] S times: 400 MB instead of 80).
// Everything at upstream gradient 1 (the caller scales; linear).  Deterministic: fixed tile -> workgroup map, dW from
// per-workgroup partials summed in block order, dF written by the tile's owner.
#include "internal.hpp"

namespace gpsa {

typedef float lm_f32x4 __attribute__((ext_vector_type(4)));

// NLT: 16-row tiles of the latent outputs (L <= 16 NLT); NPT: 16-column tiles of the outputs per wave and chunk (a chunk
// = 64 NPT outputs: W's columns are walked in chunks so that its fragments and the dW accumulators stay in registers)
// (two workgroups per CU: 193 - 223 registers; left to itself the compiler took 272 and the kernel - two barriers and an LDS
//  staging per 96 MFMAs of a wave - ran one wave per SIMD at half the MFMA rate)
// SKIP (lmc_mfma_skip_kernel; gpsa_lmc_loglik_fused_skip_f32): a NaN in Y is a missing observation - its dfo and z are
// exactly 0 BEFORE the dW and dF products, so it adds nothing to either.  The two kernels include one body as text
// (lmc_body.hpp): the default kernel keeps its name and, instruction for instruction, its code
template <int NLT, int NPT>
__global__ void __launch_bounds__(256, 2)
lmc_mfma_kernel(const float* __restrict__ F, const float* __restrict__ W, const float* __restrict__ Y,
                const float* __restrict__ noise_u, int S, long long N, int L, int P, double* __restrict__ zpart,
                int nparts, float* __restrict__ dF, float* __restrict__ dWpart) {
  constexpr bool SKIP = false;
  constexpr int LIK = GPSA_LIK_GAUSSIAN;
  constexpr const float* log_offset = nullptr;  // (the Poisson kernel's argument)
  constexpr const float* log_disp = nullptr;    // (the NB kernel's arguments)
  constexpr double* upart = nullptr;
#include "lmc_body.hpp"
}
template <int NLT, int NPT>
__global__ void __launch_bounds__(256, 2)
lmc_mfma_skip_kernel(const float* __restrict__ F, const float* __restrict__ W, const float* __restrict__ Y,
                     const float* __restrict__ noise_u, int S, long long N, int L, int P, double* __restrict__ zpart,
                     int nparts, float* __restrict__ dF, float* __restrict__ dWpart) {
  constexpr bool SKIP = true;
  constexpr int LIK = GPSA_LIK_GAUSSIAN;
  constexpr const float* log_offset = nullptr;  // (the Poisson kernel's argument)
  constexpr const float* log_disp = nullptr;    // (the NB kernel's arguments)
  constexpr double* upart = nullptr;
#include "lmc_body.hpp"
}

// LIK = GPSA_LIK_POISSON (lmc_mfma_pois_kernel; gpsa_lmc_loglik_fused_pois_f32): F W is the log rate of count outputs;
// only the closing on the accumulator registers differs (lmc_body.hpp), the NaN select is the argument ``skip``
template <int NLT, int NPT>
__global__ void __launch_bounds__(256, 2)
lmc_mfma_pois_kernel(const float* __restrict__ F, const float* __restrict__ W, const float* __restrict__ Y,
                     const float* __restrict__ log_offset, int skip, int S, long long N, int L, int P,
                     double* __restrict__ zpart, int nparts, float* __restrict__ dF, float* __restrict__ dWpart) {
  constexpr int LIK = GPSA_LIK_POISSON;
  constexpr const float* noise_u = nullptr;  // (not read)
  const bool SKIP = skip != 0;
  constexpr const float* log_disp = nullptr;  // (the NB kernel's arguments)
  constexpr double* upart = nullptr;
#include "lmc_body.hpp"
}

// LIK = GPSA_LIK_NEGBIN (lmc_mfma_nb_kernel; gpsa_lmc_loglik_fused_nb_f32): F W is the log mean of count outputs with a
// dispersion per output (log_disp [P]); the closing also sums u per output into upart [G][P] (lmc_body.hpp)
template <int NLT, int NPT>
__global__ void __launch_bounds__(256, 2)
lmc_mfma_nb_kernel(const float* __restrict__ F, const float* __restrict__ W, const float* __restrict__ Y,
                   const float* __restrict__ log_offset, const float* __restrict__ log_disp, int skip, int S, long long N,
                   int L, int P, double* __restrict__ zpart, int nparts, float* __restrict__ dF,
                   float* __restrict__ dWpart, double* __restrict__ upart) {
  constexpr int LIK = GPSA_LIK_NEGBIN;
  constexpr const float* noise_u = nullptr;  // (not read)
  const bool SKIP = skip != 0;
#include "lmc_body.hpp"
}

static inline long long lmc_mfma_smem(int NLT, int NPT) {
  const int LT = 16 * NLT, PC = 64 * NPT;
  return (long long)(LT * (PC + 4) + 16 * (LT + 1) + 4 * 16 * 17 + 4 * LT * 17) * 4;
}

template <int NLT, int NPT, bool SKIP>
static int lmc_mfma_launch_t(const float* F, const float* W, const float* Y, const float* noise_u, int S, long long N,
                             int L, int P, double* zpart, int nparts, float* dF, float* dWpart, int G, hipStream_t st) {
  const int sm = (int)lmc_mfma_smem(NLT, NPT);
  static per_device_flag attr_flag;
  bool& attr_set = attr_flag.here();
  const void* fn = SKIP ? reinterpret_cast<const void*>(&lmc_mfma_skip_kernel<NLT, NPT>)
                        : reinterpret_cast<const void*>(&lmc_mfma_kernel<NLT, NPT>);
  if (!attr_set && sm > 65536) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, sm) != hipSuccess) return GPSA_EUNSUPPORTED;
    attr_set = true;
  }
  if (SKIP)
    lmc_mfma_skip_kernel<NLT, NPT><<<G, 256, (size_t)sm, st>>>(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, dWpart);
  else
    lmc_mfma_kernel<NLT, NPT><<<G, 256, (size_t)sm, st>>>(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, dWpart);
  GPSA_LAUNCH_CHECK();
  return 0;
}

// G workgroups (the caller's partial arrays have G rows); GPSA_EUNSUPPORTED: L > 64
int lmc_mfma_launch(const float* F, const float* W, const float* Y, const float* noise_u, int S, long long N, int L,
                    int P, double* zpart, int nparts, float* dF, float* dWpart, int G, hipStream_t st) {
  if (L <= 16) return lmc_mfma_launch_t<1, 8, false>(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  if (L <= 32) return lmc_mfma_launch_t<2, 4, false>(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  if (L <= 64) return lmc_mfma_launch_t<4, 2, false>(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  return GPSA_EUNSUPPORTED;
}
// ... with the NaN entries of Y left out (gpsa_lmc_loglik_fused_skip_f32)
int lmc_mfma_skip_launch(const float* F, const float* W, const float* Y, const float* noise_u, int S, long long N, int L,
                         int P, double* zpart, int nparts, float* dF, float* dWpart, int G, hipStream_t st) {
  if (L <= 16) return lmc_mfma_launch_t<1, 8, true>(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  if (L <= 32) return lmc_mfma_launch_t<2, 4, true>(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  if (L <= 64) return lmc_mfma_launch_t<4, 2, true>(F, W, Y, noise_u, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  return GPSA_EUNSUPPORTED;
}


template <int NLT, int NPT>
static int lmc_mfma_pois_launch_t(const float* F, const float* W, const float* Y, const float* log_offset, int skip, int S,
                                  long long N, int L, int P, double* zpart, int nparts, float* dF, float* dWpart, int G,
                                  hipStream_t st) {
  const int sm = (int)lmc_mfma_smem(NLT, NPT);
  static per_device_flag attr_flag;
  bool& attr_set = attr_flag.here();
  if (!attr_set && sm > 65536) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&lmc_mfma_pois_kernel<NLT, NPT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, sm) != hipSuccess)
      return GPSA_EUNSUPPORTED;
    attr_set = true;
  }
  lmc_mfma_pois_kernel<NLT, NPT><<<G, 256, (size_t)sm, st>>>(F, W, Y, log_offset, skip, S, N, L, P, zpart, nparts, dF,
                                                             dWpart);
  GPSA_LAUNCH_CHECK();
  return 0;
}
template <int NLT, int NPT>
static int lmc_mfma_nb_launch_t(const float* F, const float* W, const float* Y, const float* log_offset,
                                const float* log_disp, int skip, int S, long long N, int L, int P, double* zpart,
                                int nparts, float* dF, float* dWpart, double* upart, int G, hipStream_t st) {
  const int sm = (int)lmc_mfma_smem(NLT, NPT);
  static per_device_flag attr_flag;
  bool& attr_set = attr_flag.here();
  if (!attr_set && sm > 65536) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&lmc_mfma_nb_kernel<NLT, NPT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, sm) != hipSuccess)
      return GPSA_EUNSUPPORTED;
    attr_set = true;
  }
  lmc_mfma_nb_kernel<NLT, NPT><<<G, 256, (size_t)sm, st>>>(F, W, Y, log_offset, log_disp, skip, S, N, L, P, zpart, nparts,
                                                           dF, dWpart, upart);
  GPSA_LAUNCH_CHECK();
  return 0;
}
// ... for a negative binomial modality (gpsa_lmc_loglik_fused_nb_f32)
int lmc_mfma_nb_launch(const float* F, const float* W, const float* Y, const float* log_offset, const float* log_disp,
                       int skip, int S, long long N, int L, int P, double* zpart, int nparts, float* dF, float* dWpart,
                       double* upart, int G, hipStream_t st) {
  if (L <= 16)
    return lmc_mfma_nb_launch_t<1, 4>(F, W, Y, log_offset, log_disp, skip, S, N, L, P, zpart, nparts, dF, dWpart, upart, G, st);
  if (L <= 32)
    return lmc_mfma_nb_launch_t<2, 2>(F, W, Y, log_offset, log_disp, skip, S, N, L, P, zpart, nparts, dF, dWpart, upart, G, st);
  if (L <= 64)
    return lmc_mfma_nb_launch_t<4, 1>(F, W, Y, log_offset, log_disp, skip, S, N, L, P, zpart, nparts, dF, dWpart, upart, G, st);
  return GPSA_EUNSUPPORTED;
}
// ... for a Poisson modality (gpsa_lmc_loglik_fused_pois_f32)
int lmc_mfma_pois_launch(const float* F, const float* W, const float* Y, const float* log_offset, int skip, int S,
                         long long N, int L, int P, double* zpart, int nparts, float* dF, float* dWpart, int G,
                         hipStream_t st) {
  if (L <= 16) return lmc_mfma_pois_launch_t<1, 8>(F, W, Y, log_offset, skip, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  if (L <= 32) return lmc_mfma_pois_launch_t<2, 4>(F, W, Y, log_offset, skip, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  if (L <= 64) return lmc_mfma_pois_launch_t<4, 2>(F, W, Y, log_offset, skip, S, N, L, P, zpart, nparts, dF, dWpart, G, st);
  return GPSA_EUNSUPPORTED;
}

}  // namespace gpsa
