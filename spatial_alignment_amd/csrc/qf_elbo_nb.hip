// panel_elbo_nb_kernel: panel_elbo_kernel (qf_elbo.hip) with the negative binomial term in the closing
// (model.likelihood = "negative_binomial"; gpsa_quadform_elbo_nb_f32 / _delta_nb_f32): the draw is a log mean,
// a = F + log_offset[n] - log_disp[l].  A kernel of its own name over the shared body, as panel_elbo_pois_kernel is: the
// other kernels' instantiations and code stay what they are.  Besides g, dmeanT and the partial sums of t it writes u per
// element to u_elems [L, C], which the entry reduces per output.  The NaN select is governed by the argument ``skip``.
#include "qf_common.hpp"

namespace gpsa {

template <int MB, int NCT, int RL, bool FULLT, bool PAIRB>
__global__ void __launch_bounds__(256, elbo_wgs_per_cu(MB, NCT))
panel_elbo_nb_kernel(ElboArgs a, const float* __restrict__ log_offset, int skip, const float* __restrict__ log_disp,
                     float* __restrict__ u_elems) {
  constexpr int LIK = GPSA_LIK_NEGBIN;
  const bool SKIP = skip != 0;
#include "qf_elbo_body.hpp"
}

GPSA_ELBO_SHAPES(GPSA_ELBO_NB_DEFINE)
template __global__ void panel_elbo_nb_kernel<13, 2, 2, true, true>(ElboArgs, const float*, int, const float*, float*);
template __global__ void panel_elbo_nb_kernel<13, 2, 4, true, true>(ElboArgs, const float*, int, const float*, float*);

}  // namespace gpsa
