// panel_elbo_pois_kernel: panel_elbo_kernel (qf_elbo.hip) with the Poisson term in the closing (model.likelihood;
// gpsa_quadform_elbo_pois_f32 / _delta_pois_f32): the draw is a log rate, eta = F + log_offset[n].  A kernel of its own
// name over the shared body, as panel_elbo_skip_kernel is: the Gaussian kernels' instantiations and code stay what they
// are.  The NaN select is governed by the argument ``skip`` (one kernel for both settings of model.skip_missing).
#include "qf_common.hpp"

namespace gpsa {

template <int MB, int NCT, int RL, bool FULLT, bool PAIRB>
__global__ void __launch_bounds__(256, elbo_wgs_per_cu(MB, NCT))
panel_elbo_pois_kernel(ElboArgs a, const float* __restrict__ log_offset, int skip) {
  constexpr int LIK = GPSA_LIK_POISSON;
  const bool SKIP = skip != 0;
  constexpr const float* log_disp = nullptr;  // (the NB kernel's arguments)
  constexpr float* u_elems = nullptr;
#include "qf_elbo_body.hpp"
}

GPSA_ELBO_SHAPES(GPSA_ELBO_POIS_DEFINE)
template __global__ void panel_elbo_pois_kernel<13, 2, 2, true, true>(ElboArgs, const float*, int);
template __global__ void panel_elbo_pois_kernel<13, 2, 4, true, true>(ElboArgs, const float*, int);

}  // namespace gpsa
