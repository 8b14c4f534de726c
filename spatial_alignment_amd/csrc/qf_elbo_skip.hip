// panel_elbo_skip_kernel: panel_elbo_kernel (qf_elbo.hip) with the NaN entries of Y left out of the likelihood
// (model.skip_missing; gpsa_quadform_elbo_skip_f32 / _delta_skip_f32).  A kernel of its own name over the shared body:
// the default kernels' instantiations and code stay what they are.
#include "qf_common.hpp"

namespace gpsa {

template <int MB, int NCT, int RL, bool FULLT, bool PAIRB>
__global__ void __launch_bounds__(256, elbo_wgs_per_cu(MB, NCT)) panel_elbo_skip_kernel(ElboArgs a) {
  constexpr bool SKIP = true;
  constexpr int LIK = GPSA_LIK_GAUSSIAN;
  constexpr const float* log_offset = nullptr;  // (the Poisson kernel's argument)
  constexpr const float* log_disp = nullptr;    // (the NB kernel's arguments)
  constexpr float* u_elems = nullptr;
#include "qf_elbo_body.hpp"
}

GPSA_ELBO_SHAPES(GPSA_ELBO_SKIP_DEFINE)
template __global__ void panel_elbo_skip_kernel<13, 2, 2, true, true>(ElboArgs);
template __global__ void panel_elbo_skip_kernel<13, 2, 4, true, true>(ElboArgs);

}  // namespace gpsa
