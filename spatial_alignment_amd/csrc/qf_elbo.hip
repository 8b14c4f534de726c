// panel_elbo_kernel: the data GP's forward, its Gaussian likelihood and the backward's abar in one pass over the
// products Omega_l alpha (the dominant kernel of the training step).
#include "qf_common.hpp"

namespace gpsa {

template <int MB, int NCT, int RL, bool FULLT, bool PAIRB>
__global__ void __launch_bounds__(256, elbo_wgs_per_cu(MB, NCT)) panel_elbo_kernel(ElboArgs a) {
  constexpr bool SKIP = false;
  constexpr int LIK = GPSA_LIK_GAUSSIAN;
  constexpr const float* log_offset = nullptr;  // (the Poisson kernel's argument)
  constexpr const float* log_disp = nullptr;    // (the NB kernel's arguments)
  constexpr float* u_elems = nullptr;
#include "qf_elbo_body.hpp"
}

GPSA_ELBO_SHAPES(GPSA_ELBO_DEFINE)
template __global__ void panel_elbo_kernel<13, 2, 2, true, true>(ElboArgs);
template __global__ void panel_elbo_kernel<13, 2, 4, true, true>(ElboArgs);

}  // namespace gpsa
