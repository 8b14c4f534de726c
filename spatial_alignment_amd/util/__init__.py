from .util import (  # noqa: F401
    ConvergenceChecker,
    LossNotDecreasingChecker,
    compute_distance,
    compute_size_factors,
    deviance_feature_selection,
    deviance_residuals,
    get_st_coordinates,
    pearson_residuals,
    poisson_deviance,
    polar_warp,
    rbf_kernel_numpy,
)
from ..image import scale_spatial_coords  # noqa: F401,E402  (the helper every script of the reference defines)
