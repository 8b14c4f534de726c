"""alias of the reference's ``gpsa.util`` (gpsa/util/__init__.py:1 exports ``rbf_kernel_numpy``)"""
from spatial_alignment_amd.util.util import (  # noqa: F401
    compute_size_factors,
    deviance_feature_selection,
    deviance_residuals,
    pearson_residuals,
    poisson_deviance,
    rbf_kernel_numpy,
)
