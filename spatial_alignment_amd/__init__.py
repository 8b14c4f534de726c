"""GPSA (Gaussian Process Spatial Alignment) training hot path for AMD MI355X (gfx950).

Same public names as the reference package (gpsa/__init__.py:1-10) for the parts on the hot path.
"""
from .autocorr import SpatialGraph, fdr_bh, spatial_autocorr, spatial_graph
from .counts import (
    CSRCounts,
    column_moments,
    count_stats,
    csr_counts,
    densify,
    deviance_feature_selection,
    deviance_residuals,
    highly_variable_genes,
    normalize_log1p,
    pearson_residuals,
    poisson_deviance,
    prepare_counts,
    size_factors,
    standardize_views,
)
from .gpr import GPRegression, gp_regress, prediction_baselines
from .image import Frame, ImagePixels, histology_modality, image_pixels, scale_spatial_coords, warp_image
from .kernels import matern12_kernel, matern32_kernel, rbf_kernel
from .models import GPSA, VariationalGPSA
from .neighbors import alignment_score, knn, knn_regress, kth_neighbor_distance, moran_i, spatial_r2
from .ot import OTAlignment, ot_align, paste_baseline, stack_slices
from .parallel import fit
from .pca import ExpressionPCA, expression_pca, init_lmc_from_pca
from .predict import predict
from .register import RigidRegistration, prealign_slices, rigid_register, rigid_scores
from .util import (
    ConvergenceChecker,
    LossNotDecreasingChecker,
    get_st_coordinates,
    polar_warp,
    rbf_kernel_numpy,
)
from .warp import transfer, unwarp, warp_field

__all__ = [
    "GPSA",
    "VariationalGPSA",
    "rbf_kernel",
    "matern12_kernel",
    "matern32_kernel",
    "rbf_kernel_numpy",
    "polar_warp",
    "get_st_coordinates",
    "LossNotDecreasingChecker",
    "ConvergenceChecker",
    "fit",
    "predict",
    "warp_field",
    "unwarp",
    "transfer",
    "knn",
    "knn_regress",
    "spatial_r2",
    "kth_neighbor_distance",
    "moran_i",
    "alignment_score",
    "spatial_graph",
    "SpatialGraph",
    "spatial_autocorr",
    "fdr_bh",
    "count_stats",
    "size_factors",
    "poisson_deviance",
    "deviance_feature_selection",
    "pearson_residuals",
    "deviance_residuals",
    "normalize_log1p",
    "standardize_views",
    "prepare_counts",
    "csr_counts",
    "CSRCounts",
    "densify",
    "column_moments",
    "highly_variable_genes",
    "gp_regress",
    "GPRegression",
    "prediction_baselines",
    "ot_align",
    "OTAlignment",
    "stack_slices",
    "paste_baseline",
    "Frame",
    "scale_spatial_coords",
    "image_pixels",
    "ImagePixels",
    "histology_modality",
    "warp_image",
    "rigid_scores",
    "rigid_register",
    "RigidRegistration",
    "prealign_slices",
    "expression_pca",
    "ExpressionPCA",
    "init_lmc_from_pca",
]
__version__ = "0.1.0"
