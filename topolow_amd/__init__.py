"""topolow_amd -- MI355X-native relaxation path of topolow's `euclidean_embedding()`.

Public surface mirrors the reference's exports for this path (NAMESPACE:26,28 and the S3
methods NAMESPACE:9,12 of the reference): `euclidean_embedding`, `create_topolow_map`,
`print_topolow`, `summary_topolow`; the native step runs in libtopolow_relax.so (HIP,
gfx950) and there is no CPU fallback.
"""
from .core import (  # noqa: F401
    RMatrix,
    Topolow,
    create_topolow_map,
    euclidean_embedding,
    prepare_layout_call,
    print_topolow,
    summary_topolow,
)
from ._native import NativeError, options, set_seed  # noqa: F401
from .subsample import check_matrix_connectivity, subsample_dissimilarity_matrix  # noqa: F401
from .prune import analyze_network_structure, prune_sparse_matrix  # noqa: F401
from .spectrum import adjust_ndim_range, data_characteristics  # noqa: F401
from .error_metrics import (  # noqa: F401
    BinnedCloud,
    Density,
    EmbeddingQualityData,
    FitStatistics,
    bw_nrd0,
    calculate_prediction_interval,
    density_default,
    embedding_quality_data,
    error_calculator_comparison,
    fit_statistics,
)
from .velocity import default_bandwidths, kernel_velocity, silverman_bandwidth  # noqa: F401
from .reduce import (  # noqa: F401
    DimReductionConfig,
    pca_scores,
    reduce_dimensions,
    scale_to_original_distances,
    temporal_map_data,
)

__all__ = ["euclidean_embedding", "create_topolow_map", "print_topolow", "summary_topolow",
           "Topolow", "RMatrix", "options", "set_seed", "NativeError", "prepare_layout_call",
           "check_matrix_connectivity", "subsample_dissimilarity_matrix", "data_characteristics",
           "adjust_ndim_range", "analyze_network_structure", "prune_sparse_matrix", "error_calculator_comparison",
           "calculate_prediction_interval", "fit_statistics", "FitStatistics", "kernel_velocity",
           "silverman_bandwidth", "default_bandwidths", "DimReductionConfig", "pca_scores", "reduce_dimensions",
           "scale_to_original_distances", "temporal_map_data", "embedding_quality_data", "EmbeddingQualityData",
           "BinnedCloud", "Density", "density_default", "bw_nrd0"]
