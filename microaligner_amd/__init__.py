"""microaligner_amd -- MI355X-native implementation of microaligner's optical-flow registration
hot path (OptFlowRegistrator.register() + Warper.warp()) behind the reference's Python API.

    from microaligner_amd import OptFlowRegistrator, Warper

mirrors `from microaligner import OptFlowRegistrator, Warper` (microaligner/__init__.py:18-20).
Compute runs in hand-written HIP kernels for gfx950 behind a C-ABI (include/microaligner_hip.h);
there is no CPU fallback.
"""
from .feature_reg import FeatureRegistrator, align_affine, DirectAffineInfo, align_translation, TranslationInfo
from .optflow_reg import OptFlowRegistrator, TileFlowCalc, Warper, farneback, compose_flows, merge_two_flows, \
    invert_flow, transform_points, FlowGrid, FlowGridError, compress_flow, flow_grid_error, smooth_flow, fold_mask, \
    repair_flow, fit_flow_affine, split_flow, join_flow, local_affine, FlowAffineInfo, FlowAffineMaps, \
    refine_flow, FlowRefineInfo, LandmarkFit, fit_landmarks, landmark_flow, landmark_points, median_flow, outlier_mask, \
    MedianInfo, fill_flow, FillInfo
from .shared_modules.registration_qc import FlowQC, RegistrationQC, assess_registration, flow_qc
from .shared_modules.residual_shift import ResidualShift, ShiftMaps, residual_shift
from .shared_modules.texture import TextureMaps, texture_maps
from .shared_modules.local_correlation import CorrelationMaps, local_correlation
from .shared_modules.normalize import LocalNormInfo, NormalizeInfo, normalize_local, normalize_percentile
from .shared_modules.morphology import grey_close, grey_dilate, grey_erode, grey_open, tophat
from .shared_modules.components import ComponentInfo, fill_holes, label_components, remove_small_objects
from .shared_modules.utils import max_project_and_normalize, pad_to_shape, transform_img_with_tmat

__all__ = ["FeatureRegistrator", "OptFlowRegistrator", "Warper", "TileFlowCalc", "farneback", "merge_two_flows", "compose_flows", "invert_flow", "transform_points", "pad_to_shape",
           "transform_img_with_tmat", "max_project_and_normalize", "assess_registration", "flow_qc", "RegistrationQC", "FlowQC",
           "residual_shift", "ResidualShift", "ShiftMaps", "FlowGrid", "FlowGridError", "compress_flow", "flow_grid_error",
           "smooth_flow", "fold_mask", "repair_flow", "fit_flow_affine", "split_flow", "join_flow", "local_affine", "FlowAffineInfo",
           "FlowAffineMaps", "texture_maps", "TextureMaps", "align_affine", "DirectAffineInfo", "refine_flow", "FlowRefineInfo",
           "LandmarkFit", "fit_landmarks", "landmark_flow", "landmark_points", "align_translation", "TranslationInfo",
           "normalize_percentile", "NormalizeInfo", "local_correlation", "CorrelationMaps", "median_flow", "outlier_mask",
           "MedianInfo", "fill_flow", "FillInfo", "normalize_local", "LocalNormInfo",
           "grey_erode", "grey_dilate", "grey_open", "grey_close", "tophat",
           "label_components", "remove_small_objects", "fill_holes", "ComponentInfo"]
__version__ = "0.1.0"
