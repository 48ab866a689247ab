"""Feature-based affine registration (counterpart of microaligner/feature_reg) and the intensity-based refinement of its
matrix."""
from .direct_affine import DirectAffineInfo, align_affine
from .feature_registrator import FeatureRegistrator

__all__ = ["FeatureRegistrator", "align_affine", "DirectAffineInfo"]
