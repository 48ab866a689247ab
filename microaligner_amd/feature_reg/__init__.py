"""Feature-based affine registration (counterpart of microaligner/feature_reg), the intensity-based refinement of its
matrix and the global translation search that stands in where it finds nothing."""
from .direct_affine import DirectAffineInfo, align_affine
from .feature_registrator import FeatureRegistrator
from .translation import TranslationInfo, align_translation

__all__ = ["FeatureRegistrator", "align_affine", "DirectAffineInfo", "align_translation", "TranslationInfo"]
