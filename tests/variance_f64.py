"""tests/variance_f32.py's formulas in float64: the reference the float32 results' rounding error is measured against. The decisions the
prose states on float32 inputs (bit-equal frames and cameras, finite inputs, the albedo threshold) are taken on the same float32 values."""
import numpy as np

import variance_f32


def reproject_moments(*args, **kwargs):
    return variance_f32.reproject_moments(*args, dtype=np.float64, **kwargs)


def spatial(*args, **kwargs):
    return variance_f32.spatial(*args, dtype=np.float64, **kwargs)


def atrous_variance_filter(*args, **kwargs):
    return variance_f32.atrous_variance_filter(*args, dtype=np.float64, **kwargs)
