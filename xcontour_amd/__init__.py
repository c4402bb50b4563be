# -*- coding: utf-8 -*-
"""
xcontour_amd -- MI355X (gfx950) implementation of the contour-coordinate hot path of
miniufo/xcontour behind the reference's own API (reference xcontour/__init__.py:2-6).

The cell-touching work (min/max, weighted multi-channel histogram with in-kernel
|grad q|^2, A(Yeq) row sums, local wave activity, the fused Keff pipeline) runs in
hand-written HIP kernels reached through the C ABI of include/xcontour_hip.h.
There is no CPU fallback.
"""
from .core import Contour2D, Table, find_contour, trace_contour, contour_polylines, coarsen, distance_to_contour, distance_profile
from .utils import equivalent_latitudes, latitude_lengths_at, cell_area, grad_metrics, \
    cartesian_metrics, Rearth, polyline_length, contour_area, fractal_dimension
from .labeled import DataArray, Dataset
from .ncio import open_dataset
from .pipeline import KeffPlan, shard_slabs
from ._native import Context, default_context, XContourHipError


def label_overlap(lab_a, lab_b, w=None, f=None):
    """The overlap of two label maps (K22, `Context.label_overlap` on the default context): numpy in, numpy out.  For callers
    that already hold two maps of `Contour2D.cal_contour_piece_labels`."""
    return default_context().label_overlap(lab_a, lab_b, w=w, f=f)


def map_to_plane(q, levels, values, dtype='float64'):
    """Per-contour vectors back on the plane (K25, `Context.contour_map` on the default context): numpy in, numpy out.  q (ny, nx)
    or (nslab, ny, nx); levels (N,) or (nslab, N); values: one vector, or a sequence of up to eight, each (N,) or (nslab, N).
    Returns np.interp(q, levels, vector) per slab -- the reference's _interp1d, decreasing levels included -- as one plane or a
    list of planes of q's shape.  For callers that hold bare arrays; labelled ones go through `Contour2D.map_to_plane`."""
    import numpy as np
    q = np.asarray(q)
    one = isinstance(values, np.ndarray) and values.ndim == 1
    out = default_context().contour_map(q[None] if q.ndim == 2 else q, levels, [values] if one else values, out_dtype=dtype)
    out = [p[0] for p in out] if q.ndim == 2 else out
    return out[0] if one else out


__version__ = "0.1.0"
