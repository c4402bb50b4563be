# -*- coding: utf-8 -*-
"""
ctypes binding of libxcontour_hip.so (C ABI: include/xcontour_hip.h).

There is NO CPU fallback: if the shared library is missing or no gfx950 device
is visible, every compute entry point raises.  `load()` only dlopen()s the
library (works on a GPU-less build box so that symbol / ABI checks can run);
`Context()` is what needs the device.
"""
import contextlib
import copy
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('XC_LIB_PATH') or os.path.join(_HERE, 'libxcontour_hip.so')   # XC_LIB_PATH: diagnostic builds only

XC_OK, XC_EBADARG, XC_EEDGES, XC_EHIP, XC_ENOMEM, XC_ENODEV = 0, -1, -2, -3, -4, -5
XC_F32, XC_F64 = 0, 1
XC_DA_NONE, XC_DA_ROW, XC_DA_PLANE, XC_DA_SLAB = 0, 1, 2, 3
XC_EDGE_NUMPY, XC_EDGE_XHISTOGRAM = 0, 1
XC_SINGLE_AUTO, XC_SINGLE_NEVER, XC_SINGLE_FORCE = 0, 1, 2
XC_MAX_INTEGRANDS = 2
MAX_SLABS_PER_LAUNCH = 65535
XC_PAD_EDGE, XC_PAD_WRAP, XC_PAD_NAN, XC_PAD_REFLECT, XC_PAD_SYMMETRIC = 0, 1, 2, 3, 4
XC_CSEG_GROUP_LEVELS = 2048      # contours one level group of K12 holds (include/xcontour_hip.h)
PAD_MODES = {'edge': XC_PAD_EDGE, 'wrap': XC_PAD_WRAP, 'constant': XC_PAD_NAN, 'reflect': XC_PAD_REFLECT,
             'symmetric': XC_PAD_SYMMETRIC}

_vp, _i32, _i64, _u64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double


class HistDesc(C.Structure):
    """struct xc_hist_desc (include/xcontour_hip.h)"""
    _fields_ = [
        ('q', _vp), ('q_dtype', _i32), ('dA_pos_finite', _i32),
        ('nslab', _i64), ('ny', _i64), ('nx', _i64),
        ('edges', _vp), ('nedge', _i64), ('edges_per_slab', _i32), ('last_closed', _i32),
        ('dA', _vp), ('dA_rank', _i32), ('prod_f32', _i32),
        ('nint', _i32), ('grad', _i32),
        ('integrand', _vp * XC_MAX_INTEGRANDS),
        ('integrand_dtype', _i32 * XC_MAX_INTEGRANDS),
        ('rdx', _vp), ('rdy', _vp),
        ('periodic_x', _i32), ('lt', _i32),
        ('reverse', _i32), ('negate', _i32),
        ('pdf', _vp), ('counts', _vp), ('cdf', _vp),
        ('deterministic', _i32), ('reserved0', _i32),
    ]


class CommInfo(C.Structure):
    """struct xc_comm_info_t (include/xcontour_hip.h)"""
    _fields_ = [('comm_count', _i32), ('comm_rank', _i32), ('comm_device', _i32), ('ctx_device', _i32),
                ('rccl_version', _i32), ('reserved0', _i32), ('rccl_path', C.c_char * 256)]


class HistVariant(C.Structure):
    """xc_hist_variant: the histogram instantiation and geometry the last xc_hist / xc_keff_dev call launched"""
    _fields_ = [(n, _i32) for n in ('kernel', 'q_dtype', 'vec', 'nint', 'grad', 'da2d', 'next', 'fast', 'e32', 'det', 'wcnt',
                                    'threads', 'ncopy', 'nstrip', 'bps', 'xcd_map', 'nchunk', 'G', 'cps', 'rpc')]


HIST_KERNELS = {0: None, 1: 'K3', 2: 'K3-det', 3: 'K3S'}


class ClenGeometry(C.Structure):
    """xc_clen_geometry: how the last xc_contour_lengths(_dev) call launched K10"""
    _fields_ = [('q_dtype', _i32), ('latlon', _i32), ('N', _i32), ('ncopy', _i32), ('G', _i32), ('ngroup', _i32),
                ('ntile', _i64), ('bps', _i32), ('bps_rule', _i32), ('nslab', _i64)]


class CscaleGeometry(C.Structure):
    """xc_cscale_geometry: how the last xc_coarsen(_dev) / xc_contour_lengths_scales(_dev) call launched k_coarsen, ratio by ratio"""
    _fields_ = [('q_dtype', _i32), ('nratio', _i32), ('block', _i32), ('ratio', _i32 * 8), ('grid_x', _i32 * 8), ('grid_y', _i32 * 8),
                ('grid_z', _i32 * 8), ('tile_y', _i32 * 8), ('tile_x', _i32 * 8)]


CLEN_BPS_RULES = {0: None, 1: 'share', 2: 'floor', 3: 'capacity', 4: 'ntile'}


class KeffDesc(C.Structure):
    """struct xc_keff_desc (include/xcontour_hip.h)"""
    _fields_ = [
        ('q', _vp), ('q_dtype', _i32), ('ctr_dtype', _i32),
        ('nslab', _i64), ('ny', _i64), ('nx', _i64),
        ('N', _i32), ('increase', _i32), ('lt', _i32), ('right_edge', _i32),
        ('dA', _vp), ('dA_rank', _i32), ('grad', _i32),
        ('grdS', _vp), ('grdS_dtype', _i32), ('prod_f32', _i32),
        ('rdx', _vp), ('rdy', _vp), ('periodic_x', _i32), ('npre', _i32),
        ('tbl', _vp), ('tbl_coord', _vp), ('preY', _vp),
        ('nkeff_mask', _f64), ('lmin_scale', _f64),
        ('ctr', _vp), ('area', _vp), ('intgrdS', _vp), ('latEq', _vp),
        ('dqdA', _vp), ('dintSdA', _vp), ('Leq2', _vp), ('Lmin', _vp), ('nkeff', _vp),
        ('counts', _vp), ('interp', _vp), ('status', _vp), ('q_next', _vp),
        ('dA_pos_finite', _i32), ('q_gen', _i32),
        ('deterministic', _i32), ('out_stride', _i32),
        ('dA_max', _f64),
        ('single_read', _i32), ('reserved0', _i32),
    ]


# name -> (restype, argtypes): every symbol include/xcontour_hip.h declares
PROTOTYPES = {
    'xc_create': (C.c_int, [C.c_int, C.POINTER(_vp)]),
    'xc_destroy': (C.c_int, [_vp]),
    'xc_last_error': (C.c_char_p, [_vp]),
    'xc_version': (C.c_char_p, []),
    'xc_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'xc_device_name': (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    'xc_device_cus': (C.c_int, [_vp, C.POINTER(C.c_int)]),
    'xc_sync': (C.c_int, [_vp]),
    'xc_stream': (_vp, [_vp]),
    'xc_trace': (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    'xc_malloc': (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    'xc_free': (C.c_int, [_vp, _vp]),
    'xc_memcpy_h2d': (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    'xc_memcpy_d2h': (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    'xc_memset': (C.c_int, [_vp, _vp, C.c_int, C.c_size_t]),
    'xc_memcpy_h2d_async': (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    'xc_stream_wait_copies': (C.c_int, [_vp]),
    'xc_keep_resident': (C.c_int, [_vp, _vp, C.c_size_t]),
    'xc_release_resident': (C.c_int, [_vp, _vp]),
    'xc_resident_lookup': (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(_vp)]),
    'xc_copies_wait_stream': (C.c_int, [_vp]),
    'xc_event_create': (C.c_int, [_vp, C.POINTER(_vp)]),
    'xc_event_destroy': (C.c_int, [_vp, _vp]),
    'xc_event_record': (C.c_int, [_vp, _vp]),
    'xc_event_elapsed_ms': (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_float)]),
    'xc_event_record_copies': (C.c_int, [_vp, _vp]),
    'xc_event_query': (C.c_int, [_vp, _vp, C.POINTER(C.c_int)]),
    'xc_minmax_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _vp]),
    'xc_minmax': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _vp]),
    'xc_levels_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    'xc_levels': (C.c_int, [_vp, _vp, C.c_int, _i64, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    'xc_contours': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    'xc_hist_dev': (C.c_int, [_vp, C.POINTER(HistDesc)]),
    'xc_hist': (C.c_int, [_vp, C.POINTER(HistDesc)]),
    'xc_rowsum_dev': (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _i64, _i64, C.c_int, _vp]),
    'xc_rowsum': (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _i64, _i64, C.c_int, _vp]),
    'xc_grad2_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, C.c_int, _vp]),
    'xc_grad2': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, C.c_int, _vp]),
    'xc_lwa_dev': (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _f64, _vp, C.c_int,
                             _i64, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp]),
    'xc_lwa': (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _f64, _vp, C.c_int,
                         _i64, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp]),
    'xc_crossing_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, C.c_int, C.c_int, _vp, C.c_int, C.c_int,
                                  _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    'xc_crossing': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, C.c_int, C.c_int, _vp, C.c_int, C.c_int,
                              _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    'xc_contour_lengths_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _vp, C.c_int, C.c_int, _vp, _vp]),
    'xc_contour_lengths': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _vp, C.c_int, C.c_int, _vp, _vp]),
    'xc_contour_line_integrals_dev': (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _f64, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    'xc_contour_line_integrals': (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _f64, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    'xc_local_contour_lengths_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    'xc_local_contour_lengths': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    # the periodic forms: the same lists with `double period` after xcoord
    'xc_contour_lengths_periodic_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _f64, _vp, C.c_int, C.c_int, _vp, _vp]),
    'xc_contour_lengths_periodic': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _f64, _vp, C.c_int, C.c_int, _vp, _vp]),
    'xc_local_contour_lengths_periodic_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _f64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    'xc_local_contour_lengths_periodic': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _f64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    'xc_contour_segments_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, C.c_int, C.c_int, _i64, _vp, _vp, _vp, _vp]),
    'xc_contour_segments': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, C.c_int, C.c_int, _i64, _vp, _vp, _vp, _vp]),
    'xc_contour_segments_periodic_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, C.c_int, C.c_int, _i64, _vp, _vp, _vp, _vp]),
    'xc_contour_segments_periodic': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, C.c_int, C.c_int, _i64, _vp, _vp, _vp, _vp]),
    'xc_join_segments': (C.c_int, [_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_contour_pieces_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, _vp, _vp, _f64, _f64, _i64,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_contour_polylines_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_last_cjoin_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_contour_overturning_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_last_coverturn_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_contour_interior_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int,
                                          _vp, C.c_int, _vp, _vp, _vp, _vp]),
    'xc_last_cinterior_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_contour_folds_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _i64,
                                       _vp, _vp, _vp, _vp, _i64, _vp] + [_vp] * 11),
    'xc_last_cfold_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_contour_distance_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, _vp, _vp, _f64, _f64, _f64,
                                          _vp, _vp, _vp, _vp]),
    'xc_set_cdist_prune': (C.c_int, [_vp, C.c_int]),
    'xc_last_cdist_profile': (C.c_int, [_vp, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(C.c_int)]),
    'xc_contour_distance_profile_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, _vp, _vp, _f64, _f64, _f64,
                                                  _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_set_cdprofile_global': (C.c_int, [_vp, C.c_int]),
    'xc_last_cdprofile_profile': (C.c_int, [_vp, _vp] + [C.POINTER(_i64)] * 4 + [C.POINTER(C.c_int)]),
    'xc_contour_map_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int]),
    'xc_contour_map': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int]),
    'xc_contour_piece_interiors_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, C.c_int,
                                                 _vp, C.c_int, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_last_cpinside_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_contour_piece_tree_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, C.c_int,
                                            _vp, C.c_int, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_last_cptree_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_contour_piece_labels_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, C.c_int,
                                              _vp, C.c_int, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                              _vp]),
    'xc_last_cplabel_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_contour_piece_props_dev': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, C.c_int,
                                             _vp, C.c_int, _i64] + [_vp] * 14 + [C.c_int, _vp, _vp, _vp, _vp, C.c_int] + [_vp] * 6),
    'xc_last_cpprops_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_label_overlap_dev': (C.c_int, [_vp, _i64, _i64, _i64, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _i64, _vp, _vp, _vp, _vp,
                                       _vp, _vp]),
    'xc_last_cpoverlap_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_ring_tracks_dev': (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp]),
    'xc_last_cptrack_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int)]),
    'xc_set_cpiece_workspace': (C.c_int, [_vp, _u64]),
    'xc_last_cpiece_profile': (C.c_int, [_vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'xc_sort_profile_dev': (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _i64, _i64, C.c_int, _vp, C.c_int,
                                      _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'xc_sort_profile': (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _i64, _i64, C.c_int, _vp, C.c_int,
                                  _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'xc_sort_profile_batch_dev': (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _i64, _i64, _i64, C.c_int,
                                            _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'xc_sort_profile_batch': (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _i64, _i64, _i64, C.c_int,
                                        _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'xc_last_sort_path': (C.c_int, [_vp, C.POINTER(C.c_int)]),
    'xc_last_keff_path': (C.c_int, [_vp, C.POINTER(C.c_int)]),
    'xc_dbg_single_stamps': (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_int)]),
    'xc_set_lwa_exact': (C.c_int, [_vp, C.c_int]),
    'xc_last_lwa_path': (C.c_int, [_vp, C.POINTER(C.c_int)]),
    'xc_keff_dev': (C.c_int, [_vp, C.POINTER(KeffDesc)]),
    'xc_keff_epilogue_dev': (C.c_int, [_vp, _vp, _vp, C.c_int, _i64, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int,
                                       C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_keff_epilogue': (C.c_int, [_vp, _vp, _vp, C.c_int, _i64, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int,
                                   C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'xc_host_gradient_wrt_area': (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _i64, _i64, _i64, _i64, _i64, _vp]),
    'xc_host_edges_from_levels': (C.c_int, [_vp, C.c_int, _i64, _i64, C.c_int, _vp, C.POINTER(C.c_int)]),
    'xc_set_kernel_timing': (C.c_int, [_vp, C.c_int]),
    'xc_last_hist_ms': (C.c_int, [_vp, C.POINTER(C.c_float)]),
    'xc_last_hist_variant': (C.c_int, [_vp, C.POINTER(HistVariant)]),
    'xc_last_clen_geometry': (C.c_int, [_vp, C.POINTER(ClenGeometry)]),
    'xc_coarsen_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, C.c_int, C.c_int, _vp]),
    'xc_coarsen': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, C.c_int, C.c_int, _vp]),
    'xc_contour_lengths_scales_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _f64, _vp, C.c_int, C.c_int,
                                                _vp, C.c_int, C.c_int, _vp, _vp]),
    'xc_contour_lengths_scales': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _f64, _f64, _vp, C.c_int, C.c_int,
                                            _vp, C.c_int, C.c_int, _vp, _vp]),
    'xc_last_cscale_geometry': (C.c_int, [_vp, C.POINTER(CscaleGeometry)]),
    'xc_set_hist_events': (C.c_int, [_vp, _vp, _vp]),
    'xc_comm_unique_id': (C.c_int, [_vp, _vp]),
    'xc_comm_init': (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    'xc_comm_create': (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, C.POINTER(_vp), C.c_char_p, C.c_size_t]),
    'xc_comm_attach': (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    'xc_comm_release': (C.c_int, [_vp]),
    'xc_comm_info': (C.c_int, [_vp, _vp]),
    'xc_comm_allgather_dev': (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    'xc_comm_finalize': (C.c_int, [_vp]),
    'xc_comm_gather_dev': (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int]),
    'xc_comm_abort': (C.c_int, [_vp]),
    'xc_comm_wait_compute': (C.c_int, [_vp]),
    'xc_compute_wait_comm': (C.c_int, [_vp]),
    'xc_comm_memcpy_d2d': (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    'xc_streams_idle': (C.c_int, [_vp, C.POINTER(C.c_int)]),
    'xc_ipc_export': (C.c_int, [_vp, _vp, _vp]),
    'xc_ipc_open': (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    'xc_ipc_close': (C.c_int, [_vp, _vp]),
    'xc_device_can_access_peer': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    'xc_synth_dev': (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _i64, _vp, _vp, _u64, C.c_int]),
}

_lib = None


class XContourHipError(Exception):
    """Raised for every non-zero status of the C ABI (the reference raises bare
    `Exception`, core.py:53-57, 1233-1251; this subclasses it)."""

    def __init__(self, code, msg):
        Exception.__init__(self, msg)
        self.code = code


def load():
    """dlopen the in-tree library and attach prototypes.  Raises (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XContourHipError(
            XC_ENODEV,
            'xcontour_amd: %s not found -- build it with `python -c "import '
            '__graft_entry__ as g; g.build()"` or `make -C xcontour_amd/csrc`. '
            'There is no CPU fallback.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_DT_CODES = {np.dtype(np.float32): XC_F32, np.dtype(np.float64): XC_F64}


def dtype_code(dt):
    c = _DT_CODES.get(dt)                                        # (a np.dtype instance: the usual argument)
    if c is None:
        c = _DT_CODES.get(np.dtype(dt))
        if c is None:
            raise XContourHipError(XC_EBADARG, 'unsupported dtype %s (float32/float64 only)' % np.dtype(dt))
    return c


def _ptr(a):
    """Host address of a C-contiguous ndarray (or None): an int, which ctypes takes for a void* argument or field.  The CALLER keeps the
    array alive until the library call has returned (every entry point here holds its arrays in locals)."""
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data


def _contig(a, dtype=None):
    """np.ascontiguousarray without the call when there is nothing to do"""
    if type(a) is np.ndarray and a.flags.c_contiguous and (dtype is None or a.dtype == dtype):
        return a
    return np.ascontiguousarray(a, dtype=dtype)


def _is_lazy(q):
    """a labeled.LazyStack (or anything with its protocol): (S, ny, nx) shape / dtype known, slabs read on `q[s0:s1]`"""
    return bool(getattr(q, '_xc_lazy_stack', False))


def _stack_in(q):
    return q if _is_lazy(q) else _contig(q)


def _stack_now(q, s0, s1):
    """slabs [s0, s1) of a stack, about to be staged on the device: a lazy stack is read now (this one batch, nothing more)"""
    if _is_lazy(q):
        return np.ascontiguousarray(q[s0:s1])
    return q if s1 - s0 == q.shape[0] else q[s0:s1]


def _check_period(period, xcoord, what):
    """the period of a periodic X direction (K10, K11) as a float, checked against the host coordinates: finite, non-zero, of the
    sign of xcoord[-1] - xcoord[0] and longer than that span; the ring needs two columns"""
    period = float(period)
    span = float(xcoord[-1] - xcoord[0]) if xcoord.size >= 2 else 0.0
    if (xcoord.size < 2 or not np.isfinite(period) or period == 0.0 or period * span < 0.0 or not abs(period) > abs(span)):
        raise XContourHipError(XC_EBADARG, '%s: period must be finite, non-zero, of the sign of xcoord[nx-1] - xcoord[0] and longer '
                               'than that span, and nx >= 2' % what)
    return period


def _part(a, slab_ndim, s0, s1):
    """what batch [s0, s1) sees of an argument: its own slabs when the argument rides on the slab axis (it has `slab_ndim` dims, the
    first of them the slabs), all of it when every slab shares it (fewer dims, or None)"""
    return a[s0:s1] if a is not None and a.ndim == slab_ndim else a


def _join(parts):
    """the results of the batches of one call, in order -> the result of the call: ndarrays are joined along axis 0 (the slabs), a
    tuple / list / dict is joined member by member (so is the list over strides of `crossing`), None stays None"""
    p0 = parts[0]
    if p0 is None:
        return None
    if isinstance(p0, dict):
        return {k: _join([p[k] for p in parts]) for k in p0}
    if isinstance(p0, (tuple, list)):
        return type(p0)(_join([p[i] for p in parts]) for i in range(len(p0)))
    return np.concatenate(parts)


def _f48(a):
    """float32 / float64 arrays as they are, anything else as float64"""
    return a if a.dtype in _DT_CODES else a.astype(np.float64)


def _weight_rank(shape, ny, nx, nslab=None, text=None):
    """XC_DA_* of a weight array from its shape: (ny,) / (ny, nx) / (nslab, ny, nx) -- the last only for callers that take per-slab
    weights (they pass `nslab`).  Any other shape raises the caller's own complaint `text` (callers without one asserted)"""
    if shape == (ny,):
        return XC_DA_ROW
    if shape == (ny, nx):
        return XC_DA_PLANE
    if nslab is not None and shape == (nslab, ny, nx):
        return XC_DA_SLAB
    if text is None:
        raise AssertionError()
    raise XContourHipError(XC_EBADARG, text)


def _check_ascending(contours, who):
    """the host entry points validate the contours; the device ones trust their caller"""
    if np.isnan(contours).any() or (np.diff(contours, axis=-1) < 0).any():
        raise XContourHipError(XC_EEDGES, '%s: contours must be ascending without NaN' % who)


def _check_map_levels(levels):
    """the levels of K25 as its host form checks them: per slab finite and strictly monotonic in the direction of the ends; a slab
    with a NaN end (an all-NaN tracer's) is let through"""
    x = levels.reshape(-1, levels.shape[-1])
    x = x[~(np.isnan(x[:, 0]) | np.isnan(x[:, -1]))]
    d = np.diff(x, axis=1)
    if (d == 0).any():
        raise XContourHipError(XC_EEDGES, 'non monotonic bins')
    up = (x[:, :1] < x[:, -1:])
    if not np.isfinite(x).all() or not np.where(up, d > 0, d < 0).all():
        raise XContourHipError(XC_EBADARG, 'xc_contour_map: the levels of every slab must be finite and strictly monotonic')


def _stack3(q):
    """a stack as the contour calls take it (an array, or a lazy stack) -> (the stack, (nslab, ny, nx))"""
    q = _stack_in(q)
    if len(q.shape) != 3:
        raise XContourHipError(XC_EBADARG, 'q must be (nslab, ny, nx)')
    return q, tuple(q.shape)


def _levels_of(contours, nslab):
    """the contours of K10 / K12 / K13 -> (contiguous float64, per-slab flag, N): (N,) or (nslab, N), N >= 1"""
    contours = _contig(contours, np.float64)
    per_slab = contours.ndim == 2
    if contours.ndim not in (1, 2) or (per_slab and contours.shape[0] != nslab) or contours.shape[-1] < 1:
        raise XContourHipError(XC_EBADARG, 'contours must be (N,) or (nslab, N)')
    return contours, per_slab, contours.shape[-1]


def _plane_coords(ycoord, xcoord, ny, nx, who):
    """the coordinates of rows / columns -> contiguous float64 (ny,) / (nx,)"""
    ycoord, xcoord = _contig(ycoord, np.float64), _contig(xcoord, np.float64)
    if ycoord.shape != (ny,) or xcoord.shape != (nx,):
        raise XContourHipError(XC_EBADARG, '%s: coordinates of length (%d, %d) for a (%d, %d) plane'
                               % (who, ycoord.size, xcoord.size, ny, nx))
    return ycoord, xcoord


def _check_finite(who, *coords):
    if not all(np.isfinite(c).all() for c in coords):
        raise XContourHipError(XC_EBADARG, '%s: coordinates must be finite' % who)


def _lengths_open(q, contours, ycoord, xcoord, period, who, period_who=None, shaped=None):
    """what K10, K15 and K26 open with, every refusal under the name it has in that form (`period_who`: the period's, where it is
    another; shaped(shape): the form's own refusal behind the stack's, K15's integrand) -> (the stack, its shape, the levels,
    per_slab, N, ycoord, xcoord, the checked period or None)"""
    q, shape = _stack3(q)
    if shaped is not None:
        shaped(shape)
    contours, per_slab, N = _levels_of(contours, shape[0])
    ycoord, xcoord = _plane_coords(ycoord, xcoord, shape[1], shape[2], who)
    if period is not None:
        _check_finite(who, xcoord)
        period = _check_period(period, xcoord, period_who or who)
    return q, shape, contours, per_slab, N, ycoord, xcoord, period


def _lengths_trusted(who, cb, ycoord, xcoord):
    """what the device forms of K10, K15 and K26 trust their caller with, for a batch's levels `cb`: the checks, in their order"""
    return (lambda: _check_ascending(cb, who), lambda: _check_finite(who, ycoord, xcoord))


def _scan(counts):
    """counts of any shape and integer type -> (the counts, their exclusive scan -- where every range starts in the packed
    order): both flat int64"""
    c = counts.ravel().astype(np.int64)
    return c, np.cumsum(c) - c


def _range_of(counts):
    """the range every record lies in, for records packed range by range (`counts` of them in each)"""
    return np.repeat(np.arange(counts.size), counts.ravel().astype(np.int64))


def _range_order(counts, key):
    """the order that sorts records packed range by range (`counts` of them in each) by `key` inside every range"""
    return np.lexsort((key, _range_of(counts)))


def _row_map(pc, first_edge):
    """The pieces of one batch as the device packed them, `pc` of them in each range -> (order, rows): `order` sorts every range
    by first_edge (the order of the tables); rows[p] is the row, counted from the start of its range, that packed position p
    has in its range's sorted table.  Whatever the device gives as an index into its packed order -- a parent, a label, the
    rings of an overlap pair -- becomes a row of the tables through `rows` (`_to_rows`)."""
    c, start = _scan(pc)
    order = _range_order(pc, first_edge)
    where = np.empty(order.size, dtype=np.int64)
    where[order] = np.arange(order.size)
    return order, where - np.repeat(start, c)


def _to_rows(idx, start, rows):
    """in place: every index >= 0 of `idx` counts inside its range's packed order, which begins at `start` (a scalar, or an array
    that broadcasts against `idx`) of the positions `rows` (`_row_map`) covers -> the row in the range's sorted table"""
    has = idx >= 0
    idx[has] = rows[(idx + start)[has]]


def _named(src, dtype, names=None):
    """the structured array `src` as one of `dtype`: every field of `src` goes to the field of its name -- of names[its name]
    where `names` renames it --, or nowhere when `dtype` has none; the fields of `dtype` beyond those are the caller's to fill"""
    out = np.empty(src.shape, dtype=dtype)
    for k in src.dtype.names:
        to = names.get(k, k) if names else k
        if to in out.dtype.names:
            out[to] = src[k]
    return out


def _row_bytes(cols):
    """bytes one entry takes in every column of `cols` together (`_Columns`)"""
    return sum(np.dtype(c[1]).itemsize * (c[2] if len(c) > 2 else 1) for c in cols)


class _Columns(object):
    """A block of columns in one device buffer: `cols` = [(name, dtype[, width]), ...] lie one behind the other in that order,
    each of `cap` entries (a column of `width` w: w sub-columns of `cap` entries).  From this one description come the
    addresses an entry point is given and the download into a structured array."""

    def __init__(self, buf, cap, cols):
        self.buf, self.at, self.type = buf, {}, {}
        off = 0
        for c in cols:
            self.at[c[0]], self.type[c[0]] = off, c[1]
            off += cap * _row_bytes([c])
        assert off <= buf.nbytes

    def ptr(self, name, wanted=True):
        """the device address of a column (None when the caller does not want it filled)"""
        return self.buf.ptr + self.at[name] if wanted else None

    def ptrs(self, names):
        return [self.buf.ptr + self.at[k] for k in names]

    def get(self, name, shape):
        return self.buf.download(shape, self.type[name], offset_bytes=self.at[name])

    def into(self, out, skip=()):
        """the first out.size entries of every column that is a field of the structured array `out` (but those of `skip`)"""
        for k in out.dtype.names:
            if k not in skip:
                out[k] = self.get(k, out.shape)
        return out


OVERTURN_SELECT = {'all': 0, 'circumpolar': 1, 'main': 2}       # how K16 / K17 select pieces: the names and the library's codes
XC_PROPS_MAXF = 8                                               # fields one K21 call takes (include/xcontour_hip.h)
XC_CMAP_MAXV = 8                                                # value vectors one K25 call takes
XC_CMAP_MAX_LDS_DOUBLES = 8192                                  # K25: (nv + 1) * N may not exceed this
XC_CMAP_TILE = 1024                                             # K25: cells a workgroup takes per step
XC_CSCALE_MAXR = 8                                              # ratios one K26 call takes
XC_CSCALE_MAXRATIO = 64                                         # K26: the largest coarsening ratio
XC_CDIST_RING = float(np.float64(np.deg2rad(np.float32(360.0))))   # K27: the one period of a sphere, float64(deg2rad(float32(360)))
XC_CDPROFILE_MAX_EDGES = 4097                                   # K28: the most bin edges one call takes
_UNSET = object()


class _RecordArgs(object):
    """The one argument check of the calls that run on K12's records (K12, K14, K16 - K23), and what it made of the arguments.  The
    caller names what applies to it.  The checks run in the order written here -- the stack and its levels (`plane`), then the
    weights and fields --, which is the order a call with two defects reports them in; a caller that reports a bad w or f first
    gives `shape` = (nslab, ny, nx) alone and calls `plane` itself afterwards.  q, contours: the stack and its levels ((N,) or
    (nslab, N), ascending); select: K16's, by name or code; periodic with min_nx 2 or 3: the ring's fewest columns; labels32:
    the plane must fit 32-bit edge labels; w, f: the weight and the integrand; fields, x: K21's.
    Attributes: q, contours, N, nslab, ny, nx, sel, periodic, w, f, fields, x, as the batches take them (contiguous, f32 / f64)."""

    def __init__(self, who, q=None, contours=None, shape=None, select=_UNSET, periodic=False, min_nx=0, labels32=False, w=None,
                 f=None, fields=(), x=None):
        self.who, self.periodic = who, periodic
        self.q = self.contours = self.N = self.sel = None
        if q is not None:
            self.plane(q, contours, select, periodic, min_nx, labels32)
        else:
            self.nslab, self.ny, self.nx = shape
        who, nslab, ny, nx = self.who, self.nslab, self.ny, self.nx
        if w is not None:
            w = _contig(w, np.float64)
            if w.shape not in ((ny, nx), (nslab, ny, nx)):
                raise XContourHipError(XC_EBADARG, '%s: w must be (ny, nx) or (nslab, ny, nx)' % who)
        if f is not None:
            f = _contig(_f48(np.asarray(f)))
            if f.shape != (nslab, ny, nx):
                raise XContourHipError(XC_EBADARG, '%s: f must be (nslab, ny, nx)' % who)
        if len(fields) > XC_PROPS_MAXF:
            raise XContourHipError(XC_EBADARG, '%s: %d fields, at most %d (XC_PROPS_MAXF)' % (who, len(fields), XC_PROPS_MAXF))
        fields = [_contig(_f48(np.asarray(a))) for a in fields]
        if any(a.shape not in ((ny, nx), (nslab, ny, nx)) for a in fields):
            raise XContourHipError(XC_EBADARG, '%s: a field must be (ny, nx) or (nslab, ny, nx)' % who)
        if x is not None:
            x = _contig(_f48(np.asarray(x)))
            if x.shape != (nslab, ny, nx):
                raise XContourHipError(XC_EBADARG, '%s: x must be (nslab, ny, nx)' % who)
        self.w, self.f, self.fields, self.x = w, f, fields, x

    def plane(self, q, contours, select=_UNSET, periodic=False, min_nx=0, labels32=False):
        """the stack, its levels and what the plane must satisfy"""
        who = self.who
        self.q, (self.nslab, ny, nx) = _stack3(q)
        self.ny, self.nx, self.periodic = ny, nx, periodic
        self.contours, _, self.N = _levels_of(contours, self.nslab)
        _check_ascending(self.contours, who)
        if _UNSET is not select:
            self.sel = sel = OVERTURN_SELECT.get(select, select) if isinstance(select, str) else select
            if isinstance(sel, bool) or sel not in (0, 1, 2):
                raise XContourHipError(XC_EBADARG, '%s: select is \'all\', \'circumpolar\' or \'main\' (0, 1, 2), not %r' % (who, select))
            if sel != 0 and not periodic:
                raise XContourHipError(XC_EBADARG, '%s: select=%r needs periodic=True (no piece goes round a plain plane)' % (who, select))
        if periodic and nx < min_nx:
            raise XContourHipError(XC_EBADARG, 'xc_contour_segments_periodic: nx >= 2' if min_nx == 2 else
                                   '%s: a periodic plane needs nx >= 3' % who)
        if labels32 and 2 * ny * nx >= 1 << 31:
            raise XContourHipError(XC_EBADARG, '%s: plane too large for 32-bit labels (2 ny nx < 2^31)' % who)

    def on(self, q, contours):
        """the same plane, weights and fields under another stack of the same shape and its (checked) levels"""
        _check_ascending(contours, self.who)
        other = copy.copy(self)
        other.q, other.contours = q, contours
        return other

    def batch(self, s0, s1):
        """what the batch of slabs [s0, s1) stages: (q -- a lazy stack is read now --, contours, w, f, fields, x)"""
        return (_stack_now(self.q, s0, s1), _part(self.contours, 2, s0, s1), _part(self.w, 3, s0, s1), _part(self.f, 3, s0, s1),
                [_part(a, 3, s0, s1) for a in self.fields], _part(self.x, 3, s0, s1))

    def slab_bytes(self, more=0):
        """the bytes one slab stages: per node the tracer, what of w, f, the fields and x rides on the slab axis, and `more`"""
        per = sum(a.dtype.itemsize for a in [self.q, self.w, self.f, self.x] + self.fields if a is not None and len(a.shape) == 3)
        return self.ny * self.nx * (per + more)


def join_segments(off, e_from, e_to):
    """xc_join_segments (host only, no device): the directed segments of `Context.contour_segments` joined into polylines.  off
    (nrange + 1,) int64, the exclusive scan of the counts; e_from / e_to (total,) int64.  Returns (order (total,) int64: segment
    indices polyline by polyline in walk order; poly_off (npoly + 1,) int64 into `order`; closed (npoly,) bool; range_poly_off
    (nrange + 1,) int64: the polylines of range r are [range_poly_off[r], range_poly_off[r+1])).  A duplicate e_from or e_to
    within a range raises."""
    off, e_from, e_to = _contig(off, np.int64), _contig(e_from, np.int64), _contig(e_to, np.int64)
    if off.ndim != 1 or off.size < 1 or e_from.ndim != 1 or e_from.shape != e_to.shape or int(off[-1]) != e_from.size:
        raise XContourHipError(XC_EBADARG, 'xc_join_segments: off must be (nrange + 1,) and end at the number of segments')
    total = e_from.size
    order, poly_off = np.empty(total, dtype=np.int64), np.empty(total + 1, dtype=np.int64)
    closed, rpo = np.empty(total, dtype=np.uint8), np.empty(off.size, dtype=np.int64)
    rc = load().xc_join_segments(off.size - 1, _ptr(off), _ptr(e_from), _ptr(e_to), _ptr(order), _ptr(poly_off), _ptr(closed), _ptr(rpo))
    if rc != XC_OK:
        raise XContourHipError(rc, 'xc_join_segments: off must start at 0 and ascend, and no edge id may repeat among the e_from or '
                               'among the e_to of a range')
    npoly = int(rpo[-1])
    return order, poly_off[:npoly + 1].copy(), closed[:npoly].astype(bool), rpo


class DeviceBuffer(object):
    """A device allocation owned by a Context (freed with the context or explicitly)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = _vp()
        ctx._check(ctx.lib.xc_malloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p.value
        ctx._buffers.append(self)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.xc_memcpy_h2d(self.ctx.handle, self.ptr, _ptr(arr), arr.nbytes))
        return self

    def upload_async(self, arr, offset_bytes=0):
        """copy on the context's copy stream (overlaps kernels already enqueued); pair with Context.stream_wait_copies()"""
        arr = np.ascontiguousarray(arr)
        assert offset_bytes + arr.nbytes <= self.nbytes
        # lifetime rule: the source must stay alive until the copy has run.  Pageable sources make hipMemcpyAsync return
        # after the copy today, but that is how the runtime behaves, not a promise (and a pinned source returns at once):
        # the context holds a reference until an event recorded on the copy stream behind this copy has completed
        ctx = self.ctx
        ctx._reap_staged()
        ctx._check(ctx.lib.xc_memcpy_h2d_async(ctx.handle, self.ptr + offset_bytes, _ptr(arr), arr.nbytes))
        ev = ctx._ev_pool.pop() if ctx._ev_pool else ctx.event()
        ctx._check(ctx.lib.xc_event_record_copies(ctx.handle, ev))
        ctx._staged.append((arr, ev))
        return self

    def download(self, shape, dtype, offset_bytes=0):
        out = np.empty(shape, dtype=dtype)
        assert offset_bytes + out.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.xc_memcpy_d2h(self.ctx.handle, _ptr(out), self.ptr + offset_bytes, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.xc_free(self.ctx.handle, self.ptr)
            self.ptr = None
            if self in self.ctx._buffers:
                self.ctx._buffers.remove(self)


class _DeviceView(object):
    """`nbytes` bytes of a DeviceBuffer from `offset_bytes` on, for a call that takes a buffer (`ptr`, `upload`); the owner frees"""

    def __init__(self, buf, offset_bytes, nbytes):
        assert 0 <= offset_bytes and offset_bytes + nbytes <= buf.nbytes
        self.ctx, self.ptr, self.nbytes = buf.ctx, buf.ptr + int(offset_bytes), int(nbytes)

    upload = DeviceBuffer.upload


class Context(object):
    """One HIP device + stream (xc_create / xc_destroy)."""

    def __init__(self, device=0):
        self.lib = load()
        h = _vp()
        rc = self.lib.xc_create(int(device), C.byref(h))
        if rc != XC_OK:
            raise XContourHipError(rc, (self.lib.xc_last_error(None) or b'').decode())
        self.handle = h
        self.device = int(device)
        self._buffers = []
        self._resident = {}          # data pointer -> ndarray registered with xc_keep_resident (kept alive here)
        self._staged = []            # (host array, event) of asynchronous uploads in flight (DeviceBuffer.upload_async): dropped once the event has completed
        self._ev_pool = []           # recycled events of completed uploads
        # host-pointer entry points stage at most this many bytes of per-slab data (tracer, integrands, per-slab weights,
        # per-slab outputs) on the device at once: larger stacks go through in batches of whole slabs (the reference's
        # histogram path is lazy / dask-friendly, core.py:158-160, 241-246)
        self.max_batch_bytes = int(os.environ.get('XC_MAX_BATCH_BYTES', 8 << 30))

    # -- plumbing
    def _check(self, rc):
        if rc != XC_OK:
            raise XContourHipError(rc, (self.lib.xc_last_error(self.handle) or b'').decode())

    def close(self):
        if getattr(self, 'handle', None):
            # the per-upload events (in flight and recycled): wait for the copy stream, then destroy them (round-5 advisor: they leaked)
            try:
                self.lib.xc_stream_wait_copies(self.handle)
                self.lib.xc_sync(self.handle)
            except Exception:
                pass
            for ev in [e for _, e in self._staged] + list(self._ev_pool):
                self.lib.xc_event_destroy(self.handle, ev)
            self._staged, self._ev_pool = [], []
            for b in list(self._buffers):
                b.free()
            self.lib.xc_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        """wait for the COMPUTE stream.  Uploads in flight on the copy stream are not waited for (a download of batch k must not
        stand behind the upload of batch k + 1): work that needs them says so with stream_wait_copies() before it is enqueued"""
        self._check(self.lib.xc_sync(self.handle))
        self._reap_staged()

    def _reap_staged(self):
        """drop the host arrays of asynchronous uploads whose copy has completed (an event per upload, polled: never blocks)"""
        if not self._staged:
            return
        keep, done = [], C.c_int()
        for arr, ev in self._staged:
            self._check(self.lib.xc_event_query(self.handle, ev, C.byref(done)))
            if done.value:
                self._ev_pool.append(ev)
            else:
                keep.append((arr, ev))
        self._staged = keep

    def stream_wait_copies(self):
        self._check(self.lib.xc_stream_wait_copies(self.handle))

    # -- resident inputs: host arrays with a device mirror (xc_keep_resident)
    def keep_resident(self, arr):
        """upload `arr` (C-contiguous ndarray) once; host-form calls whose input is this array -- or whole leading-index slices of
        it -- read the device mirror from now on.  The context keeps a reference to `arr` while it is registered (its memory
        cannot be recycled under the mirror); do not modify it in place without calling keep_resident again."""
        assert isinstance(arr, np.ndarray) and arr.flags['C_CONTIGUOUS']
        self._check(self.lib.xc_keep_resident(self.handle, _ptr(arr), arr.nbytes))
        self._resident[arr.ctypes.data] = arr
        return arr

    def release_resident(self, arr=None):
        if not getattr(self, 'handle', None):
            return
        if arr is None:
            self._check(self.lib.xc_release_resident(self.handle, None))
            self._resident.clear()
        elif arr.ctypes.data in self._resident:
            self._check(self.lib.xc_release_resident(self.handle, _ptr(arr)))
            del self._resident[arr.ctypes.data]

    def resident_ptr(self, arr):
        """device address of the mirror of `arr` (a C-contiguous ndarray, or a leading-index slice of a registered one), or None"""
        if not self._resident:
            return None
        p = _vp()
        self._check(self.lib.xc_resident_lookup(self.handle, _ptr(arr), arr.nbytes, C.byref(p)))
        return p.value

    def copies_wait_stream(self):
        self._check(self.lib.xc_copies_wait_stream(self.handle))

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._check(self.lib.xc_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def device_cus(self):
        n = C.c_int()
        self._check(self.lib.xc_device_cus(self.handle, C.byref(n)))
        return n.value

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, max(arr.nbytes, 1)).upload(arr)

    def event(self):
        e = _vp()
        self._check(self.lib.xc_event_create(self.handle, C.byref(e)))
        return e

    def record(self, ev):
        self._check(self.lib.xc_event_record(self.handle, ev))

    def elapsed_ms(self, e0, e1):
        ms = C.c_float()
        self._check(self.lib.xc_event_elapsed_ms(self.handle, e0, e1, C.byref(ms)))
        return ms.value

    def _last_int(self, fn):
        p = C.c_int()
        self._check(fn(self.handle, C.byref(p)))
        return p.value

    def last_sort_path(self):
        """K8, last call: 0 key passes only, 1 the three range-key passes sufficed, 2 they failed the check (re-sorted)"""
        return self._last_int(self.lib.xc_last_sort_path)

    def last_keff_path(self):
        """last xc_keff_dev call: 0 the min/max + histogram + finalize chain, 1 the single-read kernel (calls of one or two slabs)"""
        return self._last_int(self.lib.xc_last_keff_path)

    def last_lwa_path(self):
        """K7, last call: 0 band walk (bit-exact), 1 the O(ny log ny) interval kernel, 2 its premises failed the check"""
        return self._last_int(self.lib.xc_last_lwa_path)

    def _last_record(self, fn, rec, named, names, live):
        """a launch record as a dict of its fields: `named` through `names`, 'q_dtype' a numpy dtype -- None when `live` is unset"""
        self._check(fn(self.handle, C.byref(rec)))
        out = {f[0]: getattr(rec, f[0]) for f in rec._fields_}
        out[named] = names[out[named]]
        out['q_dtype'] = np.dtype(np.float32 if out['q_dtype'] == XC_F32 else np.float64) if out[live] else None
        return out

    def last_hist_variant(self):
        """the histogram kernel of the last hist / keff call and how it was launched (xc_last_hist_variant): a dict of the record's
        fields, 'kernel' named ('K3', 'K3-det', 'K3S'; None after a failed call) and 'q_dtype' a numpy dtype"""
        return self._last_record(self.lib.xc_last_hist_variant, HistVariant(), 'kernel', HIST_KERNELS, 'kernel')

    def last_clen_geometry(self):
        """how the last contour_lengths / contour_line_integrals call (its last batch) launched K10 / K15 (xc_last_clen_geometry): a dict of the record's fields,
        'bps_rule' named ('share', 'floor', 'capacity', 'ntile'; None when the plane has no cells) and 'q_dtype' a numpy dtype (None
        after a failed call: then every field is 0)"""
        return self._last_record(self.lib.xc_last_clen_geometry, ClenGeometry(), 'bps_rule', CLEN_BPS_RULES, 'N')

    def last_cscale_geometry(self):
        """how the last coarsen / contour_lengths_scales call (its last batch) launched k_coarsen (xc_last_cscale_geometry): a dict
        with 'q_dtype' (None after a failed call: then everything is 0), 'block' and, per ratio in the caller's order, the lists
        'ratio', 'grid' ((x, y, z) workgroups; zeros for a ratio of 1 inside contour_lengths_scales) and 'tile' ((rows, columns)
        of coarse nodes one workgroup takes)"""
        rec = CscaleGeometry()
        self._check(self.lib.xc_last_cscale_geometry(self.handle, C.byref(rec)))
        n = rec.nratio
        return {'q_dtype': (np.dtype(np.float32 if rec.q_dtype == XC_F32 else np.float64) if n else None), 'block': rec.block,
                'ratio': list(rec.ratio[:n]), 'grid': [(rec.grid_x[k], rec.grid_y[k], rec.grid_z[k]) for k in range(n)],
                'tile': [(rec.tile_y[k], rec.tile_x[k]) for k in range(n)]}

    def single_stamps(self, enable=True):
        """diagnostics: (device pointer, slots) of the single-read kernel's phase stamps; enable=False frees them"""
        ptr, n = _vp(), C.c_int()
        self._check(self.lib.xc_dbg_single_stamps(self.handle, 1 if enable else 0, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def set_kernel_timing(self, on):
        self._check(self.lib.xc_set_kernel_timing(self.handle, 1 if on else 0))

    def set_hist_events(self, e0, e1):
        self._check(self.lib.xc_set_hist_events(self.handle, e0, e1))

    def last_hist_ms(self):
        ms = C.c_float()
        self._check(self.lib.xc_last_hist_ms(self.handle, C.byref(ms)))
        return ms.value

    # -- the one collective (RCCL)
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        self._check(self.lib.xc_comm_unique_id(self.handle, buf))
        return bytes(buf.raw)

    def comm_init(self, nranks, rank, uid):
        assert len(uid) == 128
        self._check(self.lib.xc_comm_init(self.handle, int(nranks), int(rank), C.create_string_buffer(uid, 128)))

    def comm_create(self, nranks, rank, uid):
        """ncclCommInitRank WITHOUT touching this context (safe in a helper thread under a deadline): returns the communicator handle
        for `comm_attach`, raises with RCCL's text otherwise"""
        assert len(uid) == 128
        h, err = _vp(), C.create_string_buffer(512)
        rc = self.lib.xc_comm_create(self.device, int(nranks), int(rank), C.create_string_buffer(uid, 128), C.byref(h), err, 512)
        if rc != 0:
            raise XContourHipError(rc, err.value.decode('utf-8', 'replace') or 'xc_comm_create failed (%d)' % rc)
        return h.value

    def comm_attach(self, comm, nranks, rank):
        self._check(self.lib.xc_comm_attach(self.handle, comm, int(nranks), int(rank)))

    def comm_release(self, comm):
        self.lib.xc_comm_release(comm)

    def comm_info(self):
        """what RCCL itself reports about this context's communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice /
        ncclGetVersion + the file it was loaded from); comm_count 0: no RCCL communicator here"""
        i = CommInfo()
        self._check(self.lib.xc_comm_info(self.handle, C.byref(i)))
        return {'comm_count': i.comm_count, 'comm_rank': i.comm_rank, 'comm_device': i.comm_device, 'ctx_device': i.ctx_device,
                'rccl_version': i.rccl_version, 'rccl_path': i.rccl_path.decode('utf-8', 'replace')}

    def comm_allgather(self, send_ptr, recv_ptr, bytes_per_rank):
        self._check(self.lib.xc_comm_allgather_dev(self.handle, send_ptr, recv_ptr, int(bytes_per_rank)))

    def comm_finalize(self):
        self._check(self.lib.xc_comm_finalize(self.handle))

    def comm_gather(self, send_ptr, nbytes, recv_ptr, rank_stride, root=0):
        """gather to `root` over RCCL (grouped ncclSend / ncclRecv) on the comm stream: rank r's block lands at recv + r * rank_stride"""
        self._check(self.lib.xc_comm_gather_dev(self.handle, send_ptr, int(nbytes), recv_ptr, int(rank_stride), int(root)))

    def comm_abort(self):
        self._check(self.lib.xc_comm_abort(self.handle))

    # -- the comm stream (blocks leave while the next launch set computes) and the HIP IPC carrier
    def comm_wait_compute(self):
        self._check(self.lib.xc_comm_wait_compute(self.handle))

    def compute_wait_comm(self):
        self._check(self.lib.xc_compute_wait_comm(self.handle))

    def comm_memcpy_d2d(self, dst_ptr, src_ptr, nbytes):
        self._check(self.lib.xc_comm_memcpy_d2d(self.handle, dst_ptr, src_ptr, int(nbytes)))

    def streams_idle(self):
        v = C.c_int()
        self._check(self.lib.xc_streams_idle(self.handle, C.byref(v)))
        return bool(v.value)

    def sync_within(self, seconds, poll=0.002):
        """wait for the compute and comm streams like sync(), but give up after `seconds`: True when they drained"""
        import time
        t_end = time.time() + float(seconds)
        while not self.streams_idle():
            if time.time() > t_end:
                return False
            time.sleep(poll)
        return True

    def ipc_export(self, ptr):
        buf = C.create_string_buffer(64)
        self._check(self.lib.xc_ipc_export(self.handle, ptr, buf))
        return bytes(buf.raw)

    def ipc_open(self, handle):
        assert len(handle) == 64
        p = _vp()
        self._check(self.lib.xc_ipc_open(self.handle, C.create_string_buffer(handle, 64), C.byref(p)))
        return p.value

    def ipc_close(self, ptr):
        self._check(self.lib.xc_ipc_close(self.handle, ptr))

    # -- host-pointer compute entry points (numpy in, numpy out)
    def _batches(self, nslab, per_slab_bytes):
        """[(s0, s1), ...]: the slab axis cut into equal batches of whole slabs whose staged bytes stay below
        `max_batch_bytes` (and below the 65535 slabs one launch takes); one batch if everything fits"""
        b = max(1, min(int(nslab), MAX_SLABS_PER_LAUNCH, int(self.max_batch_bytes) // max(1, int(per_slab_bytes))))
        return [(s0, min(int(nslab), s0 + b)) for s0 in range(0, int(nslab), b)]

    def _batched(self, nslab, per_slab_bytes, one):
        """the batching of every host-form call: the slab axis is cut into batches of whole slabs (`_batches`) from the bytes a slab
        stages, `one(s0, s1)` does the batch of slabs [s0, s1) -- it is what reads a lazy stack -- and the results of the batches, run
        in order, are joined along the slab axis (`_join`)"""
        bt = self._batches(nslab, per_slab_bytes)
        if len(bt) <= 1:
            return one(0, nslab)
        return _join([one(s0, s1) for s0, s1 in bt])

    @contextlib.contextmanager
    def _temporaries(self, inputs, out_nbytes):
        """device copies of `inputs` and allocations of `out_nbytes` bytes for one call of a `_dev` entry point (freed on the way out)"""
        bufs = [self.to_device(a) for a in inputs] + [self.alloc(n) for n in out_nbytes]
        try:
            yield bufs
        finally:
            for b in bufs:
                b.free()

    def _twin(self, f_host, f_dev, qb, inputs, outs, args, checks=()):
        """One batch of a call that has a host form and a `_dev` twin with the same argument list.  qb: the batch of the tracer;
        inputs: the further arrays in argument order (an absent optional one is None and stays None); outs: (shape, dtype) of every
        output; args(tracer pointer, input pointers, output pointers) -> the arguments behind the handle, stated once for both forms.
        A tracer with a device mirror is read in place: `checks` -- what the host form checks itself (xc_forms.hip, the same texts)
        and the device form leaves to its caller -- are run, the inputs, then the outputs, are staged on the device, `f_dev` is called
        and the outputs come down from device memory.  Else `f_host` gets host pointers.  Returns the outputs, a list."""
        qp = self._mirror(qb)
        if not qp:
            res = [np.empty(shape, dtype=t) for shape, t in outs]
            self._check(f_host(self.handle, *args(_ptr(qb), [_ptr(a) for a in inputs], [_ptr(o) for o in res])))
            return res
        for check in checks:
            check()
        there = [a for a in inputs if a is not None]
        with self._temporaries(there, [int(np.prod(shape, dtype=np.int64)) * np.dtype(t).itemsize for shape, t in outs]) as bufs:
            din, dout = iter(bufs[:len(there)]), bufs[len(there):]
            ins = [None if a is None else next(din).ptr for a in inputs]
            self._check(f_dev(self.handle, *args(qp, ins, [b.ptr for b in dout])))
            return [b.download(shape, t) for b, (shape, t) in zip(dout, outs)]

    def _minmax_of(self, q):
        nslab = q.shape[0]
        out = np.empty((nslab, 2), dtype=np.float64)
        self._check(self.lib.xc_minmax(self.handle, _ptr(q), dtype_code(q.dtype), nslab,
                                       int(q.size // nslab), _ptr(out)))
        return out

    def minmax(self, q):
        """q: (nslab, ny, nx) or (nslab, ncell) f32/f64 -> (nslab, 2) f64"""
        q = _stack_in(q)
        nslab = q.shape[0]
        return self._batched(nslab, q.nbytes // max(1, nslab), lambda s0, s1: self._minmax_of(_stack_now(q, s0, s1)))

    def contours(self, q, N, increase, ctr_dtype, right_edge=XC_EDGE_XHISTOGRAM, want_minmax=False):
        """cal_contours(int) in one call (xc_contours): q (nslab, ny, nx) -> levels (nslab, N) float64 [, minmax (nslab, 2)]"""
        q = _stack_in(q)
        nslab = q.shape[0]

        def one(s0, s1):
            if s1 - s0 < nslab or _is_lazy(q):                   # a part of the stack (or a lazy one): its min/max alone, the
                return None, self._minmax_of(_stack_now(q, s0, s1))      # levels follow from the joined min/max below
            ctr = np.empty((nslab, N), dtype=np.float64)
            mm = np.empty((nslab, 2), dtype=np.float64) if want_minmax else None
            self._check(self.lib.xc_contours(self.handle, _ptr(q), dtype_code(q.dtype), nslab, int(q.size // nslab), int(N),
                                             int(bool(increase)), dtype_code(ctr_dtype), int(right_edge), _ptr(mm), _ptr(ctr), None, None))
            return ctr, mm
        ctr, mm = self._batched(nslab, q.nbytes // max(1, nslab), one)
        if ctr is None:
            ctr = self.levels(mm, q.dtype, N, increase, ctr_dtype, right_edge)[0]
        return (ctr, mm) if want_minmax else ctr

    def trace(self, reset=True):
        """seconds the host-form calls spent staging inputs / handing results over / waiting for the stream since the last reset"""
        out = (C.c_double * 3)()
        self._check(self.lib.xc_trace(self.handle, 1 if reset else 0, out))
        return {'stage_in_s': out[0], 'hand_over_s': out[1], 'sync_wait_s': out[2]}

    def levels(self, minmax, q_dtype, N, increase, ctr_dtype, right_edge=XC_EDGE_XHISTOGRAM):
        minmax = np.ascontiguousarray(minmax, dtype=np.float64)
        nslab = minmax.shape[0]
        ctr = np.empty((nslab, N), dtype=np.float64)
        edges = np.empty((nslab, N + 1), dtype=np.float64)
        status = np.empty(nslab, dtype=np.int32)
        self._check(self.lib.xc_levels(self.handle, _ptr(minmax), dtype_code(q_dtype), nslab, int(N),
                                       int(bool(increase)), dtype_code(ctr_dtype), int(right_edge),
                                       _ptr(ctr), _ptr(edges), _ptr(status)))
        return ctr, edges, status

    def hist(self, q, edges, dA=None, integrands=(), grad=None, last_closed=True, lt=True,
             reverse=False, prod_f32=False, negate=False, want=('pdf', 'counts', 'cdf'), deterministic=False):
        """q: (nslab, ny, nx); edges: (nedge,) or (nslab, nedge) ascending f64.
        dA: None | (ny,) | (ny,nx) | (nslab,ny,nx) (converted to f64).
        grad: None or (rdx, rdy, periodic_x).  deterministic: order-free fixed-point sums (bit-reproducible).
        Returns dict of requested outputs."""
        q = _stack_in(q)
        assert q.ndim == 3
        nslab, ny, nx = q.shape
        integrands = [v if _is_lazy(v) else np.asarray(v) for v in integrands]     # (nested lists are fine, as for q)
        d = HistDesc()
        d.q_dtype = dtype_code(q.dtype)
        d.ny, d.nx = ny, nx
        edges = _contig(edges, np.float64)
        d.nedge = edges.shape[-1]
        d.edges_per_slab = 1 if edges.ndim == 2 else 0
        if edges.ndim == 2 and edges.shape[0] != nslab:
            raise XContourHipError(XC_EBADARG, 'edges must be (nedge,) or (nslab, nedge)')
        d.last_closed = 1 if last_closed else 0
        if dA is not None:                                   # (else XC_DA_NONE, a null pointer: the descriptor's zeros)
            dA = _contig(dA, np.float64)
            d.dA_rank = _weight_rank(dA.shape, ny, nx, nslab, 'dA must be (ny,), (ny,nx) or (nslab,ny,nx)')
        d.prod_f32 = 1 if prod_f32 else 0
        d.nint = len(integrands)
        if d.nint > XC_MAX_INTEGRANDS:
            raise XContourHipError(XC_EBADARG, 'at most %d integrands per pass' % XC_MAX_INTEGRANDS)
        per = q.dtype.itemsize + (8 if d.dA_rank == XC_DA_SLAB else 0)        # bytes per cell that a batch stages
        for i, v in enumerate(integrands):
            if v.shape != q.shape:
                raise XContourHipError(XC_EBADARG, 'integrand shape must equal tracer shape')
            d.integrand_dtype[i] = dtype_code(v.dtype)
            per += np.dtype(v.dtype).itemsize
        if grad is not None:
            rdx = np.ascontiguousarray(grad[0], dtype=np.float64)
            rdy = np.ascontiguousarray(grad[1], dtype=np.float64)
            assert rdx.shape == (ny,) and rdy.shape == (ny,)
            d.grad, d.rdx, d.rdy, d.periodic_x = 1, _ptr(rdx), _ptr(rdy), 1 if grad[2] else 0
        d.lt, d.reverse, d.negate = 1 if lt else 0, 1 if reverse else 0, 1 if negate else 0
        d.deterministic = 1 if deterministic else 0
        nch, nbin = 1 + d.nint + d.grad, d.nedge - 1

        def one(s0, s1):
            qb, eb, db = _stack_now(q, s0, s1), _part(edges, 2, s0, s1), _part(dA, 3, s0, s1)
            vb = [_contig(_stack_now(v, s0, s1)) for v in integrands]
            d.q, d.nslab, d.edges, d.dA = _ptr(qb), s1 - s0, _ptr(eb), _ptr(db)
            for i, v in enumerate(vb):
                d.integrand[i] = v.ctypes.data
            out = {}
            if 'pdf' in want:
                out['pdf'] = np.empty((s1 - s0, nch, nbin), dtype=np.float64)
                d.pdf = _ptr(out['pdf'])
            if 'cdf' in want:
                out['cdf'] = np.empty((s1 - s0, nch, nbin), dtype=np.float64)
                d.cdf = _ptr(out['cdf'])
            if 'counts' in want:
                out['counts'] = np.empty((s1 - s0, nbin), dtype=np.uint64)
                d.counts = _ptr(out['counts'])
            self._check(self.lib.xc_hist(self.handle, C.byref(d)))
            return out
        return self._batched(nslab, ny * nx * per, one)      # more than one launch / one arena takes: batches of whole slabs

    def rowsum(self, mask, dA, ny, nx, multiply=False):
        if mask is not None:
            mask = _f48(np.ascontiguousarray(mask))
            assert mask.shape == (ny, nx)
        rank = XC_DA_NONE
        if dA is not None:
            dA = np.ascontiguousarray(dA, dtype=np.float64)
            rank = _weight_rank(dA.shape, ny, nx)
        out = np.empty(ny, dtype=np.float64)
        self._check(self.lib.xc_rowsum(self.handle, _ptr(mask), dtype_code(mask.dtype) if mask is not None else XC_F64,
                                       _ptr(dA), rank, ny, nx, 1 if multiply else 0, _ptr(out)))
        return out

    def keff_epilogue(self, pdf, ctr, tbl, tbl_coord, increase=True, lt=True, ctr_dtype=np.float64, preY=None,
                      nkeff_mask=1e5, lmin_scale=2.0 * np.pi * 6371200.0):
        """K5 / K6 alone (xc_keff_epilogue): pdf (nslab, 2, N) per-bin sums of dA and integrand * dA in ascending-value bin
        order, ctr (nslab, N) levels in level order -> dict of the Keff vectors (nslab, N) (+ 'interp' (nslab, 9, npre))."""
        pdf = np.ascontiguousarray(pdf, dtype=np.float64); ctr = np.ascontiguousarray(ctr, dtype=np.float64)
        assert pdf.ndim == 3 and pdf.shape[1] == 2 and ctr.shape == (pdf.shape[0], pdf.shape[2])
        nslab, _, N = pdf.shape
        tbl = np.ascontiguousarray(tbl, dtype=np.float64); crd = np.ascontiguousarray(tbl_coord, dtype=np.float64)
        assert tbl.shape == crd.shape and tbl.ndim == 1
        names = ('area', 'intgrdS', 'latEq', 'dqdA', 'dintSdA', 'Leq2', 'Lmin', 'nkeff')
        out = {k: np.empty((nslab, N), dtype=np.float64) for k in names}
        pre = None if preY is None else np.ascontiguousarray(preY, dtype=np.float64)
        interp = None if pre is None else np.empty((nslab, 9, len(pre)), dtype=np.float64)
        self._check(self.lib.xc_keff_epilogue(self.handle, _ptr(pdf), _ptr(ctr), dtype_code(np.dtype(ctr_dtype)), nslab, N,
                                              1 if increase else 0, 1 if lt else 0, _ptr(tbl), _ptr(crd), len(tbl),
                                              _ptr(pre), 0 if pre is None else len(pre), float(nkeff_mask), float(lmin_scale),
                                              *[_ptr(out[k]) for k in names], _ptr(interp)))
        if interp is not None:
            out['interp'] = interp
        return out

    def grad2(self, q, rdx, rdy, periodic_x=True):
        q = _stack_in(q)
        assert q.ndim == 3
        nslab, ny, nx = q.shape
        rdx = np.ascontiguousarray(rdx, dtype=np.float64)
        rdy = np.ascontiguousarray(rdy, dtype=np.float64)

        def one(s0, s1):
            qb = _stack_now(q, s0, s1)
            out = np.empty(qb.shape, dtype=np.float64)
            self._check(self.lib.xc_grad2(self.handle, _ptr(qb), dtype_code(q.dtype), s1 - s0, ny, nx,
                                          _ptr(rdx), _ptr(rdy), 1 if periodic_x else 0, _ptr(out)))
            return out
        return self._batched(nslab, ny * nx * (q.dtype.itemsize + 8), one)

    def contour_map(self, q, levels, values, out_dtype=np.float64):
        """Contour vectors back on the plane (K25, xc_contour_map).  q (nslab, ny, nx) f32/f64 (or a lazy stack); levels (N,) or
        (nslab, N), N >= 2, strictly monotonic in either direction and finite per slab (a slab whose first or last level is NaN
        gives NaN everywhere); values: a sequence of 1 .. XC_CMAP_MAXV arrays (N,) or (nslab, N).  Per slab and vector
        out = np.interp(q, X, F) in float64, X, F the levels and the vector, both reversed when not levels[0] < levels[-1]
        (the reference's _interp1d), bit for bit; out_dtype float32 rounds that once.  Returns the list of planes (nslab, ny, nx),
        one per vector.  A tracer with a device mirror (keep_resident) is read in place through the _dev entry point."""
        q, (nslab, ny, nx) = _stack3(q)
        out_dtype = np.dtype(out_dtype)
        qcode, ocode = dtype_code(q.dtype), dtype_code(out_dtype)
        levels = _contig(levels, np.float64)
        if levels.ndim not in (1, 2) or (levels.ndim == 2 and levels.shape[0] != nslab) or levels.shape[-1] < 2:
            raise XContourHipError(XC_EBADARG, 'xc_contour_map: levels must be (N,) or (nslab, N) with N >= 2')
        N = levels.shape[-1]
        values = [_contig(v, np.float64) for v in values]
        nv = len(values)
        if not 1 <= nv <= XC_CMAP_MAXV:
            raise XContourHipError(XC_EBADARG, 'xc_contour_map: 1 to %d value vectors, not %d' % (XC_CMAP_MAXV, nv))
        for v in values:
            if v.shape not in ((N,), (nslab, N)):
                raise XContourHipError(XC_EBADARG, 'xc_contour_map: every value vector must be (N,) or (nslab, N) like the levels, N = %d' % N)
        if (nv + 1) * N > XC_CMAP_MAX_LDS_DOUBLES:
            raise XContourHipError(XC_EBADARG, 'xc_contour_map: (nv + 1) * N must not exceed %d' % XC_CMAP_MAX_LDS_DOUBLES)
        flags =(C.c_int * nv)(*[1 if v.ndim == 2 else 0 for v in values])

        def one(s0, s1):
            n = s1 - s0
            qb, lb_ = _stack_now(q, s0, s1), _part(levels, 2, s0, s1)
            vb = [_part(v, 2, s0, s1) for v in values]
            return self._twin(self.lib.xc_contour_map, self.lib.xc_contour_map_dev, qb, [lb_] + vb, [((n, ny, nx), out_dtype)] * nv,
                              lambda pq, ins, outs: (pq, qcode, n, ny, nx, ins[0], N, 1 if levels.ndim == 2 else 0, nv,
                                                     (_vp * nv)(*ins[1:]), flags, (_vp * nv)(*outs), ocode),
                              checks=[lambda: _check_map_levels(lb_)])
        return self._batched(nslab, ny * nx * (q.dtype.itemsize + nv * out_dtype.itemsize), one)

    def crossing(self, q, contours, area, stride=1, pad_x=0, pad_mode='edge', full_width=False):
        """Box-counting contour crossing (xc_crossing).  q (nslab, ny, nx) f32/f64; contours (N,) or
        (nslab, N) ASCENDING f64; area (ny, nx) or (nslab, ny, nx) f32/f64.
        Returns (lengths f64 (nslab, N), box counts uint64 (nslab, N))."""
        q = _stack_in(q)
        assert q.ndim == 3
        nslab, ny, nx = q.shape
        contours = np.ascontiguousarray(contours, dtype=np.float64)
        per_slab = contours.ndim == 2
        if per_slab and contours.shape[0] != nslab:
            raise XContourHipError(XC_EBADARG, 'contours must be (N,) or (nslab, N)')
        area = _f48(np.ascontiguousarray(area))
        if area.shape not in ((ny, nx), (nslab, ny, nx)):
            raise XContourHipError(XC_EBADARG, 'area must be (ny, nx) or (nslab, ny, nx)')
        if pad_mode not in PAD_MODES:
            raise XContourHipError(XC_EBADARG, 'pad mode must be one of %s' % sorted(PAD_MODES))
        N = contours.shape[-1]
        if np.ndim(stride) > 0:
            for t in stride:
                if int(t) < 1:
                    raise XContourHipError(XC_EBADARG, 'stride must be >= 1')
            _check_ascending(contours, 'xc_crossing')
        # what every batch hands to xc_crossing / xc_crossing_dev between the tracer and the stride
        shape = (ny, nx, int(pad_x), PAD_MODES[pad_mode])
        flags = (N, 1 if per_slab else 0)
        aflags = (dtype_code(area.dtype), 1 if area.ndim == 3 else 0)

        def one(s0, s1):
            n = s1 - s0
            qb, cb, ab = _stack_now(q, s0, s1), _part(contours, 2, s0, s1), _part(area, 3, s0, s1)
            if np.ndim(stride) > 0:
                # several strides on the same padded slab: one upload, one device call per stride
                # (`stride` may be a list; returns lists of results in the same order)
                with self._temporaries([qb, cb, ab], [n * N * 8, n * N * 8]) as (dq, dc, da, dl, dn):
                    out = []
                    for t in stride:
                        self._check(self.lib.xc_crossing_dev(self.handle, dq.ptr, dtype_code(q.dtype), n, *shape, dc.ptr, *flags,
                                                             da.ptr, *aflags, int(t), 1 if full_width else 0, dl.ptr, dn.ptr))
                        out.append((dl.download((n, N), np.float64), dn.download((n, N), np.uint64)))
                return out
            lens = np.empty((n, N), dtype=np.float64)
            cnts = np.empty((n, N), dtype=np.uint64)
            self._check(self.lib.xc_crossing(self.handle, _ptr(qb), dtype_code(q.dtype), n, *shape, _ptr(cb), *flags,
                                             _ptr(ab), *aflags, int(stride), 1 if full_width else 0, _ptr(lens), _ptr(cnts)))
            return lens, cnts
        return self._batched(nslab, ny * nx * (q.dtype.itemsize + (area.dtype.itemsize if area.ndim == 3 else 0)), one)

    def _mirror(self, qb):
        """device address of the mirror of a batch of the tracer (keep_resident), or None"""
        return self.resident_ptr(qb) if isinstance(qb, np.ndarray) and qb.flags.c_contiguous else None

    def _ring_forms(self, name, period):
        """K10 / K11, plain or periodic: (the host entry point, the _dev one, what their argument lists hold between xcoord and the
        radius: the period, in the periodic forms)"""
        if period is not None:
            name, period = name + '_periodic', (period,)
        return getattr(self.lib, name), getattr(self.lib, name + '_dev'), period or ()

    def contour_lengths(self, q, contours, ycoord, xcoord, radius=0.0, period=None):
        """Marching-squares contour lengths (xc_contour_lengths).  q (nslab, ny, nx) f32/f64 (or a lazy stack); contours (N,) or
        (nslab, N) ASCENDING f64; ycoord (ny,) / xcoord (nx,) the coordinates of rows / columns (radians when radius > 0).
        radius > 0: great-circle lengths times radius; 0: Cartesian.  Returns (lengths f64 (nslab, N), NaN where the total is 0;
        segment counts uint64 (nslab, N)).  A tracer with a device mirror (keep_resident) is read in place through the _dev
        entry point.  period: None -- the plane has two free edges in X --, or the period of the X coordinate (in its units:
        radians when radius > 0; of the sign of xcoord[-1] - xcoord[0] and longer than that span): the cell between the last and
        the first column is traced too (xc_contour_lengths_periodic), as on the plane with column 0 appended one period on."""
        who = 'xc_contour_lengths'
        q, (nslab, ny, nx), contours, per_slab, N, ycoord, xcoord, period = _lengths_open(q, contours, ycoord, xcoord, period, who,
                                                                                           'xc_contour_lengths_periodic')
        f_host, f_dev, ring = self._ring_forms(who, period)
        mid = ring + (float(radius),)

        def one(s0, s1):
            n = s1 - s0
            qb, cb = _stack_now(q, s0, s1), _part(contours, 2, s0, s1)
            return tuple(self._twin(f_host, f_dev, qb, [ycoord, xcoord, cb], [((n, N), np.float64), ((n, N), np.uint64)],
                                    lambda pq, ins, outs: (pq, dtype_code(q.dtype), n, ny, nx, *ins[:2], *mid, ins[2], N,
                                                           1 if per_slab else 0, *outs),
                                    checks=_lengths_trusted(who, cb, ycoord, xcoord)))
        return self._batched(nslab, ny * nx * q.dtype.itemsize, one)

    def coarsen(self, q, ratio, skipna=False):
        """The block means of K26 alone (xc_coarsen).  q (nslab, ny, nx) f32/f64 (or a lazy stack) -> float64 (nslab, ny // ratio,
        nx // ratio): blocks from index 0, trailing rows and columns dropped, every value promoted to float64, each block summed row
        by row, left to right, then top to bottom, and divided once by ratio * ratio.  skipna: NaN nodes are left out and the divisor
        is the number of nodes used (a block of none is NaN); else a block with a NaN node is NaN.  1 <= ratio <= XC_CSCALE_MAXRATIO.
        A tracer with a device mirror (keep_resident) is read in place through the _dev entry point."""
        q, (nslab, ny, nx) = _stack3(q)
        qcode, r = dtype_code(q.dtype), int(ratio)
        if not 1 <= r <= XC_CSCALE_MAXRATIO or ny // r < 1 or nx // r < 1:
            raise XContourHipError(XC_EBADARG, 'xc_coarsen: ratio %d is outside 1 .. %d or leaves no coarse node of a (%d, %d) plane'
                                   % (r, XC_CSCALE_MAXRATIO, ny, nx))
        cny, cnx = ny // r, nx // r

        def one(s0, s1):
            n = s1 - s0
            return self._twin(self.lib.xc_coarsen, self.lib.xc_coarsen_dev, _stack_now(q, s0, s1), [], [((n, cny, cnx), np.float64)],
                              lambda pq, ins, outs: (pq, qcode, n, ny, nx, r, 1 if skipna else 0, *outs))[0]
        return self._batched(nslab, ny * nx * q.dtype.itemsize + cny * cnx * 8, one)

    def contour_lengths_scales(self, q, contours, ycoord, xcoord, ratios, radius=0.0, period=None, skipna=False):
        """Contour lengths at coarsened resolutions (K26, xc_contour_lengths_scales): `contour_lengths` of the block-averaged tracer
        for every ratio of `ratios` (1 .. XC_CSCALE_MAXR of them, each in 1 .. XC_CSCALE_MAXRATIO, any order), the tracer uploaded
        once and coarsened on the GPU (`coarsen`'s rule; the coordinates take the same block means in float64).  q, contours, ycoord,
        xcoord, radius, period as for `contour_lengths`; a ratio must leave two coarse rows and, on a plain plane, two coarse columns;
        on a periodic one it must divide nx.  Returns (lengths f64 (nratio, nslab, N), segment counts uint64 (nratio, nslab, N)),
        row k bit for bit what `contour_lengths` returns for the coarse plane and coordinates of ratios[k]."""
        who = 'xc_contour_lengths_scales'
        q, (nslab, ny, nx), contours, per_slab, N, ycoord, xcoord, period = _lengths_open(q, contours, ycoord, xcoord, period, who)
        ratios = [int(r) for r in ratios]
        nr = len(ratios)
        if not 1 <= nr <= XC_CSCALE_MAXR:
            raise XContourHipError(XC_EBADARG, '%s: 1 to %d ratios, not %d' % (who, XC_CSCALE_MAXR, nr))
        for r in ratios:
            if not 1 <= r <= XC_CSCALE_MAXRATIO:
                raise XContourHipError(XC_EBADARG, '%s: ratio %d is outside 1 .. %d' % (who, r, XC_CSCALE_MAXRATIO))
            if ny // r < 2 or (period is None and nx // r < 2):
                raise XContourHipError(XC_EBADARG, '%s: ratio %d leaves fewer than 2 coarse rows or columns of a (%d, %d) plane' % (who, r, ny, nx))
            if period is not None and nx % r:
                raise XContourHipError(XC_EBADARG, '%s: ratio %d does not divide nx = %d of a periodic plane' % (who, r, nx))
        rr = (C.c_int * nr)(*ratios)
        mid = (0.0 if period is None else period, float(radius), rr, nr, 1 if skipna else 0)

        def one(s0, s1):
            n = s1 - s0
            qb, cb = _stack_now(q, s0, s1), _part(contours, 2, s0, s1)
            res = self._twin(self.lib.xc_contour_lengths_scales, self.lib.xc_contour_lengths_scales_dev, qb, [ycoord, xcoord, cb],
                             [((nr, n, N), np.float64), ((nr, n, N), np.uint64)],
                             lambda pq, ins, outs: (pq, dtype_code(q.dtype), n, ny, nx, *ins[:2], *mid, ins[2], N, 1 if per_slab else 0, *outs),
                             checks=_lengths_trusted(who, cb, ycoord, xcoord))
            return tuple(list(a) for a in res)
        lens, cnts = self._batched(nslab, ny * nx * q.dtype.itemsize, one)       # (lists over the ratios: `_join` joins each along the slabs)
        return np.stack(lens), np.stack(cnts)

    def contour_line_integrals(self, q, f, contours, ycoord, xcoord, radius=0.0, period=None):
        """Integrals of a field along contours (K15, xc_contour_line_integrals).  q and contours, ycoord, xcoord, radius, period as for
        `contour_lengths`; f: the integrand, f32/f64, of q's shape (an array).  On K10's segments, each with the integrand mapped onto
        its end points u, v like the coordinates: integral = sum of 0.5 (F(u) + F(v)) len, length = sum of len, both over the segments
        whose F(u) and F(v) are not NaN, nseg their number.  Returns (integral f64 (nslab, N), length f64 (nslab, N), nseg uint64
        (nslab, N)); integral and length are NaN where the length is 0, and a level that met an infinite term has a NaN integral.
        A tracer with a device mirror (keep_resident) is read in place through the _dev entry point."""
        who = 'xc_contour_line_integrals'
        f = _f48(_contig(f))

        def shaped(shape):
            if tuple(f.shape) != shape:
                raise XContourHipError(XC_EBADARG, '%s: the integrand must have the shape of q, %r' % (who, shape))
        q, (nslab, ny, nx), contours, per_slab, N, ycoord, xcoord, period = _lengths_open(q, contours, ycoord, xcoord, period, who,
                                                                                           shaped=shaped)
        mid = (0.0 if period is None else period, float(radius))

        def one(s0, s1):
            n = s1 - s0
            qb, fb, cb = _stack_now(q, s0, s1), _part(f, 3, s0, s1), _part(contours, 2, s0, s1)
            return tuple(self._twin(self.lib.xc_contour_line_integrals, self.lib.xc_contour_line_integrals_dev, qb, [fb, ycoord, xcoord, cb],
                                    [((n, N), np.float64), ((n, N), np.float64), ((n, N), np.uint64)],
                                    lambda pq, ins, outs: (pq, dtype_code(q.dtype), ins[0], dtype_code(f.dtype), n, ny, nx, *ins[1:3], *mid,
                                                           ins[3], N, 1 if per_slab else 0, *outs),
                                    checks=_lengths_trusted(who, cb, ycoord, xcoord)))
        return self._batched(nslab, ny * nx * (q.dtype.itemsize + f.dtype.itemsize), one)

    @contextlib.contextmanager
    def _two_pass(self, call, dcount, shape, nbytes, always=False):
        """A count-only call, then a sized one.  call(0, []) is the entry point with no room and no outputs: it leaves the counts
        (`shape` uint64) in `dcount`; their sum, the total, sizes the outputs -- one allocation per entry of nbytes(total) --,
        which call(total, outputs) fills.  Nothing counted: no second call and no outputs, unless `always`.  Yields (counts, total,
        outputs); the outputs are freed on the way out."""
        rc = call(0, [])
        if rc not in (XC_OK, 1):                                 # (1: there is something, and no room was given)
            self._check(rc)
        cnt = dcount.download(shape, np.uint64)
        total = int(cnt.sum())
        with self._temporaries([], nbytes(total) if total or always else []) as outs:
            if outs:
                self._check(call(total, outs))
            yield cnt, total, outs

    def _with_segment_records(self, periodic, qb, cb, use, inputs=(), out_nbytes=(), per_segment=()):
        """K12's two passes over one batch, everything staged once.  Uploaded: the tracer `qb` (unless it has a device mirror), the
        contours `cb` ((N,) or one row per slab) and the caller's further `inputs`; allocated: the counts and one buffer per entry
        of `out_nbytes`.  A count-only call gives the total, which sizes the three record buffers, and one of b bytes per segment
        for every b of `per_segment`, of the second call (none without segments).  Returns
        use(counts (n, N) uint64, total, count buffer, buffers of `inputs`, buffers of `out_nbytes`,
        [e_from, e_to, pts, *per-segment buffers] or []); every device buffer is freed on the way out."""
        f = self.lib.xc_contour_segments_periodic_dev if periodic else self.lib.xc_contour_segments_dev
        n, ny, nx = qb.shape
        N, nin = cb.shape[-1], len(inputs)
        qp = self._mirror(qb)
        with self._temporaries(([] if qp else [qb]) + [cb] + list(inputs), [n * N * 8] + list(out_nbytes)) as bufs:
            rest = bufs[0 if qp else 1:]
            dn = rest[1 + nin]
            head = (self.handle, qp or bufs[0].ptr, dtype_code(qb.dtype), n, ny, nx, rest[0].ptr, N, 1 if cb.ndim == 2 else 0)

            def k12(total, recs):
                return f(*head, total, dn.ptr, *([b.ptr for b in recs[:3]] or [None] * 3))
            with self._two_pass(k12, dn, (n, N), lambda total: [total * b for b in (8, 8, 32) + tuple(per_segment)]) as (cnt, total, recs):
                return use(cnt, total, dn, rest[1:1 + nin], rest[2 + nin:], recs)

    @staticmethod
    def _record_run(a, total, ins, recs):
        """the arguments every entry point on K12's records takes, from what `_with_segment_records` hands to `use` -> ([e_from, e_to,
        pts] -- three None without segments --, [w, w_per_slab, f, f_dtype]: the weights `a.w` and the integrand `a.f` lead `ins`)"""
        has_w, has_f = a.w is not None, a.f is not None
        return ([b.ptr for b in recs[:3]] if total else [None] * 3, [ins[0].ptr if has_w else None, 1 if has_w and a.w.ndim == 3 else 0,
                                                                     ins[has_w].ptr if has_f else None, dtype_code(a.f.dtype) if has_f else 0])

    def contour_segments(self, q, contours, periodic=False):
        """Marching-squares contour segments (K12, xc_contour_segments_dev; periodic=True: xc_contour_segments_periodic_dev).  q (nslab, ny, nx) f32/f64 (or a lazy stack); contours
        (N,) or (nslab, N) ASCENDING f64 without NaN.  Returns (count uint64 (nslab, N); e_from, e_to int64 (total,): the ids of the
        grid edges the start / end of each directed segment lie on -- horizontal (r, c)-(r, c+1): 2 (r nx + c), vertical
        (r, c)-(r+1, c): 2 (r nx + c) + 1 --; pts float64 (total, 4): (r1, c1, r2, c2) in index space).  Segments are packed by
        (slab, contour): range (s, k) starts at the exclusive scan of `count`; segments whose end points coincide are kept.
        Inside a range the segments are sorted by e_from (unique there), so the result is the same on every call.  Every batch
        is staged once: a count-only call sizes the buffers of the second.  periodic=True: X is a ring of nx cell columns (nx >= 2):
        the seam cell between the last column and the first is traced too, its columns run from nx-1 to nx, and its right edge has
        column 0's id, 2 r nx + 1 -- the records of the plane with column 0 appended as column nx, ids folded onto the ring."""
        a = _RecordArgs('xc_contour_segments', q, contours, periodic=periodic, min_nx=2)

        def download(cnt, total, dn, ins, outs, recs):
            if total == 0:
                return cnt, np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64), np.empty((0, 4), dtype=np.float64)
            df, dt, dp = recs
            ef, et, pts = df.download((total,), np.int64), dt.download((total,), np.int64), dp.download((total, 4), np.float64)
            o = _range_order(cnt, ef)
            return cnt, ef[o], et[o], pts[o]

        def one(s0, s1):
            return self._with_segment_records(periodic, *a.batch(s0, s1)[:2], download)
        return self._batched(a.nslab, a.slab_bytes(), one)

    # the per-piece table of `contour_pieces`: one record per connected piece of a contour
    PIECE_DTYPE = np.dtype([('first_edge', np.int64), ('nseg', np.int64), ('closed', np.bool_), ('winding', np.int32),
                            ('length', np.float64), ('area', np.float64), ('row_min', np.float64), ('row_max', np.float64)])

    def set_cpiece_workspace(self, nbytes):
        """cap, in bytes, on the edge tables K13 builds for one group of ranges (xc_set_cpiece_workspace; default 1 GiB; one range
        is always allowed; the result does not depend on it)"""
        self._check(self.lib.xc_set_cpiece_workspace(self.handle, int(nbytes)))

    def _last_profile(self, name, stages, groups=True):
        """xc_last_<name>_profile: the device times of the stages of the last batch as `<stage>_ms`, then `rounds`[, `groups`]"""
        ms = (C.c_double * len(stages))()
        counts = [C.c_int(0) for _ in range(2 if groups else 1)]
        self._check(getattr(self.lib, 'xc_last_%s_profile' % name)(self.handle, C.cast(ms, _vp), *[C.byref(c) for c in counts]))
        out = {s + '_ms': v for s, v in zip(stages, ms)}
        out.update(zip(('rounds', 'groups'), (c.value for c in counts)))
        return out

    def last_cpiece_profile(self):
        """device times of the last `contour_pieces` batch under set_kernel_timing(True): dict(table_ms, rounds_ms, roots_ms,
        reduce_ms, rounds, groups)"""
        return self._last_profile('cpiece', ('table', 'rounds', 'roots', 'reduce'))

    def contour_pieces(self, q, contours, ycoord, xcoord, radius=0.0, period=None):
        """The connected pieces of every contour and their statistics (K13, xc_contour_pieces_dev, on the device records of K12,
        xc_contour_segments[_periodic]_dev: the segment records are never downloaded).  q, contours, ycoord, xcoord, radius and
        period as for `contour_lengths` (period not None: X is a ring).  Returns (piece_count uint64 (nslab, N), table): `table`
        a structured array (PIECE_DTYPE) of all pieces packed by (slab, contour) -- range (s, k) starts at the exclusive scan of
        piece_count --, each range sorted by first_edge (unique there): the order of the polylines of `join_segments`.
          first_edge  the smallest e_from of the piece;  nseg  its segments;  closed  a ring;  winding  of a ring on a periodic plane;
          length  the sum of K10's segment lengths (times radius), 0.0 for a piece of coincident-end segments only;
          area  S = 1/2 sum (Ya' + Yb') (Xa - Xb), Y' = sin(Y) and S radius^2 when radius > 0; NaN for an open piece;
          row_min, row_max  the extent in index-space rows."""
        a = _RecordArgs('xc_contour_pieces', q, contours)
        ny, nx, N = a.ny, a.nx, a.N
        ycoord, xcoord = _plane_coords(ycoord, xcoord, ny, nx, 'xc_contour_pieces')
        _check_finite('xc_contour_pieces', ycoord, xcoord)
        radius = float(radius)
        periodic = period is not None
        if periodic:
            period = _check_period(period, xcoord, 'xc_contour_pieces')
        dt = self.PIECE_DTYPE
        # one piece record per segment at most: six 8-byte columns, then two 4-byte ones
        cols = [(k, dt[k]) for k in ('first_edge', 'nseg', 'length', 'area', 'row_min', 'row_max')] + [('closed', np.int32), ('winding', np.int32)]

        def pieces(cnt, total, dn, ins, outs, recs):
            if total == 0:
                return np.zeros(cnt.shape, dtype=np.uint64), np.empty(0, dtype=dt)
            (dy, dx), (dpc,), (df, dto, dp, drec) = ins, outs, recs
            at = _Columns(drec, total, cols)
            self._check(self.lib.xc_contour_pieces_dev(
                self.handle, cnt.size, dn.ptr, df.ptr, dto.ptr, dp.ptr, ny, nx, 1 if periodic else 0, dy.ptr, dx.ptr,
                period if periodic else 0.0, radius, total, dpc.ptr,
                *at.ptrs(('first_edge', 'nseg', 'closed', 'winding', 'length', 'area', 'row_min', 'row_max'))))
            pc = dpc.download(cnt.shape, np.uint64)
            out = at.into(np.empty(int(pc.sum()), dtype=dt))
            return pc, out[_range_order(pc, out['first_edge'])]

        def one(s0, s1):
            # beside K12's records: the coordinates, the piece counts, and the piece records
            return self._with_segment_records(periodic, *a.batch(s0, s1)[:2], pieces, inputs=(ycoord, xcoord),
                                              out_nbytes=((s1 - s0) * N * 8,), per_segment=(_row_bytes(cols),))
        return self._batched(a.nslab, a.slab_bytes(), one)

    def last_cjoin_profile(self):
        """device times of the last `contour_polylines` batch under set_kernel_timing(True): dict(table_ms, label_ms, rank_ms,
        place_ms, gather_ms, rounds, groups)"""
        return self._last_profile('cjoin', ('table', 'label', 'rank', 'place', 'gather'))

    def contour_polylines(self, q, contours, periodic=False):
        """The contours joined into polylines on the device (K14, xc_contour_polylines_dev, on the device records of K12): what
        `contour_segments` and `join_segments` give together, with the records already in walk order -- only those and the
        per-polyline table are downloaded, nothing is sorted on the host.  q, contours and periodic as for `contour_segments`.
        Returns (count uint64 (nslab, N); e_from_walk int64 (total,) and pts_walk float64 (total, 4): e_from[walk] and pts[walk] of
        `contour_segments` / `join_segments`, bit for bit; poly_off (npoly + 1,) int64 into them; closed (npoly,) bool; rpo
        (nrange + 1,) int64: the polylines of range r are [rpo[r], rpo[r+1])) -- with walk = arange(total), the arguments of
        core.contour_polylines."""
        a = _RecordArgs('xc_contour_polylines', q, contours, periodic=periodic, min_nx=2, labels32=True)
        ny, nx, N = a.ny, a.nx, a.N
        cols = [('nseg', np.int64), ('first', np.int64), ('closed', np.int32)]       # one polyline per segment at most

        def polylines(cnt, total, dn, ins, outs, recs):
            if total == 0:
                return (cnt, np.empty(0, dtype=np.int64), np.empty((0, 4), dtype=np.float64), np.empty(0, dtype=np.int64),
                        np.empty(0, dtype=bool), np.zeros(cnt.shape, dtype=np.uint64))
            (dpc,), (df, dto, dp, dfw, dpw, drec) = outs, recs
            at = _Columns(drec, total, cols)
            self._check(self.lib.xc_contour_polylines_dev(self.handle, cnt.size, dn.ptr, df.ptr, dto.ptr, dp.ptr, ny, nx, total,
                                                          dpc.ptr, *at.ptrs(('nseg', 'closed', 'first')), dpw.ptr, dfw.ptr, None))
            pc = dpc.download(cnt.shape, np.uint64)
            npoly = int(pc.sum())
            return (cnt, dfw.download((total,), np.int64), dpw.download((total, 4), np.float64), at.get('nseg', (npoly,)),
                    at.get('closed', (npoly,)).astype(bool), pc)

        def one(s0, s1):
            # beside K12's records: the polyline counts, the walk-ordered e_from and pts, and the polyline records
            return self._with_segment_records(periodic, *a.batch(s0, s1)[:2], polylines,
                                              out_nbytes=((s1 - s0) * N * 8,), per_segment=(8, 32, _row_bytes(cols)))
        cnt, efw, ptw, nseg, closed, pc = self._batched(a.nslab, a.slab_bytes(), one)
        poly_off = np.concatenate([[0], np.cumsum(nseg, dtype=np.int64)])
        rpo = np.concatenate([[0], np.cumsum(pc.ravel().astype(np.int64))])
        return cnt, efw, ptw, poly_off, closed, rpo

    # how `contour_overturning` selects pieces: the names and the library's codes
    OVERTURN_SELECT = OVERTURN_SELECT

    def last_coverturn_profile(self):
        """device times of the last `contour_overturning` batch under set_kernel_timing(True): dict(table_ms, rounds_ms, select_ms,
        count_ms, rounds, groups)"""
        return self._last_profile('coverturn', ('table', 'rounds', 'select', 'count'))

    def contour_overturning(self, q, contours, periodic=False, select='main'):
        """Where the contours are overturned (K16, xc_contour_overturning_dev, on the device records of K12: the segment records
        are never downloaded): the crossings of every meridian with the selected pieces of every contour.  q, contours and
        periodic as for `contour_segments`; select: 'all' / 0 every piece, 'circumpolar' / 1 every ring of winding != 0, 'main' / 2
        per contour the one such ring with the most segments (ties: the smallest first_edge) -- the last two on a periodic plane
        only.  A crossing is a segment's start point on a vertical grid edge (e_from odd), or the end point on one of an open
        piece's last segment; its column is (id >> 1) % nx, its row the record's.  Returns (ncross int32, row_lo, row_hi float64
        (nslab, N, nx): the crossings of a column, their smallest / largest row, NaN without one; nsel int32, main_first_edge
        int64, main_nseg int64, main_winding int32 (nslab, N): the selected pieces, and the ring 'main' picks (-1, 0, 0 without
        one) under the key `contour_pieces` lists it by).  A column with ncross >= 3 is overturned."""
        a = _RecordArgs('xc_contour_overturning', q, contours, select=select, periodic=periodic, min_nx=2, labels32=True)
        ny, nx, N = a.ny, a.nx, a.N
        types = (np.int32, np.float64, np.float64, np.int32, np.int64, np.int64, np.int32)

        def overturning(cnt, total, dn, ins, outs, recs):
            n = cnt.shape[0]
            shapes = [(n, N, nx)] * 3 + [(n, N)] * 4
            if total == 0:
                fill = (0, np.nan, np.nan, 0, -1, 0, 0)
                return tuple(np.full(sh, v, dtype=t) for sh, v, t in zip(shapes, fill, types))
            df, dto, dp = recs
            self._check(self.lib.xc_contour_overturning_dev(self.handle, cnt.size, dn.ptr, df.ptr, dto.ptr, dp.ptr, ny, nx,
                                                            1 if periodic else 0, int(a.sel), *[b.ptr for b in outs]))
            return tuple(b.download(sh, t) for b, sh, t in zip(outs, shapes, types))

        def one(s0, s1):
            # beside K12's records: the seven dense outputs -- 20 bytes per (contour, column), 24 per contour
            n = s1 - s0
            return self._with_segment_records(periodic, *a.batch(s0, s1)[:2], overturning,
                                              out_nbytes=tuple(n * N * b for b in (nx * 4, nx * 8, nx * 8, 4, 8, 8, 4)))
        return self._batched(a.nslab, a.slab_bytes() + N * nx * 20, one)

    def last_cinterior_profile(self):
        """device times of the last `contour_interior` batch under set_kernel_timing(True): dict(table_ms, rounds_ms, select_ms,
        scan_ms, rounds, groups)"""
        return self._last_profile('cinterior', ('table', 'rounds', 'select', 'scan'))

    def contour_interior(self, q, contours, w=None, f=None, periodic=False, select='main', flip=False, return_mask=False):
        """What the selected pieces of every contour bound (K17, xc_contour_interior_dev, on the device records of K12: the segment
        records are never downloaded).  q, contours, periodic and select as for `contour_overturning`.  A node (r, c) is INSIDE
        when the selected pieces cross the grid line of column c between row 0 and row r an odd number of times (K16's meridian
        crossings, one flag per vertical edge), the other nodes when `flip`.  w: None (weight 1), (ny, nx) or (nslab, ny, nx)
        float64; f: None or (nslab, ny, nx) f32/f64.  Returns (n_in int64, sum_w float64, sum_wf float64 or None (nslab, N): the
        inside nodes, the sum of w and of w f over them -- exact sums rounded once, NaN terms skipped, an infinite term gives NaN
        --[, mask bool (nslab, N, ny, nx)]).  Only these cross to the host."""
        a = _RecordArgs('xc_contour_interior', q, contours, select=select, periodic=periodic, min_nx=2, labels32=True, w=w, f=f)
        ny, nx, N = a.ny, a.nx, a.N
        has_f, want_mask = a.f is not None, bool(return_mask)

        def interior(cnt, total, dn, ins, outs, recs):
            n = cnt.shape[0]
            dni, dsw = outs[:2]
            dsf, dm = (outs[2] if has_f else None), (outs[-1] if want_mask else None)
            rec, wf = self._record_run(a, total, ins, recs)
            self._check(self.lib.xc_contour_interior_dev(
                self.handle, cnt.size, dn.ptr, *rec, ny, nx, 1 if periodic else 0, int(a.sel), 1 if flip else 0, N, *wf,
                dni.ptr, dsw.ptr, dsf.ptr if has_f else None, dm.ptr if want_mask else None))
            res = (dni.download((n, N), np.int64), dsw.download((n, N), np.float64), dsf.download((n, N), np.float64) if has_f else None)
            return res + ((dm.download((n, N, ny, nx), np.uint8).view(np.bool_),) if want_mask else ())

        def one(s0, s1):
            # beside K12's records: the weights and the integrand, three 8-byte results per contour, and the mask when asked for
            n = s1 - s0
            qb, cb, wb, fb = a.batch(s0, s1)[:4]
            nb = [n * N * 8, n * N * 8] + ([n * N * 8] if has_f else []) + ([n * N * ny * nx] if want_mask else [])
            return self._with_segment_records(periodic, qb, cb, interior, inputs=[v for v in (wb, fb) if v is not None], out_nbytes=nb)
        return self._batched(a.nslab, a.slab_bytes(N if want_mask else 0), one)

    def set_cdist_prune(self, on):
        """whether `contour_distance` skips the blocks of segments that cannot hold a node's nearest one (xc_set_cdist_prune;
        default on; the result does not depend on it: for tests and A/B timing)"""
        self._check(self.lib.xc_set_cdist_prune(self.handle, 1 if on else 0))

    def last_cdist_profile(self):
        """the last xc_contour_distance_dev call: dict(table_ms, binning_ms, distance_ms -- device times under
        set_kernel_timing(True) --, pairs_visited, pairs_total: the (node, segment) pairs it evaluated / an unpruned call
        evaluates, groups)"""
        ms = (C.c_double * 3)()
        pv, pt, g = _i64(0), _i64(0), C.c_int(0)
        self._check(self.lib.xc_last_cdist_profile(self.handle, C.cast(ms, _vp), C.byref(pv), C.byref(pt), C.byref(g)))
        return {'table_ms': ms[0], 'binning_ms': ms[1], 'distance_ms': ms[2], 'pairs_visited': pv.value, 'pairs_total': pt.value,
                'groups': g.value}

    def _cdist_args(self, who, q, contours, ycoord, xcoord, radius, period, select, max_distance, **more):
        """the argument check K27 and K28 share (`more`: the weights and fields of `_RecordArgs`) -> (the checked arguments,
        ycoord, xcoord, radius, period, the cap as the library takes it)"""
        periodic = period is not None
        a = _RecordArgs(who, q, contours, select=select, periodic=periodic, min_nx=2, labels32=True, **more)
        ny, nx = a.ny, a.nx
        ycoord, xcoord = _plane_coords(ycoord, xcoord, ny, nx, who)
        _check_finite(who, ycoord, xcoord)
        radius = float(radius)
        if not (np.isfinite(radius) and radius >= 0.0):
            raise XContourHipError(XC_EBADARG, '%s: radius must be finite and >= 0' % who)
        if periodic:
            period = _check_period(period, xcoord, who)
            if radius > 0.0 and abs(period) != XC_CDIST_RING:
                raise XContourHipError(XC_EBADARG, '%s: on the sphere the period is float64(deg2rad(float32(+-360))), '
                                       'not %r: the plane is a sphere or none' % (who, period))
        cap = 0.0 if max_distance is None else float(max_distance)
        if np.isnan(cap):
            raise XContourHipError(XC_EBADARG, '%s: max_distance is NaN' % who)
        return a, ycoord, xcoord, radius, period, cap

    def _cdist_groups(self, a, ncg, coords, out_nbytes, per_node, payload, periodic, signed, flip):
        """the frame K27 and K28 share.  The contours of the checked arguments `a` go `ncg` at a time; a group of Ng stages, beside
        K12's records, `coords`, then a's weights and fields, and allocates out_nbytes(n, Ng) for a batch of n slabs -- a slab
        counts per_node bytes per node and contour toward the batch cap.  With `signed` three more buffers trail them: K17's two
        sums and its mask, made there with the same select and `flip`.  payload(head, inputs, outputs, mask pointer or None, n,
        Ng) makes the entry's call behind `head`, the arguments up to `select`, and downloads; the groups' results are joined
        along the contour axis."""
        ny, nx, N = a.ny, a.nx, a.N

        def group(k0, k1):
            g = a.on(a.q, np.ascontiguousarray(a.contours[..., k0:k1]))
            g.N = Ng = k1 - k0

            def call(cnt, total, dn, ins, outs, recs):
                head = (self.handle, cnt.size, dn.ptr, *self._record_run(g, total, ins, recs)[0], ny, nx, 1 if periodic else 0, int(a.sel))
                if signed:                                       # K17's mask, made where it is used
                    self._check(self.lib.xc_contour_interior_dev(*head, 1 if flip else 0, Ng, None, 0, None, 0, outs[-3].ptr, outs[-2].ptr,
                                                                 None, outs[-1].ptr))
                return payload(head, ins, outs, outs[-1].ptr if signed else None, cnt.shape[0], Ng)

            def one(s0, s1):
                n = s1 - s0
                qb, cb, wb, _, fb, _ = g.batch(s0, s1)
                nb = out_nbytes(n, Ng) + ([n * Ng * 8, n * Ng * 8, n * Ng * ny * nx] if signed else [])
                return self._with_segment_records(periodic, qb, cb, call, inputs=list(coords) + ([wb] if wb is not None else []) + fb,
                                                  out_nbytes=nb)
            return self._batched(a.nslab, g.slab_bytes(Ng * per_node), one)

        parts = [group(k0, min(N, k0 + ncg)) for k0 in range(0, N, ncg)]
        if len(parts) == 1:
            return parts[0]
        if isinstance(parts[0], tuple):
            return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(len(parts[0])))
        return np.concatenate(parts, axis=1)

    def contour_distance(self, q, contours, ycoord, xcoord, radius=0.0, period=None, select='all', max_distance=None, signed=False,
                         flip=False, return_nearest=False):
        """How far every node lies from every contour (K27, xc_contour_distance_dev, on the device records of K12: the segment
        records are never downloaded).  q, contours, ycoord, xcoord, radius and period as for `contour_pieces` (period not None: X
        is a ring; with radius > 0 the period must be that of the sphere, XC_CDIST_RING, of either sign); select as for
        `contour_overturning`.  Plane (radius 0): the Euclidean distance to the nearest point of the selected pieces' segments, on
        a ring the shortest over the images one period either way; sphere: the great-circle distance times radius.
        max_distance (None, <= 0 or inf: no cap): nodes farther away get +inf.  signed: the distance is negative where K17's
        mask (`contour_interior` with the same select and `flip`) is set -- the mask is made and used on the device.  Returns dist
        float64 (nslab, N, ny, nx), +inf where a contour has no selected segment[, edge, piece int64 (nslab, N, ny, nx): the e_from
        of the nearest segment (ties: the smallest) and the first_edge of its piece, -1 where dist is infinite].  The contours are
        taken in groups, so that the device holds no more output planes than one batch may stage."""
        a, ycoord, xcoord, radius, period, cap = self._cdist_args('xc_contour_distance', q, contours, ycoord, xcoord, radius, period, select,
                                                                  max_distance)
        ny, nx = a.ny, a.nx
        signed, near = bool(signed), bool(return_nearest)
        per_node = 8 + (16 if near else 0) + (1 if signed else 0)            # the bytes of one node's outputs, per contour
        ncg = max(1, min(a.N, int(self.max_batch_bytes) // (ny * nx * per_node)))

        def distance(head, ins, outs, mask, n, Ng):
            (dy, dx), dd = ins, outs[0]
            self._check(self.lib.xc_contour_distance_dev(*head, dy.ptr, dx.ptr, period if period is not None else 0.0, radius, cap, mask,
                                                         dd.ptr, *([b.ptr for b in outs[1:3]] if near else [None] * 2)))
            res = (dd.download((n, Ng, ny, nx), np.float64),)
            return res + tuple(b.download((n, Ng, ny, nx), np.int64) for b in outs[1:3]) if near else res[0]

        # beside K12's records: the coordinates, the planes of dist[, edge, piece] (and for the sign what `_cdist_groups` adds)
        return self._cdist_groups(a, ncg, (ycoord, xcoord), lambda n, Ng: [n * Ng * ny * nx * 8] * (3 if near else 1), per_node, distance,
                                  period is not None, signed, flip)

    def set_cdprofile_global(self, on):
        """whether every tile of `contour_distance_profile` adds its terms straight to the global words instead of an LDS window
        (xc_set_cdprofile_global; default off; the result does not depend on it: for tests and A/B timing)"""
        self._check(self.lib.xc_set_cdprofile_global(self.handle, 1 if on else 0))

    def last_cdprofile_profile(self):
        """the last xc_contour_distance_profile_dev call: dict(table_ms, binning_ms, distance_ms, bound_ms, finish_ms -- device
        times under set_kernel_timing(True) --, pairs_visited, pairs_total as `last_cdist_profile`, tiles_window, tiles_global:
        the tiles that accumulated in the LDS window / on the global words, groups)"""
        ms = (C.c_double * 5)()
        n, g = [_i64(0) for _ in range(4)], C.c_int(0)
        self._check(self.lib.xc_last_cdprofile_profile(self.handle, C.cast(ms, _vp), *[C.byref(v) for v in n], C.byref(g)))
        out = {k + '_ms': v for k, v in zip(('table', 'binning', 'distance', 'bound', 'finish'), ms)}
        out.update(zip(('pairs_visited', 'pairs_total', 'tiles_window', 'tiles_global'), (v.value for v in n)))
        out['groups'] = g.value
        return out

    def contour_distance_profile(self, q, contours, ycoord, xcoord, edges, w=None, fields=(), radius=0.0, period=None, select='all',
                                 max_distance=None, signed=False, flip=False):
        """Composites by distance from every contour (K28, xc_contour_distance_profile_dev, on the device records of K12): the
        distance of `contour_distance` -- same arguments, same bits -- binned on the device into `edges` (float64, finite,
        strictly ascending, 2 to XC_CDPROFILE_MAX_EDGES of them; M = len(edges) - 1 bins; in the distance's units, negative
        values with `signed`), and reduced there.  A node with distance d lies in bin b when edges[b] <= d < edges[b + 1], and
        d == edges[M] in bin M - 1 (np.histogram's rule); nodes with an infinite distance or outside the edges lie in none.
        w: None (weight 1), (ny, nx) or (nslab, ny, nx) float64; fields: at most XC_PROPS_MAXF f32 / f64 arrays, (ny, nx) or
        (nslab, ny, nx).  Returns (nodes int64 (nslab, N, M), area float64 (nslab, N, M): the sum of w, sums float64
        (nslab, N, nf, M): the sums of w f_m, each product rounded once, flags int32 (nslab, N, 1 + nf): where a term of the area
        or of field m, at a node inside a bin, was +-inf -- a NaN term sets nothing).  The sums are exact sums rounded once (NaN terms skipped, an infinite term makes that
        bin's sum NaN): the same bits whatever the order, the workspace or the batches.  No plane crosses to the host; the only
        per-node buffer beside the inputs is K17's mask with `signed`, and the contours are taken in groups under it."""
        who = 'xc_contour_distance_profile'
        edges = np.ascontiguousarray(np.asarray(edges, dtype=np.float64))
        if (edges.ndim != 1 or not 2 <= edges.size <= XC_CDPROFILE_MAX_EDGES or not np.isfinite(edges).all()
                or not (np.diff(edges) > 0.0).all()):
            raise XContourHipError(XC_EBADARG, '%s: edges must be 2 to 4097 finite, strictly ascending float64 values' % who)
        fields = tuple(fields)
        if len(fields) > XC_PROPS_MAXF:
            raise XContourHipError(XC_EBADARG, '%s: at most 8 fields (XC_PROPS_MAXF)' % who)
        a, ycoord, xcoord, radius, period, cap = self._cdist_args(who, q, contours, ycoord, xcoord, radius, period, select, max_distance,
                                                                  w=w, fields=fields)
        ny, nx, N, M, nf = a.ny, a.nx, a.N, edges.size - 1, len(a.fields)
        signed, has_w = bool(signed), a.w is not None
        # a contour takes one byte per node on the device (K17's mask) when signed, and no plane at all when not
        ncg = max(1, min(N, int(self.max_batch_bytes) // (ny * nx))) if signed else N

        def profile(head, ins, outs, mask, n, Ng):
            (dy, dx), dw, dfl = ins[:2], (ins[2] if has_w else None), ins[2 + has_w:]
            dnod, dar, dflag = outs[:3]
            dsum = outs[3] if nf else None
            fp = (_vp * max(nf, 1))(*[b.ptr for b in dfl])
            fd = (C.c_int * max(nf, 1))(*[dtype_code(v.dtype) for v in a.fields])
            fs = (C.c_int * max(nf, 1))(*[1 if v.ndim == 3 else 0 for v in a.fields])
            self._check(self.lib.xc_contour_distance_profile_dev(
                *head, dy.ptr, dx.ptr, period if period is not None else 0.0, radius, cap, mask, edges.size, _ptr(edges),
                Ng, dw.ptr if has_w else None, 1 if has_w and a.w.ndim == 3 else 0, nf, C.cast(fp, _vp), C.cast(fd, _vp),
                C.cast(fs, _vp), dnod.ptr, dar.ptr, dsum.ptr if nf else None, dflag.ptr))
            sums = (np.ascontiguousarray(np.moveaxis(dsum.download((nf, n, Ng, M), np.float64), 0, 2)) if nf
                    else np.empty((n, Ng, 0, M), dtype=np.float64))
            return (dnod.download((n, Ng, M), np.int64), dar.download((n, Ng, M), np.float64), sums,
                    dflag.download((n, Ng, 1 + nf), np.int32))

        def out_nbytes(n, Ng):
            return [n * Ng * M * 8, n * Ng * M * 8, n * Ng * (1 + nf) * 4] + ([nf * n * Ng * M * 8] if nf else [])

        # beside K12's records: the coordinates, the weights and the fields; the tables of nodes, area, flags and sums (and for the
        # sign what `_cdist_groups` adds)
        return self._cdist_groups(a, ncg, (ycoord, xcoord), out_nbytes, 1 if signed else 0, profile, period is not None, signed, flip)

    # the per-event table of `contour_folds`: the library's record, the two tongues (0 under, 1 over) side by side
    FOLD_DTYPE = np.dtype([('c_west', np.int32), ('c_east', np.int32), ('ncol', np.int32), ('ncross_max', np.int32),
                           ('row_lo', np.float64), ('row_hi', np.float64), ('nodes', np.int64, (2,)), ('area', np.float64, (2,)),
                           ('mx', np.float64, (2,)), ('my', np.float64, (2,)), ('integral', np.float64, (2,))])

    def last_cfold_profile(self):
        """device times of the last `contour_folds` call of the library under set_kernel_timing(True): dict(table_ms, rounds_ms,
        select_ms, columns_ms, runs_ms, scan_ms, rounds, groups)"""
        return self._last_profile('cfold', ('table', 'rounds', 'select', 'columns', 'runs', 'scan'))

    def contour_folds(self, q, contours, w=None, f=None, periodic=False, select='main', gap=0):
        """The folds of every contour gathered into events (K24, xc_contour_folds_dev, on the device records of K12: the segment
        records are never downloaded).  q, contours, periodic, select, w and f as for `contour_interior`.  A column is FOLDED when
        the selected pieces cross its grid line three times or more; its fold nodes are those between the lowest and the highest
        crossed edge, of tongue 0 ('under') where the crossings between the lowest one and the node are even in number, else of
        tongue 1 ('over').  An EVENT is a maximal run of folded columns with at most `gap` unfolded columns between consecutive
        ones, round the seam on a periodic plane.  One K12 call, then a count-only call and a sized one.  Returns (ncross int32,
        row_lo, row_hi float64 (nslab, N, nx): `contour_overturning`'s; col_event int32 (nslab, N, nx): the event of a folded
        column within its contour, else -1; event_count uint64 (nslab, N); events: a structured array (FOLD_DTYPE) of all events
        packed by (slab, contour), each range ordered by c_west -- c_west, c_east, ncol, ncross_max, row_lo, row_hi, and per tongue
        nodes, area (the sum of w), mx, my (of w dx, w row; dx the columns east of c_west), integral (of w f; NaN without f) --
        exact sums rounded once, NaN terms skipped, an infinite term makes that sum of that tongue of that event NaN)."""
        a = _RecordArgs('xc_contour_folds', q, contours, select=select, periodic=periodic, min_nx=2, labels32=True, w=w, f=f)
        ny, nx, N = a.ny, a.nx, a.N
        if isinstance(gap, bool) or not isinstance(gap, (int, np.integer)) or not 0 <= gap < nx:
            raise XContourHipError(XC_EBADARG, 'xc_contour_folds: gap must be an int in [0, nx), not %r' % (gap,))
        has_f = a.f is not None
        dt = self.FOLD_DTYPE
        cols = [(k,) + ((dt[k].base, 2) if dt[k].shape else (dt[k],)) for k in
                ('row_lo', 'row_hi', 'nodes', 'area', 'mx', 'my', 'integral', 'c_west', 'c_east', 'ncol', 'ncross_max')]
        dense = (np.int32, np.float64, np.float64, np.int32)

        def folds(cnt, total, dn, ins, outs, recs):
            n = cnt.shape[0]
            dec = outs[4]
            rec, wf = self._record_run(a, total, ins, recs)
            head = (self.handle, cnt.size, dn.ptr, *rec, ny, nx, 1 if periodic else 0, int(a.sel), N, *wf, int(gap), *[b.ptr for b in outs[:4]])

            def k24(cap, evs):
                at = _Columns(evs[0], cap, cols) if evs else None
                names = ('c_west', 'c_east', 'ncol', 'ncross_max', 'row_lo', 'row_hi', 'nodes', 'area', 'mx', 'my', 'integral')
                ptrs = [at.ptr(k, k != 'integral' or has_f) for k in names] if evs else [None] * 11
                return self.lib.xc_contour_folds_dev(*head, cap, dec.ptr, *ptrs)
            with self._two_pass(k24, dec, (n, N), lambda ne: [ne * _row_bytes(cols)]) as (ec, ne, evs):
                ev = np.empty(ne, dtype=dt)
                if ne:
                    at = _Columns(evs[0], ne, cols)
                    for k in dt.names:
                        if k == 'integral' and not has_f:
                            ev[k] = np.nan
                        elif dt[k].shape:
                            ev[k] = at.buf.download((ne, 2), dt[k].base, offset_bytes=at.at[k])
                        else:
                            ev[k] = at.get(k, (ne,))
                return tuple(b.download((n, N, nx), t) for b, t in zip(outs[:4], dense)) + (ec, ev)

        def one(s0, s1):
            # beside K12's records: the weights and the integrand, the four dense outputs -- 24 bytes per (contour, column) --, the event counts
            n = s1 - s0
            qb, cb, wb, fb = a.batch(s0, s1)[:4]
            nb = [n * N * nx * 4, n * N * nx * 8, n * N * nx * 8, n * N * nx * 4, n * N * 8]
            return self._with_segment_records(periodic, qb, cb, folds, inputs=[v for v in (wb, fb) if v is not None], out_nbytes=nb)
        return self._batched(a.nslab, a.slab_bytes() + N * nx * 24, one)

    # the per-piece table of `contour_piece_interiors`: K13's key fields and what the piece encloses
    PIECE_INTERIOR_DTYPE = np.dtype([('first_edge', np.int64), ('nseg', np.int64), ('closed', np.bool_), ('winding', np.int32),
                                     ('n_in', np.int64), ('sum_w', np.float64), ('sum_wf', np.float64)])

    def last_cpinside_profile(self):
        """device times of the last `contour_piece_interiors` batch under set_kernel_timing(True): dict(table_ms, rounds_ms,
        roots_ms, walk_ms, rounds, groups)"""
        return self._last_profile('cpinside', ('table', 'rounds', 'roots', 'walk'))

    def contour_piece_interiors(self, q, contours, w=None, f=None, periodic=False, flip=False):
        """What EVERY piece of every contour bounds (K18, xc_contour_piece_interiors_dev, on the device records of K12: the segment
        records are never downloaded).  q, contours, periodic, w, f and flip as for `contour_interior`; periodic needs nx >= 3.  For
        one ring the rule is `contour_interior`'s with that ring alone selected: a node (r, c) is inside a ring of winding 0 when the
        ring crosses the grid line of column c between row 0 and row r an odd number of times; for a ring of winding != 0 the other
        nodes when `flip`.  The nodes of a ring nested inside another count for the outer one too: `contour_piece_tree` gives the nesting.
        Returns (piece_count uint64 (nslab, N), table): `table` a structured array (PIECE_INTERIOR_DTYPE) of all pieces packed by
        (slab, contour) -- range (s, k) starts at the exclusive scan of piece_count --, each range sorted by first_edge: its rows line
        up with those of `contour_pieces`.  first_edge, nseg, closed, winding are that method's; n_in the inside nodes, sum_w the sum
        of w over them (None: weight 1), sum_wf that of w f (NaN without f) -- exact sums rounded once, NaN terms skipped, an infinite
        term makes that sum of that piece NaN.  An open piece bounds nothing: n_in -1, NaN sums."""
        return self._ring_tables('interiors', q, contours, w, f, periodic, flip)

    # the per-piece table of `contour_piece_tree`: that of `contour_piece_interiors` and where the piece hangs in the tree of its range
    PIECE_TREE_DTYPE = np.dtype(PIECE_INTERIOR_DTYPE.descr + [('parent', np.int64), ('depth', np.int32), ('nchild', np.int32),
                                                              ('n_net', np.int64), ('net_w', np.float64), ('net_wf', np.float64)])

    def last_cptree_profile(self):
        """device times of the last `contour_piece_tree` batch under set_kernel_timing(True): dict(table_ms, rounds_ms, roots_ms,
        walk_ms, tree_ms, rounds, groups)"""
        return self._last_profile('cptree', ('table', 'rounds', 'roots', 'walk', 'tree'))

    def contour_piece_tree(self, q, contours, w=None, f=None, periodic=False, flip=False):
        """Which piece of every contour is nested in which (K19, xc_contour_piece_tree_dev, on the device records of K12).  Arguments,
        packing and row order as for `contour_piece_interiors`, whose fields come first, bit for bit.  A ring encloses another ring of
        its (slab, contour) range when it holds all of the other's inside nodes.  Further fields: `parent` the ROW, counted from the
        start of the piece's own range (rows in first_edge order), of the innermost ring that encloses the piece, -1 for none; `depth`
        0 without parent, else the parent's + 1; `nchild` the rings whose parent the piece is; `n_net`, `net_w`, `net_wf` what
        n_in, sum_w, sum_wf become when the inside nodes of the children are taken out (exact sums rounded once; NaN exactly where
        the gross sum is).  An open piece is transparent: parent -1, depth 0, nchild 0, n_net -1, NaN net sums."""
        return self._ring_tables('tree', q, contours, w, f, periodic, flip)

    def last_cplabel_profile(self):
        """device times of the last `contour_piece_labels` batch under set_kernel_timing(True): dict(table_ms, rounds_ms, roots_ms,
        walk_ms, tree_ms, label_ms, rounds, groups)"""
        return self._last_profile('cplabel', ('table', 'rounds', 'roots', 'walk', 'tree', 'label'))

    def contour_piece_labels(self, q, contours, w=None, f=None, periodic=False, flip=False):
        """Which ring HOLDS every node (K20, xc_contour_piece_labels_dev, on the device records of K12).  Arguments as for
        `contour_piece_tree`.  Returns (piece_count, table, labels): the first two are `contour_piece_tree`'s, bit for bit; `labels`
        int32 (nslab, N, ny, nx) names per (slab, contour) the innermost ring round each node -- the one of its inside set (that of
        `contour_piece_interiors`) with the fewest nodes -- as the ROW of that range's rows of `table` (first_edge order, counted from
        the start of the range, like `parent`), -1 where no ring holds the node.  Open pieces never appear.  The nodes with label p
        are those `n_net`, `net_w`, `net_wf` of row p sum over; depth[label] + 1 rings hold a node."""
        a = _RecordArgs('xc_contour_piece_labels', q, contours, periodic=periodic, min_nx=3, labels32=True, w=w, f=f)

        def one(s0, s1):
            lshape = (s1 - s0, a.N, a.ny, a.nx)
            with self._temporaries([], [4 * lshape[0] * lshape[1] * lshape[2] * lshape[3]]) as (dmap,):
                pc, tab, rows, _ = self._piece_records('labels', a, s0, s1, flip, dest=dmap)
                if not rows.size:                                # no piece in the batch: no node is in a ring
                    return pc, tab, np.full(lshape, -1, dtype=np.int32)
                lab = dmap.download(lshape, np.int32)
            # the entry's label is a position inside the range as it packed the rows: -> the row of the range's sorted table
            _to_rows(lab, _scan(pc)[1].reshape(lshape[:2] + (1, 1)), rows)
            return pc, tab, lab
        return self._batched(a.nslab, a.slab_bytes(4 * a.N), one)

    XC_PROPS_MAXF = XC_PROPS_MAXF

    def last_cpprops_profile(self):
        """device times of the last `contour_piece_props` batch under set_kernel_timing(True): dict(table_ms, rounds_ms, roots_ms,
        walk_ms, tree_ms, scan_ms, fold_ms, rounds, groups)"""
        return self._last_profile('cpprops', ('table', 'rounds', 'roots', 'walk', 'tree', 'scan', 'fold'))

    def contour_piece_props(self, q, contours, w=None, fields=(), x=None, periodic=False, flip=False):
        """What every ring HOLDS of further fields (K21, xc_contour_piece_props_dev, on the device records of K12): the reductions
        over `contour_piece_labels`' map without the map.  q, contours, w, periodic and flip as for `contour_piece_tree` (no
        integrand).  fields: a sequence of at most XC_PROPS_MAXF f32 / f64 arrays, each (ny, nx) -- one plane for all slabs, uploaded
        once per batch -- or (nslab, ny, nx); x: the extremum field (nslab, ny, nx) f32 / f64, or None.  Returns (piece_count,
        table, props): the first two are `contour_piece_tree`'s, bit for bit; `props` a dict over the rows of `table`: 'net' and
        'gross' f64 (npiece, nf), the sums of w g_m over the nodes labelled with the ring and over its whole inside set (exact sums
        rounded once; NaN terms skipped; an infinite term makes that field's sum NaN for the ring that holds it and, gross, for every
        ring round it); with x 'x_min', 'x_max' f64 and 'at_min', 'at_max' int64 (else None): the extremum of x over the ring's
        net nodes that are not NaN and the flat node r nx + c it sits on (-0.0 below +0.0, ties to the smallest node; NaN and -1
        without such a node).  Open pieces: NaN and -1."""
        a = _RecordArgs('xc_contour_piece_props', q, contours, periodic=periodic, min_nx=3, labels32=True, w=w, fields=tuple(fields), x=x)

        def one(s0, s1):
            pc, tab, _, props = self._piece_records('props', a, s0, s1, flip)
            return pc, tab, props
        return self._batched(a.nslab, a.slab_bytes(), one)

    def _ring_tables(self, stage, q, contours, w, f, periodic, flip):
        """`contour_piece_interiors` / `contour_piece_tree`: the tables of stage 'interiors' / 'tree', batch by batch"""
        a = _RecordArgs('xc_contour_piece_' + stage, q, contours, periodic=periodic, min_nx=3, labels32=True, w=w, f=f)
        return self._batched(a.nslab, a.slab_bytes(), lambda s0, s1: self._piece_records(stage, a, s0, s1, flip)[:2])

    # K21's columns behind a ring's record: the sums per field, net and gross, then the extremum of x and where it sits
    _PROPS_X = [('x_min', np.float64), ('x_max', np.float64), ('at_min', np.int64), ('at_max', np.int64)]

    def _labels_on_device(self, a, s0, s1, flip, dest):
        """the 'labels' stage of `_piece_records` for a caller that keeps the map on the device: `dest` holds the map afterwards
        -- -1 everywhere when the batch had no segments.  Returns (piece_count, table, rows)"""
        pc, tab, rows, _ = self._piece_records('labels', a, s0, s1, flip, dest=dest)
        if not rows.size:
            dest.upload(np.full(pc.shape + (a.ny, a.nx), -1, dtype=np.int32))
        return pc, tab, rows

    def _piece_records(self, stage, a, s0, s1, flip, dest=None):
        """The ring records of ONE batch, slabs [s0, s1) of the checked arguments `a`, through the entry point of `stage`: the
        stages are cumulative -- 'interiors' (K18), 'tree' (K19: + the nesting), then 'labels' (K20: + the map, written to `dest`, a
        DeviceBuffer or view of the caller's, where it stays) or 'props' (K21: + the sums and extrema of a.fields, a.x).  Returns
        (piece_count (n, N), table, rows, props): the table of the stage (PIECE_INTERIOR_DTYPE, from 'tree' on PIECE_TREE_DTYPE),
        every range sorted by first_edge; `rows` (`_row_map`), which turns what the device counts in its packed order -- the
        labels in `dest` -- into rows of the table; `props` K21's columns in the table's order, None for the other stages.  A
        batch without segments has no rows and leaves `dest` as it was (`_labels_on_device` fills it)."""
        tree = stage != 'interiors'
        qb, cb, wb, fb, fields, xb = a.batch(s0, s1)
        ny, nx, N, periodic = a.ny, a.nx, a.N, a.periodic
        nfld, has_w, has_f, has_x = len(fields), wb is not None, fb is not None, xb is not None
        dt = self.PIECE_TREE_DTYPE if tree else self.PIECE_INTERIOR_DTYPE
        # one piece record per segment at most: the table's 8-byte columns, then its others as 4-byte ones, then K21's
        cols = [(k, dt[k]) for k in dt.names if dt[k].itemsize == 8] + [(k, np.int32) for k in dt.names if dt[k].itemsize != 8]
        if stage == 'props':
            cols += [('net', np.float64, nfld), ('gross', np.float64, nfld)] + self._PROPS_X

        def records(cnt, total, dn, ins, outs, recs):
            if total == 0:
                return (np.zeros(cnt.shape, dtype=np.uint64), np.empty(0, dtype=dt), np.empty(0, dtype=np.int64),
                        self._ring_props(None, 0, 0, nfld, has_x, None) if stage == 'props' else None)
            dpc, at = outs[0], _Columns(recs[3], total, cols)
            p = at.ptr
            rec, wf = self._record_run(a, total, ins, recs)
            args = [self.handle, cnt.size, dn.ptr, *rec, ny, nx, 1 if periodic else 0, 1 if flip else 0, N, *wf, total, dpc.ptr,
                    p('first_edge'), p('nseg'), p('closed'), p('winding'), p('n_in'), p('sum_w'), p('sum_wf', has_f)]
            if tree:
                args += [p('parent'), p('depth'), p('nchild'), p('n_net'), p('net_w'), p('net_wf', has_f)]
            if stage == 'labels':
                args.append(dest.ptr)
            if stage == 'props':
                dflds = ins[has_w + has_f:has_w + has_f + nfld]
                gp = (_vp * max(nfld, 1))(*[b.ptr for b in dflds])
                gd = (C.c_int * max(nfld, 1))(*[dtype_code(v.dtype) for v in fields])
                gs = (C.c_int * max(nfld, 1))(*[1 if v.ndim == 3 else 0 for v in fields])
                args += [nfld, C.cast(gp, _vp), C.cast(gd, _vp), C.cast(gs, _vp), ins[-1].ptr if has_x else None,
                         dtype_code(xb.dtype) if has_x else 0, p('net', nfld), p('gross', nfld)] + [p(k, has_x) for k, _ in self._PROPS_X]
            self._check(getattr(self.lib, 'xc_contour_piece_%s_dev' % stage)(*args))
            pc = dpc.download(cnt.shape, np.uint64)
            out = np.empty(int(pc.sum()), dtype=dt)
            nof = [k for k in ('sum_wf', 'net_wf') if not has_f and k in dt.names]
            for k in nof:
                out[k] = np.nan
            at.into(out, skip=nof)
            order, rows = _row_map(pc, out['first_edge'])
            if tree:
                _to_rows(out['parent'], 0, rows)                 # the entry's parent is an index into the rows as it packed them
            return pc, out[order], rows, self._ring_props(at, out.size, total, nfld, has_x, order) if stage == 'props' else None
        # beside K12's records: the weights, the integrand, the fields and the extremum field, the piece counts, and the piece records
        ins = [v for v in (wb, fb) if v is not None] + fields + ([xb] if has_x else [])
        return self._with_segment_records(periodic, qb, cb, records, inputs=ins, out_nbytes=((s1 - s0) * N * 8,),
                                          per_segment=(_row_bytes(cols),))

    def _ring_props(self, at, npiece, total, nfld, has_x, order):
        """K21's per-piece columns out of the record block `at` (of capacity `total`), as rows in the table's sorted order"""
        cols = {}
        for name in ('net', 'gross'):                            # sub-column m of a per-field column starts at m * capacity
            cols[name] = (np.ascontiguousarray(at.get(name, (nfld, total))[:, :npiece].T[order]) if nfld and npiece
                          else np.empty((npiece, nfld)))
        for name, t in self._PROPS_X:
            cols[name] = None if not has_x else at.get(name, (npiece,))[order] if npiece else np.empty(0, dtype=t)
        return cols

    # the rows of `label_overlap` and `contour_piece_overlap`: one per pair of labels that share a node
    OVERLAP_DTYPE = np.dtype([('a', np.int32), ('b', np.int32), ('n', np.int64), ('sum_w', np.float64), ('sum_wf', np.float64)])

    def last_cpoverlap_profile(self):
        """device times of the last xc_label_overlap_dev call (the last batch of `label_overlap` / `contour_piece_overlap`) under
        set_kernel_timing(True): dict(runs_ms, accumulate_ms, finish_ms, rounds (0), groups)"""
        return self._last_profile('cpoverlap', ('runs', 'accumulate', 'finish'))

    def _overlap_rows(self, nrange, ny, nx, ncont, pa, pb, wb=None, fb=None):
        """K22 on two maps that lie on the device (pa, pb: device addresses), with the call's slices of w and f (host arrays or
        None) staged for it: a count-only call, then a sized one -> (pair_count uint64 (nrange,), the rows (OVERLAP_DTYPE) packed
        by range, in the call's own order)"""
        dt = self.OVERLAP_DTYPE
        cols = [(k, dt[k]) for k in dt.names]                    # the 4-byte columns, then the 8-byte ones
        has_w, has_f = wb is not None, fb is not None
        with self._temporaries([v for v in (wb, fb) if v is not None], [nrange * 8]) as bufs:
            dpc = bufs[-1]
            head = (self.handle, nrange, ny, nx, ncont, pa, pb, bufs[0].ptr if has_w else None, 1 if has_w and wb.ndim == 3 else 0,
                    bufs[has_w].ptr if has_f else None, dtype_code(fb.dtype) if has_f else 0)
            block = []                                           # the row block of the sized call, described once

            def k22(total, outs):
                block[:] = [_Columns(b, total, cols) for b in outs]
                at = [block[0].ptr(k, k != 'sum_wf' or has_f) for k in dt.names] if outs else [None] * 5
                return self.lib.xc_label_overlap_dev(*head, total, dpc.ptr, *at)
            with self._two_pass(k22, dpc, (nrange,), lambda total: [total * _row_bytes(cols)]) as (pc, total, outs):
                rows = np.empty(total, dtype=dt)
                rows['sum_wf'] = np.nan
                if total:
                    block[0].into(rows, skip=() if has_f else ('sum_wf',))
                return pc, rows

    @staticmethod
    def _sorted_overlap(pc, rows):
        """rows packed by range -> each range sorted by (a, b)"""
        return rows[np.lexsort((rows['b'], rows['a'], _range_of(pc)))]

    def label_overlap(self, lab_a, lab_b, w=None, f=None):
        """Which labels of two maps share nodes (K22, xc_label_overlap_dev): the contingency table of two label maps, built on the
        device.  lab_a, lab_b int32 of one shape, (nrange, ny, nx) -- every range its own slab -- or (nslab, N, ny, nx): the maps
        of `contour_piece_labels` of two fields.  w None (weight 1), (ny, nx) or (nslab, ny, nx) f64; f None or (nslab, ny, nx)
        f32 / f64.  Any negative label is "no ring" and comes back as -1.  Returns (pair_count uint64 (nrange,) or (nslab, N),
        rows): `rows` a structured array (OVERLAP_DTYPE) packed by range -- range r starts at the exclusive scan of pair_count --,
        each range sorted by (a, b): one row per pair of labels that occurs on a node, the pair (-1, -1) left out, with n the
        nodes of the pair, sum_w the sum of w and sum_wf that of w f over them (NaN without f): exact sums rounded once, NaN terms
        skipped, an infinite term makes that sum of that pair NaN."""
        who = 'xc_label_overlap'
        lab_a, lab_b = _contig(lab_a, np.int32), _contig(lab_b, np.int32)
        if lab_a.ndim not in (3, 4) or lab_a.shape != lab_b.shape or lab_a.size == 0:
            raise XContourHipError(XC_EBADARG, '%s: two maps of one shape, (nrange, ny, nx) or (nslab, N, ny, nx)' % who)
        lead, (ny, nx) = lab_a.shape[:-2], lab_a.shape[-2:]
        nslab, N = lead[0], (lead[1] if len(lead) == 2 else 1)
        lab_a, lab_b = lab_a.reshape(nslab, N, ny, nx), lab_b.reshape(nslab, N, ny, nx)
        wf = _RecordArgs(who, shape=(nslab, ny, nx), w=w, f=f)

        def one(s0, s1):
            with self._temporaries([lab_a[s0:s1], lab_b[s0:s1]], []) as (da, db):
                pc, rows = self._overlap_rows((s1 - s0) * N, ny, nx, N, da.ptr, db.ptr, _part(wf.w, 3, s0, s1), _part(wf.f, 3, s0, s1))
            return pc.reshape(s1 - s0, N), self._sorted_overlap(pc, rows)
        pc, rows = self._batched(nslab, wf.slab_bytes(2 * 4 * N), one)
        return pc.reshape(lead), rows

    def contour_piece_overlap(self, qa, qb, contours, contours_b=None, w=None, f=None, periodic=False, flip=False):
        """Which rings of two fields share nodes (K20 on each field, then K22, xc_label_overlap_dev): both label maps stay on the
        device, only the two piece tables and the overlap rows are downloaded.  qa, qb (nslab, ny, nx) of one shape; contours
        (levels of qa) and contours_b (levels of qb; None: `contours`) (N,) or (nslab, N), ascending; w, f, periodic and flip as
        for `contour_piece_tree`, the same for both fields.  Returns (pc_a, table_a, pc_b, table_b, pair_count, rows): the first
        four are `contour_piece_tree`'s of the two fields, bit for bit; pair_count uint64 (nslab, N) and `rows` (OVERLAP_DTYPE)
        as for `label_overlap`, with a and b the ROWS of the range's rows of table_a / table_b (counted from the start of the
        range, like `parent`), -1 for "in no ring"; range (s, k) pairs level k of qa with level k of qb."""
        who = 'xc_contour_piece_overlap'
        qa, (nslab, ny, nx) = _stack3(qa)
        qb, shape_b = _stack3(qb)
        if tuple(shape_b) != (nslab, ny, nx):
            raise XContourHipError(XC_EBADARG, '%s: the two fields must have one shape' % who)
        ca, _, N = _levels_of(contours, nslab)
        cb, _, Nb = _levels_of(contours if contours_b is None else contours_b, nslab)
        if Nb != N:
            raise XContourHipError(XC_EBADARG, '%s: as many levels for the one field as for the other' % who)
        a = _RecordArgs(who, shape=(nslab, ny, nx), w=w, f=f)   # (a bad w or f is reported before a bad level)
        a.plane(qa, ca, periodic=periodic, min_nx=3, labels32=True)
        b = a.on(qb, cb)
        slot = N * ny * nx * 4

        def one(s0, s1):
            n = s1 - s0
            with self._temporaries([], [n * slot, n * slot]) as maps:
                ta, tb = (self._labels_on_device(v, s0, s1, flip, m) for v, m in zip((a, b), maps))
                pc, rows = self._overlap_rows(n * N, ny, nx, N, maps[0].ptr, maps[1].ptr, _part(a.w, 3, s0, s1), _part(a.f, 3, s0, s1))
            # the device labels are positions in each call's packed order: -> rows of the first_edge-sorted tables
            for key, t in (('a', ta), ('b', tb)):
                _to_rows(rows[key], _scan(t[0])[1][_range_of(pc)], t[2])
            return ta[0], ta[1], tb[0], tb[1], pc.reshape(n, N), self._sorted_overlap(pc, rows)
        return self._batched(nslab, a.slab_bytes(qb.dtype.itemsize + 2 * 4 * N), one)

    # the rows of `ring_tracks`: one per track
    TRACK_DTYPE = np.dtype([('first_ring', np.int64), ('first_step', np.int32), ('last_step', np.int32), ('nrings', np.int64),
                            ('nsplit', np.int64), ('nmerge', np.int64)])
    # what `contour_piece_tracks` adds per ring, per link and per track
    RING_TRACK_DTYPE = np.dtype([('track', np.int64), ('nprev', np.int32), ('nnext', np.int32)])
    TRACK_LINK_DTYPE = np.dtype([('step', np.int32)] + OVERLAP_DTYPE.descr[:4] + [('linked', np.bool_)])
    PIECE_TRACK_DTYPE = np.dtype([('first_step', np.int32), ('first_row', np.int64), ('last_step', np.int32), ('nrings', np.int64),
                                  ('nsplit', np.int64), ('nmerge', np.int64)])

    def last_cptrack_profile(self):
        """the last xc_ring_tracks_dev call: dict(accept_ms, rounds_ms, finish_ms -- device times under set_kernel_timing(True) --,
        rounds: the hook / compress rounds, the last, unchanged one included)"""
        return self._last_profile('cptrack', ('accept', 'rounds', 'finish'), groups=False)

    def ring_tracks(self, ring_step, ring_size, link_a, link_b, link_n, min_overlap=0.0):
        """The connected components of a ring graph (K23, xc_ring_tracks_dev): ring_step int32 (nring,), ring_size int64 (nring,) or
        None (min_overlap 0 only), link_a / link_b / link_n int64 (nlink,), any negative index "no ring".  A link is accepted when
        a >= 0, b >= 0, n >= 1 and n >= min_overlap * min(size[a], size[b]).  Everything is uploaded once; a count-only call, then
        a sized one; only the outputs come back.  Returns dict(root int64, track int64, nprev int32, nnext int32 (nring,); link_ok
        bool (nlink,); tracks (TRACK_DTYPE) in the order of their first rings)."""
        ring_step = _contig(ring_step, np.int32)
        la, lb, ln = (_contig(a, np.int64) for a in (link_a, link_b, link_n))
        nring, nlink = ring_step.size, la.size
        if ring_step.ndim != 1 or la.ndim != 1 or lb.shape != la.shape or ln.shape != la.shape:
            raise XContourHipError(XC_EBADARG, 'xc_ring_tracks: ring_step (nring,), link_a, link_b and link_n (nlink,)')
        if ring_size is not None:
            ring_size = _contig(ring_size, np.int64)
            if ring_size.shape != ring_step.shape:
                raise XContourHipError(XC_EBADARG, 'xc_ring_tracks: ring_size must be (nring,)')
        if nring == 0:
            if nlink:
                raise XContourHipError(XC_EBADARG, 'xc_ring_tracks: links without rings')
            return dict(root=np.empty(0, np.int64), track=np.empty(0, np.int64), nprev=np.empty(0, np.int32), nnext=np.empty(0, np.int32),
                        link_ok=np.empty(0, np.bool_), tracks=np.empty(0, dtype=self.TRACK_DTYPE))
        # per ring root, track (8 bytes), nprev, nnext (4 bytes); per track four 8-byte and two 4-byte columns
        ring_cols = [('root', np.int64), ('track', np.int64), ('nprev', np.int32), ('nnext', np.int32)]
        dt = self.TRACK_DTYPE
        track_cols = [(k, dt[k]) for k in ('first_ring', 'nrings', 'nsplit', 'nmerge', 'first_step', 'last_step')]
        ins = [ring_step] + ([ring_size] if ring_size is not None else []) + ([la, lb, ln] if nlink else [])
        with self._temporaries(ins, [8]) as bufs:
            dsize = bufs[1].ptr if ring_size is not None else None
            dl = [b.ptr for b in bufs[-4:-1]] if nlink else [None] * 3
            head = (self.handle, nring, nlink, bufs[0].ptr, dsize, *dl, float(min_overlap))
            dnt = bufs[-1]

            def k23(nt, outs):
                if not outs:
                    return self.lib.xc_ring_tracks_dev(*head, *[None] * 5, 0, dnt.ptr, *[None] * 6)
                rat = _Columns(outs[0], nring, ring_cols).ptrs(k for k, _ in ring_cols)
                return self.lib.xc_ring_tracks_dev(*head, *rat, outs[1].ptr, nt, dnt.ptr, *_Columns(outs[2], nt, track_cols).ptrs(dt.names))
            sizes = lambda nt: [nring * _row_bytes(ring_cols), max(nlink, 1), nt * _row_bytes(track_cols)]       # noqa: E731
            with self._two_pass(k23, dnt, (1,), sizes, always=True) as (_, nt, (dring, dok, drow)):
                ring = _Columns(dring, nring, ring_cols)
                out = {k: ring.get(k, (nring,)) for k, _ in ring_cols}
                out['link_ok'] = dok.download((nlink,), np.uint8).astype(np.bool_)
                out['tracks'] = _Columns(drow, nt, track_cols).into(np.empty(nt, dtype=dt))
        return out

    def contour_piece_tracks(self, q, contours, w=None, f=None, periodic=False, flip=False, min_overlap=0.0):
        """The rings of a stack of fields FOLLOWED through the stack (K20 on every step ONCE, K22 between consecutive steps, K23,
        xc_ring_tracks_dev, over all of them).  q (nstep, ny, nx): the steps of one series, in order; contours, w, f, periodic and
        flip as for `contour_piece_tree`; min_overlap in [0, 1]: a link counts when its shared nodes are at least that fraction of
        the smaller ring's n_net (0: any shared node).
        The steps are cut into batches from `max_batch_bytes`.  A batch of n steps writes its label maps into slots 1 .. n of one
        device buffer of (n + 1) maps; slot 0 is the last map of the batch before, copied device to device, so ONE K22 call per
        batch pairs slot j with slot j + 1 -- range (t, k) pairs step t - 1 with step t at level k -- and no map reaches the host.
        K22 runs without f and with w as given (a per-step w: the earlier step's).
        Returns (piece_count, table, ring, link_count, links, track_count, tracks): the first two are `contour_piece_tree`'s, bit
        for bit; `ring` (RING_TRACK_DTYPE) lines up with `table`: track a row of the level's rows of `tracks`, nprev / nnext the
        accepted links to the step before / after; link_count uint64 (nstep - 1, N) and `links` (TRACK_LINK_DTYPE) packed by
        (step, level), each range sorted by (a, b): K22's rows of step `step` against step + 1 (a, b rows of the two ranges' sorted
        tables, -1 "in no ring") with `linked`; track_count uint64 (N,) and `tracks` (PIECE_TRACK_DTYPE) packed by level, in the
        order of their first rings' (step, row).  An open piece has no links and is a track of one."""
        who = 'xc_contour_piece_tracks'
        q, (nstep, ny, nx) = _stack3(q)
        contours, _, N = _levels_of(contours, nstep)
        mo = float(min_overlap)
        if not 0.0 <= mo <= 1.0:
            raise XContourHipError(XC_EBADARG, '%s: min_overlap must lie in [0, 1]' % who)
        a = _RecordArgs(who, shape=(nstep, ny, nx), w=w, f=f)   # (a bad w or f is reported before a bad level)
        a.plane(q, contours, periodic=periodic, min_nx=3, labels32=True)
        bt = self._batches(nstep, a.slab_bytes(4 * N))
        slot = N * ny * nx * 4
        nb0 = bt[0][1] - bt[0][0]
        pcs, tabs, lcs, lks = [], [], [], []
        last = None                                              # of the step before the batch: (its piece counts (1, N), its rows)
        with self._temporaries([], [(nb0 + 1) * slot]) as (maps,):
            for s0, s1 in bt:
                n = s1 - s0
                if last is not None:                             # the map of the step before: slot n of the batch before -> slot 0
                    self.comm_wait_compute()
                    self.comm_memcpy_d2d(maps.ptr, maps.ptr + nb0 * slot, slot)
                    self.compute_wait_comm()
                pc, tab, rows = self._labels_on_device(a, s0, s1, flip, _DeviceView(maps, slot, n * slot))
                pcs.append(pc)
                tabs.append(tab)
                first = 1 if last is None else 0                 # the slot of the earlier field of the batch's first pair
                if n - first:
                    # K22 runs without f and with w as given -- a per-step w: the earlier step's
                    lc, lk = self._overlap_rows((n - first) * N, ny, nx, N, maps.ptr + first * slot, maps.ptr + (first + 1) * slot,
                                                _part(a.w, 3, s0 + first - 1, s1 - 1))
                    # the device labels are positions in each step's packed order: -> rows of the first_edge-sorted tables
                    spc = pc if last is None else np.concatenate([last[0], pc])
                    srows = rows if last is None else np.concatenate([last[1], rows])
                    start = _scan(spc)[1].reshape(spc.shape)
                    rng = _range_of(lc)
                    for key, j in (('a', 0), ('b', 1)):
                        _to_rows(lk[key], start[rng // N + j, rng % N], srows)
                    lk = _named(self._sorted_overlap(lc, lk), self.TRACK_LINK_DTYPE)
                    lk['step'] = s0 + first - 1 + rng // N
                    lcs.append(lc.reshape(n - first, N))
                    lks.append(lk)
                last = (pc[-1:], rows[int(pc[:-1].sum()):])
        pc, tab = np.concatenate(pcs), np.concatenate(tabs)
        lc = np.concatenate(lcs) if lcs else np.zeros((0, N), dtype=np.uint64)
        links = np.concatenate(lks) if lks else np.empty(0, dtype=self.TRACK_LINK_DTYPE)
        # ring indices, level-major: all steps of level 0, then level 1, ...: base[t, k] is the first ring of range (t, k)
        cnt = pc.astype(np.int64).reshape(nstep, N)
        base = _scan(cnt.T)[1].reshape(N, nstep).T
        lvl0 = np.concatenate([base[0], [cnt.sum()]])            # where every level starts
        npiece = tab.size
        where = np.repeat(base.ravel(), cnt.ravel()) + np.arange(npiece) - np.repeat(_scan(cnt)[1], cnt.ravel())
        ring_step, ring_size = np.empty(npiece, dtype=np.int32), np.empty(npiece, dtype=np.int64)
        ring_step[where] = _range_of(cnt) // N
        ring_size[where] = tab['n_net']
        lrange = _range_of(lc)
        lstep, llev = lrange // N, lrange % N
        la = np.where(links['a'] >= 0, base[lstep, llev] + links['a'], -1) if links.size else np.empty(0, dtype=np.int64)
        lb = np.where(links['b'] >= 0, base[np.minimum(lstep + 1, nstep - 1), llev] + links['b'], -1) if links.size else np.empty(0, dtype=np.int64)
        got = self.ring_tracks(ring_step, ring_size, la, lb, links['n'], mo)
        links['linked'] = got['link_ok']
        # every level's rings are contiguous, so its tracks are a run of dense ids: the level's base is taken off
        trows = got['tracks']
        tlev = np.searchsorted(lvl0, trows['first_ring'], side='right') - 1
        tcount = np.bincount(tlev, minlength=N)[:N].astype(np.uint64)
        ring = np.empty(npiece, dtype=self.RING_TRACK_DTYPE)
        ring['track'] = got['track'][where] - _scan(tcount)[1][_range_of(cnt) % N]
        ring['nprev'], ring['nnext'] = got['nprev'][where], got['nnext'][where]
        tracks = _named(trows, self.PIECE_TRACK_DTYPE)
        tracks['first_row'] = trows['first_ring'] - base[trows['first_step'], tlev]
        return pc, tab, ring, lc, links, tcount, tracks

    def local_contour_lengths(self, q, ycoord, xcoord, window, stride, min_periods, levels=None, radius=0.0, period=None):
        """Sliding-window contour lengths (xc_local_contour_lengths).  q (nslab, ny, nx) f32/f64 (or a lazy stack); ycoord (ny,) /
        xcoord (nx,) as for contour_lengths; window (wy, wx) nodes, both >= 2; stride (sy, sx), both >= 1: the windows are centred
        on the nodes (0, sy, 2 sy, ...) x (0, sx, ...) and clipped to the plane.  levels: None -- every window is traced at its
        NaN-skipping mean (NaN with fewer than `min_periods` valid nodes) --, a scalar, or an array over (nslab, nwy, nwx) /
        (nwy, nwx).  Returns (lengths f64 (nslab, nwy, nwx), NaN where the total is 0; the levels used f64; segment counts
        uint64).  A tracer with a device mirror (keep_resident) is read in place through the _dev entry point.  period: None, or
        the period of the X coordinate as for contour_lengths: windows are then not clipped in X but run on round the ring
        (xc_local_contour_lengths_periodic; the window must not be wider than the ring, wx <= nx)."""
        q, (nslab, ny, nx) = _stack3(q)
        (wy, wx), (sy, sx) = (int(v) for v in window), (int(v) for v in stride)
        if wy < 2 or wx < 2:
            raise XContourHipError(XC_EBADARG, 'xc_local_contour_lengths: the window must be at least 2 x 2 nodes')
        if sy < 1 or sx < 1:
            raise XContourHipError(XC_EBADARG, 'xc_local_contour_lengths: strides must be >= 1')
        ycoord, xcoord = _plane_coords(ycoord, xcoord, ny, nx, 'xc_local_contour_lengths')
        _check_finite('xc_local_contour_lengths', ycoord, xcoord)
        if period is not None:
            period = _check_period(period, xcoord, 'xc_local_contour_lengths_periodic')
            if wx > nx:
                raise XContourHipError(XC_EBADARG, 'xc_local_contour_lengths_periodic: the window must not be wider than the ring '
                                       '(wx <= nx)')
        nwy, nwx = -(-ny // sy), -(-nx // sx)
        if levels is not None:
            levels = np.asarray(levels, dtype=np.float64)
            if levels.shape not in ((), (nwy, nwx), (nslab, nwy, nwx)):
                raise XContourHipError(XC_EBADARG, 'levels must be a scalar, (nwy, nwx) or (nslab, nwy, nwx)')
            levels = np.ascontiguousarray(np.broadcast_to(levels, (nslab, nwy, nwx)))
        f_host, f_dev, ring = self._ring_forms('xc_local_contour_lengths', period)
        rest = ring + (float(radius), wy, wx, sy, sx, int(min_periods))
        ob = nwy * nwx * 8

        def one(s0, s1):
            n = s1 - s0
            qb, lb = _stack_now(q, s0, s1), _part(levels, 3, s0, s1)
            wins = (n, nwy, nwx)
            return tuple(self._twin(f_host, f_dev, qb, [ycoord, xcoord, lb], [(wins, np.float64), (wins, np.float64), (wins, np.uint64)],
                                    lambda pq, ins, outs: (pq, dtype_code(q.dtype), n, ny, nx, *ins[:2], *rest, ins[2], *outs)))
        return self._batched(nslab, ny * nx * q.dtype.itemsize + 4 * ob, one)

    def lwa(self, q, Q, coord, dA, dA_max, M=None, increase=True, part=0, mask_idx=None, variant=0, exact=None):
        """`exact`: None (default) -- planes of up to 512 rows are summed in numpy's own order (bit-exact band walk), larger ones by
        the O(ny log ny) interval kernel when the reference state is monotone (checked on the device); True -- the band walk for
        every plane; False -- the interval kernel for every plane whose premises hold: they are checked HERE, on the host copy of
        Q, the coordinate and the tracer (Q finite, s Q non-decreasing, the coordinate strictly monotone, no infinite tracer
        cell -- NaN cells are fine), and vouched for to the library,
        so the call is one launch (xc_set_lwa_exact modes 0 / 1 / 3); agreement ~1e-13 of the plane's largest value."""
        q = _stack_in(q)
        assert q.ndim == 3
        nslab, ny, nx = q.shape
        Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(nslab, ny)
        coord = np.ascontiguousarray(coord, dtype=np.float64)
        dA = np.ascontiguousarray(dA, dtype=np.float64)
        dr = _weight_rank(dA.shape, ny, nx)
        mr = XC_DA_NONE
        if M is not None:
            M = np.ascontiguousarray(M, dtype=np.float64)
            mr = _weight_rank(M.shape, ny, nx)
        nmask = 0 if mask_idx is None else len(mask_idx)
        mi = np.ascontiguousarray(mask_idx, dtype=np.int32) if nmask else None
        vouch = exact is not None and not exact and variant == 0
        if vouch:
            sg = 1.0 if increase else -1.0
            dc = np.diff(coord)
            dc_ok = bool((dc > 0).all() or (dc < 0).all())

        def one(s0, s1):
            qb, Qb = _stack_now(q, s0, s1), Q[s0:s1]
            out = np.empty(qb.shape, dtype=np.float64)
            mo = np.empty((s1 - s0, nmask, ny, nx), dtype=np.int8) if nmask else None
            mode = 0 if exact is None else (1 if exact else 0)
            if vouch:
                # FINITE, not only NaN-free: an infinite Q_j would make (Q'_j - c) * S0 = inf * 0 = NaN where the reference sums to 0
                ok = bool(np.isfinite(Qb).all()) and bool((np.diff(sg * Qb, axis=1) >= 0).all()) and dc_ok and not bool(np.isinf(qb).any())
                mode = 3 if ok else 1
            self._check(self.lib.xc_set_lwa_exact(self.handle, mode))
            try:
                self._check(self.lib.xc_lwa(self.handle, _ptr(qb), dtype_code(q.dtype), _ptr(Qb), _ptr(coord),
                                            _ptr(dA), dr, float(dA_max), _ptr(M), mr, s1 - s0, ny, nx,
                                            1 if increase else 0, int(part), int(variant), _ptr(mi), nmask, _ptr(out), _ptr(mo)))
            finally:
                self.lib.xc_set_lwa_exact(self.handle, 0)
            return out, mo
        return self._batched(nslab, ny * nx * (q.dtype.itemsize + 8 + nmask), one)

    def sort_profile(self, q, dA=None, mask=None, targets=None, tbl=None, coord=None,
                     want_sorted=False, want_acum=False, negate=False):
        """Exact adiabatic rearrangement (xc_sort_profile_batch).  q (ny, nx): one plane -> scalars / 1-D arrays
        as before; q (nslab, ny, nx): a stack sorted by ONE set of launches -> leading slab dim on every
        output ('nvalid' (nslab,), 'Q' (nslab, J), 'q_sorted' / 'acum' (nslab, ny*nx), 'bpe' (nslab,)).
        dA: None | (ny,) | (ny, nx) | (nslab, ny, nx); mask: (ny, nx) or (nslab, ny, nx)."""
        q = _stack_in(q)
        single = q.ndim == 2
        if single:
            q = q[None]
        assert q.ndim == 3
        nslab, ny, nx = q.shape
        rank = XC_DA_NONE
        if dA is not None:
            dA = np.ascontiguousarray(dA, dtype=np.float64)
            rank = _weight_rank(dA.shape, ny, nx, nslab, 'dA must be (ny,), (ny, nx) or (nslab, ny, nx)')
        per_slab = 0
        if mask is not None:
            mask = _f48(np.ascontiguousarray(mask))
            if mask.shape == (nslab, ny, nx) and not (single and mask.ndim == 2):
                per_slab = 1
            elif mask.shape != (ny, nx):
                raise XContourHipError(XC_EBADARG, 'mask must be (ny, nx) or (nslab, ny, nx)')
        J = ntbl = 0
        if targets is not None:
            targets = np.ascontiguousarray(targets, dtype=np.float64)
            J = len(targets)
        if tbl is not None:
            tbl = np.ascontiguousarray(tbl, dtype=np.float64)
            coord = np.ascontiguousarray(coord, dtype=np.float64)
            ntbl = len(tbl)
        # staged per slab: the tracer, per-slab mask / dA, the requested full-length outputs and the sort's own four work arrays
        per = ny * nx * (q.dtype.itemsize + 32 + (8 if want_sorted else 0) + (8 if want_acum else 0) +
                         (8 if rank == XC_DA_SLAB else 0) + (8 if per_slab else 0))

        def one(s0, s1):
            n = s1 - s0
            qb, db, mb = _stack_now(q, s0, s1), _part(dA, 3, s0, s1), _part(mask, 3, s0, s1)
            Q = np.empty((n, J), dtype=np.float64) if targets is not None else None
            qs = np.empty((n, ny * nx), dtype=np.float64) if want_sorted else None
            ac = np.empty((n, ny * nx), dtype=np.float64) if want_acum else None
            nv = np.zeros(n, dtype=np.uint32)
            bpe = np.zeros(n, dtype=np.float64) if tbl is not None else None
            self._check(self.lib.xc_sort_profile_batch(self.handle, _ptr(qb), dtype_code(q.dtype), _ptr(mb),
                                                       dtype_code(mask.dtype) if mask is not None else XC_F64, per_slab,
                                                       _ptr(db), rank, n, ny, nx, 1 if negate else 0, _ptr(targets), J,
                                                       _ptr(tbl), _ptr(coord), ntbl,
                                                       _ptr(Q), _ptr(qs), _ptr(ac), _ptr(nv), _ptr(bpe)))
            out = {'nvalid': nv.astype(np.int64), 'Q': Q, 'q_sorted': qs, 'acum': ac, 'bpe': bpe}
            return {k: v for k, v in out.items() if v is not None}
        out = self._batched(nslab, per, one)
        if single:                                           # a plane in: scalars / 1-D arrays out
            out = {k: v[0] for k, v in out.items()}
            out['nvalid'] = int(out['nvalid'])
            if 'bpe' in out:
                out['bpe'] = float(out['bpe'])
        return out


_default_ctx = {}


def default_context(device=0):
    """Process-wide context per device (created on first use)."""
    ctx = _default_ctx.get(device)
    if ctx is None or ctx.handle is None:
        ctx = Context(device)
        _default_ctx[device] = ctx
    return ctx
