# -*- coding: utf-8 -*-
"""A stand-in for libxcontour_hip.so, for the tests that pin the host layer of `_native.Context` without a GPU
(test_host_batching.py: K1 - K13; test_host_ring_records.py: K14 - K23)."""
import ctypes as C

import numpy as np

# position of `nslab` in the argument list of the entry points that take it by value (include/xcontour_hip.h); for the entry points
# that run on K12's records and see no slabs, the position of `nrange` (xc_ring_tracks_dev: of `nring`)
_NSLAB_ARG = {'xc_minmax': 3, 'xc_levels': 3, 'xc_contours': 3, 'xc_grad2': 3, 'xc_crossing': 3, 'xc_crossing_dev': 3,
              'xc_contour_lengths': 3, 'xc_contour_lengths_dev': 3, 'xc_lwa': 10, 'xc_sort_profile_batch': 8,
              'xc_contour_lengths_periodic': 3, 'xc_contour_lengths_periodic_dev': 3,
              'xc_local_contour_lengths': 3, 'xc_local_contour_lengths_dev': 3,
              'xc_local_contour_lengths_periodic': 3, 'xc_local_contour_lengths_periodic_dev': 3,
              'xc_contour_segments_dev': 3, 'xc_contour_segments_periodic_dev': 3, 'xc_contour_pieces_dev': 1,
              'xc_contour_polylines_dev': 1, 'xc_contour_overturning_dev': 1, 'xc_contour_interior_dev': 1,
              'xc_contour_piece_interiors_dev': 1, 'xc_contour_piece_tree_dev': 1, 'xc_contour_piece_labels_dev': 1,
              'xc_contour_piece_props_dev': 1, 'xc_label_overlap_dev': 1, 'xc_ring_tracks_dev': 1, 'xc_contour_folds_dev': 1}
_K12 = ('xc_contour_segments_dev', 'xc_contour_segments_periodic_dev')
DEV = 1 << 40                           # where the stand-in's device allocations start
RES = 1 << 44                           # where the stand-in's device mirror of a resident array starts


class _Lib(object):
    """every xc_* entry point returns XC_OK and leaves its outputs alone; compute entry points are recorded: (name, nslab) in
    `calls`, (name, every positional argument) in `args`; the bytes of every xc_malloc in `mallocs`.  `d2h_u64`: None -- a
    download reads zeros --, or a callable (this library) -> the value every uint64 of the next download holds (a count download
    of twos takes K12 / K13 into their second pass; K12's count-only call then returns 1, as the library's does).
    `resident_base`: None -- xc_resident_lookup finds nothing --, or the host address of the one registered array, whose mirror
    starts at RES.
    `on`: entry point -> callable (this library, the arguments) -> status, run after the call is recorded: a scripted kernel, which
    writes its outputs with `poke(device address, array)`.  A download that starts at a poked address, or where an upload went,
    reads what lies there (zeros behind it), whichever call asks and in whatever order: the script is tied to WHERE a column lies,
    not to when it is fetched."""

    def __init__(self):
        self.calls, self.args, self.mallocs = [], [], []
        self.d2h_u64 = self.resident_base = None
        self._next = self._base = DEV                                # the next allocation; the first one _take has not seen
        self.on, self.mem, self.allocs = {}, {}, []                  # allocs: (address, bytes) of every xc_malloc ever made

    def __getattr__(self, name):
        if name == 'xc_malloc':
            return self._malloc
        if name == 'xc_memcpy_d2h':
            return self._d2h
        if name == 'xc_memcpy_h2d':
            return self._h2d
        if name == 'xc_resident_lookup':
            return self._lookup
        if name == 'xc_hist':
            return lambda h, dref: (self.calls.append((name, int(dref._obj.nslab))), 0)[1]
        if name in _NSLAB_ARG:
            return lambda *a: self._record(name, a)
        return lambda *a: 0

    def _record(self, name, a):
        self.calls.append((name, int(a[_NSLAB_ARG[name]])))
        self.args.append((name, tuple(a)))
        if name in self.on:
            return self.on[name](self, a)
        return 1 if name in _K12 and a[9] == 0 and self.d2h_u64 is not None and self.d2h_u64(self) else 0

    def _malloc(self, h, n, pref):
        self.mallocs.append(int(n))
        self.allocs.append((self._next, int(n)))
        pref._obj.value = self._next
        self._next += (int(n) + 4095) & ~4095
        return 0

    def poke(self, addr, arr):
        self.mem[int(addr)] = np.ascontiguousarray(arr).tobytes()

    def _h2d(self, h, dst, src, n):
        self.mem[int(dst)] = C.string_at(src, n)
        return 0

    def _d2h(self, h, dst, src, n):
        C.memset(dst, 0, n)
        if src in self.mem:
            b = self.mem[src][:n]
            C.memmove(dst, b, len(b))
            return 0
        v = self.d2h_u64(self) if self.d2h_u64 is not None else 0
        if v:
            (C.c_uint64 * (n // 8)).from_address(dst)[:] = [v] * (n // 8)
        return 0

    def _lookup(self, h, p, n, pref):
        pref._obj.value = None if self.resident_base is None else RES + (p - self.resident_base)
        return 0

    def where(self, v):
        """an argument as a test states it: a device address -> ('dev', the bytes of its allocation, the offset in it), so that it
        does not depend on the order of the allocations; a host pointer -> 'host'; anything else as it is"""
        if isinstance(v, C.c_void_p):
            return 'host'
        if isinstance(v, int) and not isinstance(v, bool) and DEV <= v < RES:
            for at, n in self.allocs:
                if at <= v < at + max(n, 1):
                    return ('dev', n, v - at)
            return ('dev', None, v)
        return v
