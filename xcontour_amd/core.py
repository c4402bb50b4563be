# -*- coding: utf-8 -*-
"""
Contour2D / Table -- the reference's public API for the contour-coordinate hot
path (reference xcontour/core.py:16-1195), backed by the HIP kernels of
libxcontour_hip.so.

Same class / method names, keyword arguments, result names ('AeqCTbl', 'd<name>dA',
'Leq2', 'nkeff', 'LWA', 'LAPE', 'lwm...', 'cm...'), dims ('contour', the equivalent
dim, 'new') and error behaviour (bare `Exception` with the reference's messages).

Division of labour
  * everything that touches a full (ny, nx) slab -- min/max, the weighted histograms,
    the conditional integrals, the A(Yeq) row sums, |grad q|^2, local wave activity --
    runs on the GPU through `_native.Context` (no CPU fallback: without the library or
    a gfx950 device these methods raise);
  * O(N) algebra on contour vectors (np.interp, np.gradient, ratios) is host numpy,
    exactly the calls the reference itself makes (core.py:480-483, 635, 963-964,
    1427-1430).  The batched `keff()` extension runs even that on the device.

Extensions over the reference (all optional, defaults follow the snapshot):
  * contour sets may differ per leading (time, level, ...) index in the *_hist methods
    (the reference only supports a `time` loop, core.py:1259-1294);
  * `right_edge='xhistogram'|'numpy'` selects the last-bin rule: the default is what the reference
    runs (xhistogram: last edge + 1e-8 in the edge dtype, half-open), 'numpy' closes the last bin;
  * `cal_squared_gradient`, `keff` (fused pipeline), `metric=` in cal_local_wave_activity;
  * `deterministic=True`: order-free fixed-point sums in every histogram pass (include/xcontour_hip.h, "Deterministic
    sums"): bit-identical results between runs and shardings, like the reference's np.bincount; it also keeps
    cal_local_wave_activity / cal_local_APE on the band walk that sums in numpy's order (`exact=True`) for every plane size.
"""
import ctypes as C
import types

import numpy as np

from . import _native as nat
from . import labeled as lb
from .utils import Rearth, grad_metrics, table_from_rowsums, last_row_included


_F48 = (np.dtype(np.float32), np.dtype(np.float64))
_EDGE_CODES = {'numpy': nat.XC_EDGE_NUMPY, 'xhistogram': nat.XC_EDGE_XHISTOGRAM}
_ABSENT = object()                       # an argument the method does not have (None is a value a caller can give)


def _as_labeled_1d(arr, dim):
    arr = np.asarray(arr)
    return lb.DataArray(arr, (dim,), {dim: arr})


class Contour2D(object):
    """
    This class is designed for performing the 2D contour analysis.
    (reference core.py:16-70)
    """

    def __init__(self, trcr, dA, dims, dimEq, arakawa='A',
                 increase=True, lt=False, check_mono=False, dtype=np.float32,
                 device=0, right_edge='xhistogram', deterministic=False, resident=False):
        if len(dimEq) != 1:
            raise Exception('dimEq should be one dimension e.g., {"Y","lat"}')

        if len(dims) != 2:
            raise Exception('dims should be a 2D plane')

        if right_edge not in ('numpy', 'xhistogram'):
            raise Exception('right_edge should be "numpy" or "xhistogram"')

        self.dA = dA
        self.arakawa = arakawa
        self.tracer = trcr
        self.dims = dims
        self.dimNs = list(dims.keys())        # dim names,  ['X', 'Y', 'Z']
        self.dimVs = list(dims.values())      # dim values, ['lon', 'lat', 'Z']
        self.dimEqN = list(dimEq.keys())[0]   # equiv. dim name
        self.dimEqV = list(dimEq.values())[0]  # equiv. dim value
        self.lt = lt
        self.dtype = dtype
        self.check_mono = check_mono
        self.increase = increase
        self.right_edge = right_edge
        self.device = device
        self.deterministic = bool(deterministic)     # order-free fixed-point sums (bit-reproducible; ~1.3x the histogram pass)
        # resident=True: the tracer, the weights, the table mask and the LAST integrand handed to THIS object are uploaded once and
        # stay on the device between calls (the reference's Keff sequence passes them to four calls in a row; every call used to
        # cross PCIe again).  Do not modify them in place afterwards without calling touch().  The same holds for the small arrays handed to
        # keff() (table, lat / lon or rdx / rdy, preY): while the SAME objects come again, a resident object takes their contents as
        # unchanged (the key of its plan is not rebuilt from their bytes: ~25 us per call); touch() forgets that too.
        self.resident = bool(resident)
        self._memo = {}
        if self.dimEqV not in self.dimVs:
            raise Exception('dimEq should be one of dims')
        self._xdim = [d for d in self.dimVs if d != self.dimEqV][0]

    # ------------------------------------------------------------------ plumbing
    def touch(self):
        """resident=True: the tracer / weights were modified in place -- forget the device mirrors (the next call uploads again)"""
        for _, v in self.__dict__.get('_memo', {}).values():
            try:
                self.ctx.release_resident(v[0])
            except Exception:
                pass
        self._memo = {}
        self.__dict__.pop('_keff_last', None)
        self.__dict__.pop('_dmax_memo', None)

    def _keep(self, key, src, make):
        """memoised (array, ...) tuple whose first element stays registered as a resident input of the context.  The memo is
        keyed on the IDENTITY of the object it was made from: `c.tracer = other_field` (or `c.dA = ...`) drops the old mirror
        and registers the new field on the next call (round-3 advisor: the old key survived a reassignment).  What is
        registered is always a PRIVATE host copy, never the caller's own array: the context finds mirrors by host address,
        and another (non-resident) object handing the same ndarray to the library must not be served this object's mirror."""
        ent = self._memo.get(key)
        if ent is not None and ent[0] is src:
            return ent[1]
        if ent is not None:
            try:
                self.ctx.release_resident(ent[1][0])
            except Exception:
                pass
            del self._memo[key]
        t = make()
        a = t[0]
        raw = lb.unwrap(src)[0] if lb.is_labeled(src) else src
        if isinstance(raw, np.ndarray) and np.shares_memory(a, raw):
            a = a.copy()
            t = (a,) + tuple(t[1:])
        self.ctx.keep_resident(a)
        self._memo[key] = (src, t)
        return t

    def close(self):
        """Release the device buffers kept between keff() calls (also done when the object is collected)."""
        if self.__dict__.get('_memo'):
            self.touch()
        for plan in self.__dict__.pop('_keff_plans', {}).values():
            try:
                plan.free()
            except Exception:
                pass

    def __del__(self):
        self.close()

    @property
    def ctx(self):
        return nat.default_context(self.device)

    def _plane(self, arr):
        """labelled array -> (values (S, ny, nx) C-contiguous -- or a LazyStack of that shape for a lazy source --, lead dims,
        lead shape, coords)"""
        if self.resident and arr is self.tracer and not lb.is_lazy_data(lb.unwrap(arr, lazy=True)[0]):
            def make():
                v, lead, lshape, coords = self._plane_of(arr)
                return np.ascontiguousarray(self._float(v)), lead, lshape, coords
            return self._keep('tracer', arr, make)
        return self._plane_of(arr)

    def _plane_of(self, arr):
        v, dims, coords, _ = lb.unwrap(arr, lazy=True)
        if self.dimEqV not in dims or self._xdim not in dims:
            raise Exception('array should have the dims %s' % self.dimVs)
        lead = tuple(d for d in dims if d not in (self.dimEqV, self._xdim))
        if lb.is_lazy_data(v):
            # a lazy stack stays lazy (the reference: dask='allowed', core.py:242, 258): the native entry points read it
            # in batches of whole slabs below Context.max_batch_bytes
            st = lb.LazyStack(v, [dims.index(d) for d in lead], dims.index(self.dimEqV), dims.index(self._xdim))
            return st, lead, st.lshape, coords
        order = [dims.index(d) for d in lead] + [dims.index(self.dimEqV), dims.index(self._xdim)]
        v = np.ascontiguousarray(np.transpose(v, order))
        lshape = v.shape[:-2]
        return v.reshape((-1,) + v.shape[-2:]), lead, lshape, coords

    def _float(self, v):
        if getattr(v, '_xc_lazy_stack', False):
            return v                                                    # converts as it reads
        return nat._f48(v)

    def _dA_array(self, ny, nx, nslab):
        """self.dA -> (float64 ndarray of shape (ny,), (ny,nx) or (nslab,ny,nx), was_f32)"""
        if self.resident:
            # one mirror per (ny, nx) unless the weights carry leading (time, ...) dims: a (ny,) / (ny, nx) result does not depend on nslab
            if lb.is_labeled(self.dA):
                raw, dd, _, _ = lb.unwrap(self.dA, lazy=True)
                stack = len([d for d, n in zip(dd, raw.shape) if d in self.dimVs or n != 1]) > 2
            else:
                stack = np.ndim(self.dA) > 2
            return self._keep(('dA', ny, nx, nslab if stack else 0), self.dA, lambda: self._dA_array_of(ny, nx, nslab))
        return self._dA_array_of(ny, nx, nslab)

    def _dA_array_of(self, ny, nx, nslab):
        if lb.is_labeled(self.dA):
            v, dims, _, _ = lb.unwrap(self.dA)
            keep = [i for i, n in enumerate(v.shape) if not (n == 1 and dims[i] not in self.dimVs)]
            v = v.reshape([v.shape[i] for i in keep])
            dims = tuple(dims[i] for i in keep)
            if dims == (self.dimEqV,):
                pass
            elif set(dims) == set(self.dimVs) and len(dims) == 2:
                if dims[0] != self.dimEqV:
                    v = v.T
            elif self.dimEqV in dims and self._xdim in dims:
                lead = [d for d in dims if d not in self.dimVs]
                order = [dims.index(d) for d in lead] + [dims.index(self.dimEqV), dims.index(self._xdim)]
                v = np.transpose(v, order).reshape((-1, ny, nx))
                if v.shape[0] != nslab:
                    raise Exception('dA leading dims do not match the tracer')
            else:
                raise Exception('dA should be defined on %s' % self.dimVs)
        else:
            v = np.asarray(self.dA)
        was_f32 = v.dtype == np.float32
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape not in ((ny,), (ny, nx), (nslab, ny, nx)):
            raise Exception('dA of shape %r does not match the (%d, %d) plane' % (v.shape, ny, nx))
        return v, was_f32

    def _eq_coord(self, arr):
        _, _, coords, _ = lb.unwrap(arr, lazy=True)
        if self.dimEqV not in coords:
            raise Exception('no coordinate values for %s' % self.dimEqV)
        return np.asarray(coords[self.dimEqV])

    def _wrap_contour(self, values, lead, lshape, coords, name, like, ccoord, shared=None):
        """`shared`: a coords dict built by an earlier call for the same (lead, contour) layout -- the nine outputs of keff() share one"""
        out = values.reshape(tuple(lshape) + (values.shape[-1],))
        c = shared
        if c is None:
            c = {d: np.asarray(coords[d]) for d in lead if d in coords}
            c['contour'] = np.asarray(ccoord)
        return lb.wrap(out, tuple(lead) + ('contour',), c, name, like, trusted=True)

    def _in_dim_order(self, v, like, lead, lshape):
        """a plane-shaped result `v` (S, ny, nx) of the labelled input `like` -> (the input's dims, `v` with the leading dims
        unfolded and the axes in the input's own order)"""
        dims = lb.unwrap(like, lazy=True)[1]
        full = tuple(lead) + (self.dimEqV, self._xdim)
        return dims, np.transpose(v.reshape(tuple(lshape) + v.shape[-2:]), [full.index(d) for d in dims])

    # ------------------------------------------------------------------ A(Yeq) table
    def _table_rows(self, mask, multiply):
        if self.resident:
            ent = self._memo.get(('mask',))
            if ent is not None and ent[0] is mask:                      # the same mask object again: its plane is already registered
                m0 = ent[1][0]
                ny, nx = m0.shape
                dA, _ = self._dA_array(ny, nx, 1)
                return self.ctx.rowsum(m0, dA[0] if dA.ndim == 3 else dA, ny, nx, multiply=multiply)
        m, lead, lshape, _ = self._plane(mask)
        if m.shape[0] != 1:
            raise Exception('mask should be a 2D plane (it is assumed not to change with time)')
        ny, nx = m.shape[1:]
        dA, _ = self._dA_array(ny, nx, 1)
        if dA.ndim == 3:
            dA = dA[0]
        m0 = self._float(np.asarray(m[0]))
        if self.resident:
            # the mask is time-invariant by contract (core.py:156): with resident inputs it crosses PCIe once, like tracer and weights
            m0 = self._keep(('mask',), mask, lambda: (np.ascontiguousarray(m0),))[0]
        return self.ctx.rowsum(m0, dA, ny, nx, multiply=multiply)

    def cal_area_eqCoord_table(self, mask):
        """
        Discretized relation table between area and equivalent coordinate by strict
        conditional integration (reference core.py:73-147).  Keeps the input coordinate
        order; the end point is overwritten with the total masked area.
        """
        coord = self._eq_coord(mask)
        rows = self._table_rows(mask, multiply=True)      # r_i = sum_x mask*dA
        eqDimIncre = coord[-1] > coord[0]
        same = (eqDimIncre == self.increase)
        less = same if self.lt else (not same)                            # core.py:103-128
        # tbl[j] = sum_{i: c_i < c_j} r_i  (or '>'); coordinates are strictly monotone rows
        order = np.argsort(coord, kind='stable')
        rs = rows[order]
        cs = coord[order]
        cum = np.concatenate(([0.0], np.cumsum(rs)))                      # cum[i] = sum of rows < i
        suf = np.concatenate((np.cumsum(rs[::-1])[::-1], [0.0]))          # suf[i] = sum of rows >= i
        lo = np.searchsorted(cs, coord, side='left')                      # rows strictly below
        hi = np.searchsorted(cs, coord, side='right')                     # rows at or below
        tbl = np.abs(cum[lo]) if less else np.abs(suf[hi])
        maxArea = abs(cum[-1])                                            # core.py:133
        if tbl[-1] > tbl[0]:                                              # core.py:136-140
            tbl[-1] = maxArea
        else:
            tbl[0] = maxArea
        tbl = lb.wrap(tbl, (self.dimEqV,), {self.dimEqV: coord}, 'AeqCTbl', mask)
        if self.check_mono:
            _check_monotonicity(tbl, self.dimEqV)
        return Table(tbl, self.dimEqV)

    def cal_area_eqCoord_table_hist(self, mask):
        """
        Discretized relation table between area and equivalent coordinate, histogram
        semantics (reference core.py:150-203): the histogram of the coordinate field
        against its own values degenerates to per-row sums of dA where mask == 1
        (one GPU pass), then cumsum / `cdf[-1]-cdf` on the host.
        """
        coord = self._eq_coord(mask)
        rows = self._table_rows(mask, multiply=False)
        yIncre = not (coord[-1] < coord[0])                               # core.py:180-182
        ylt = self.lt if (self.increase == yIncre) else (not self.lt)     # core.py:184-188
        rows_asc = rows if yIncre else rows[::-1]
        # the last row sits ON the last bin edge: kept by numpy's closed last bin, kept by xhistogram only
        # if `edge + 1e-8` is representable in the coordinate dtype (core.py:1307 -> xhistogram)
        tbl = table_from_rowsums(rows_asc, ylt, last_row_included(coord, self.right_edge))
        cs = coord if yIncre else coord[::-1]                             # core.py:195-198
        tbl = lb.wrap(tbl, (self.dimEqV,), {self.dimEqV: cs.copy()}, 'AeqCTbl', mask)
        if self.check_mono:
            _check_monotonicity(tbl, self.dimEqV)
        return Table(tbl, self.dimEqV)

    # ------------------------------------------------------------------ contours
    def cal_contours(self, levels=10):
        """
        Contour levels of the tracer from its minimum to maximum values
        (reference core.py:205-266).  int: N equally spaced levels per slab (GPU
        min/max + level kernel, exact dtype rules); array: given levels.
        """
        return self._contours_of(self.tracer, levels)

    def _contours_of(self, tracer, levels):
        """cal_contours on any tracer of the object's plane (cal_equivalent_coordinate_map takes one)"""
        q, lead, lshape, coords = self._plane(tracer)
        q = self._float(q)
        if type(levels) is int or isinstance(levels, np.integer):
            ctr = self.ctx.contours(q, int(levels), self.increase, self.dtype).astype(self.dtype)      # K1 + levels, one call, one sync
            ccoord = np.arange(levels, dtype=np.float64).astype(self.dtype)     # = np.linspace(0.0, levels - 1.0, levels, dtype): its step is exactly 1
        else:
            levs = np.asarray(levels)
            mmin = self.ctx.minmax(q)[:, 0].astype(q.dtype)
            ctr = ((mmin - mmin)[:, None] + levs[None, :]).astype(self.dtype)   # core.py:254
            ccoord = levs
        return self._wrap_contour(ctr, lead, lshape, coords, lb.unwrap(tracer, lazy=True)[3], tracer, ccoord)

    def _contour_values(self, contour, nslab, lead, lshape):
        """-> ndarray (nslab, N) of levels (per slab or broadcast) in their own dtype"""
        if lb.is_labeled(contour):
            v, dims, _, _ = lb.unwrap(contour)
            if 'contour' not in dims:
                raise Exception('contour should have a "contour" dim')
            if dims == tuple(lead) + ('contour',) and v.shape[:-1] == tuple(lshape):
                return np.ascontiguousarray(v).reshape(nslab, -1)        # what cal_contours returns for this tracer: already (lead..., contour)
            keep = [i for i, n in enumerate(v.shape) if not (n == 1 and dims[i] != 'contour')]
            v = v.reshape([v.shape[i] for i in keep])
            dims = tuple(dims[i] for i in keep)
            cl = [d for d in dims if d != 'contour']
            v = np.transpose(v, [dims.index(d) for d in cl] + [dims.index('contour')])
            if cl:
                full = [d for d in lead if d in cl]
                if full != cl:
                    v = np.transpose(v, [cl.index(d) for d in full] + [len(cl)])
                shp = [lshape[lead.index(d)] if d in cl else 1 for d in lead] + [v.shape[-1]]
                v = np.broadcast_to(v.reshape(shp), tuple(lshape) + (v.shape[-1],))
                return np.ascontiguousarray(v).reshape(nslab, -1)
            v = v.reshape(-1)
        elif type(contour) in [np.ndarray, list]:
            v = np.asarray(contour)
        else:
            raise Exception('bins should be numpy.array or xarray.DataArray')
        return np.broadcast_to(v[None, :], (nslab, v.shape[0]))

    def cal_contours_at(self, predef, table):
        """Contours at prescribed equivalent coordinates (reference core.py:269-313)."""
        return self._contours_at(predef, table, hist=False)

    def cal_contours_at_hist(self, predef, table):
        """Contours at prescribed equivalent coordinates (reference core.py:316-360)."""
        return self._contours_at(predef, table, hist=True)

    def _contours_at(self, predef, table, hist):
        if len(predef.shape) != 1:
            raise Exception('predef should be a 1D array')
        if type(predef) in [np.ndarray]:
            predef = _as_labeled_1d(predef, 'new')
        N = predef.size
        ctr = self.cal_contours(N)
        area = self.cal_integral_within_contours_hist(ctr) if hist else self.cal_integral_within_contours(ctr)
        dimEq = table.lookup_coordinates(area).rename('Z')
        pd = lb.unwrap(predef, lazy=True)[1][0]
        qIntp = self.interp_to_coords(predef.squeeze(), dimEq, ctr.squeeze()) \
            .rename({pd: 'contour'}).rename(lb.unwrap(ctr, lazy=True)[3])
        v, dims, coords, name = lb.unwrap(qIntp)
        coords['contour'] = np.linspace(0, N - 1, N, dtype=self.dtype)
        return lb.wrap(v, dims, coords, name, qIntp)

    # ------------------------------------------------------------------ conditional integrals
    def _hist_inputs(self, tracer, integrands, fused=False):
        """tracer, weights and integrands as a histogram pass takes them -> (q (S, ny, nx), lead dims, lead shape, coords, dA,
        [integrand (S, ny, nx), ...], [its product with dA stays float32?, ...]).  An integrand on its own goes through
        `_integrand_plane` (resident objects register it as THE ('integrand',) mirror); the integrands of a `fused` pass register nothing"""
        q, lead, lshape, coords = self._plane(tracer)
        q = self._float(q)
        nslab, ny, nx = q.shape
        dA, dA_f32 = self._dA_array(ny, nx, nslab)
        gs, flags = [], []
        for it in integrands:
            g = self._float(self._plane(it)[0]) if fused else self._integrand_plane(it)
            if g.shape != q.shape:
                g = np.ascontiguousarray(np.broadcast_to(np.asarray(g), q.shape))
            gs.append(g)
            flags.append(bool(g.dtype == np.float32 and dA_f32))           # f32*f32 stays f32 (core.py:444)
        return q, lead, lshape, coords, dA, gs, flags

    def _hist_cdfs(self, contour, tracer, integrands, channels, fused=False):
        """CDF of dA (channel 0) and of every integrand*dA (channel 1 + i) within the contours in ONE K3 pass -> the `channels` asked
        for, each wrapped as cal_integral_within_contours_hist returns it; None when the integrands cannot share a launch (more than
        XC_MAX_INTEGRANDS, or mixed f32/f64 products)."""
        q, lead, lshape, coords, dA, gs, flags = self._hist_inputs(tracer, integrands, fused)
        if len(gs) > nat.XC_MAX_INTEGRANDS or len(set(flags)) > 1:
            return None
        b = self._contour_values(contour, q.shape[0], list(lead), list(lshape))
        edges, binc, last_closed = _edges_from_levels(b, self.right_edge)
        out = self.ctx.hist(q, edges, dA=dA, integrands=gs, last_closed=last_closed, lt=self.lt,
                            reverse=not binc, prod_f32=bool(flags and flags[0]), want=('cdf',), deterministic=self.deterministic)
        binNum = np.arange(b.shape[1]).astype(np.float32)                  # core.py:1255-1257
        name = 'histogram_%s' % lb.unwrap(tracer, lazy=True)[3]
        res = []
        for c in channels:
            res.append(self._wrap_contour(out['cdf'][:, c, :], lead, lshape, coords, name, tracer, binNum))
            if self.check_mono:
                _check_monotonicity(res[-1], 'contour')
        return res

    def _integrand_plane(self, integrand):
        """(S, ny, nx) values of an integrand.  resident=True: the LAST integrand handed to this object keeps a device mirror too, keyed
        on the identity of the labelled array like tracer and weights -- the squared gradient goes to cal_integral_within_contours_hist,
        to cal_contour_mean_hist and to keff() in one analysis and used to cross PCIe each time (140 us per 7 MB at the reference's
        demo size, more than everything else in the call together).  Same contract: do not modify it in place without touch()."""
        if self.resident and lb.is_labeled(integrand) and not lb.is_lazy_data(lb.unwrap(integrand, lazy=True)[0]):
            return self._keep(('integrand',), integrand, lambda: (np.ascontiguousarray(self._float(self._plane_of(integrand)[0])),))[0]
        return self._float(self._plane(integrand)[0])

    def cal_integral_within_contours_hist(self, contour, tracer=None, integrand=None):
        """
        Integral of a masked variable within pre-calculated tracer contours, using the
        histogram method (reference core.py:412-460 + _histogram 1202-1325).
        One GPU pass: weights `dA` (or `integrand*dA`, fillna(0)), CDF by cumsum,
        `cdf[-1]-cdf` if not lt, flipped so that out[k] <-> contour[k].
        """
        integ = [] if integrand is None else [integrand]
        return self._hist_cdfs(contour, self.tracer if tracer is None else tracer, integ, [len(integ)])[0]

    def cal_integral_within_contours(self, contour, tracer=None, integrand=None):
        """
        Conditional integral within each tracer contour, strict comparison at every level
        (reference core.py:363-409): out[k] = sum dA*integrand*[q < c_k] (lt) or [q > c_k].
        Evaluated with the same GPU histogram: half-open bins below each sorted level
        (the tracer is negated in-kernel for the '>' case).
        """
        if tracer is None:
            tracer = self.tracer
        q, lead, lshape, coords, dA, integ, flags = self._hist_inputs(tracer, [] if integrand is None else [integrand])
        nslab, prod_f32 = q.shape[0], bool(flags and flags[0])
        if type(contour) in [np.ndarray]:
            contour = _as_labeled_1d(contour, 'contour')
        b = self._contour_values(contour, nslab, list(lead), list(lshape)).astype(np.float64)
        N = b.shape[1]
        out = np.empty((nslab, N), dtype=np.float64)
        # per-slab sorted unique levels (in -q space for '>'); edges = [-inf, levels...]
        sgn = 1.0 if self.lt else -1.0
        uniq = [np.unique(sgn * b[s]) for s in range(nslab)]
        nu = [len(u) for u in uniq]
        if min(nu) != max(nu) or np.isnan(b).any():
            groups = [[s] for s in range(nslab)]
        else:
            groups = [list(range(nslab))]
        for grp in groups:
            e = np.stack([np.concatenate(([-np.inf], uniq[s])) for s in grp])
            res = self.ctx.hist(q[grp], e, dA=dA if dA.ndim < 3 else dA[grp],
                                integrands=[g[grp] for g in integ], last_closed=False, lt=True,
                                negate=not self.lt, prod_f32=prod_f32, want=('cdf',), deterministic=self.deterministic)
            cdf = res['cdf'][:, 1 if integ else 0, :]
            for i, s in enumerate(grp):
                out[s] = cdf[i][np.searchsorted(uniq[s], sgn * b[s])]
        name = 'intVar' if integrand is None else lb.unwrap(integrand, lazy=True)[3]
        ccoord = lb.unwrap(contour, lazy=True)[2].get('contour', np.arange(N))
        intVar = self._wrap_contour(out, lead, lshape, coords, name, tracer, ccoord)
        if self.check_mono:
            _check_monotonicity(intVar, 'contour')
        return intVar

    # ------------------------------------------------------------------ O(N) contour-space algebra (host numpy, as in the reference)
    def cal_gradient_wrt_area(self, var, area):
        """d(var)/d(area) by centred differences along 'contour' (reference core.py:463-488)."""
        v, dims, coords, name = lb.unwrap(var)
        a, adims, acoords, _ = lb.unwrap(area)
        ax = dims.index('contour')
        k = coords.get('contour')
        ka = acoords.get('contour')
        # the usual layout -- contour last, the area on the same dims (or one profile for all), plain float arrays with their float contour
        # index: one host call in the library (xc_host_gradient_wrt_area: numpy's arithmetic, 29 -> ~8 us at the reference's demo size)
        if (k is not None and ka is not None and ax == v.ndim - 1 and v.ndim <= 2 and type(v) is np.ndarray and type(a) is np.ndarray
                and (adims == dims or adims == ('contour',)) and a.shape[-1] == v.shape[-1] and v.shape[-1] >= 2
                and v.dtype in _F48 and a.dtype in _F48 and type(k) is np.ndarray and type(ka) is np.ndarray
                and k.dtype in _F48 and ka.dtype in _F48 and k.shape == ka.shape == (v.shape[-1],)
                and v.strides[-1] == v.itemsize and a.strides[-1] == a.itemsize and v.strides[0] % v.itemsize == 0
                and a.strides[0] % a.itemsize == 0 and k.flags.c_contiguous and ka.flags.c_contiguous):
            out = np.empty(v.shape, dtype=np.float64 if (v.dtype.itemsize | a.dtype.itemsize) == 8 or v.dtype != a.dtype else v.dtype)
            n = v.shape[-1]
            rc = nat.load().xc_host_gradient_wrt_area(v.ctypes.data, v.dtype.itemsize == 8, k.ctypes.data, k.dtype.itemsize == 8,
                                                      a.ctypes.data, a.dtype.itemsize == 8, ka.ctypes.data, ka.dtype.itemsize == 8,
                                                      v.size // n, n, a.size // n, v.strides[0] // v.itemsize, a.strides[0] // a.itemsize,
                                                      out.ctypes.data)
            if rc == 0:
                return lb.wrap(out, dims, coords, 'dvardA' if name is None else 'd' + name + 'dA', var, trusted=True)
        k = np.asarray(k if k is not None else np.arange(v.shape[ax]))
        ka = np.asarray(ka if ka is not None else np.arange(a.shape[adims.index('contour')]))
        with np.errstate(divide='ignore', invalid='ignore'):
            dfVar = _gradient_edge1(v, k, ax)
            dfArea = _gradient_edge1(a, ka, adims.index('contour'))
            dVardA = dfVar / _align(dfArea, adims, dims)
        return lb.wrap(dVardA, dims, coords, 'dvardA' if name is None else 'd' + name + 'dA', var)

    def cal_contour_weigh_mean(self, contour, integrand, area=None):
        """Thickness-weighted line average (reference core.py:491-520)."""
        intA = self.cal_integral_within_contours(contour, integrand=integrand)
        if area is None:
            area = self.cal_integral_within_contours(contour)
        lmA = self.cal_gradient_wrt_area(intA, area)
        iname = lb.unwrap(integrand, lazy=True)[3]
        return lmA.rename('lwm' if iname is None else 'lwm' + iname)

    def cal_contour_weigh_mean_hist(self, contour, integrand, area=None):
        """Thickness-weighted line average, histogram method (reference core.py:523-552)."""
        intA = self.cal_integral_within_contours_hist(contour, integrand=integrand)
        if area is None:
            area = self.cal_integral_within_contours_hist(contour)
        lmA = self.cal_gradient_wrt_area(intA, area)
        iname = lb.unwrap(integrand, lazy=True)[3]
        return lmA.rename('lwm' if iname is None else 'lwm' + iname)

    def cal_contour_mean(self, contour, integrand, grdm, area=None):
        """Along-contour average (reference core.py:555-583)."""
        return self._contour_mean(contour, integrand, grdm, area, self.cal_contour_weigh_mean)

    def cal_contour_mean_hist(self, contour, integrand, grdm, area=None):
        """Along-contour average, histogram method (reference core.py:586-616)."""
        return self._contour_mean(contour, integrand, grdm, area, self.cal_contour_weigh_mean_hist)

    def _contour_mean(self, contour, integrand, grdm, area, fn):
        iv, idims, icoords, iname = lb.unwrap(integrand, lazy=True)
        gv, gdims, _, _ = lb.unwrap(grdm, lazy=True)
        if (lb.is_lazy_data(iv) or lb.is_lazy_data(gv)) and tuple(gdims) == tuple(idims) and tuple(gv.shape) == tuple(iv.shape):
            prod = lb.wrap(lb.LazyProduct(iv, gv), idims, icoords, None, integrand)      # stays lazy: multiplied batch by batch
        else:
            prod = lb.wrap(np.asarray(iv) * _align(np.asarray(gv), gdims, idims), idims, icoords, None, integrand)
        fused = self._integrals_hist(contour, [prod, grdm]) if fn == self.cal_contour_weigh_mean_hist else None
        if fused is not None:
            # area, int(integrand*grdm) and int(grdm) as three weight channels of ONE histogram
            # pass (the reference: four passes, core.py:523-552 called twice from 586-616)
            a_cdf, (intU, intL) = fused
            if area is None:
                area = a_cdf
            upper = self.cal_gradient_wrt_area(intU, area)
            lower = self.cal_gradient_wrt_area(intL, area)
        else:
            upper = fn(contour, prod, area=area)
            lower = fn(contour, grdm, area=area)
        uv, udims, ucoords, _ = lb.unwrap(upper)
        with np.errstate(divide='ignore', invalid='ignore'):
            lmA = uv / lb.unwrap(lower)[0]
        return lb.wrap(lmA, udims, ucoords, 'cm' if iname is None else 'cm' + iname, upper)

    def _integrals_hist(self, contour, integrands):
        """CDF of dA and of every integrand*dA within the contours in ONE K3 pass ->
        (area, [integral_i]), each exactly what cal_integral_within_contours_hist returns; None when
        the integrands cannot share a launch (more than XC_MAX_INTEGRANDS, or mixed f32/f64 products)."""
        res = self._hist_cdfs(contour, self.tracer, integrands, range(1 + len(integrands)), fused=True)
        return None if res is None else (res[0], res[1:])

    def cal_sqared_equivalent_length(self, dgrdSdA, dqdA):
        """Leq2 = d[int |grad q|^2]/dA / (dq/dA)^2 (reference core.py:619-637)."""
        a, dims, coords, _ = lb.unwrap(dgrdSdA)
        b, bdims, _, _ = lb.unwrap(dqdA)
        with np.errstate(divide='ignore', invalid='ignore'):
            Leq2 = a / _align(b, bdims, dims) ** 2
        return lb.wrap(Leq2, dims, coords, 'Leq2', dgrdSdA)

    def cal_normalized_Keff(self, Leq2, Lmin, mask=1e5):
        """Normalized effective diffusivity (reference core.py:945-966)."""
        a, dims, coords, _ = lb.unwrap(Leq2)
        b, bdims, _, _ = lb.unwrap(Lmin)
        b = _align(b, bdims, dims)
        with np.errstate(divide='ignore', invalid='ignore'):
            nkeff = a / b / b
            nkeff = np.where(nkeff < mask, nkeff, np.nan)
        return lb.wrap(nkeff, dims, coords, 'nkeff', Leq2)

    def interp_to_dataset(self, predef, dimEq, vs):
        """Interpolate variables to prescribed equivalent coordinates and merge them
        (reference core.py:1017-1047)."""
        re = []
        if isinstance(vs, dict):
            for var in vs:
                re.append(self.interp_to_coords(predef, dimEq, vs[var]).rename(var))
        else:
            for var in vs:
                re.append(self.interp_to_coords(predef, dimEq, var).rename(lb.unwrap(var, lazy=True)[3]))
        return lb.merge(re, re[0])

    def interp_to_coords(self, predef, eqCoords, var, interpDim='contour'):
        """np.interp from the contour dim to predefined equivalent coordinates, per leading
        index (reference core.py:1050-1100); direction from the first slab (1080-1088)."""
        dimTmp = 'new'
        if isinstance(predef, (np.ndarray, list)):
            predef = _as_labeled_1d(np.asarray(predef), dimTmp)
        else:
            dimTmp = lb.unwrap(predef, lazy=True)[1][0]
        pv = np.asarray(lb.unwrap(predef)[0])
        ev, edims, _, _ = lb.unwrap(eqCoords)
        vv, vdims, vcoords, vname = lb.unwrap(var)
        vals = ev
        while len(vals.shape) > 1:
            vals = vals[0]
        increasing = bool(vals[0] < vals[-1])
        ev = np.moveaxis(ev, edims.index(interpDim), -1)
        vv2 = np.moveaxis(vv, vdims.index(interpDim), -1)
        lead = tuple(d for d in vdims if d != interpDim)
        elead = tuple(d for d in edims if d != interpDim)
        ev = _align(ev, elead + (interpDim,), lead + (interpDim,))
        ev = np.broadcast_to(ev, vv2.shape)
        out = np.empty(vv2.shape[:-1] + (len(pv),), dtype=np.float64)
        for idx in np.ndindex(*vv2.shape[:-1]):
            out[idx] = _interp1d(pv, ev[idx], vv2[idx], increasing)
        coords = {d: vcoords[d] for d in lead if d in vcoords}
        coords[dimTmp] = pv
        return lb.wrap(out, lead + (dimTmp,), coords, vname, var)

    # ------------------------------------------------------------------ local wave activity
    def cal_contour_crossing(self, ctr, stride=1, mode='edge', full_width=False):
        """
        Whether (and over what length) contours cross grid boxes, 'box-counting' method
        (reference core.py:640-693 and its numba kernel _contour_crossing, 1490-1566).

        One GPU pass per stride serves all contours of all slabs (K9, xc_crossing): the
        tracer is padded on the X side by max(stride) columns (`mode` as in
        DataArray.pad: 'edge', 'wrap', 'constant' (NaN), 'reflect', 'symmetric'), boxes of
        stride x stride cells are tested corner by corner and each crossed box counts
        sqrt(area) * stride.  Like the reference, the area is read at the coarse box
        indices and only the first Jn-1 box columns are scanned (core.py:1521, 1560);
        `full_width=True` (an extension) scans all of them.  Returns an array over
        (..., contour) in `self.dtype`, or a list of them when `stride` is iterable.
        """
        from collections.abc import Iterable
        if isinstance(stride, Iterable):
            strides, isiterable = [int(t) for t in stride], True
        else:
            strides, isiterable = [int(stride)], False
        maxStride = max(strides)
        if min(strides) < 1:
            raise Exception('stride should be a positive integer')
        if mode not in nat.PAD_MODES:
            raise Exception('unsupported pad mode %r (one of %s)' % (mode, sorted(nat.PAD_MODES)))
        dims = lb.unwrap(self.tracer, lazy=True)[1]
        if [d for d in dims if d in self.dimVs] != [self.dimEqV, self._xdim]:
            raise Exception('cal_contour_crossing expects the tracer stored as (..., %s, %s)' % (self.dimEqV, self._xdim))
        has_x = 'X' in self.dims                                               # core.py:673-679
        if has_x and self.dims['X'] != self._xdim:
            raise Exception('the X dim should be the fastest-varying dim of the plane')
        q, lead, lshape, coords = self._plane(self.tracer)
        q = self._float(q)
        nslab, ny, nx = q.shape
        area, was_f32 = self._dA_array(ny, nx, nslab)
        if area.ndim == 1:
            area = np.broadcast_to(area[:, None], (ny, nx))
        if was_f32:
            area = area.astype(np.float32)             # the reference takes np.sqrt in the area's own dtype
        bs, order, ccoord = self._sorted_levels(ctr, nslab, lead, lshape)
        re = []
        results = self.ctx.crossing(q, bs, area, stride=strides, pad_x=maxStride if has_x else 0,
                                    pad_mode=mode, full_width=full_width)      # one upload for all strides
        for lens, _ in results:
            out = _level_order(lens, order)
            re.append(self._wrap_contour(out.astype(self.dtype), lead, lshape, coords, None, self.tracer, ccoord))
        return re if isiterable else re[0]

    def _sorted_levels(self, ctr, nslab, lead, lshape):
        """the levels of every slab as the contour kernels take them: float64, ascending, a NaN level as +inf (it is never crossed --
        it crosses no cell --; neither is +inf) -> (sorted levels (nslab, N), the stable order that sorted them -- `_level_order`
        undoes it --, the 'contour' coordinate of the result)"""
        b = np.array(self._contour_values(ctr, nslab, list(lead), list(lshape)), dtype=np.float64)
        b[np.isnan(b)] = np.inf
        order = np.argsort(b, axis=1, kind='stable')
        ccoord = lb.unwrap(ctr, lazy=True)[2].get('contour') if lb.is_labeled(ctr) else None
        if ccoord is None:
            ccoord = np.arange(b.shape[1]).astype(self.dtype)
        return np.take_along_axis(b, order, axis=1), order, ccoord

    # ------------------------------------------------------------------ contour lengths
    @staticmethod
    def _x_period(periodic, xdeg, latlon, who, plain=False):
        """the `periodic` argument of cal_contour_lengths / cal_local_contour_lengths -> None (X has two free edges) or the period
        handed to the library, a float64 in the units of the X coordinates it gets: float64(P), with latlon=True
        float64(deg2rad(float32(P))) -- the cast chain of the coordinates themselves.  `xdeg`: the X coordinate as given, after
        its cast to float32.  True: 360 degrees, along the direction the coordinate runs in.
        plain=True (find_contours, which never casts): `xdeg` is the coordinate as given in float64, True is 360 whatever
        `latlon`, and the period comes back as float64(P), in the coordinate's own units."""
        if periodic is None or periodic is False or (isinstance(periodic, np.bool_) and not periodic):
            return None
        span = float(xdeg[-1]) - float(xdeg[0]) if xdeg.size >= 2 else 0.0
        if periodic is True or isinstance(periodic, np.bool_):
            if not latlon and not plain:
                raise Exception('%s: periodic=True needs latlon=True (there is no default period for a Cartesian plane: '
                                'give periodic=<the period>)' % who)
            P = -360.0 if span < 0 else 360.0
        else:
            try:
                P = float(periodic)
            except (TypeError, ValueError):
                raise Exception('%s: periodic should be False, True or the period as a number' % who)
        if xdeg.size < 2:
            raise Exception('%s: periodic needs at least two columns along the periodic dim' % who)
        if not np.isfinite(P) or P == 0.0:
            raise Exception('%s: periodic should be a finite, non-zero period, not %r' % (who, periodic))
        if P * span < 0.0:
            raise Exception('%s: periodic=%r runs against the X coordinate (%r ... %r): give it the sign of last - first'
                            % (who, periodic, float(xdeg[0]), float(xdeg[-1])))
        if not abs(P) > abs(span):
            raise Exception('%s: periodic=%r is too short: the X coordinate already spans %r' % (who, periodic, abs(span)))
        return float(np.float64(np.deg2rad(np.float32(P)))) if latlon and not plain else float(np.float64(P))

    def _plane_dcoords(self, who, tracer, hint=''):
        """-> (the data a contour method works on, its coordinates: both plane dims must have values)"""
        data = self.tracer if tracer is None else tracer
        dcoords = lb.unwrap(data, lazy=True)[2]
        for d in (self.dimEqV, self._xdim):
            if d not in dcoords:
                raise Exception('%s needs coordinate values for the plane dim %s%s' % (who, d, hint))
        return data, dcoords

    def _contour_coords(self, who, tracer, latlon, periodic):
        """what cal_contour_lengths, cal_local_contour_lengths and cal_contour_pieces open with -> (the data, its coordinates,
        [ycoord, xcoord] as handed to the library -- cast to float32 as the reference does (core.py:1003-1004), to radians in
        float32 under `latlon`, then to float64 --, the period from `_x_period`)"""
        data, dcoords = self._plane_dcoords(who, tracer)
        f32 = [np.asarray(dcoords[d]).astype(np.float32) for d in (self.dimEqV, self._xdim)]
        fdef = [(np.deg2rad(v) if latlon else v).astype(np.float64) for v in f32]
        return data, dcoords, fdef, self._x_period(periodic, f32[1], latlon, who)

    def _float_plane(self, data):
        """`_plane` with the values through `_float`: what the contour kernels read"""
        q, lead, lshape, coords = self._plane(data)
        return self._float(q), lead, lshape, coords

    @staticmethod
    def _in_caller_order(order, lead, *per_range):
        """per-range lists in sorted-level order (range s * N + j: slab s, sorted level j; `order` from `_sorted_levels`) ->
        for each of them the nesting out[slab][k] with every level where the caller put it, out[k] without leading dims"""
        nslab, N = order.shape
        where = order.tolist()
        outs = []
        for vals in per_range:
            out = [[None] * N for _ in range(nslab)]
            for s, row in enumerate(where):
                for j, k in enumerate(row):                      # j: the sorted level; k: where the caller put it
                    out[s][k] = vals[s * N + j]
            outs.append(out if lead else out[0])
        return outs

    def _length_open(self, who, contours, tracer, latlon, periodic, integrand=_ABSENT):
        """what the length family (K10, K15, K26) opens with, its steps in the order a call's defects are reported in -> (q, K15's
        integrand on the tracer's dims or None, the sorted levels, fdef, the period, the radius, wrap: a (nslab, N) array per SORTED
        level -> the labelled result in the caller's level order).  K27 has a refusal of its own between these steps and takes them itself"""
        if type(contours) in [int, list]:
            contours = self.cal_contours(contours)
        data, _, fdef, period = self._contour_coords(who, tracer, latlon, periodic)
        q, lead, lshape, coords = self._float_plane(data)
        g = None if integrand is _ABSENT else self._aligned_plane(who, integrand, data, q.shape)
        bs, order, ccoord = self._sorted_levels(contours, q.shape[0], lead, lshape)

        def wrap(v):
            return self._wrap_contour(_level_order(v, order).astype(self.dtype), lead, lshape, coords, None, data, ccoord)
        return q, g, bs, fdef, period, Rearth if latlon else 0.0, wrap

    def cal_contour_lengths(self, contours, tracer=None, latlon=False, periodic=False):
        """
        Perimeter of every contour (reference core.py:969-1014, _contour_lengths 1437-1487 and
        utils.contour_length 565-608): the total length of what skimage's find_contours(plane, c)
        traces, one GPU pass per slab for all contours (K10, xc_contour_lengths).

        `contours`: an int or list goes through cal_contours; a labelled array over (..., contour)
        may differ per slab.  Rows are the equivalent dim and columns the other plane dim; their
        coordinates are cast to float32 as the reference does (core.py:1003-1004) and, with
        latlon=True, converted to radians in float32; segments are then great-circle arcs times
        Rearth, else Cartesian distances.  A cell with a NaN corner contributes nothing, and
        contours do not wrap across the X seam (skimage does neither) unless `periodic`: True --
        360 degrees, with latlon=True only -- or the period in the X coordinate's units (degrees
        with latlon=True; of the sign of last - first and longer than that span).  The cell
        between the last and the first column is then traced too, so a contour that circles the
        pole is closed.  A contour of total length 0
        -- a level outside the field's range, at its minimum or maximum, or NaN -- gives NaN
        (utils.py:603-604).  With latlon=True the latitude is the plane's real latitude whatever the
        tracer's dim order (the reference would read longitude as latitude on an (X, Y) tracer).
        Sums are bit-reproducible.  Returns (..., contour) in `self.dtype`.
        """
        q, _, bs, fdef, period, radius, wrap = self._length_open('cal_contour_lengths', contours, tracer, latlon, periodic)
        return wrap(self.ctx.contour_lengths(q, bs, fdef[0], fdef[1], radius=radius, period=period)[0])

    def cal_contour_lengths_coarsened(self, contours, ratios, tracer=None, latlon=False, periodic=False, skipna=False):
        """
        cal_contour_lengths of the block-averaged tracer at every ratio of `ratios` (K26, xc_contour_lengths_scales): the
        marching-squares half of the reference's fractal-dimension script (tests/test_fractal.py:60-73), whose
        cal_contour_lengths(ctr, tracer=coarsen(tracer, ratio)) runs once per ruler.  The tracer goes to the GPU once and is
        coarsened there: coarse node (I, J) of ratio r is the mean of the block [I r, I r + r) x [J r, J r + r) -- trailing
        rows and columns dropped, every value in float64, summed row by row, left to right and top to bottom, divided once --
        and its coordinates are the float64 block means of the coordinates K10 gets (after the float32 cast and deg2rad of
        cal_contour_lengths; nothing is cast again).  skipna=True leaves NaN nodes out of a block and divides by the nodes
        used; else a block with a NaN node is NaN.  `contours`, `tracer`, `latlon`, `periodic` as for cal_contour_lengths; a
        ratio (1 .. 64) must leave two coarse rows and columns and, with `periodic`, divide the number of columns.  Ratio 1
        is cal_contour_lengths itself, bit for bit.  Returns a list with one (..., contour) array in `self.dtype` per
        ratio, or one array for a bare int; any number of ratios (eight per GPU call).
        """
        from collections.abc import Iterable
        who = 'cal_contour_lengths_coarsened'
        isiterable = isinstance(ratios, Iterable)
        rs = [int(r) for r in ratios] if isiterable else [int(ratios)]
        if not rs or min(rs) < 1 or max(rs) > nat.XC_CSCALE_MAXRATIO:
            raise Exception('%s: ratios should be integers in 1 .. %d' % (who, nat.XC_CSCALE_MAXRATIO))
        q, _, bs, fdef, period, radius, wrap = self._length_open(who, contours, tracer, latlon, periodic)
        m = nat.XC_CSCALE_MAXR
        re = [wrap(l) for k in range(0, len(rs), m)
              for l in self.ctx.contour_lengths_scales(q, bs, fdef[0], fdef[1], rs[k:k + m], radius=radius, period=period, skipna=skipna)[0]]
        return re if isiterable else re[0]

    def coarsen(self, ratio, tracer=None, skipna=False):
        """
        The block-averaged tracer of cal_contour_lengths_coarsened as a labelled array (K26's kernel alone, xc_coarsen): what
        the reference's script passes on as `tracerS`.  float64, the dims in the tracer's order, the other dims' coordinates
        and the name kept; the two plane dims carry the float64 block means of their coordinates AS GIVEN (no float32 cast).
        """
        data = self.tracer if tracer is None else tracer
        q, lead, lshape, coords = self._float_plane(data)
        r = int(ratio)
        tdims, g = self._in_dim_order(self.ctx.coarsen(q, r, skipna=skipna), data, lead, lshape)
        coords = dict(coords)
        for d in (self.dimEqV, self._xdim):
            if d in coords:
                coords[d] = _block_means(coords[d], r)
        return lb.wrap(g, tdims, coords, lb.unwrap(data, lazy=True)[3], data)

    def _aligned_plane(self, who, integrand, data, shape):
        """a labelled integrand over the dims of `data` (the tracer a contour method works on) in any order -> its values as
        (S, ny, nx), the slabs in the tracer's order; `shape`: the tracer's own (S, ny, nx)"""
        if not lb.is_labeled(integrand):
            raise Exception('%s: the integrand should be a labelled array over the tracer\'s dims' % who)
        v, dims, _, _ = lb.unwrap(integrand)
        ddims = lb.unwrap(data, lazy=True)[1]
        if len(dims) != len(ddims) or set(dims) != set(ddims):
            raise Exception('%s: the integrand has the dims %r, the tracer %r' % (who, tuple(dims), tuple(ddims)))
        lead = [d for d in ddims if d not in (self.dimEqV, self._xdim)]
        order = [dims.index(d) for d in lead] + [dims.index(self.dimEqV), dims.index(self._xdim)]
        g = np.transpose(np.asarray(v), order)
        g = g.reshape((-1,) + g.shape[-2:])
        if g.shape != tuple(shape):
            raise Exception('%s: the integrand has the shape %r on the tracer\'s dims, the tracer %r' % (who, g.shape, tuple(shape)))
        return np.ascontiguousarray(self._float(g))

    def _line_integrals(self, who, contours, integrand, tracer, latlon, periodic):
        """one K15 call behind cal_contour_line_integral / cal_contour_line_mean, opened like cal_contour_lengths -> (integral, length,
        both (nslab, N) float64 per SORTED level, wrap: such an array -> the labelled result in the caller's level order)"""
        q, g, bs, fdef, period, radius, wrap = self._length_open(who, contours, tracer, latlon, periodic, integrand)
        integ, lens, _ = self.ctx.contour_line_integrals(q, g, bs, fdef[0], fdef[1], radius=radius, period=period)
        return integ, lens, wrap

    def cal_contour_line_integral(self, contours, integrand, tracer=None, latlon=False, periodic=False, return_length=False):
        """
        The integral of `integrand` along every contour, evaluated on the traced contour itself (K15,
        xc_contour_line_integrals): wind speed along a PV contour, |grad q| along a tracer contour, LWA along the
        reference state's contour.  (cal_contour_mean is the area-derivative estimate, which needs a second field and is
        smeared over the bin width.)  Build-defined: the reference has no counterpart.

        `contours`, `tracer`, `latlon`, `periodic`, the float32 cast of the coordinates and the order of the levels are
        handled exactly as in cal_contour_lengths, and the segments are the ones that method sums.  `integrand`: a
        labelled array over the tracer's dims in any order, of the tracer's shape.  It is mapped onto a segment's two end
        points like the coordinates are (linear along the grid edge the point lies on, the node's value on a node), and
        the segment adds 0.5 (F(u) + F(v)) times its length.  A segment with a NaN end-point value is left out of the
        integral AND of the length returned here; a contour of total length 0 gives NaN; a contour that meets an
        infinite value gives a NaN integral.  With latlon=True lengths are great-circle arcs times Rearth.  Sums are
        bit-reproducible.  Returns (..., contour) in `self.dtype`; with return_length=True (integral, length), the length
        over the same segments (cal_contour_lengths' own value when the integrand has no NaN).
        """
        integ, lens, wrap = self._line_integrals('cal_contour_line_integral', contours, integrand, tracer, latlon, periodic)
        return (wrap(integ), wrap(lens)) if return_length else wrap(integ)

    def cal_contour_line_mean(self, contours, integrand, tracer=None, latlon=False, periodic=False):
        """
        The mean of `integrand` along every contour: cal_contour_line_integral divided by the length of the same segments
        (one float64 division; the radius of latlon=True cancels).  NaN where the length is NaN.  Arguments as for
        cal_contour_line_integral.  Returns (..., contour) in `self.dtype`.
        """
        integ, lens, wrap = self._line_integrals('cal_contour_line_mean', contours, integrand, tracer, latlon, periodic)
        with np.errstate(invalid='ignore', divide='ignore'):
            return wrap(integ / lens)

    def cal_local_contour_lengths(self, window, stride=1, levels=None, min_periods=None, tracer=None, latlon=False,
                                  return_levels=False, periodic=False):
        """
        Contour length in a sliding window (the loop of the reference's tests/test_localLength.py: rolling(center=True)
        .construct(stride=) and one find_contours call per window), all windows of all slabs in one GPU pass (K11,
        xc_local_contour_lengths).

        `window` and `stride`: an int, or a {dim: int} dict over the two plane dims (window >= 2 nodes, stride >= 1).  Windows
        are centred on the nodes 0, stride, 2 stride, ... of each plane dim, own the nodes [centre - window // 2,
        centre - window // 2 + window - 1] and are clipped at the plane's edges (no wrap across the X seam unless `periodic`:
        True or a period, as for cal_contour_lengths -- windows then run on round the ring along the non-equivalent plane dim
        instead of being clipped there, and must not be wider than the ring).  Every window is
        traced on its own, as a small plane, at ONE level: `levels` -- a scalar, or an array over (..., windows along the
        equivalent dim, windows along the other plane dim) -- or, by default, the window's NaN-skipping mean, NaN when the
        window holds fewer than `min_periods` valid nodes (None: the full window, as xarray's rolling does).  The length
        follows cal_contour_lengths: the same coordinates (float32 first, radians in float32 with latlon=True), the same
        segments, NaN for a total of 0 or a NaN level; sums are bit-reproducible.  `tracer`: another field on the same
        dims, e.g. the latitude itself for the length of a latitude arc across each window.
        Returns (..., equivalent dim, other plane dim) labelled with the centre nodes' coordinates, in `self.dtype`; with
        return_levels=True also the levels used (float64, same shape).
        """
        pdims = (self.dimEqV, self._xdim)

        def pair(v, what, least):
            if isinstance(v, dict):
                if set(v) != set(pdims):
                    raise Exception('%s should give a value for each of the plane dims %s' % (what, list(pdims)))
                v = tuple(int(v[d]) for d in pdims)
            else:
                v = (int(v), int(v))
            if min(v) < least:
                raise Exception('%s should be at least %d' % (what, least))
            return v
        win, st = pair(window, 'window', 2), pair(stride, 'stride', 1)
        data, dcoords, fdef, period = self._contour_coords('cal_local_contour_lengths', tracer, latlon, periodic)
        if period is not None and win[1] > fdef[1].size:
            raise Exception('window should not be wider than the periodic dim %s: %d > %d nodes' % (self._xdim, win[1], fdef[1].size))
        q, lead, lshape, coords = self._float_plane(data)
        nslab, ny, nx = q.shape
        nw = (-(-ny // st[0]), -(-nx // st[1]))
        if levels is not None:
            if lb.is_labeled(levels):
                lv, ldims, _, _ = lb.unwrap(levels)
                if set(ldims) != set(lead + pdims):
                    raise Exception('levels should be defined on %s' % list(lead + pdims))
                levels = np.transpose(lv, [ldims.index(d) for d in lead + pdims])
            levels = np.asarray(levels, dtype=np.float64)
            if levels.ndim > 2:
                if levels.shape != tuple(lshape) + nw:
                    raise Exception('levels of shape %r do not match the %r windows of %r slabs' % (levels.shape, nw, tuple(lshape)))
                levels = levels.reshape((nslab,) + nw)
        mp = win[0] * win[1] if min_periods is None else int(min_periods)
        lens, lvls, _ = self.ctx.local_contour_lengths(q, fdef[0], fdef[1], win, st, mp, levels=levels,
                                                       radius=Rearth if latlon else 0.0, period=period)
        c = {d: np.asarray(coords[d]) for d in lead if d in coords}
        for d, t in zip(pdims, st):
            c[d] = np.asarray(dcoords[d])[::t]
        dims = tuple(lead) + pdims
        out = lb.wrap(lens.astype(self.dtype).reshape(tuple(lshape) + nw), dims, c, 'local_length', data)
        if return_levels:
            return out, lb.wrap(lvls.reshape(tuple(lshape) + nw), dims, c, 'level', data)
        return out

    # ------------------------------------------------------------------ contour pieces
    # a piece as the facade returns it: the library's record (Context.PIECE_DTYPE) with the row extent on the equivalent dim's coordinate
    PIECE_FIELDS = [({'row_min': 'y_min', 'row_max': 'y_max'}.get(f, f), nat.Context.PIECE_DTYPE[f]) for f in nat.Context.PIECE_DTYPE.names]

    def cal_contour_pieces(self, contours, tracer=None, latlon=False, periodic=False):
        """
        The connected pieces of every contour, one record each, computed on the GPU (K12's segments joined and reduced on
        the device, K13, xc_contour_pieces_dev): what the reference's scripts get by tracing a level with skimage and looping
        over the polylines (tests/test_clength.py: contour_length(seg) per piece; tests/test_breaking.py: the largest contour
        round the pole; utils.contour_area).  Only the per-piece table crosses to the host.

        `contours`, the coordinates (float32 cast; float32 radians with latlon=True), `periodic` and the order of the levels
        are handled exactly as in cal_contour_lengths, so the lengths of a level's pieces add up to that method's value.  A
        piece is a ring, or an open polyline that starts and ends on the plane's edge or beside a NaN cell.

        Returns, per level, a numpy structured array with one row per piece, in the order of
        find_contours(..., return_closed=True) (by the smallest grid-edge id the piece touches):
          first_edge  that id;  nseg  the piece's segments;  closed  True for a ring;
          winding  of a ring on a periodic plane: +1 / -1 when it goes round the ring of columns, else 0;
          length   Cartesian, or great-circle arcs times Rearth with latlon=True;
          area     S = 1/2 sum over the directed segments a -> b of (Ya' + Yb') (Xa - Xb), with Y' = Y, or Y' = sin(Y) and
                   S Rearth^2 with latlon=True (the shoelace formula on the equal-area plane); NaN for an open piece.  For a
                   ring with winding 0, |S| is the enclosed area (utils.contour_area of its vertices), and S > 0 where the
                   ring encloses values above the level when both coordinates ascend (each descending coordinate flips the
                   sign).  For a ring with winding != 0, S is the signed area between the ring and the line Y' = 0: on the
                   sphere the polar cap it bounds measures 2 pi Rearth^2 -/+ S;
          y_min, y_max  the piece's extent along the equivalent dim: its smallest / largest index-space row mapped with
                   np.interp onto that coordinate as given (swapped where the coordinate descends).
        Unlike find_contours, a piece whose segments all have coincident end points (fewer than two distinct vertices) is
        NOT dropped: it stays, with length 0.  The result is out[k] when the tracer has no leading dims, else out[slab][k]
        with the leading dims flattened in the tracer's order.  A NaN level, or a level without segments, gives an empty array.
        Every field is bit-reproducible.
        """
        if type(contours) in [int, list]:
            contours = self.cal_contours(contours)
        data, dcoords, fdef, period = self._contour_coords('cal_contour_pieces', tracer, latlon, periodic)
        q, lead, lshape, _ = self._float_plane(data)
        bs, order, _ = self._sorted_levels(contours, q.shape[0], lead, lshape)
        pc, tab = self.ctx.contour_pieces(q, bs, fdef[0], fdef[1], radius=Rearth if latlon else 0.0, period=period)
        yg = np.asarray(dcoords[self.dimEqV], dtype=np.float64)
        rec = np.empty(tab.size, dtype=self.PIECE_FIELDS)
        for f in tab.dtype.names:
            if f in rec.dtype.names:
                rec[f] = tab[f]
        if tab.size:
            rec['y_min'], rec['y_max'] = self._rows_to_eq(yg, tab['row_min'], tab['row_max'])
        return self._in_caller_order(order, lead, self._per_range(rec, pc))[0]

    # ------------------------------------------------------------------ contour overturning
    def cal_contour_overturning(self, contours, tracer=None, periodic=False, select='main'):
        """
        Where every contour is overturned, computed on the GPU (K12's segments, K13's pieces, K16, xc_contour_overturning_dev):
        how often each meridian -- each column of the plane -- meets the selected pieces of a contour, and between which
        latitudes.  The reference's tests/test_breaking.py keeps "the largest contour fully encircling the pole" and stops
        there; this is the step after it.  Build-defined: the reference has no counterpart.

        `contours`, `tracer` and the order of the levels as for cal_contour_pieces; `periodic` as for find_contours (False, True
        or the period in the X coordinate's own units).  `select`: 'all' -- every piece --, 'circumpolar' -- every ring that goes
        round the ring of columns (winding != 0) --, or 'main': per contour the one such ring with the most segments (ties: the
        smallest first_edge).  The last two need `periodic`.

        A crossing is a vertex of a selected piece that lies on a grid line along the equivalent dim (between the nodes (r, c)
        and (r + 1, c)); every vertex counts once.  Returns a Dataset.  Over (..., contour, X): `ncross`, the crossings of that
        column (int32), and `y_lo` / `y_hi`, the lowest / highest of them along the equivalent dim: the index-space rows mapped
        with np.interp onto that coordinate as given (swapped where the coordinate descends, like cal_contour_pieces' y_min /
        y_max), NaN where ncross is 0.  Over (..., contour): `nsel`, the selected pieces, and `main_first_edge` (-1: none),
        `main_nseg`, `main_winding` (0: none): the ring 'main' picks, under the `first_edge` by which cal_contour_pieces lists it
        (filled under every `select` on a periodic plane).  A column of the main ring with ncross >= 3 is overturned, and
        y_hi - y_lo there is the depth of the fold.  Every value is bit-reproducible.
        """
        p = self._piece_names('cal_contour_overturning', contours, select)
        self._piece_plane(p, tracer, periodic)
        self._piece_levels(p)
        ncross, row_lo, row_hi, nsel, mfe, mns, mw = self.ctx.contour_overturning(p.q, p.bs, periodic=p.ring, select=select)
        y_lo, y_hi = self._rows_to_eq(p.yg, row_lo, row_hi)
        out = [self._on_contours(p, name, v, (self._xdim,)) for name, v in (('ncross', ncross), ('y_lo', y_lo), ('y_hi', y_hi))]
        out += [self._on_contours(p, name, v)
                for name, v in (('nsel', nsel), ('main_first_edge', mfe), ('main_nseg', mns), ('main_winding', mw))]
        return lb.merge(out, p.data)

    def cal_integral_inside_contours(self, contours, tracer=None, integrand=None, periodic=False, select='main', side='upper',
                                     return_mask=False):
        """
        Area, node count and integral of what the SELECTED pieces of every contour bound, computed on the GPU (K12's segments,
        K13's pieces, K16's selection, K17, xc_contour_interior_dev).  Build-defined: the reference has no counterpart.

        cal_integral_within_contours is the reference's threshold rule: it sums dA over every node with q > c (or q < c), so a
        blob or a filament that broke away from the vortex stays in the vortex's bucket.  This method follows the contour
        itself: with select='main' the region is bounded by the one ring cal_contour_overturning calls main -- "the largest
        contour fully encircling the pole" of the reference's tests/test_breaking.py --, whatever the tracer does elsewhere,
        and the difference from the threshold integral is what has been shed.

        `contours`, `tracer`, `periodic`, `select` and the order of the levels as for cal_contour_overturning.  A vertex of a
        selected piece on a grid line along the equivalent dim, between the nodes (r, c) and (r + 1, c), is a crossing of
        column c (every such grid edge counts once).  Walking a column from its first row, a node is on the far side when the
        crossings passed so far are odd in number.  `side`: 'upper' takes the side of the row with the larger equivalent-dim
        coordinate -- the far side when that coordinate ascends, else the near one --, 'lower' the other.  With select='all'
        on a NaN-free tracer the far side of level c is exactly (q > c) != (q[first row] > c), column by column; beside NaN
        cells the crossings are those the segments of find_contours have, and a crossing no NaN-free cell sees is none.

        The weight is this object's dA; `integrand`: a labelled array like the tracer, or None.  Returns a Dataset over
        (..., contour): `area`, the sum of dA over the nodes of the region, `nodes`, their number (int64), and with an
        integrand `integral`, the sum of dA * integrand, each product rounded once.  The sums are exact sums of their float64
        terms rounded once: bit-reproducible, whatever the order; a NaN term is skipped, an infinite one gives NaN.  With
        return_mask=True also `mask`, bool over (..., contour, Y, X).  A NaN level, or one no contour follows, has the whole
        plane on one side.
        """
        p = self._piece_prep('cal_integral_inside_contours', contours, tracer, integrand, periodic, side, select, min_nx=2)
        res = self.ctx.contour_interior(p.q, p.bs, w=p.dA, f=p.g, periodic=p.ring, select=select, flip=p.flip, return_mask=return_mask)
        out = [self._on_contours(p, name, v) for name, v in (('area', res[1]), ('nodes', res[0]), ('integral', res[2])) if v is not None]
        if return_mask:
            out.append(self._on_contours(p, 'mask', res[3], (self.dimEqV, self._xdim)))
        return lb.merge(out, p.data)

    # ------------------------------------------------------------------ distance to contours
    def _distance_open(self, who, contours, tracer, latlon, periodic, select, side):
        """the opening of the two distance methods: the names, the plane with the coordinates the kernels take, a selection that
        needs a ring, the values, the levels sorted, and `flip` from `side` -> (the namespace `_on_contours` closes with, the
        coordinates as the kernels take them, the period, the radius)"""
        p = self._piece_names(who, contours, select, side)
        p.data, p.dcoords, fdef, period = self._contour_coords(who, tracer, latlon, periodic)
        if select != 'all' and period is None:
            raise Exception('%s: select=%r needs periodic (no contour goes round a plane with two free edges): give '
                            'periodic=True or the period, or select=\'all\'' % (who, select))
        p.q, p.lead, p.lshape, p.coords = self._float_plane(p.data)
        p.nslab, p.ny, p.nx = p.q.shape
        p.bs, p.order, p.ccoord = self._sorted_levels(p.contours, p.nslab, p.lead, p.lshape)
        p.yg = np.asarray(fdef[0])
        ascends = p.yg.size < 2 or p.yg[-1] >= p.yg[0]
        p.flip = (side == 'upper') != bool(ascends)
        return p, fdef, period, (Rearth if latlon else 0.0)

    def cal_distance_to_contours(self, contours, tracer=None, latlon=False, periodic=False, select='all', side='upper', signed=False,
                                 max_distance=None, return_nearest=False):
        """
        How far every node of the plane lies from every contour, computed on the GPU (K12's segments, K13's pieces, K16's
        selection, K27, xc_contour_distance_dev): the cross-contour coordinate of front-relative and edge-relative composites
        -- distance from the vortex edge, from a jet axis, from an SSH front; "within 500 km of the main ring" as a mask.  The
        reference's scripts trace a level and query a KD-tree on the host (tests/test_breaking.py).  Build-defined.

        `contours`, the coordinates (float32 cast; float32 radians with latlon=True), `periodic` and the order of the levels
        are handled exactly as in cal_contour_pieces; `select` as in cal_contour_overturning ('circumpolar' and 'main' need
        `periodic`).  The distance is to the nearest point of the selected pieces' segments: Euclidean in the coordinates'
        units -- on a periodic plane the shortest over the images one period either way --, or with latlon=True the
        great-circle distance in metres (Rearth; `periodic` is then True or 360).  `max_distance` (same units; None: no cap):
        nodes farther away get NaN.  signed=True: negative on the `side` that cal_integral_inside_contours marks for the same
        `select` (the mask is made and used on the device).

        Returns a labelled (..., contour, Y, X) array in `self.dtype`, the levels where the caller put them; NaN where the
        level is NaN or has no selected piece, and beyond `max_distance`.  With return_nearest=True a Dataset of `distance`,
        `edge` (int64: the grid-edge id of the nearest segment's start -- its cell is row (id >> 1) // nx, column (id >> 1) % nx;
        among equally near segments the smallest id) and `piece` (int64: the row of that segment's piece in the level's
        cal_contour_pieces table); both -1 where the distance is NaN.  The Cartesian distance is bit-reproducible.

        The result is N full planes per slab: this is meant for a few levels, not for a whole contour set.
        """
        who = 'cal_distance_to_contours'
        p, fdef, period, radius = self._distance_open(who, contours, tracer, latlon, periodic, select, side)
        res = self.ctx.contour_distance(p.q, p.bs, fdef[0], fdef[1], radius=radius, period=period, select=select,
                                        max_distance=max_distance, signed=signed, flip=p.flip, return_nearest=return_nearest)
        dist = res[0] if return_nearest else res
        dist = np.where(np.isinf(dist), np.nan, dist).astype(self.dtype)
        plane = (self.dimEqV, self._xdim)
        if not return_nearest:
            return self._on_contours(p, None, dist, plane)
        edge, piece = res[1], res[2]
        # the piece as the row of the level's cal_contour_pieces table: the tables list a range's pieces by ascending first_edge
        pc, tab = self.ctx.contour_pieces(p.q, p.bs, fdef[0], fdef[1], radius=radius, period=period)
        c, start = nat._scan(pc)
        flat = piece.reshape((c.size,) + piece.shape[2:])
        for r in range(c.size):
            has = flat[r] >= 0
            flat[r][has] = np.searchsorted(tab['first_edge'][start[r]:start[r] + c[r]], flat[r][has])
        out = [self._on_contours(p, name, v, plane) for name, v in (('distance', dist), ('edge', edge), ('piece', piece))]
        return lb.merge(out, p.data)

    def cal_contour_distance_profile(self, contours, bins, fields=None, tracer=None, latlon=False, periodic=False, select='all',
                                     side='upper', signed=False, max_distance=None):
        """
        Composites by distance from every contour, computed on the GPU in one call (K12's segments, K13's pieces, K16's
        selection, K27's search, K28, xc_contour_distance_profile_dev): per contour and distance bin the number of nodes, their
        area and the area-weighted integrals of up to eight fields -- the mean of a field as a function of the (signed) distance
        from the vortex edge, from a jet axis, from a front.  It is np.histogram(distance, bins, weights=dA * field) of
        cal_distance_to_contours, level by level, without the planes: the distance of every node is binned where it is made
        and only (contours x bins) numbers per quantity cross to the host, so a whole contour set and a stack are fine.
        Build-defined.

        `contours`, the coordinates, `periodic`, `select`, `side`, `signed`, `max_distance` and the order of the levels are
        handled exactly as in cal_distance_to_contours, and the distance is that method's, bit for bit.  `bins`: the bin
        edges, ascending, in the distance's units (metres with latlon=True; negative values with signed=True).  The bin rule
        is np.histogram's: a node with distance d lies in bin b when bins[b] <= d < bins[b + 1], and d == bins[-1] lies in the
        last bin; a node with no distance (NaN in cal_distance_to_contours: no selected piece, beyond `max_distance`) or outside
        the edges lies in none.  `fields`: a dict name -> labelled array over the tracer's dims (or over the plane's two dims,
        or a 2-D numpy plane), or one labelled array (named by its name, else 'field'), as in cal_contour_piece_props.  The
        weight is this object's dA.

        Returns a Dataset over (..., contour, distance_bin); the coordinate `distance_bin` holds the bin centres, `bin_lo` and
        `bin_hi` the edges of every bin.  `nodes` (int64): the nodes of the bin; `area`: the sum of dA over them; per field
        `<name>`: the sum of dA * field, each product rounded once; `<name>_mean`: that integral over `area`, NaN where
        `area` is 0.  The sums are exact sums of their float64 terms rounded once: in the Cartesian case every number is
        bit-reproducible, whatever the launch geometry or the batches (with latlon=True the sums are exact too, of the
        distances that device's asin gives).  A NaN term is skipped and an infinite one makes that bin's sum NaN; `nodes` and
        `area` count the node all the same, so `<name>_mean` is a true mean only for a field without NaN: for a field with
        gaps, put the mask into dA.  A NaN level, or one no contour follows, has zeros.
        """
        who = 'cal_contour_distance_profile'
        p, fdef, period, radius = self._distance_open(who, contours, tracer, latlon, periodic, select, side)
        edges = np.asarray(bins, dtype=np.float64)
        if edges.ndim != 1 or edges.size < 2 or not np.isfinite(edges).all() or not (np.diff(edges) > 0).all():
            raise Exception('%s: bins should be at least two finite, ascending edges' % who)
        if fields is None:
            user = {}
        elif isinstance(fields, dict):
            user = dict(fields)
        else:
            user = {getattr(fields, 'name', None) or 'field': fields}
        if len(user) > self.ctx.XC_PROPS_MAXF:
            raise Exception('%s: %d fields, more than the %d one call takes' % (who, len(user), self.ctx.XC_PROPS_MAXF))
        clash = [k for k in user if k in ('nodes', 'area') or k + '_mean' in user]
        if clash:
            raise Exception('%s: the field name %r collides with a variable of the result' % (who, clash[0]))
        planes = self._field_planes(who, user, p.q)
        self._piece_weights(p, None)
        nodes, area, sums, _ = self.ctx.contour_distance_profile(p.q, p.bs, fdef[0], fdef[1], edges, w=p.dA, fields=planes, radius=radius,
                                                                 period=period, select=select, max_distance=max_distance,
                                                                 signed=signed, flip=p.flip)
        lo, hi = edges[:-1], edges[1:]
        p.dcoords = dict(p.dcoords)
        p.dcoords['distance_bin'] = 0.5 * (lo + hi)
        out = [('nodes', nodes), ('area', area)]
        with np.errstate(divide='ignore', invalid='ignore'):
            for m, name in enumerate(user):
                out += [(name, sums[:, :, m]), (name + '_mean', np.where(area == 0.0, np.nan, sums[:, :, m] / area))]
        arrs = [self._on_contours(p, name, np.ascontiguousarray(v), ('distance_bin',)) for name, v in out]
        if lb.is_xarray(p.data):
            arrs = [a.assign_coords(bin_lo=('distance_bin', lo), bin_hi=('distance_bin', hi)) for a in arrs]
        else:
            arrs = [a.assign_coords({'bin_lo': lo, 'bin_hi': hi}) for a in arrs]
        return lb.merge(arrs, p.data)

    # ------------------------------------------------------------------ contour folds
    # an event as the facade returns it: where it sits, and what each tongue holds
    FOLD_FIELDS = ([(k, np.int32) for k in ('c_west', 'c_east', 'ncol', 'ncross_max', 'width')] +
                   [(k, np.float64) for k in ('x_west', 'x_east', 'y_lo', 'y_hi')] +
                   [(k + t, d) for k, d in (('nodes', np.int64), ('area', np.float64), ('integral', np.float64), ('cy', np.float64),
                                            ('cx', np.float64)) for t in ('_under', '_over')] + [('orientation', np.int8)])

    @staticmethod
    def _fold_x(col, xg, period):
        """fractional columns -> the X coordinate: np.interp over the columns; on a ring column nx is xg[0] + period, and a column
        past it runs on by the period"""
        nx = xg.size
        if period is None:
            return np.interp(col, np.arange(nx), xg)
        k = np.floor(col / nx)
        return np.interp(col - k * nx, np.arange(nx + 1), np.append(xg, xg[0] + period)) + k * period

    def cal_contour_folds(self, contours, tracer=None, integrand=None, periodic=False, select='main', gap=0):
        """
        The wave-breaking events of every contour, computed on the GPU (K12's segments, K13's pieces, K16's selection, K17's
        crossing flags, K24, xc_contour_folds_dev): which runs of overturned meridians form one event, where it sits, how much
        each event has folded over and which way it leans.  cal_contour_overturning says which columns are overturned and
        cal_integral_inside_contours what the ring bounds; this is the step after both.  Build-defined: the reference has no
        counterpart.  Only the per-column arrays and one small table per contour cross to the host.

        `contours`, `tracer`, `periodic`, `select`, the order of the levels and the errors as for cal_contour_overturning;
        `integrand` and the weight (this object's dA) as for cal_integral_inside_contours.  `gap`: an int >= 0 (and below the
        number of columns).

        A column is folded when the selected pieces cross its grid line three times or more (ncross >= 3).  Its fold nodes are
        the nodes between the lowest and the highest crossed grid edge (in index space, rows counted from the first).  Walking up
        from the lowest crossing, the nodes passed before the next crossing form the tongue `under`, those after it `over`, and
        so on in turn: `under` is air from beyond the lowest crossing lying under air of the first row's side, `over` is air of
        the first row's side lying over it.  An event is a maximal run of folded columns with at most `gap` unfolded columns
        between consecutive ones; on a periodic plane the last column is followed by the first, and an event across the seam has
        c_east < c_west.

        Returns (cols, events).  `cols`: a Dataset over (..., contour, X) -- `ncross`, `y_lo`, `y_hi`: cal_contour_overturning's,
        bit for bit; `event` (int32): the index of the column's event in its contour's table, -1 for none (an unfolded column
        bridged by `gap` too).  `events`: per level a numpy structured array with one row per event, ordered by c_west -- out[k]
        when the tracer has no leading dims, else out[slab][k] with the leading dims flattened, like cal_contour_pieces:
          c_west, c_east  the first column, the last folded column;  ncol  its folded columns;  ncross_max  the most crossings;
          width  (c_east - c_west) mod nx + 1;  x_west, x_east  the X coordinate at those columns;
          y_lo, y_hi  the extent of the crossings along the equivalent dim, mapped and swapped like cal_contour_overturning's;
          nodes_under, nodes_over  the fold nodes of each tongue;  area_*  the sum of dA over them;  integral_*  the sum of
          dA * integrand, each product rounded once (NaN without an integrand);
          cy_*  the dA-weighted mean row of the tongue mapped with np.interp onto the equivalent dim's coordinate;  cx_*  the
          dA-weighted mean column, counted east from c_west, mapped onto the X coordinate (past the last column it runs on by
          the period, like find_contours' rings);
          orientation (int8)  the sign of the mean column of `over` minus that of `under`: +1 when the overlying tongue leans
          east of the underlying one, -1 west, 0 where either tongue has area 0 or NaN.  Which sign is cyclonic and which
          anticyclonic depends on the hemisphere and on whether the tracer increases towards the pole (`increase`): that is
          left to the caller.
        The sums are exact sums of their float64 terms rounded once: bit-reproducible, whatever the order; a NaN term is
        skipped, an infinite one makes that sum of that tongue NaN.  A NaN level, or a level without segments, gives an empty array.
        """
        who = 'cal_contour_folds'
        p = self._piece_names(who, contours, select)
        if isinstance(gap, (bool, np.bool_)) or not isinstance(gap, (int, np.integer)) or gap < 0:
            raise Exception('%s: gap should be an int >= 0, not %r' % (who, gap))
        self._piece_plane(p, tracer, periodic)
        yg, xg, nx = p.yg, p.xg, p.nx
        if gap >= nx:
            raise Exception('%s: gap=%r should be below the %d columns of the plane' % (who, gap, nx))
        self._piece_levels(p)
        self._piece_weights(p, integrand)
        ncross, row_lo, row_hi, cev, ec, tab = self.ctx.contour_folds(p.q, p.bs, w=p.dA, f=p.g, periodic=p.ring, select=select, gap=int(gap))
        # the columns, every level where the caller put it
        y_lo, y_hi = self._rows_to_eq(yg, row_lo, row_hi)
        cols = lb.merge([self._on_contours(p, name, v, (self._xdim,))
                         for name, v in (('ncross', ncross), ('y_lo', y_lo), ('y_hi', y_hi), ('event', cev))], p.data)
        # the events
        rec = np.zeros(tab.size, dtype=self.FOLD_FIELDS)
        for k in ('c_west', 'c_east', 'ncol', 'ncross_max'):
            rec[k] = tab[k]
        rec['width'] = (tab['c_east'] - tab['c_west']) % nx + 1
        rec['x_west'], rec['x_east'] = xg[tab['c_west']], xg[tab['c_east']]
        rec['y_lo'], rec['y_hi'] = self._rows_to_eq(yg, tab['row_lo'], tab['row_hi'])
        rows = np.arange(yg.size)
        with np.errstate(all='ignore'):
            mcol = tab['mx'] / tab['area']                       # the mean column east of c_west, per tongue
            mrow = tab['my'] / tab['area']
            for t, name in enumerate(('_under', '_over')):
                rec['nodes' + name], rec['area' + name], rec['integral' + name] = tab['nodes'][:, t], tab['area'][:, t], tab['integral'][:, t]
                rec['cy' + name] = np.interp(mrow[:, t], rows, yg)
                rec['cx' + name] = self._fold_x(tab['c_west'] + mcol[:, t], xg, p.period)
            lean = mcol[:, 1] - mcol[:, 0]
            ok = ~np.isnan(tab['area']).any(axis=1) & (tab['area'] != 0.0).all(axis=1) & ~np.isnan(lean)
            rec['orientation'] = np.where(ok, np.sign(np.where(ok, lean, 0.0)), 0.0).astype(np.int8)
        return cols, self._in_caller_order(p.order, p.lead, self._per_range(rec, ec))[0]

    def cal_integral_inside_pieces(self, contours, tracer=None, integrand=None, periodic=False, side='upper'):
        """
        Area, node count and integral of what EVERY piece of every contour bounds, computed on the GPU in one call (K12's
        segments, K13's pieces, K18, xc_contour_piece_interiors_dev).  Build-defined: the reference has no counterpart.

        cal_integral_inside_contours measures one selection per contour -- with select='main' the vortex itself -- and leaves
        out what the vortex has shed.  A cut-off low, a shed filament or a blob of stratospheric air is a closed piece that
        does not go round the pole (winding 0); this method says, for each of them, how many nodes it encloses, how much dA
        (the sum of this object's dA over those nodes, not the planar shoelace `area` of cal_contour_pieces) and how much of
        an integrand.

        `contours`, `tracer` and the order of the levels as for cal_contour_pieces; `periodic` (False, True or the period; it
        needs at least three columns), the weight and `integrand` as for cal_integral_inside_contours.  For one ring the rule is that
        method's with the ring alone selected: walking a column from its first row, a node is inside a ring of winding 0 when
        the ring has been crossed an odd number of times.  For a ring that goes round the pole, `side` picks the region as
        in cal_integral_inside_contours ('upper': the side of the larger equivalent-dim coordinate).  The interior is that of
        the ring ALONE: the nodes of a ring nested inside it are counted, not subtracted -- cal_contour_piece_tree says which
        piece is nested in which and gives the same figures net of the nested pieces.

        Returns, per level (out[k], or out[slab][k] with leading dims), a numpy structured array with one row per piece in
        first_edge order: its rows line up with those of cal_contour_pieces.  first_edge, nseg, closed, winding are that
        method's; `nodes` the inside nodes (int64), `area` the sum of dA over them, and with an integrand `integral`, the sum
        of dA * integrand, each product rounded once.  The sums are exact sums of their float64 terms rounded once; a NaN
        term is skipped, an infinite one gives NaN.  An open piece bounds nothing: nodes -1, area and integral NaN.  A NaN
        level, or a level without segments, gives an empty array.
        """
        p = self._piece_prep('cal_integral_inside_pieces', contours, tracer, integrand, periodic, side)
        pc, tab = self.ctx.contour_piece_interiors(p.q, p.bs, w=p.dA, f=p.g, periodic=p.ring, flip=p.flip)
        return self._ring_tables(p, pc, tab)

    def cal_contour_piece_tree(self, contours, tracer=None, integrand=None, periodic=False, side='upper'):
        """
        Which piece of every contour is NESTED in which, and what every ring bounds net of the rings inside it, computed on
        the GPU in one call (K12's segments, K13's pieces, K18's interiors, K19, xc_contour_piece_tree_dev).  Build-defined: the
        reference has no counterpart.

        cal_integral_inside_pieces returns a flat list of rings, each with all it encloses.  A cut-off low with a warm core, a
        vortex with a hole, an eddy with a ring round it are rings inside rings; this method returns the hierarchy that
        polygon libraries give with their rings (holes, RETR_TREE): a ring encloses another ring of the same level when it holds
        all of the other's inside nodes, and a ring's parent is the innermost ring that encloses it.

        Arguments, validation, the nesting of the return and the row order (first_edge) are those of
        cal_integral_inside_pieces, and so are its fields, bit for bit.  Each level's structured array has beside them
        `parent` (int64: the ROW of the parent in this same array, -1 for none), `depth` (int32: 0 without parent, else the
        parent's + 1), `nchild` (int32: the rings whose parent this is), and over the inside nodes that lie inside no child
        `nodes_net` (int64), `area_net` and, with an integrand, `integral_net` (float64): exact sums rounded once like `area`
        and `integral`, NaN exactly where those are.  For a ring that goes round the pole `side` picks the inside, so the
        nesting of such rings reverses with it.  An open piece bounds nothing and is transparent: parent -1, depth 0, nchild
        0, nodes_net -1, NaN net sums, and it is nobody's parent.
        """
        p = self._piece_prep('cal_contour_piece_tree', contours, tracer, integrand, periodic, side)
        pc, tab = self.ctx.contour_piece_tree(p.q, p.bs, w=p.dA, f=p.g, periodic=p.ring, flip=p.flip)
        return self._ring_tables(p, pc, tab)

    def cal_contour_piece_labels(self, contours, tracer=None, integrand=None, periodic=False, side='upper'):
        """
        Which ring of every contour HOLDS each node, computed on the GPU in one call (K12's segments, K13's pieces, K18's
        interiors, K19's tree, K20, xc_contour_piece_labels_dev).  Build-defined: the reference has no counterpart.

        cal_contour_piece_tree says how many nodes, how much dA and how much of one integrand every ring bounds, gross and net
        of the rings inside it.  This method adds WHICH nodes those are -- the label image that image libraries return beside
        their ring tree --, which is what the centroid of a cut-off low, the extremum of the tracer inside a ring, a composite of
        further fields over one ring, or the overlap of today's blobs with yesterday's need.

        Arguments and validation are those of cal_contour_piece_tree.  Returns (tree, labels): `tree` is exactly what
        cal_contour_piece_tree returns for the same arguments; `labels` is a labelled int32 array over (..., contour, Y, X), laid
        out and coordinated like the `mask` of cal_integral_inside_contours, levels where the caller put them.  labels[..., k, r,
        c] is the ROW in that level's array of `tree` of the innermost ring round node (r, c) -- of the rings whose inside set
        (cal_integral_inside_pieces') holds the node, the one with the fewest nodes --, -1 where no ring holds it.  Open pieces
        bound nothing and never appear.  The nodes labelled p are the nodes `nodes_net`, `area_net` and `integral_net` of row p
        sum over, and depth[label] + 1 rings hold a node.  A NaN level, or a level without segments, is -1 everywhere.
        """
        p = self._piece_prep('cal_contour_piece_labels', contours, tracer, integrand, periodic, side)
        pc, tab, lab = self.ctx.contour_piece_labels(p.q, p.bs, w=p.dA, f=p.g, periodic=p.ring, flip=p.flip)
        return self._ring_tables(p, pc, tab), self._on_contours(p, 'labels', lab, (self.dimEqV, self._xdim))

    def _field_planes(self, who, user, q):
        """the caller's fields (name -> labelled array over the tracer's dims or over the plane's two dims, or a 2-D numpy plane)
        as the kernels read them: (nslab, ny, nx), or (ny, nx) for one plane that every slab shares"""
        planes = []
        for v in user.values():
            v = self._float(self._plane_of(v)[0]) if lb.is_labeled(v) else nat._f48(np.asarray(v))
            if v.ndim == 3 and v.shape[0] == 1 and v.shape != q.shape:
                v = v[0]
            if v.shape not in (tuple(q.shape[1:]), tuple(q.shape)):
                raise Exception('%s: a field should lie over the tracer\'s dims or over the plane\'s two dims' % who)
            planes.append(v)
        return planes

    def cal_contour_piece_props(self, contours, fields=None, extremum=None, tracer=None, latlon=False, periodic=False, side='upper',
                                centroid=True):
        """
        What every ring of every contour HOLDS of further fields -- sums of up to eight fields, the extremum of one field and
        where it sits, the ring's centroid --, computed on the GPU in one call (K12's segments, K13's pieces, K18's interiors,
        K19's tree, K21, xc_contour_piece_props_dev).  Build-defined: the reference has no counterpart.

        These are the reductions one would take over the map of cal_contour_piece_labels (np.bincount(labels, weights=...),
        a minimum per label): here every node is read once on the device, no map is allocated or downloaded, and only the
        per-ring table crosses to the host.

        `contours`, `tracer`, `periodic`, `side`, the order of the levels and the nesting of the return (out[k], or
        out[slab][k] with leading dims) are those of cal_contour_piece_tree.  `fields`: a dict name -> labelled array over the
        tracer's dims (or over the plane's two dims alone, or a 2-D numpy plane: one plane for every slab).  `extremum`: a
        labelled array like the tracer; None: the tracer as the kernels see it; False: no extremum.

        Each level's structured array has cal_contour_piece_tree's fields without an integrand (first_edge ... nodes, area,
        parent, depth, nchild, nodes_net, area_net), bit for bit, and beside them
          per field    `<name>`: the sum of dA * field over the ring's inside nodes (gross), `<name>_net`: over the inside nodes
                       that lie inside no child (the nodes labelled with the ring) -- exact sums rounded once, each product
                       rounded once; a NaN term is skipped; an infinite term makes that field NaN for the ring that holds the
                       node and, gross, for every ring round it;
          extremum     `vmin_net`, `vmax_net`: the smallest and largest value that is not NaN over the net nodes (-0.0 below
                       +0.0), `vmin`, `vmax` the same over all inside nodes (folded over the ring's subtree on the host); their
                       places on the coordinates as given `vmin_y`, `vmin_x`, `vmax_y`, `vmax_x` and `vmin_net_y`, `vmin_net_x`,
                       `vmax_net_y`, `vmax_net_x`: of equal values the node of smallest r * nx + c.  NaN where there is none.
          centroid=True  the moments `mom0`, `mom1`[, `mom2`] (gross) and `mom0_net` ...: the sums of dA * plane for the planes
                       below, float64, built from the coordinates as given, and `centroid_y`, `centroid_x` from the GROSS moments
                       (m0, m1, m2 = mom0, mom1, mom2):
            latlon=True             planes cos(lat) cos(lon), cos(lat) sin(lon), sin(lat) (degrees -> radians in float64)
                                    centroid_y = degrees(arctan2(m2, hypot(m0, m1)))
                                    centroid_x = degrees(arctan2(m1, m0)) % 360
            Cartesian, not periodic planes y, x (no mom2)
                                    centroid_y = m0 / area
                                    centroid_x = m1 / area
            Cartesian, period P     planes y, cos(2 pi (x - x[0]) / P), sin(2 pi (x - x[0]) / P)
                                    centroid_y = m0 / area
                                    centroid_x = (arctan2(m2, m1) % (2 pi)) * P / (2 pi) + x[0]
                       NaN where the moments are NaN and where the vector (m0, m1, m2), (m1, m2) or `area` is zero.
        An open piece holds nothing: NaN everywhere.  More than 8 fields (the caller's plus the moments) raise.
        """
        who = 'cal_contour_piece_props'
        p = self._piece_prep(who, contours, tracer, None, periodic, side)
        q, ny, nx = p.q, p.ny, p.nx
        user = dict(fields or {})
        moments = self._moment_planes(p.yg, p.xg, latlon, p.period) if centroid else []
        names_g = list(user) + ['mom%d' % k for k in range(len(moments))]
        if len(names_g) > self.ctx.XC_PROPS_MAXF:
            raise Exception('%s: %d fields and %d moment planes are %d, more than the %d one call takes'
                            % (who, len(user), len(moments), len(names_g), self.ctx.XC_PROPS_MAXF))
        planes = self._field_planes(who, user, q)
        if extremum is None:
            xq = q[0:p.nslab] if getattr(q, '_xc_lazy_stack', False) else q
        elif extremum is False:
            xq = None
        else:
            xq = self._float(self._plane_of(extremum)[0])
            if xq.shape != q.shape:
                xq = np.ascontiguousarray(np.broadcast_to(np.asarray(xq), q.shape))
        pc, tab, pr = self.ctx.contour_piece_props(q, p.bs, w=p.dA, fields=planes + moments, x=xq, periodic=p.ring, flip=p.flip)
        rec = self._with_props(who, self._table([tab], self._PIECE_NAMES, p.drop), pc, pr, names_g, len(user), xq is not None,
                               p.yg, p.xg, latlon, p.period)
        return self._in_caller_order(p.order, p.lead, self._per_range(rec, pc))[0]

    def cal_contour_piece_overlap(self, contours, other, other_contours=None, tracer=None, integrand=None, periodic=False,
                                  side='upper'):
        """
        Which rings of the tracer's contours share nodes with which rings of ANOTHER field's -- the other day, the other
        member --, computed on the GPU (K20, xc_contour_piece_labels_dev, on either field, then K22, xc_label_overlap_dev).
        Build-defined: the reference has no counterpart.

        This is the step that follows a cut-off low or a shed filament from one day to the next: the contingency table of
        the two label maps of cal_contour_piece_labels (np.unique over the pairs of labels, np.bincount for every sum).  Both
        maps stay on the device; only the two ring tables and the sparse table of pairs cross to the host.  For a ring `a` of
        the tracer the best match is the `b` of its rows with the most `nodes` or `area`; a ring that is born or dies shows as
        a row with -1 on the other side.

        `contours`, `tracer`, `integrand`, `periodic`, `side`, the order of the levels and the nesting of the return are
        those of cal_contour_piece_tree.  `other`: a labelled array with the dims and the shape of the tracer, validated and
        staged like it.  `other_contours`: the levels of `other` (None: `contours`), as many as `contours`: level k of the one
        field is paired with level k of the other, so they must ascend where `contours` ascend (a NaN level sorts last).

        Returns (tree_a, tree_b, overlap).  The trees are exactly what cal_contour_piece_tree returns for the two fields (the
        same `integrand` for both).  overlap[k] (overlap[slab][k] with leading dims) is a structured array, sorted by (a, b),
        with one row per pair of rings that share at least one node: `a`, `b` (int32) the ROWS of tree_a[k] and tree_b[k] of
        the innermost ring round the node in either field, -1 for "in no ring" (nodes in no ring of both fields have no row);
        `nodes` (int64) the shared nodes, `area` the sum of dA over them and `integral` that of dA * integrand (NaN without
        an integrand): exact sums rounded once, a NaN term skipped, an infinite one gives NaN.  The rows of one `a` partition
        the nodes labelled `a`: their `nodes` add up to nodes_net of that row of tree_a, and likewise for `b`.  These are NET
        overlaps, of the nodes labelled with the rings; the gross overlap of two rings with all that is nested in them is the
        sum over both subtrees (`parent`) and is left to the caller.  A level that is NaN or without segments in both fields
        gives an empty array.
        """
        who = 'cal_contour_piece_overlap'
        p = self._piece_prep(who, contours, tracer, integrand, periodic, side)
        if not lb.is_labeled(other):
            raise Exception('%s: other should be a labelled array over the dims of the tracer' % who)
        qb, lead_b, lshape_b, _ = self._float_plane(self._plane_dcoords(who, other)[0])
        if tuple(qb.shape) != tuple(p.q.shape) or list(lead_b) != list(p.lead) or list(lshape_b) != list(p.lshape):
            raise Exception('%s: other should have the dims and the shape of the tracer' % who)
        if other_contours is None:
            other_contours = p.contours
        elif type(other_contours) in [int, list]:
            other_contours = self.cal_contours(other_contours)
        bs_b, order_b, _ = self._sorted_levels(other_contours, p.nslab, p.lead, p.lshape)
        if not np.array_equal(p.order, order_b):
            # range (slab, j) pairs the j-th SORTED level of either field: they must be the same level of the caller's
            raise Exception('%s: other_contours should ascend where contours ascend (the levels of the two fields are paired '
                            'in the order given, and both are traced in ascending order)' % who)
        pc, tab, pc_b, tab_b, pairs, rows = self.ctx.contour_piece_overlap(p.q, qb, p.bs, contours_b=bs_b, w=p.dA, f=p.g,
                                                                           periodic=p.ring, flip=p.flip)
        packed = [(self._table([t], self._PIECE_NAMES, p.drop), n) for t, n in ((tab, pc), (tab_b, pc_b))]
        packed.append((self._table([rows], self._PIECE_NAMES), pairs))
        return tuple(self._in_caller_order(p.order, p.lead, *[self._per_range(rec, n) for rec, n in packed]))

    def cal_contour_piece_tracks(self, contours, along, tracer=None, integrand=None, periodic=False, side='upper', min_overlap=0.0):
        """
        The rings of every contour FOLLOWED along a leading dim of the tracer -- every cut-off low, shed filament and vortex
        fragment from birth to death, with splits and mergers --, computed on the GPU (K20, xc_contour_piece_labels_dev, ONCE
        per step; K22, xc_label_overlap_dev, between consecutive steps; K23, xc_ring_tracks_dev, over the whole stack).
        Build-defined: the reference has no counterpart.

        This replaces a loop of cal_contour_piece_overlap(tracer[t], tracer[t + 1]) calls and a union-find over their rows on
        the host: there every step is traced and labelled twice, here once; the label maps stay on the device in a sliding
        window; the connected components of the ring graph are found on the device.

        `contours`, `tracer`, `integrand`, `periodic`, `side` and the order of the levels are those of cal_contour_piece_tree.
        `along` names a LEADING dim of the tracer, for instance time; anything else raises.  The other leading dims are
        independent series.  Level k of one step is followed into level k of the next, so the levels of a series must ascend
        in the same order at every step.  `min_overlap` in [0, 1]: a link between two rings counts when their shared nodes are at
        least that fraction of the smaller ring's nodes_net (exactly: float64(nodes) >= min_overlap * float64(min(nodes_net[a],
        nodes_net[b])), the product rounded once); 0: any shared node.

        Returns (tree, links, tracks).
        tree     what cal_contour_piece_tree returns for the same arguments, bit for bit, nested the same way over all leading
                 dims, with three more fields per ring: `track` (int64: a row of that series' tracks[k]; an open piece bounds
                 nothing, has no links and is a track of one), `nprev`, `nnext` (int32: the accepted links to rings of the step
                 before / after).
        links    links[series][k] (links[k] when `along` is the only leading dim; the series are the other leading dims
                 flattened in the tracer's order): a structured array sorted by (step, a, b): `step` (int32) the index along
                 `along` of the EARLIER field; `a`, `b` (int32) rows of tree[step][k] and tree[step + 1][k], -1 for "in no
                 ring" -- exactly cal_contour_piece_overlap's rows of the two steps, all kept; `nodes`, `area` as there;
                 `linked` (bool) whether the link was accepted.  These are that method's NET overlaps, of the nodes labelled
                 with the ring (the innermost ring round them), not of all a ring encloses.
        tracks   tracks[series][k]: one row per track, in the order of its first ring's (step, row): `first_step`, `first_row`
                 (the first ring is tree[first_step][k][first_row]), `last_step`, `nrings`, `nsplit` (its rings with nnext >= 2),
                 `nmerge` (its rings with nprev >= 2).  A track is a connected component of the accepted links: after a merger the
                 merged rings share one track.
        """
        who = 'cal_contour_piece_tracks'
        p = self._piece_prep(who, contours, tracer, integrand, periodic, side)
        lead, lshape, order, nslab = p.lead, p.lshape, p.order, p.nslab
        if along not in lead:
            raise Exception('%s: along should name a leading dim of the tracer (one of %r), not %r' % (who, tuple(lead), along))
        ax = list(lead).index(along)
        # the slabs of every series, in step order: the other leading dims, flattened in the tracer's order, are the series
        series = np.moveaxis(np.arange(nslab).reshape(tuple(lshape)), ax, -1).reshape(-1, lshape[ax])
        if (order[series] != order[series[:, :1]]).any():
            raise Exception('%s: the levels of a series should ascend in the same order at every step (level k of one step is '
                            'followed into level k of the next, and every step is traced in ascending order)' % who)
        qs = p.q[0:nslab] if getattr(p.q, '_xc_lazy_stack', False) else p.q
        N = order.shape[1]
        trees, links, rows = [None] * (nslab * N), [], []
        for sl in series:
            pc, tab, ring, lcount, lk, tcount, tr = self.ctx.contour_piece_tracks(
                qs[sl], p.bs[sl], w=p.dA[sl] if p.dA.ndim == 3 else p.dA, f=None if p.g is None else p.g[sl], periodic=p.ring, flip=p.flip,
                min_overlap=min_overlap)
            by_step = self._per_range(self._table([tab, ring], self._PIECE_NAMES, p.drop), pc)
            for t, s in enumerate(sl.tolist()):
                trees[s * N:(s + 1) * N] = by_step[t * N:(t + 1) * N]
            ov = self._table([lk], self._PIECE_NAMES)
            by_range = self._per_range(ov, lcount)               # packed by (step, level): a level's ranges, joined, are sorted by step
            per_level = [np.concatenate(by_range[j::N]) if by_range else ov[:0].copy() for j in range(N)]
            where = order[sl[0]].tolist()                        # j: the sorted level; where[j]: where the caller put it
            for vals, out in ((per_level, links), (self._per_range(tr, tcount), rows)):
                out.append([None] * N)
                for j, k in enumerate(where):
                    out[-1][k] = vals[j]
        tree = self._in_caller_order(order, lead, trees)[0]
        return (tree, links[0], rows[0]) if len(lead) == 1 else (tree, links, rows)

    @staticmethod
    def _moment_planes(yg, xg, latlon, period):
        """the planes whose dA-weighted sums give a ring's centroid (cal_contour_piece_props states them): float64 (ny, nx) each"""
        yg, xg = np.asarray(yg, dtype=np.float64), np.asarray(xg, dtype=np.float64)
        shape = (yg.size, xg.size)
        if latlon:
            lat, lon = np.deg2rad(yg)[:, None], np.deg2rad(xg)[None, :]
            planes = [np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat) * np.ones_like(lon)]
        elif period is None:
            planes = [yg[:, None] * np.ones(shape), xg[None, :] * np.ones(shape)]
        else:
            a = 2 * np.pi * (xg - xg[0]) / period
            planes = [yg[:, None] * np.ones(shape), np.cos(a)[None, :] * np.ones(shape), np.sin(a)[None, :] * np.ones(shape)]
        return [np.ascontiguousarray(p, dtype=np.float64) for p in planes]

    @staticmethod
    def _centroid_of(m, area, latlon, period, x0):
        """(centroid_y, centroid_x) from the gross moments m[0], m[1][, m[2]] and the gross area: the formulas of
        cal_contour_piece_props, verbatim"""
        with np.errstate(all='ignore'):
            if latlon:
                m0, m1, m2 = m
                cy = np.degrees(np.arctan2(m2, np.hypot(m0, m1)))
                cx = np.degrees(np.arctan2(m1, m0)) % 360
                zero = (m0 == 0) & (m1 == 0) & (m2 == 0)
            elif period is None:
                m0, m1 = m
                cy = m0 / area
                cx = m1 / area
                zero = area == 0
            else:
                m0, m1, m2 = m
                cy = m0 / area
                cx = (np.arctan2(m2, m1) % (2 * np.pi)) * period / (2 * np.pi) + x0
                zero = (area == 0) | ((m1 == 0) & (m2 == 0))
        bad = zero | np.isnan(cy) | np.isnan(cx)
        return np.where(bad, np.nan, cy), np.where(bad, np.nan, cx)

    @staticmethod
    def _order_key(v):
        """the monotone uint64 key of float64 values: unsigned order of the keys = order of the values, -0.0 below +0.0"""
        b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
        sign = np.uint64(1) << np.uint64(63)
        return np.where(b & sign != 0, ~b, b | sign)

    @staticmethod
    def _gross_extrema(parent, depth, v_net, at_net, largest):
        """the extremum over a ring's whole subtree from the net extrema of its rings: `parent` GLOBAL rows (-1: none), `v_net` NaN
        and `at_net` -1 where a ring has none -> (v, at).  Deepest rings first, one vectorised step per depth level; among rings
        the smaller value wins (`largest`: the larger), then the smaller flat node."""
        v, at = np.array(v_net, dtype=np.float64), np.array(at_net, dtype=np.int64)
        key = Contour2D._order_key(v)
        if largest:
            key = ~key
        has = at >= 0
        for d in range(int(depth.max()) if depth.size else 0, 0, -1):
            kids = np.flatnonzero((depth == d) & has & (parent >= 0))
            if not kids.size:
                continue
            o = kids[np.lexsort((at[kids], key[kids], parent[kids]))]          # by parent, then value, then node
            best = o[np.concatenate([[True], parent[o][1:] != parent[o][:-1]])]   # the best child of every parent
            par = parent[best]
            take = ~has[par] | (key[best] < key[par]) | ((key[best] == key[par]) & (at[best] < at[par]))
            best, par = best[take], par[take]
            v[par], at[par], key[par], has[par] = v[best], at[best], key[best], True
        return v, at

    def _piece_prep(self, who, contours, tracer, integrand, periodic, side, select=_ABSENT, min_nx=3):
        """the opening of the methods that run on K12's records, in one call: what the six cal_*piece* methods and
        cal_integral_inside_contours do before their own call.  Four steps, which report a call's defects in this order; a method
        with a check of its own between two of them (cal_contour_folds' `gap`) or without weights (cal_contour_overturning) takes
        the steps one by one.  Returns the namespace they fill: who, contours, select, side; data, dcoords, yg, xg, period, ring, q,
        lead, lshape, coords, nslab, ny, nx; bs, order, ccoord; dA, g, flip, and `drop`: the fields of the ring tables that an
        absent integrand leaves out"""
        p = self._piece_names(who, contours, select, side)
        self._piece_plane(p, tracer, periodic, min_nx)
        self._piece_levels(p)
        self._piece_weights(p, integrand)
        return p

    def _piece_names(self, who, contours, select=_ABSENT, side=_ABSENT):
        """step 1: contours from an int or list, then the names `select` and `side`, where the method has them"""
        p = types.SimpleNamespace(who=who, select=select, side=side)
        if type(contours) in [int, list]:
            contours = self.cal_contours(contours)
        p.contours = contours
        if select is not _ABSENT and select not in nat.Context.OVERTURN_SELECT:
            raise Exception('%s: select should be one of %s, not %r' % (who, sorted(nat.Context.OVERTURN_SELECT), select))
        if side is not _ABSENT and side not in ('upper', 'lower'):
            raise Exception('%s: side should be \'upper\' or \'lower\', not %r' % (who, side))
        return p

    def _piece_plane(self, p, tracer, periodic, min_nx=2):
        """step 2: the plane and its coordinates, the period, a selection that needs a ring, the values the kernels read, the
        ring's fewest columns (`_x_period` asks for two; the ring methods for three)"""
        who = p.who
        p.data, p.dcoords = self._plane_dcoords(who, tracer)
        p.yg, p.xg = (np.asarray(p.dcoords[d], dtype=np.float64) for d in (self.dimEqV, self._xdim))
        p.period = self._x_period(periodic, p.xg, False, who, plain=True)
        p.ring = p.period is not None
        if p.select not in (_ABSENT, 'all') and not p.ring:
            raise Exception('%s: select=%r needs periodic (no contour goes round a plane with two free edges): give '
                            'periodic=True or the period, or select=\'all\'' % (who, p.select))
        p.q, p.lead, p.lshape, p.coords = self._float_plane(p.data)
        p.nslab, p.ny, p.nx = p.q.shape
        if p.ring and p.nx < min_nx:
            raise Exception('%s: periodic needs at least three columns along the periodic dim' % who)

    def _piece_levels(self, p):
        """step 3: the levels sorted"""
        p.bs, p.order, p.ccoord = self._sorted_levels(p.contours, p.nslab, p.lead, p.lshape)

    def _piece_weights(self, p, integrand):
        """step 4: dA as a plane, the integrand, `flip` from `side` (nothing reads it where the method has none)"""
        p.dA = self._dA_array(p.ny, p.nx, p.nslab)[0]
        if p.dA.ndim == 1:
            p.dA = np.ascontiguousarray(np.broadcast_to(p.dA[:, None], (p.ny, p.nx)))
        p.g = None
        if integrand is not None:
            p.g = self._integrand_plane(integrand)
            if p.g.shape != p.q.shape:
                p.g = np.ascontiguousarray(np.broadcast_to(np.asarray(p.g), p.q.shape))
        ascends = p.yg.size < 2 or p.yg[-1] >= p.yg[0]
        p.flip = (p.side == 'upper') != bool(ascends)
        p.drop = () if p.g is not None else ('sum_wf', 'net_wf')

    def _on_contours(self, p, name, v, trailing=()):
        """the closing: a result (nslab, N, ...) per SORTED level -> the labelled array `name` over (lead dims, 'contour', the plane
        dims `trailing`), every level where the caller put it"""
        if not hasattr(p, 'cc'):                                 # built once per call: lb.wrap takes from it what the dims name
            p.cc = {d: np.asarray(p.coords[d]) for d in p.lead if d in p.coords}
            p.cc['contour'] = np.asarray(p.ccoord)
            p.cc.update((d, np.asarray(p.dcoords[d])) for d in (self.dimEqV, self._xdim))
        p.cc.update((d, np.asarray(p.dcoords[d])) for d in trailing if d not in p.cc)    # (a dim of the result alone: distance_bin)
        v = _level_order(v, p.order.reshape(p.order.shape + (1,) * (v.ndim - 2)))
        return lb.wrap(v.reshape(tuple(p.lshape) + v.shape[1:]), tuple(p.lead) + ('contour',) + tuple(trailing), p.cc, name, p.data)

    @staticmethod
    def _rows_to_eq(yg, lo, hi):
        """index-space rows `lo` <= `hi` -> (the smaller, the larger) of their places on the equivalent dim's coordinate `yg` as
        given: np.interp of either, swapped where the coordinate descends"""
        rows = np.arange(yg.size)
        ya, yb = np.interp(lo, rows, yg), np.interp(hi, rows, yg)
        return np.minimum(ya, yb), np.maximum(ya, yb)

    # the fields of the library's tables under the names this class returns them by
    _PIECE_NAMES = {'n_in': 'nodes', 'sum_w': 'area', 'sum_wf': 'integral', 'n_net': 'nodes_net', 'net_w': 'area_net',
                    'net_wf': 'integral_net', 'n': 'nodes'}

    @staticmethod
    def _table(srcs, names=None, drop=(), more=()):
        """one structured array with the fields of `srcs` (structured arrays of one length) side by side -- renamed through `names`,
        without those of `drop` --, then the fields `more` = [(name, dtype), ...], which are left to the caller to fill"""
        names = names or {}
        keep = [(s, f) for s in srcs for f in s.dtype.names if f not in drop]
        out = np.empty(srcs[0].size, dtype=[(names.get(f, f), s.dtype[f]) for s, f in keep] + list(more))
        for s, f in keep:
            out[names.get(f, f)] = s[f]
        return out

    @staticmethod
    def _per_range(rec, counts):
        """records packed range by range, `counts` of them in each -> a list with every range's own array"""
        poff = np.concatenate([[0], np.cumsum(counts.ravel().astype(np.int64))])
        return [rec[a:b].copy() for a, b in zip(poff[:-1], poff[1:])]

    def _ring_tables(self, p, pc, tab):
        """the packed table of a ring call under this class's field names -> nested per level, in the caller's order"""
        return self._in_caller_order(p.order, p.lead, self._per_range(self._table([tab], self._PIECE_NAMES, p.drop), pc))[0]

    def _with_props(self, who, rec, pc, pr, names_g, nuser, has_x, yg, xg, latlon, period):
        """the packed table of cal_contour_piece_tree with K21's columns beside it (cal_contour_piece_props names them)"""
        nx = xg.size
        cols = []
        for m, name in enumerate(names_g):
            cols += [(name, pr['gross'][:, m]), (name + '_net', pr['net'][:, m])]
        if has_x:
            # parent is a row of the piece's own range: -> a row of the packed table
            c, start = nat._scan(pc)
            gpar = np.where(rec['parent'] >= 0, rec['parent'] + np.repeat(start, c), -1)
            ext = {'vmin_net': (pr['x_min'], pr['at_min']), 'vmax_net': (pr['x_max'], pr['at_max']),
                   'vmin': self._gross_extrema(gpar, rec['depth'], pr['x_min'], pr['at_min'], False),
                   'vmax': self._gross_extrema(gpar, rec['depth'], pr['x_max'], pr['at_max'], True)}
            cols += [(k, ext[k][0]) for k in ('vmin_net', 'vmax_net', 'vmin', 'vmax')]
            for k in ('vmin', 'vmax', 'vmin_net', 'vmax_net'):
                at = ext[k][1]
                there = at >= 0
                cols += [(k + '_y', np.where(there, yg[np.maximum(at, 0) // nx], np.nan)),
                         (k + '_x', np.where(there, xg[np.maximum(at, 0) % nx], np.nan))]
        if len(names_g) > nuser:
            cy, cx = self._centroid_of([pr['gross'][:, m] for m in range(nuser, len(names_g))], rec['area'], latlon, period,
                                       float(xg[0]))
            cols += [('centroid_y', cy), ('centroid_x', cx)]
        taken = set(rec.dtype.names)
        for name, _ in cols:
            if name in taken:
                raise Exception('%s: the field name %r is taken' % (who, name))
            taken.add(name)
        out = self._table([rec], more=[(name, np.float64) for name, _ in cols])
        for name, v in cols:
            out[name] = v
        return out

    # ------------------------------------------------------------------ contour polylines
    def find_contours(self, contours, tracer=None, index=False, return_closed=False, periodic=False, return_winding=False):
        """
        The contours themselves: every level traced into polylines on the GPU (K12, xc_contour_segments, and the host join
        xc_join_segments).  The reference's scripts do this with skimage's find_contours through a `find_contour` helper that
        is not part of the reference snapshot this package was built against, so what follows is build-defined.

        `contours` as for cal_contour_lengths: an int or list goes through cal_contours; a labelled array over (..., contour)
        may differ per slab; levels in any order, a NaN level has no polylines.  The segments are those cal_contour_lengths
        sums (same case table, saddles, NaN cells; no wrap across the X seam unless `periodic`), directed, and joined by
        matching the grid edges their end points lie on -- no float comparison.  A polyline's vertices are the start of its
        first segment and the end of every segment; consecutive equal vertices are merged, polylines left with fewer than two
        vertices are dropped, and a closed polyline (a ring) repeats its first vertex at the end.  An open polyline starts and
        ends on the plane's edge or beside a NaN cell.  The polylines of a level are ordered by the smallest grid-edge id they
        touch.

        Each polyline is an (n, 2) float64 array [row, column] = [equivalent dim, other plane dim]: with index=True in index
        space, else mapped onto the plane's coordinates AS GIVEN with np.interp(., arange(n), coord) in float64 (no float32
        cast, unlike cal_contour_lengths).  Returns out[k] -- a list of arrays per level -- when the tracer has no leading dims,
        else out[slab][k] with the leading dims flattened in the tracer's order; with return_closed=True also the same nesting
        of bools (True: a ring), with return_winding=True also the same nesting of ints (below): out[, closed][, winding].

        `periodic`: False, True or the period, the values cal_contour_lengths takes (K12's periodic form,
        xc_contour_segments_periodic).  The cell between the last and the first column is then traced too, so a contour that
        circles the pole is one ring.  The period is in the X coordinate's units as given, in float64 (no float32 cast, no
        radians); True is 360 along the direction the coordinate runs in; it has the sign of last - first, is longer than that
        span, and the ring has at least two columns.  With index=True only its truth value matters and no coordinates are
        needed.  A polyline runs on continuously past the seam instead of jumping back: in walk order every segment has an
        integer lap m, 0 for the first, one more each time the walk leaves the seam cell through its right edge into column 0
        and one less the other way.  With index=True a vertex column is c + nx m, c in [0, nx] as the kernel wrote it (one
        float64 addition: it rounds once where m != 0); else x = np.interp(c, arange(nx + 1), [x..., x[0] + P]) + m P.  Rows
        map as ever.  The winding number W of a ring is the number of times it goes round the ring of columns, signed by its
        direction of travel in X: 0 for an ordinary ring, +1 or -1 for one that circles the globe; 0 for an open polyline.  A
        ring still repeats its first vertex, but with W != 0 its last vertex is the first displaced by W nx columns (W P in
        coordinates).  Without `periodic` every winding number is 0.

        The same tracing with the join on the GPU, and all polylines as one vertex array: `trace_contours` (join='device',
        packed=True); this method is trace_contours with join='host' and packed=False.
        """
        return self.trace_contours(contours, tracer=tracer, index=index, return_closed=return_closed, periodic=periodic,
                                   return_winding=return_winding)

    def trace_contours(self, contours, tracer=None, index=False, return_closed=False, periodic=False, return_winding=False,
                       join='host', packed=False):
        """
        find_contours -- every argument before `join` and the nested return are find_contours', which states the rule -- with a
        choice of where the segments are joined and of the form of the result.

        `join`: 'host' -- the segment records are downloaded, sorted and joined on one host thread (xc_join_segments) -- or
        'device': the join runs on the GPU (K14, xc_contour_polylines_dev) and only the walk-ordered records and the polyline
        table are downloaded; the result is the same bit for bit.  The device join numbers edges in 32 bits: a plane with
        2 ny nx >= 2^31 raises and names join='host'.  Any other value raises.

        `packed`: True -- instead of one small array per polyline, ONE (M, 2) float64 vertex array for the whole call, built
        with array operations only (no Python loop over polylines): returns (verts, vert_off, closed, winding, span).  Polyline
        p has the vertices verts[vert_off[p]:vert_off[p + 1]] -- the same vertices, by the same rule, as the array the nested
        return holds for it --, closed[p] (bool) and winding[p] (int64); span (N, 2), or (nslab, N, 2) with leading dims, int64:
        the polylines of level k (where the caller put it) of slab s are [span[s, k, 0], span[s, k, 1]), in the nested order.
        return_closed / return_winding do not apply.
        """
        if join not in ('host', 'device'):
            raise Exception('trace_contours: join must be \'host\' or \'device\', got %r' % (join,))
        if type(contours) in [int, list]:
            contours = self.cal_contours(contours)
        if index:                                                # no coordinates needed, and only the truth value of `periodic`
            data, cds, period, ring = self.tracer if tracer is None else tracer, [None, None], None, bool(periodic)
        else:                                                    # the coordinates as given, in float64, and the period in their units
            data, dcoords = self._plane_dcoords('find_contours', tracer, ' (or index=True)')
            cds = [np.asarray(dcoords[d], dtype=np.float64) for d in (self.dimEqV, self._xdim)]
            period = self._x_period(periodic, cds[1], False, 'find_contours', plain=True)
            ring = period is not None
        q, lead, lshape, _ = self._float_plane(data)
        nslab, nx = q.shape[0], q.shape[2]
        if ring and nx < 2:
            raise Exception('find_contours: periodic needs at least two columns along the periodic dim')
        bs, order, _ = self._sorted_levels(contours, nslab, lead, lshape)
        if join == 'device':
            _check_device_join(q.shape[1], nx)
            cnt, _, pts, poff, closed, rpo = self.ctx.contour_polylines(q, bs, periodic=ring)
            walk = np.arange(pts.shape[0], dtype=np.int64)
        else:
            cnt, ef, et, pts = self.ctx.contour_segments(q, bs, periodic=ring)
            off = np.concatenate([[0], np.cumsum(cnt.ravel().astype(np.int64))])
            walk, poff, closed, rpo = nat.join_segments(off, ef, et)
        if packed:
            verts, voff, cl, wd, rk = contour_polylines(walk, poff, closed, rpo, pts, nx=nx if ring else None,
                                                        ycoord=cds[0], xcoord=cds[1], period=period, packed=True)
            N = order.shape[1]
            span = np.empty((nslab, N, 2), dtype=np.int64)                   # per sorted level -> where the caller put it
            np.put_along_axis(span, order[:, :, None], np.stack([rk[:-1], rk[1:]], axis=1).reshape(nslab, N, 2), axis=1)
            return verts, voff, cl, wd, (span if lead else span[0])
        polys, cl, wd = contour_polylines(walk, poff, closed, rpo, pts, nx=nx if ring else None,
                                          ycoord=cds[0], xcoord=cds[1], period=period)
        out, flags, winds = self._in_caller_order(order, lead, polys, cl, wd)
        res = (out,) + ((flags,) if return_closed else ()) + ((winds,) if return_winding else ())
        return res if len(res) > 1 else out

    # ------------------------------------------------------------------ local wave activity
    def cal_local_wave_activity(self, q, Q, mask_idx=None, part='all', metric=None, exact=None):
        """
        Local finite-amplitude wave activity density (reference core.py:696-799;
        Huang and Nakamura 2016).  The J-iteration python loop of the reference is one
        GPU kernel.  `metric=None` follows the snapshot (M = dA, core.py:789); pass the
        1-D length metric (e.g. dy) for the legacy grid.get_metric form (core.py:787-788).
        Planes of up to 512 rows are summed in numpy's own order (bit-identical to the reference's nansum); larger ones take
        an O(ny log ny)-per-column path that needs a monotone Q (checked; else the exact walk runs) and agrees to ~1e-13;
        `exact=True` keeps the bit-exact walk everywhere, `exact=False` takes the interval path for every plane with a monotone Q.
        """
        return self._lwa(q, Q, mask_idx, part, metric, 'LWA', exact=exact)

    def cal_local_wave_activity2(self, q, Q, mask_idx=None, part='all', metric=None):
        """The impulse-Casimir flavoured variant (reference core.py:802-905): qe = q[row j] - Q
        with the opposite sign convention; same GPU kernel family."""
        return self._lwa(q, Q, mask_idx, part, metric, 'LWA', variant=1)

    def cal_local_APE(self, q, Q, mask_idx=None, part='all', metric=None, exact=None):
        """Local available potential energy density (reference core.py:908-942)."""
        return self._lwa(q, Q, mask_idx, part, metric, 'LAPE', exact=exact)

    def _lwa(self, q, Q, mask_idx, part, metric, name, variant=0, exact=None):
        part = part.lower()
        if part not in ['all', 'upper', 'lower']:
            raise Exception('invalid part, should be in [\'all\', \'upper\', \'lower\']')
        qv, lead, lshape, coords = self._plane(q)
        qv = self._float(qv)
        nslab, ny, nx = qv.shape
        eq = self._eq_coord(q)
        if mask_idx is not None and max(mask_idx) >= len(eq):
            raise Exception('indices in mask_idx out of boundary')
        Qv, Qdims, _, _ = lb.unwrap(Q)
        if self.dimEqV not in Qdims:
            raise Exception('Q should be defined on %s' % self.dimEqV)
        # Q's leading dims in the TRACER's leading-dim order (missing ones broadcast), so that slab s of q meets row s of Q
        Ql = [d for d in Qdims if d != self.dimEqV]
        extra = [d for d in Ql if d not in lead]
        if extra:
            raise Exception('Q has dims %r that q does not have' % extra)
        order = [d for d in lead if d in Ql]
        Qv = np.transpose(Qv, [Qdims.index(d) for d in order] + [Qdims.index(self.dimEqV)])
        shp = [lshape[lead.index(d)] if d in Ql else 1 for d in lead] + [ny]
        Qv = np.ascontiguousarray(np.broadcast_to(Qv.reshape(shp), tuple(lshape) + (ny,)), dtype=np.float64).reshape(nslab, ny)
        dA, _ = self._dA_array(ny, nx, 1)
        if dA.ndim == 3:
            dA = dA[0]
        # wei = dA / dA.max(), core.py:723-724 (NaN-skipping, like xarray's max).  A maximum is exact wherever it is taken: on the host
        # (np.fmax skips NaN; a GPU pass for it was 24-64 us of a 170-260 us call), once per weights object when the object is resident
        memo = self.__dict__.get('_dmax_memo') if self.resident else None
        if memo is not None and memo[0] is dA:
            dmax = memo[1]
        else:
            dmax = float(np.fmax.reduce(dA, axis=None))
            if self.resident:
                self.__dict__['_dmax_memo'] = (dA, dmax)
        M = None
        if metric is not None:
            M = np.asarray(lb.unwrap(metric)[0] if lb.is_labeled(metric) else metric, dtype=np.float64).squeeze()
        pcode = {'all': 0, 'upper': 1, 'lower': 2}[part]
        if exact is None and self.deterministic:
            exact = True         # deterministic=True promises run-to-run identical bits: the interval kernel's LDS atomics add in arrival order
        lwa, masks = self.ctx.lwa(qv, Qv, eq.astype(np.float64), dA, dmax, M=M, increase=self.increase,
                                  part=pcode, mask_idx=mask_idx, variant=variant, exact=exact)
        qdims, out = self._in_dim_order(lwa, q, lead, lshape)                  # .transpose(*q.dims), core.py:793
        c = dict(coords)
        c[self.dimEqV] = eq
        LWA = lb.wrap(out, qdims, c, name, q)
        if mask_idx is None:
            return LWA
        contours, mlist = [], []
        Ql_coords = {d: coords[d] for d in lead if d in coords}
        for i, j in enumerate(mask_idx):
            contours.append(lb.wrap(Qv[:, j].reshape(lshape) if lshape else Qv[0, j], tuple(lead), Ql_coords, lb.unwrap(Q, lazy=True)[3], q))
            mlist.append(lb.wrap(self._in_dim_order(masks[:, i].astype(np.int64), q, lead, lshape)[1], qdims, c, None, q))
        return LWA, contours, mlist

    # ------------------------------------------------------------------ extensions
    def cal_squared_gradient(self, tracer=None, lat=None, lon=None, rdx=None, rdy=None, periodic_x=True):
        """|grad q|^2 on the GPU (build-defined stencil; the reference takes grdS as an input,
        SURVEY F7).  Metrics from `lat, lon` (degrees, sphere) or explicit per-row `rdx, rdy`."""
        if tracer is None:
            tracer = self.tracer
        q, lead, lshape, coords = self._plane(tracer)
        q = self._float(q)
        if rdx is None:
            rdx, rdy = grad_metrics(lat if lat is not None else coords[self.dimEqV],
                                    lon if lon is not None else coords[self._xdim])
        g = self.ctx.grad2(q, rdx, rdy, periodic_x)
        tdims, g = self._in_dim_order(g, tracer, lead, lshape)
        name = lb.unwrap(tracer, lazy=True)[3]
        return lb.wrap(g, tdims, coords, 'grdS' + (name or ''), tracer)

    def _map_vector(self, who, what, v, nslab, lead, lshape):
        """levels or a per-contour vector of map_to_plane, through `_contour_values` like the levels of every contour call -> float64
        (N,) when every slab shares it, else (nslab, N).  Leading dims are those of the tracer, or none"""
        if lb.is_labeled(v):
            raw, dims, _, _ = lb.unwrap(v, lazy=True)
            if 'contour' not in dims:
                raise Exception('%s: %s should have a "contour" dim' % (who, what))
            shared = True
            for d, n in zip(dims, raw.shape):
                if d == 'contour' or n == 1:
                    continue
                shared = False
                if d not in lead or lshape[list(lead).index(d)] != n:
                    raise Exception('%s: the leading dims of %s do not match the tracer\'s %r' % (who, what, dict(zip(lead, lshape))))
        else:
            v, shared = np.asarray(v), True
            if v.ndim != 1:
                raise Exception('%s: %s should be a labelled array with a "contour" dim or a 1-D array' % (who, what))
        b = self._contour_values(v, nslab, list(lead), list(lshape))
        return np.ascontiguousarray(b[0] if shared else b, dtype=np.float64)

    def map_to_plane(self, contour, vs, tracer=None, dtype=np.float64):
        """
        Per-contour quantities back on the plane (K25, xc_contour_map): every node gets var(contour) evaluated at its own
        tracer value -- the equivalent latitude of every node, nkeff painted onto the plane.  This is the inverse of
        interp_to_coords (reference core.py:1050-1100): the same _interp1d (core.py:1405-1434) with x = the tracer of the
        node, xf = the contour levels, yf = the variable; the direction comes from levels[0] < levels[-1] per slab, nodes
        outside the levels get the end values, a NaN node stays NaN.  Build-defined: the reference has no counterpart.

        `contour`: what cal_contours returns (levels per leading index), or a 1-D array of levels for all slabs; at least
        two levels, strictly monotonic.  `vs`: a labelled array with a 'contour' dim, or a Dataset / dict of up to eight of
        them (the result of keff(), or a part of it); leading dims are those of the tracer, or none.  One pass over the
        tracer serves all of them.  Returns a plane with the tracer's dims and coords in `dtype` (float64, or float32:
        rounded once), or a Dataset of planes under the names of `vs`.
        """
        who = 'map_to_plane'
        data = self.tracer if tracer is None else tracer
        q, lead, lshape, coords = self._float_plane(data)
        nslab = q.shape[0]
        if np.dtype(dtype) not in _F48:
            raise Exception('%s: dtype should be float32 or float64' % who)
        levels = self._map_vector(who, 'contour', contour, nslab, lead, lshape)
        single = lb.is_labeled(vs)
        if single:
            items = [(lb.unwrap(vs, lazy=True)[3], vs)]
        elif isinstance(vs, dict):
            items = list(vs.items())
        elif hasattr(vs, 'data_vars'):
            items = [(k, vs[k]) for k in vs.data_vars]
        else:
            raise Exception('%s: vs should be a labelled array with a "contour" dim, or a Dataset / dict of them' % who)
        if not 1 <= len(items) <= nat.XC_CMAP_MAXV:
            raise Exception('%s: one to %d variables per call, not %d' % (who, nat.XC_CMAP_MAXV, len(items)))
        vals = [self._map_vector(who, 'variable %r' % (k,), v, nslab, lead, lshape) for k, v in items]
        for (k, _), v in zip(items, vals):
            if v.shape[-1] != levels.shape[-1]:
                raise Exception('%s: variable %r has %d values along "contour", the contours %d' % (who, k, v.shape[-1], levels.shape[-1]))
        try:
            planes = self.ctx.contour_map(q, levels, vals, out_dtype=dtype)
        except nat.XContourHipError as e:
            if e.code == nat.XC_EEDGES:
                raise Exception('non monotonic bins')                      # the reference's text (core.py:1233-1251)
            raise
        out = []
        for (k, _), g in zip(items, planes):
            tdims, g = self._in_dim_order(g, data, lead, lshape)
            out.append(lb.wrap(g, tdims, coords, k, data))
        return out[0] if single else lb.merge(out, out[0])

    def cal_equivalent_coordinate_map(self, contour, table, tracer=None, displacement=False):
        """
        The equivalent coordinate of every node of the plane (the equivalent-latitude map), named '<eq dim>Eq': the chain
        cal_contours -> cal_integral_within_contours_hist -> table.lookup_coordinates -> map_to_plane in one call.  Like
        interp_to_coords this is the N-contour HISTOGRAM approximation: the area inside a contour is the histogram's, the
        coordinate between two contours is linear in the tracer, and it converges to the exact map as N grows (the exact one
        would come from the sort of cal_sorted_profile carrying cell indices; not provided).

        `contour`: an int N (N equally spaced levels per slab) or levels as cal_contours takes them, or its result.
        `table`: the A(Yeq) table.  displacement=True: also returns the row coordinate of every node minus the map (Y - Yeq,
        the geometry behind local wave activity), named '<eq dim>Disp'; one host subtraction.
        """
        data = self.tracer if tracer is None else tracer
        ctr = contour if lb.is_labeled(contour) else self._contours_of(data, contour)
        area = self.cal_integral_within_contours_hist(ctr, tracer=data)
        eq = table.lookup_coordinates(area).rename(self.dimEqV + 'Eq')
        m = self.map_to_plane(ctr, eq, tracer=data)
        if not displacement:
            return m
        v, dims, coords, _ = lb.unwrap(m)
        y = np.asarray(self._eq_coord(data), dtype=np.float64)
        shp = [len(y) if d == self.dimEqV else 1 for d in dims]
        return m, lb.wrap(y.reshape(shp) - v, dims, coords, self.dimEqV + 'Disp', data)

    def cal_sorted_profile(self, table, tracer=None, mask=None, return_sorted=False):
        """
        EXACT adiabatically sorted reference state Q(Yeq) (the reference only has the
        N-contour histogram approximation `interp_to_coords(..., ctr)`, core.py:1050-1100, which
        converges to this as N grows).  The valid cells of the slab are radix-sorted on the GPU
        together with their areas; Q at equivalent coordinate y_j is the sorted value at the
        cumulative area the table assigns to y_j (a tracer decreasing with the coordinate value is
        handled by sorting -q).
        Returns Q on the table's coordinate (and the sorted values if `return_sorted`).
        """
        if tracer is None:
            tracer = self.tracer
        q, lead, lshape, coords = self._plane(tracer)
        q = self._float(q)
        nslab, ny, nx = q.shape
        dA, _ = self._dA_array(ny, nx, nslab)
        m = None if mask is None else self._float(self._plane(mask)[0])
        if m is not None and m.shape[0] not in (1, nslab):
            raise Exception('mask leading dims do not match the tracer')
        tv = np.asarray(lb.unwrap(table._table)[0], dtype=np.float64)
        if tv.ndim != 1:
            raise Exception('cal_sorted_profile needs a time-invariant table')
        # cumulative area on the small-coordinate side of y_j, whatever (increase, lt) built the table
        below = tv if table._incVl == table._incCd else tv[0] + tv[-1] - tv
        cs = table._coord
        if not table._incCd:                                   # ascending coordinate order for the lookup
            below, cs = below[::-1], cs[::-1]
        # `increase` refers to the INDEX of the equivalent dim (core.py:44-46): the sorted tracer
        # grows with the coordinate VALUE iff increase == (coordinate grows with index)
        eq = self._eq_coord(tracer)
        up = bool(self.increase) == bool(eq[-1] > eq[0])
        sgn = 1.0 if up else -1.0
        # the whole stack in ONE set of launches (segmented sort), in batches that keep the workspace
        # (4 x 8 B per cell + outputs) below ~2 GiB
        per = max(1, int((2 << 30) // (ny * nx * 8 * (6 if return_sorted else 5))))
        Qs, sorted_ = [], []
        for k0 in range(0, nslab, per):
            sl = slice(k0, min(nslab, k0 + per))
            mk = None if m is None else (m[sl] if m.shape[0] == nslab and nslab > 1 else m[0])
            res = self.ctx.sort_profile(q[sl], dA=dA[sl] if dA.ndim == 3 else dA, mask=mk,
                                        targets=below, want_sorted=return_sorted, negate=not up)
            Qs.append(sgn * res['Q'])
            if return_sorted:
                sorted_ += [sgn * res['q_sorted'][i][:int(res['nvalid'][i])] for i in range(sl.stop - sl.start)]
        Qs = [np.concatenate(Qs, axis=0)]
        c = {d: coords[d] for d in lead if d in coords}
        c[self.dimEqV] = cs
        Q = lb.wrap(Qs[0].reshape(tuple(lshape) + (len(cs),)), tuple(lead) + (self.dimEqV,), c,
                    lb.unwrap(tracer, lazy=True)[3], tracer)
        if return_sorted:
            return Q, (sorted_[0] if nslab == 1 and not lead else sorted_)
        return Q

    def _keff_key(self, batch, nbuf, N, q, g, dA, periodic_x, nkeff_mask, tbl, tbl_coord, preY, rdx, rdy):
        """The plan owns the device copies of everything static (dA, metrics, table, preY) and the work buffers:
        it is kept between calls, so a second keff() on the same grid only uploads the tracer.  Key = the
        configuration + the bytes of the small arrays + a fingerprint of dA (shape, ends and a strided sample:
        dA is the grid metric, not something callers edit in place between calls)."""
        def small(a):
            return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()
        flat = dA.reshape(-1)
        slab_dA = dA.ndim == 3
        # a per-slab dA travels with every batch (like the tracer): only its shape enters the key
        dkey = ('slab',) if slab_dA else (flat[::max(1, flat.size // 512)].tobytes(), float(flat[0]), float(flat[-1]))       # (hashing a 32 KB sample was 20 us per call)
        return (batch, nbuf) + q.shape[1:] + (int(N), q.dtype.str, np.dtype(self.dtype).str, None if g is None else g.dtype.str,
                bool(periodic_x), float(nkeff_mask), bool(self.increase), bool(self.lt), self.right_edge, self.device, self.deterministic,
                dA.shape[-2:] if slab_dA else dA.shape, dkey,
                small(tbl), small(tbl_coord), small(preY), small(rdx), small(rdy))

    def _keff_keep(self, key, plan):
        """`_keff_plans`: key -> the plan keff() took out for this call, back in as the most recently used (last) of at most two"""
        plans = self.__dict__['_keff_plans']
        plans[key] = plan
        while len(plans) > 2:
            plans.pop(next(iter(plans))).free()

    def keff(self, N, table, grdS=None, preY=None, lat=None, lon=None, rdx=None, rdy=None,
             periodic_x=True, nkeff_mask=1e5, max_batch_bytes=8 << 30):
        """
        Fused Keff pipeline for every leading index at once:
        three kernel launches, no host round trip.  Returns a Dataset of
        ctr, area, intgrdS, latEq, dqdA, dintSdA, Leq2, Lmin, nkeff on 'contour'
        (+ '<name>_eq' on `preY` if given).  Stacks whose tracer (+ grdS) exceeds `max_batch_bytes`
        go through the device in equal batches of whole slabs.
        """
        from .pipeline import KeffPlan, OUT_NAMES
        q, lead, lshape, coords = self._plane(self.tracer)
        q = self._float(q)
        nslab, ny, nx = q.shape
        dA, dA_f32 = self._dA_array(ny, nx, nslab)
        slab_dA = dA.ndim == 3                              # weights with a leading (time, ...) dim, core.py:1271-1274
        tv, tdims, tcoords, _ = lb.unwrap(table._table)
        if tv.ndim != 1:
            raise Exception('keff() needs a time-invariant A(Yeq) table')
        if len(tv) != ny:
            raise Exception('the A(Yeq) table has %d entries but the tracer has %d rows along %s' % (len(tv), ny, self.dimEqV))
        g = None
        # resident objects: the same argument OBJECTS as in the last call -> the same plan key (see __init__), nothing re-derived from bytes
        idents = (table, grdS, preY, lat, lon, rdx, rdy, self.tracer, self.dA, N, periodic_x, nkeff_mask, max_batch_bytes, nslab,
                  self.increase, self.lt, self.right_edge, self.device, self.deterministic, np.dtype(self.dtype).str) if self.resident else None
        last = self.__dict__.get('_keff_last') if self.resident else None
        fast = last is not None and len(last[0]) == len(idents) and all(a is b or (type(a) in (int, float, bool, str) and type(a) is type(b) and a == b) for a, b in zip(last[0], idents))
        plans = self.__dict__.setdefault('_keff_plans', {})
        key = last[1] if fast and last[1] in plans else None
        if grdS is not None:
            g = self._integrand_plane(grdS)
        elif rdx is None and key is None:                    # (a plan that is still there holds the metrics on the device; an evicted one is rebuilt from them)
            la = np.ascontiguousarray(lat if lat is not None else coords[self.dimEqV])
            lo = np.ascontiguousarray(lon if lon is not None else coords[self._xdim])
            mk = (la.tobytes(), lo.tobytes(), la.dtype.str, lo.dtype.str)
            memo = self.__dict__.get('_metrics_memo')
            if memo is None or memo[0] != mk:                    # the metrics of a grid are computed once per object and grid
                memo = self.__dict__['_metrics_memo'] = (mk, grad_metrics(la, lo))
            rdx, rdy = memo[1]
        per_slab = ny * nx * (q.dtype.itemsize + (0 if g is None else g.dtype.itemsize) + (8 if slab_dA else 0))
        batch = int(min(nslab, max(1, int(max_batch_bytes) // per_slab), 65535))
        # more than one batch: the device holds TWO (half the budget each), the upload of batch k + 1 runs on the copy
        # stream while batch k computes
        nbuf = 1
        if batch < nslab:
            nbuf = 2
            batch = int(min(nslab, max(1, int(max_batch_bytes) // (2 * per_slab)), 65535))
        if key is None:
            key = self._keff_key(batch, nbuf, N, q, g, dA, periodic_x, nkeff_mask, tv, tcoords[table._dimEq], preY, rdx, rdy)
        if self.resident:
            self.__dict__['_keff_last'] = (idents, key)
        plan = plans.pop(key, None)
        if plan is None:
            plan = KeffPlan(self.ctx, nbuf * batch, ny, nx, N, q.dtype, self.dtype, dA=dA[:min(nslab, nbuf * batch)] if slab_dA else dA,
                            rdx=rdx, rdy=rdy,
                            periodic_x=periodic_x, tbl=tv, tbl_coord=tcoords[table._dimEq], preY=preY,
                            increase=self.increase, lt=self.lt, right_edge=self.right_edge,
                            nkeff_mask=nkeff_mask, grdS_dtype=None if g is None else g.dtype,
                            prod_f32=bool(g is not None and g.dtype == np.float32 and dA_f32),
                            detect_row_dA=not slab_dA, deterministic=self.deterministic, out_slabs=batch, nslots=nbuf,
                            counts=False)                      # (Keff never looks at the cell counts: a third of K3's LDS atomics saved)
        if slab_dA:
            plan.desc.dA_pos_finite = int(bool(np.isfinite(dA).all() and (dA >= 0).all()))
            fin = np.abs(dA[np.isfinite(dA)])
            plan.desc.dA_max = float(fin.max()) if fin.size else 0.0      # over EVERY slab: a valid bound for each batch uploaded below
        try:
            res = plan.run_stack(q, batch, nbuf, g=g, dA=dA if slab_dA else None, mirrors=self.resident)
        except Exception:
            plan.free()
            raise
        self._keff_keep(key, plan)
        ccoord = np.arange(N, dtype=np.float64).astype(self.dtype)      # = np.linspace(0.0, N - 1.0, N, dtype): its step is exactly 1
        out = []
        shared = {d: np.asarray(coords[d]) for d in lead if d in coords}
        shared['contour'] = ccoord
        for name in OUT_NAMES:
            out.append(self._wrap_contour(res[name], lead, lshape, coords, name, self.tracer, ccoord, shared=shared))
        if preY is not None:
            c = {d: coords[d] for d in lead if d in coords}
            c['new'] = np.asarray(preY)
            for name in OUT_NAMES:
                v = res[name + '_eq'].reshape(tuple(lshape) + (len(preY),))
                out.append(lb.wrap(v, tuple(lead) + ('new',), c, name + '_eq', self.tracer))
        return lb.merge(out, out[0])


class Table(object):
    """
    One-to-one mapping table between two monotonic quantities, y = F(x) with y the
    values and x the coordinates (reference core.py:1103-1195).
    """

    def __init__(self, table, dimEq):
        v, dims, coords, _ = lb.unwrap(table)
        ax = dims.index(dimEq)
        if v.ndim == 1:
            areaInc = bool(v[-1] > v[0])
        else:
            tmp = np.take(v, -1, axis=ax) > np.take(v, 0, axis=ax)
            if (tmp == True).all():              # noqa: E712  (mirrors core.py:1123-1128)
                areaInc = True
            elif (tmp == False).all():           # noqa: E712
                areaInc = False
            else:
                raise Exception('not every time or level is increasing/decreasing')
        self._table = table
        self._coord = np.asarray(coords[dimEq])
        self._dimEq = dimEq
        self._incVl = areaInc
        self._incCd = bool(self._coord[-1] > self._coord[0])

    def lookup_coordinates(self, values):
        """For y = F(x), get coordinates (x) given values (y) (reference core.py:1136-1174)."""
        tv, tdims, _, _ = lb.unwrap(self._table)
        if lb.is_labeled(values):
            v, dims, coords, name = lb.unwrap(values)
        else:
            v, dims, coords, name = np.asarray(values), None, {}, None
        tv = np.moveaxis(tv, tdims.index(self._dimEq), -1)
        if tv.ndim > 1 and dims is not None:
            tl = tuple(d for d in tdims if d != self._dimEq)
            vl = tuple(d for d in dims if d != 'contour')
            tv = np.broadcast_to(_align(tv, tl + (self._dimEq,), vl + (self._dimEq,)),
                                 tuple(v.shape[dims.index(d)] for d in vl) + (tv.shape[-1],))
        out = np.empty(v.shape, dtype=tv.dtype)
        if dims is not None and 'contour' in dims and v.ndim > 1 and tv.ndim == 1:
            # ONE table for every slab (the usual case: the mask does not depend on time / level): np.interp is elementwise, so the
            # whole stack goes through one call instead of one per slab (15 slabs: 43 -> ~8 us; the result is the same numbers)
            out = np.asarray(_interp1d(v, tv, self._coord, self._incVl)).astype(tv.dtype, copy=False)
        elif dims is not None and 'contour' in dims and v.ndim > 1:
            vv = np.moveaxis(v, dims.index('contour'), -1)
            oo = np.empty(vv.shape, dtype=tv.dtype)
            for idx in np.ndindex(*vv.shape[:-1]):
                t = tv[idx] if tv.ndim > 1 else tv
                oo[idx] = _interp1d(vv[idx], t, self._coord, self._incVl)
            out = np.moveaxis(oo, -1, dims.index('contour'))
        else:
            if tv.ndim > 1:
                raise Exception('table with leading dims needs labelled values')
            out = np.asarray(_interp1d(v, tv, self._coord, self._incVl)).astype(tv.dtype)
        if dims is None:
            return out
        return lb.wrap(out, dims, coords, name, values)

    def lookup_values(self, coords):
        """For y = F(x), get values (y) given coordinates (x) (reference core.py:1176-1195;
        the snapshot references an undefined attribute there, SURVEY F5 -- restated as intended)."""
        tv = lb.unwrap(self._table)[0]
        if tv.ndim != 1:
            raise Exception('lookup_values needs a 1D table')
        cv = np.asarray(lb.unwrap(coords)[0] if lb.is_labeled(coords) else coords)
        re = _interp1d(cv, self._coord, tv, self._incCd)
        if lb.is_labeled(coords):
            _, d, c, n = lb.unwrap(coords)
            return lb.wrap(re, d, c, n, coords)
        return re


"""
Below are the private helper methods
"""


def _edges_from_levels(b, right_edge):
    """Ascending histogram edges from per-slab levels `b` (nslab, N) in the levels' own
    dtype (reference core.py:1296-1305) + the last-bin rule.  Raises like the reference
    when two adjacent levels coincide (core.py:1233-1251)."""
    b = np.asarray(b)
    if b.ndim == 2 and b.dtype in _F48 and b.flags.c_contiguous and b.shape[0] >= 1 and b.shape[1] >= 1 and right_edge in _EDGE_CODES:
        # the same rule in one host call of the library (xc_host_edges_from_levels: the reference's checks and texts included)
        edges = np.empty((b.shape[0], b.shape[1] + 1), dtype=np.float64)
        inc = C.c_int(0)
        lib = nat.load()
        if lib.xc_host_edges_from_levels(b.ctypes.data, b.dtype.itemsize == 8, b.shape[0], b.shape[1], _EDGE_CODES[right_edge],
                                         edges.ctypes.data, inc) != 0:
            raise Exception((lib.xc_last_error(None) or b'').decode())
        return edges, bool(inc.value), right_edge != 'xhistogram'
    if (b[:, 1:] == b[:, :-1]).any():
        raise Exception('non monotonic bins')
    n1 = b.shape[1] - 1
    if n1 < 1:
        raise Exception('need at least two contour levels')
    with np.errstate(invalid='ignore'):
        # every slab at once (a Python loop with np.insert per slab was 110 us of a 160 us call at the reference's demo size); the
        # arithmetic stays in the levels' own dtype, as np.insert's cast of the new edge does (core.py:1300-1304)
        first, last = b[:, 0], b[:, -1]
        binc = bool(first[0] < last[0])
        other = (first < last) != binc
        if other.any() and not np.isnan(b[other]).any(axis=1).all():
            raise Exception('not every time or level is increasing/decreasing')
        edges = np.empty((b.shape[0], b.shape[1] + 1), dtype=b.dtype)
        if binc:
            edges[:, 1:] = b
            edges[:, 0] = first - (last - first) / n1
        else:
            edges[:, 1:] = b[:, ::-1]
            edges[:, 0] = last - (first - last) / n1
    last_closed = True
    if right_edge == 'xhistogram':
        edges[:, -1] += 1e-8                                           # in the levels' own dtype, like `edge + 1e-8` on the array
        last_closed = False
    return edges.astype(np.float64), binc, last_closed


def contour_polylines(walk, poff, closed, rpo, pts, nx=None, ycoord=None, xcoord=None, period=None, packed=False):
    """
    The vertex rule of Contour2D.find_contours on the host (no device): the joined segments -> polylines, laps and winding
    numbers.  walk (total,) int64: segment indices polyline by polyline in walk order; poff (npoly + 1,) into `walk`; closed
    (npoly,) bool; rpo (nrange + 1,): the polylines of range r are [rpo[r], rpo[r+1]) -- what _native.join_segments returns --;
    pts (total, 4) float64 (r1, c1, r2, c2) in index space, as Context.contour_segments returns them.  nx: None, or the number
    of columns of a plane traced with a periodic X direction (columns in [0, nx], the seam cell's right edge at nx).  ycoord /
    xcoord: None (index space) or the plane's coordinates in float64; period: the X period, with xcoord and nx.

    Vertices: the start of the first segment and the end of every segment, consecutive equal vertices merged, polylines left
    with fewer than two vertices dropped.  With nx, a segment's lap m counts the passes through the seam before it in walk
    order: between one segment's end column and the next one's start column the jump is 0, +nx (m + 1: from the seam cell's
    right edge, column nx, into column 0) or -nx (m - 1); its columns are c + nx m in index space and
    np.interp(c, arange(nx + 1), [xcoord..., xcoord[0] + period]) + m period in coordinates.  The winding number of a ring is
    m_last + (c_end[last] - c_start[first]) / nx, an integer; of an open polyline, 0.
    Returns (polys, closed, winding): per range a list of (n, 2) float64 arrays [row, column], of bools and of ints.
    packed=True: the same polylines in ONE array, built with array operations only (no Python loop over polylines): returns
    (verts (M, 2) float64, vert_off (nkept + 1,) int64, closed (nkept,) bool, winding (nkept,) int64, range_off (nrange + 1,)
    int64): kept polyline p has the vertices verts[vert_off[p]:vert_off[p+1]], and those of range r are
    [range_off[r], range_off[r+1]) -- polys[r][k] is polyline range_off[r] + k.
    """
    walk, poff, rpo = np.asarray(walk, dtype=np.int64), np.asarray(poff, dtype=np.int64), np.asarray(rpo, dtype=np.int64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    r1, c1, r2, c2 = (pts[walk, i] for i in range(4))                      # in walk order
    ring = nx is not None
    npoly = poff.size - 1
    wind = np.zeros(npoly, dtype=np.int64)
    if ring:
        nx = int(nx)
        heads = poff[:-1]
        jump = np.zeros(walk.size, dtype=np.float64)
        jump[1:] = c2[:-1] - c1[1:]
        jump[heads] = 0.0
        step = (jump == float(nx)).astype(np.int64) - (jump == -float(nx)).astype(np.int64)
        if ((jump != 0.0) & (step == 0)).any():
            raise Exception('contour_polylines: consecutive segments that are neither adjacent nor one ring apart')
        run = np.cumsum(step)
        m = run - np.repeat(run[heads], np.diff(poff))                      # segmented cumulative sum: 0 at every head
        if npoly:
            last = poff[1:] - 1
            w = m[last] + ((c2[last] - c1[heads]) / float(nx)).astype(np.int64)
            wind = np.where(np.asarray(closed, dtype=bool), w, 0)
    if ycoord is not None:
        ycoord, xcoord = np.asarray(ycoord, dtype=np.float64), np.asarray(xcoord, dtype=np.float64)
        yi = np.arange(ycoord.size)
        xi, xe = (np.arange(nx + 1), np.concatenate([xcoord, [xcoord[0] + period]])) if ring else (np.arange(xcoord.size), xcoord)
        if walk.size:
            r1, r2 = np.interp(r1, yi, ycoord), np.interp(r2, yi, ycoord)
            c1, c2 = np.interp(c1, xi, xe), np.interp(c2, xi, xe)
        if ring:
            c1, c2 = c1 + m * float(period), c2 + m * float(period)
    elif ring:
        c1, c2 = c1 + (nx * m).astype(np.float64), c2 + (nx * m).astype(np.float64)
    S, E = np.stack([r1, c1], axis=1), np.stack([r2, c2], axis=1)
    if packed:
        return _packed_polylines(S, E, poff, np.asarray(closed, dtype=bool), wind, rpo)
    polys, cl, wd = [], [], []
    for r in range(rpo.size - 1):
        ps, cs, ws = [], [], []
        for p in range(int(rpo[r]), int(rpo[r + 1])):
            a, b = int(poff[p]), int(poff[p + 1])
            v = np.concatenate([S[a:a + 1], E[a:b]])
            keep = np.concatenate([[True], (v[1:] != v[:-1]).any(axis=1)])
            if int(keep.sum()) < 2:
                continue
            ps.append(np.ascontiguousarray(v[keep]))
            cs.append(bool(closed[p]))
            ws.append(int(wind[p]))
        polys.append(ps); cl.append(cs); wd.append(ws)
    return polys, cl, wd


def _check_device_join(ny, nx):
    """trace_contours(join='device'): K14 numbers the grid edges of a plane in 32 bits"""
    if 2 * int(ny) * int(nx) >= 1 << 31:
        raise Exception('trace_contours: join=\'device\' numbers the grid edges in 32 bits and a (%d, %d) plane has 2 ny nx '
                        '>= 2^31 of them: use join=\'host\'' % (ny, nx))


def _packed_polylines(S, E, poff, closed, wind, rpo):
    """the vertex rule of contour_polylines for all polylines at once.  S, E (total, 2): start and end of every segment in walk
    order.  Polyline p (segments [a, b)) has the candidate vertices S[a], E[a], ..., E[b-1]: they stand at [a + p, b + p + 1) of
    one candidate array; a candidate stays when it heads its polyline or differs from the candidate before it; a polyline
    stays when two or more of its candidates do."""
    total, npoly = S.shape[0], poff.size - 1
    if npoly == 0:
        return (np.empty((0, 2), dtype=np.float64), np.zeros(1, dtype=np.int64), np.empty(0, dtype=bool),
                np.empty(0, dtype=np.int64), np.zeros(rpo.size, dtype=np.int64))
    nseg = np.diff(poff)
    heads = poff[:-1] + np.arange(npoly, dtype=np.int64)                    # where each polyline's first candidate stands
    V = np.empty((total + npoly, 2), dtype=np.float64)
    V[heads] = S[poff[:-1]]
    V[np.arange(total, dtype=np.int64) + np.repeat(np.arange(1, npoly + 1, dtype=np.int64), nseg)] = E
    keep = np.ones(total + npoly, dtype=bool)
    keep[1:] = (V[1:] != V[:-1]).any(axis=1)
    keep[heads] = True
    nvert = np.add.reduceat(keep.astype(np.int64), heads)
    stays = nvert >= 2
    keep &= np.repeat(stays, nseg + 1)
    vert_off = np.concatenate([[0], np.cumsum(nvert[stays])]).astype(np.int64)
    range_off = np.concatenate([[0], np.cumsum(stays)]).astype(np.int64)[rpo]
    return np.ascontiguousarray(V[keep]), vert_off, closed[stays], np.asarray(wind, dtype=np.int64)[stays], range_off


def find_contour(data, dims, level, period=[None, None], periodic=False):
    """
    The polylines of ONE level of a 2-D labelled field, in the call shape of the reference's scripts
    (tests/test_clength.py:615: find_contour(tr1[0], ['YC', 'XC'], 1.15076609, period=[None, None])): `dims` = [ydim, xdim].
    Returns a list of (n, 2) float64 arrays [y, x] in the field's coordinates -- Contour2D.find_contours([level])[0], which
    states the rule.  Periodic tracing is not supported yet: an entry of `period` that is not None raises.
    A periodic X direction goes through the keyword `periodic` instead -- False, True (360) or the period in xdim's units --,
    handed to Contour2D.find_contours(periodic=...), which states what it means: the seam cell is traced, polylines run on
    past the seam, and a contour that circles the globe is one ring.
    `trace_contour` is this function with the join on the GPU on request.
    """
    return trace_contour(data, dims, level, period=period, periodic=periodic)


def trace_contour(data, dims, level, period=[None, None], periodic=False, join='host'):
    """find_contour with `join` passed through to Contour2D.trace_contours: 'host' (find_contour itself) or 'device' (the join on
    the GPU, K14); the same polylines bit for bit."""
    if period is not None and any(p is not None for p in period):
        # (a periodic X direction: the keyword `periodic` of this function, not `period`)
        raise NotImplementedError('find_contour: period=%r is not supported yet (only [None, None]: no wrap across the plane\'s '
                                  'edges)' % (period,))
    ydim, xdim = dims
    ddims = lb.unwrap(data, lazy=True)[1]
    if len(ddims) != 2 or set(ddims) != {ydim, xdim}:
        raise Exception('find_contour expects a 2-D field on the dims %s' % [ydim, xdim])
    cm = Contour2D(data, 1.0, {'X': xdim, 'Y': ydim}, {'Y': ydim}, dtype=np.float64)
    return cm.trace_contours(np.array([float(level)]), periodic=periodic, join=join)[0]


def distance_to_contour(data, dims, level, period=[None, None], periodic=False, latlon=False):
    """
    The distance from every node of a 2-D labelled field to ONE of its levels, beside `find_contour` and in its call shape:
    `dims` = [ydim, xdim], `period` must be [None, None], a periodic X direction goes through `periodic`.  Returns the labelled
    (ydim, xdim) array Contour2D.cal_distance_to_contours([level], latlon=latlon, periodic=periodic) gives for that level, which
    states the rule (coordinate units; metres with latlon=True; NaN when nothing is at that level).
    """
    if period is not None and any(p is not None for p in period):
        raise NotImplementedError('distance_to_contour: period=%r is not supported (only [None, None]: use `periodic`)' % (period,))
    ydim, xdim = dims
    ddims = lb.unwrap(data, lazy=True)[1]
    if len(ddims) != 2 or set(ddims) != {ydim, xdim}:
        raise Exception('distance_to_contour expects a 2-D field on the dims %s' % [ydim, xdim])
    cm = Contour2D(data, 1.0, {'X': xdim, 'Y': ydim}, {'Y': ydim}, dtype=np.float64)
    return cm.cal_distance_to_contours(np.array([float(level)]), latlon=latlon, periodic=periodic).isel({'contour': 0})


def distance_profile(data, dims, level, bins, fields=None, dA=1.0, period=[None, None], periodic=False, latlon=False, signed=False,
                     side='upper', max_distance=None):
    """
    Composites by distance from ONE level of a 2-D labelled field, beside `distance_to_contour` and in its call shape: `dims` =
    [ydim, xdim], `period` must be [None, None], a periodic X direction goes through `periodic`.  `bins`, `fields`, `signed`, `side`
    and `max_distance` as in Contour2D.cal_contour_distance_profile, which states the bin rule; `dA`: the weight, a labelled array
    on the plane or a number (1.0: `area` counts nodes).  Returns that method's Dataset for the level, over (distance_bin,).
    """
    if period is not None and any(p is not None for p in period):
        raise NotImplementedError('distance_profile: period=%r is not supported (only [None, None]: use `periodic`)' % (period,))
    ydim, xdim = dims
    ddims = lb.unwrap(data, lazy=True)[1]
    if len(ddims) != 2 or set(ddims) != {ydim, xdim}:
        raise Exception('distance_profile expects a 2-D field on the dims %s' % [ydim, xdim])
    if np.ndim(dA) == 0:                                             # a number: the same weight on every row
        dA = np.full(lb.unwrap(data, lazy=True)[0].shape[ddims.index(ydim)], float(dA))
    cm = Contour2D(data, dA, {'X': xdim, 'Y': ydim}, {'Y': ydim}, dtype=np.float64)
    ds = cm.cal_contour_distance_profile(np.array([float(level)]), bins, fields=fields, latlon=latlon, periodic=periodic, signed=signed,
                                         side=side, max_distance=max_distance)
    return lb.merge([v.isel({'contour': 0}) for v in ds.values()], data)


def coarsen(data, dims, ratio, skipna=False):
    """The block-averaged field of `Contour2D.coarsen` (K26) for a labelled array that has no Contour2D yet: `dims` = (row dim,
    column dim) of the plane, any further dims lead.  Returns the coarse labelled array with block-mean coordinates."""
    ydim, xdim = dims
    return Contour2D(data, 1.0, {'X': xdim, 'Y': ydim}, {'Y': ydim}, dtype=np.float64).coarsen(ratio, skipna=skipna)


def _block_means(c, r):
    """float64 means of the blocks [I r, I r + r) of a 1-D coordinate, summed in order from each block's first value (K26's rule
    for coordinates); the values that fill no block are dropped"""
    b = np.asarray(c, dtype=np.float64)
    b = b[:b.size // r * r].reshape(-1, r)
    s = b[:, 0].copy()
    for k in range(1, r):
        s = s + b[:, k]
    return s / float(r)


def _level_order(vals, order):
    """results per SORTED level (`Contour2D._sorted_levels`) -> in the order the levels were given"""
    out = np.empty_like(vals)
    np.put_along_axis(out, order, vals, axis=1)
    return out


def _align(v, vdims, dims):
    """Reshape/transposes `v` (with dims `vdims`, a subset of `dims`) for broadcasting
    against an array with dims `dims`."""
    if vdims is None or tuple(vdims) == tuple(dims):
        return v
    present = [d for d in dims if d in vdims]
    if len(present) != len(vdims):
        raise Exception('dims %r are not a subset of %r' % (vdims, dims))
    v = np.transpose(v, [list(vdims).index(d) for d in present])
    shape = [v.shape[present.index(d)] if d in present else 1 for d in dims]
    return v.reshape(shape)


def _check_monotonicity(var, dim):
    """Raise if `var` has a zero step along `dim` (reference core.py:1328-1355)."""
    v, dims, _, _ = lb.unwrap(var)
    dfvar = np.diff(v, axis=dims.index(dim))
    if not dfvar.all():
        pos = np.argwhere(dfvar == 0)[0]
        raise Exception('not monotonic var at\n' + str(dict(zip(dims, pos))))


def _gradient_edge1(f, x, axis):
    """np.gradient(f, x, axis=axis, edge_order=1) -- bit for bit -- for the case every caller here has: a floating `f` and a 1-D
    coordinate `x` with CONSTANT spacing (the contour index 0 .. N-1).  numpy then takes its uniform branch: interior
    (f[2:] - f[:-2]) / (2. * dx), ends (f[1] - f[0]) / dx and (f[-1] - f[-2]) / dx with dx = np.diff(x)[0] (a scalar of x's dtype);
    what np.gradient spends 15 us per call on at these sizes is dispatching, not arithmetic.  Anything else goes to np.gradient."""
    f = np.asanyarray(f); x = np.asanyarray(x)
    n = f.shape[axis]
    if (type(f) is not np.ndarray or f.dtype.kind != 'f' or x.ndim != 1 or x.dtype.kind != 'f' or n < 2 or x.shape[0] != n
            or f.dtype.itemsize < 4 or x.dtype.itemsize < 4):
        return np.gradient(f, x, axis=axis, edge_order=1)
    d = np.diff(x)
    if not (d == d[0]).all():
        return np.gradient(f, x, axis=axis, edge_order=1)
    dx = d[0]                                                    # numpy: `diffx = diffx[0]` -- an x.dtype scalar
    fm = np.moveaxis(f, axis, 0)
    out = np.empty_like(f)                                       # numpy: the output has f's dtype; the quotients are cast into it
    om = np.moveaxis(out, axis, 0)
    om[1:-1] = (fm[2:] - fm[:-2]) / (2. * dx)
    om[0] = (fm[1] - fm[0]) / dx
    om[-1] = (fm[-1] - fm[-2]) / dx
    return out


def _interp1d(x, xf, yf, inc=True):
    """np.interp taking into account the decreasing case (reference core.py:1405-1434)."""
    if inc:
        return np.interp(x, xf, yf)
    return np.interp(x, xf[::-1], yf[::-1])
