/*
 * xcontour_hip.h -- C ABI of libxcontour_hip.so: the MI355X (gfx950) implementation
 * of the contour-coordinate hot path of miniufo/xcontour.
 *
 * The reference (pure Python, /root/reference/xcontour/core.py) has no FFI seam of
 * its own; the seam this library fills is the pair of third-party calls that touch
 * every grid cell,
 *     xhistogram.xarray.histogram(var, bins=[edges], dim=dims, weights=w)   core.py:1284, 1307
 *     (var * dA).sum(dims)                                                  core.py:1376
 * plus the per-slab reductions and O(N) contour-space algebra around them.  Each
 * entry point below names the reference lines it replaces.  INTEGRATION.md shows
 * the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only: pointers, sizes, ints, doubles.  No C++ types cross.
 *   - every function returns an int status (XC_OK == 0, negative on error);
 *     xc_last_error(ctx) gives a message for the calling thread's last failure.
 *   - a "slab" is one (time, level) 2-D field of ny rows (the equivalent dim,
 *     lat/Z) by nx columns (lon/X), row-major with X fastest; slabs of a batch
 *     are contiguous: [nslab][ny][nx].
 *   - functions ending in _dev take DEVICE pointers and only enqueue work on the
 *     context's HIP stream (call xc_sync to wait); the same name without _dev
 *     takes HOST pointers (caller-owned, C-contiguous), stages them through a
 *     context-owned device arena and returns after the results are in the
 *     caller's buffers.
 *   - one context == one HIP device + one stream; calls on one context must be
 *     serialised by the caller; different contexts may be used concurrently.
 */
#ifndef XCONTOUR_HIP_H
#define XCONTOUR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xc_ctx xc_ctx;

/* status codes */
#define XC_OK        0
#define XC_EBADARG  (-1)   /* bad argument (null pointer, size, dtype, unsupported shape) */
#define XC_EEDGES   (-2)   /* bin edges not strictly ascending (reference: 'non monotonic bins', core.py:1233-1251) */
#define XC_EHIP     (-3)   /* HIP runtime error */
#define XC_ENOMEM   (-4)   /* device or host allocation failed */
#define XC_ENODEV   (-5)   /* no usable gfx950 device */

/* element types */
#define XC_F32 0
#define XC_F64 1

/* rank of the area-weight array dA (always passed as float64) */
#define XC_DA_NONE  0      /* weight 1 for every cell                       */
#define XC_DA_ROW   1      /* dA[ny]          one value per row             */
#define XC_DA_PLANE 2      /* dA[ny][nx]      shared by all slabs           */
#define XC_DA_SLAB  3      /* dA[nslab][ny][nx]                             */

/* last-bin rule (see oracle/xcontour_oracle.py header) */
#define XC_EDGE_NUMPY      0   /* last bin closed on the right (np.histogram)          */
#define XC_EDGE_XHISTOGRAM 1   /* last edge += 1e-8 in the edge dtype, bin half-open   */

#define XC_MAX_INTEGRANDS 2

/* X padding of xc_crossing: the `mode` of DataArray.pad / np.pad (core.py:674-676) */
#define XC_PAD_EDGE      0
#define XC_PAD_WRAP      1
#define XC_PAD_NAN       2     /* mode='constant' (xarray fills floats with NaN)      */
#define XC_PAD_REFLECT   3
#define XC_PAD_SYMMETRIC 4

/* ------------------------------------------------------------------ context */
int         xc_create(int device_id, xc_ctx** out);
int         xc_destroy(xc_ctx* ctx);
const char* xc_last_error(xc_ctx* ctx);          /* ctx may be NULL (creation errors) */
const char* xc_version(void);
int         xc_device_count(int* out_count);     /* visible HIP devices (a launcher maps local rank -> device with it) */
int         xc_device_name(xc_ctx* ctx, char* buf, size_t buflen);
int         xc_device_cus(xc_ctx* ctx, int* out_cus);
int         xc_sync(xc_ctx* ctx);
void*       xc_stream(xc_ctx* ctx);              /* the hipStream_t, for interop */
/* Where the host-form entry points of this context spent their time since the last reset, in seconds: out3[0] staging inputs
 * (memcpy into the pinned bounce buffer + enqueue, or the runtime's staged copy of a large block), out3[1] handing results over
 * (enqueue + memcpy out of the pinned buffer), out3[2] waiting for the stream.  Diagnostic (tools/facade_time.py --breakdown). */
int         xc_trace(xc_ctx* ctx, int reset, double* out3);

/* device memory + HIP-event timing on the context's stream */
int xc_malloc(xc_ctx* ctx, size_t bytes, void** out_dptr);
int xc_free(xc_ctx* ctx, void* dptr);
int xc_memcpy_h2d(xc_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int xc_memcpy_d2h(xc_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int xc_memset(xc_ctx* ctx, void* dptr, int value, size_t bytes);
/* Resident inputs (no reference call site: the reference keeps everything in host memory).  The reference's Keff sequence hands
 * the SAME tracer to cal_contours and twice to cal_integral_within_contours_hist, the same weights to every call; the host-form
 * entry points upload their inputs on every call (~1 ms per 52 MB cfg2 slab over PCIe).  xc_keep_resident uploads `bytes` at
 * `host_ptr` once into memory the library owns; from then on any host-form entry point whose input lies inside
 * [host_ptr, host_ptr + bytes) -- the array itself or whole slabs of it -- takes it from that mirror on the device instead
 * (xc_minmax / xc_hist read the mirror in place; the others, and xc_memcpy_h2d[_async] from such a source, copy device to device).
 * The caller must not modify (or free) the host array while it is registered; calling xc_keep_resident on the same pointer
 * again refreshes the mirror; xc_release_resident(ctx, host_ptr) drops one entry, xc_release_resident(ctx, NULL) all.
 * Python: Contour2D(..., resident=True). */
int xc_keep_resident(xc_ctx* ctx, const void* host_ptr, size_t bytes);
int xc_release_resident(xc_ctx* ctx, const void* host_ptr);
/* the device address of the mirror of [host_ptr, host_ptr + bytes), or NULL if those bytes are not inside a registered array: a
 * caller that drives the _dev entry points itself (the fused pipeline) points its descriptor at the mirror instead of copying it */
int xc_resident_lookup(xc_ctx* ctx, const void* host_ptr, size_t bytes, void** out_dev);

/* Uploads that overlap compute: xc_memcpy_h2d_async copies on the context's second (copy) stream and returns when the
 * host buffer may be reused (pageable memory: when the copy is done; kernels enqueued earlier on the compute stream run
 * meanwhile).  xc_stream_wait_copies makes everything enqueued on the compute stream AFTER the call wait for the copies
 * issued so far; xc_copies_wait_stream makes later copies wait for the compute work enqueued so far (before a buffer that
 * kernels still read is overwritten). */
int xc_memcpy_h2d_async(xc_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int xc_stream_wait_copies(xc_ctx* ctx);
int xc_copies_wait_stream(xc_ctx* ctx);
int xc_event_create(xc_ctx* ctx, void** out_event);
int xc_event_destroy(xc_ctx* ctx, void* event);
int xc_event_record(xc_ctx* ctx, void* event);
int xc_event_elapsed_ms(xc_ctx* ctx, void* start, void* stop, float* out_ms);  /* waits for `stop` */
int xc_event_record_copies(xc_ctx* ctx, void* event);   /* record on the COPY stream: done once the uploads issued so far have landed */
int xc_event_query(xc_ctx* ctx, void* event, int* out_done);   /* 1 when the event has completed, 0 while it has not; never blocks */

/* ------------------------------------------------------------------ K1  min / max
 * Replaces tracer.min(dim=dimVs), tracer.max(dim=dimVs)            core.py:224-225
 * NaN-skipping; an all-NaN slab gives NaN, NaN.  out_minmax: double[nslab][2].    */
int xc_minmax_dev(xc_ctx* ctx, const void* q, int q_dtype,
                  int64_t nslab, int64_t ncell, double* out_minmax);
int xc_minmax(xc_ctx* ctx, const void* q, int q_dtype,
              int64_t nslab, int64_t ncell, double* out_minmax);

/* ------------------------------------------------------------------ levels + edges
 * Replaces cal_contours(int levels)   core.py:222-249  (exact dtype rules: SURVEY 8-a2)
 * and the edge construction of _histogram  core.py:1296-1305.
 * minmax: double[nslab][2] as produced by xc_minmax.
 * ctr:    double[nslab][N]   levels rounded to ctr_dtype, in level order
 *         (ctr[0] == min if increase else max).
 * edges:  double[nslab][N+1] ascending histogram edges (dummy left edge first).
 * status: int32[nslab] 0 ok, 1 = two adjacent levels coincide (reference raises).    */
int xc_levels_dev(xc_ctx* ctx, const double* minmax, int q_dtype, int64_t nslab,
                  int N, int increase, int ctr_dtype, int right_edge,
                  double* ctr, double* edges, int32_t* status);
int xc_levels(xc_ctx* ctx, const double* minmax, int q_dtype, int64_t nslab,
              int N, int increase, int ctr_dtype, int right_edge,
              double* ctr, double* edges, int32_t* status);

/* cal_contours(int levels) (core.py:205-249) as ONE host-form call: xc_minmax + xc_levels without the round trip between them --
 * one upload of the tracer (or none: a resident one), one result hand-over, one synchronisation.  out_ctr double[nslab][N]; out_minmax
 * (double[nslab][2]), out_edges (double[nslab][N+1]) and out_status (int32[nslab]) may be NULL. */
int xc_contours(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ncell, int N, int increase, int ctr_dtype,
                int right_edge, double* out_minmax, double* out_ctr, double* out_edges, int32_t* out_status);

/* ------------------------------------------------------------------ K3+K5  weighted multi-channel histogram + CDF
 * Replaces histogram(var, bins=[edges], dim=dims, weights=w) + cumsum + lt flip
 *          core.py:1307-1323 (and the per-time loop 1259-1294: edges may differ per slab)
 *          and the weights of cal_integral_within_contours_hist   core.py:443-449.
 * One pass over the tracer accumulates nchan = 1 + nint + (grad ? 1 : 0) channels:
 *   channel 0            : dA                      (fillna(0))
 *   channel 1..nint      : integrand_i * dA        (fillna(0); product in f32 if prod_f32)
 *   last (if grad != 0)  : |grad q|^2 * dA computed in-kernel from q (build-defined
 *                          stencil, oracle grad2_sphere), using per-row rdx, rdy.
 * bin k = [edges[k], edges[k+1]); NaN / out-of-range cells dropped; last bin closed
 * iff last_closed.  nbin = nedge - 1.
 * Outputs (any may be NULL): pdf double[nslab][nchan][nbin]; counts uint64[nslab][nbin];
 * cdf double[nslab][nchan][nbin] = cumsum(pdf) (if !lt: cdf[-1]-cdf), reversed along
 * the bin axis iff reverse (decreasing levels, core.py:454-455).                     */
typedef struct xc_hist_desc {
    const void*   q;            int32_t q_dtype;  int32_t dA_pos_finite;  /* caller verified: dA finite and >= 0 (optional speed-up) */
    int64_t       nslab, ny, nx;
    const double* edges;        int64_t nedge;    int32_t edges_per_slab; int32_t last_closed;
    const double* dA;           int32_t dA_rank;  int32_t prod_f32;
    int32_t       nint;         int32_t grad;
    const void*   integrand[XC_MAX_INTEGRANDS];
    int32_t       integrand_dtype[XC_MAX_INTEGRANDS];
    const double* rdx;          /* [ny] 1/(2 dx)  per row (grad only)            */
    const double* rdy;          /* [ny] 1/(y[jn]-y[js]) per row (grad only)      */
    int32_t       periodic_x;   int32_t lt;
    int32_t       reverse;      int32_t negate;       /* negate: bin -q instead of q (right-closed bins on q) */
    double*       pdf;
    uint64_t*     counts;
    double*       cdf;
    int32_t       deterministic;/* != 0: order-free fixed-point sums (see "Deterministic sums" below); 0: float64 LDS atomics */
    int32_t       reserved0;
} xc_hist_desc;
int xc_hist_dev(xc_ctx* ctx, const xc_hist_desc* d);
int xc_hist(xc_ctx* ctx, const xc_hist_desc* d);

/* Deterministic sums (`deterministic != 0` in xc_hist_desc / xc_keff_desc).  The reference's per-bin sums come out of
 * np.bincount inside xhistogram (core.py:1284, 1307): the same input gives the same bits.  The default histogram pass
 * adds float64 weights with LDS atomics (and, in xc_keff_dev launches of FEW slabs -- more than 64 blocks per slab -- the
 * blocks' sums with global float64 atomics into per-slab accumulators), so the last bits of pdf / cdf (area, intgrdS) depend
 * on the order of arrival and differ from run to run (~1e-13 relative).  With `deterministic` every (bin, channel) owns a
 * fixed-point SUPERACCUMULATOR instead: four 48-bit limbs on a fixed grid below a window top that follows from bounds known
 * before the pass (max |dA|; for the in-kernel squared gradient 2 ((max - min) max(rdx, rdy))^2 max |dA| from K1's extrema; for a
 * supplied integrand max |integrand| max |dA|, from one extra min / max pass over it).  A weight is cut once to its leading 49
 * significant bits -- a function of the cell alone -- and added as two integer chunks (ds_add_u64) to the two adjacent limbs its
 * bits fall into, whatever its magnitude; the limbs are summed exactly and converted ONCE to float64 (round half to even).
 * Integer addition is associative: results are bit-identical between runs, launch geometries, slabs per launch and numbers
 * of ranks.  ONE pass over the cells (rounds 3-4 needed two: a per-bin scale came from a maximum pass): measured 1.3x the
 * default pass.  Precision: 2^-49 relative per weight anywhere in the 180 bits below the bound (the pole row of
 * a lat-lon grid carries squared gradients 2^100 times the typical ones: both keep their 49 bits); weights further down
 * lose their last bits, zeros and denormals contribute nothing; a bin that received an infinite weight reports NaN.
 * Levels, edges and counts are the same bits in both modes.  oracle/xcontour_oracle.py: deterministic_bin_sums.
 * Limit: the LDS histogram of this mode holds 5 words per channel and bin -- up to ~1700 contours with two weight channels (the Keff
 * layout), ~850 with four; beyond that the call fails with XC_EBADARG (the default sums take about three times as many). */

/* ------------------------------------------------------------------ K2  row sums for the A(Yeq) table
 * Replaces the degenerate histogram of cal_area_eqCoord_table_hist   core.py:176-193
 * rows[i] = sum_x dA[i,x] * [mask[i,x] == 1]; the prefix / end-point rules
 * are O(ny) host work.  mask may be NULL (all ones).
 * multiply != 0: rows[i] = nansum_x mask[i,x] * dA[i,x]  (the xarray twin, core.py:109-133). */
int xc_rowsum_dev(xc_ctx* ctx, const void* mask, int mask_dtype, const double* dA, int dA_rank,
                  int64_t ny, int64_t nx, int multiply, double* out_rows);
int xc_rowsum(xc_ctx* ctx, const void* mask, int mask_dtype, const double* dA, int dA_rank,
              int64_t ny, int64_t nx, int multiply, double* out_rows);

/* ------------------------------------------------------------------ K4  |grad q|^2 (stand-alone)
 * No reference call site (grdS is an input there); build-defined stencil.
 * out: double[nslab][ny][nx].                                                        */
int xc_grad2_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                 const double* rdx, const double* rdy, int periodic_x, double* out);
int xc_grad2(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
             const double* rdx, const double* rdy, int periodic_x, double* out);

/* ------------------------------------------------------------------ K7  local wave activity / local APE
 * Replaces the python loop of cal_local_wave_activity   core.py:752-791
 *   lwa[j,x] = - sum_y' (q[y',x]-Q[j]) * mask3(j,y',x) * (dA[y',x]/dAmax) * M[y',x]
 * coord: double[ny] equivalent-coordinate values; Q: double[nslab][ny];
 * dA / M: float64, rank XC_DA_ROW or XC_DA_PLANE (M_rank may be XC_DA_NONE -> M = dA,
 * the snapshot text core.py:789).  part: 0 all, 1 upper, 2 lower.
 * variant 0: cal_local_wave_activity (qe = q - Q[j]); 1: cal_local_wave_activity2 core.py:802-905
 * (qe = q[row j] - Q, opposite sign convention).
 * out_lwa: double[nslab][ny][nx].  mask_idx: int32[nmask] rows whose mask3 is returned
 * in out_masks int8[nslab][nmask][ny][nx] (values -1/0/1); nmask may be 0.           */
int xc_lwa_dev(xc_ctx* ctx, const void* q, int q_dtype, const double* Q, const double* coord,
               const double* dA, int dA_rank, double dA_max, const double* M, int M_rank,
               int64_t nslab, int64_t ny, int64_t nx, int increase, int part, int variant,
               const int32_t* mask_idx, int nmask, double* out_lwa, int8_t* out_masks);
int xc_lwa(xc_ctx* ctx, const void* q, int q_dtype, const double* Q, const double* coord,
           const double* dA, int dA_rank, double dA_max, const double* M, int M_rank,
           int64_t nslab, int64_t ny, int64_t nx, int increase, int part, int variant,
           const int32_t* mask_idx, int nmask, double* out_lwa, int8_t* out_masks);

/* Planes of more than 512 rows take an O(ny log ny)-per-column path (variant 0): because the sorted reference state Q is
 * monotone, the targets j a cell contributes to form one interval, so one binary search in Q and four adds into a
 * difference array replace the walk over every (target, row) pair; per-column prefix sums finish.  The premises -- Q finite
 * (no NaN, no infinity), s*Q non-decreasing (s = +1 if increase else -1), the coordinate strictly monotone, no INFINITE tracer cell
 * (found by the interval kernel itself; NaN cells are fine) -- are checked ON THE DEVICE first (a
 * flag the kernels gate themselves on: no host round trip, the _dev form stays asynchronous); if they fail the band walk
 * enqueued behind the interval kernel runs instead.  Same sums in
 * another order: agreement with the band walk ~1e-13 of the column's largest value (tests 1e-9), not bit for bit.
 * xc_set_lwa_exact(ctx, mode): 0 automatic (above), 1 the bit-exact band walk for every plane, 2 the interval kernel for every plane
 * (checked on the device), 3 the same with the premises vouched for by the caller -- it has looked at Q, the coordinate and the
 * tracer (no infinite cell) on the host: one launch, no check (a plane of 256 x 512: 15.8 us for the band walk, see DESIGN.md for the interval kernel).  xc_last_lwa_path: 0 band walk, 1 interval
 * kernel, 2 its premises failed the check (waits for the call when the device decided). */
int xc_set_lwa_exact(xc_ctx* ctx, int exact);
int xc_last_lwa_path(xc_ctx* ctx, int* out_path);

/* ------------------------------------------------------------------ K8  exact adiabatic rearrangement (radix sort)
 * No reference call site (the reference "sorts" by histogram CDF + table lookup);
 * SURVEY 8-a9, pinned by oracle.sorted_profile.  One slab: drop NaN / mask != 1 cells, stable
 * ascending radix sort of (q, dA) pairs, Acum = cumsum(dA_sorted),
 *   Q[j] = q_sorted[min(searchsorted(Acum, targets[j], 'right'), nvalid-1)]   (increase, lt case)
 *   bpe  = sum_i q_sorted[i] * z*(Acum[i] - dA_i/2) * dA_i,  z* = np.interp(., tbl, coord)
 * negate != 0 sorts -q (decreasing tracers; outputs are values of -q).
 * mask may be NULL; dA_rank NONE / ROW / PLANE; any of out_Q (double[J]), out_qsorted
 * (double[ny*nx], invalid cells at the end), out_acum (double[ny*nx]), out_nvalid (uint32),
 * out_bpe (double, needs tbl/coord) may be NULL.                                        */
int xc_sort_profile_dev(xc_ctx* ctx, const void* q, int q_dtype, const void* mask, int mask_dtype,
                        const double* dA, int dA_rank, int64_t ny, int64_t nx, int negate,
                        const double* targets, int J, const double* tbl, const double* coord, int ntbl,
                        double* out_Q, double* out_qsorted, double* out_acum, uint32_t* out_nvalid, double* out_bpe);
int xc_sort_profile(xc_ctx* ctx, const void* q, int q_dtype, const void* mask, int mask_dtype,
                    const double* dA, int dA_rank, int64_t ny, int64_t nx, int negate,
                    const double* targets, int J, const double* tbl, const double* coord, int ntbl,
                    double* out_Q, double* out_qsorted, double* out_acum, uint32_t* out_nvalid, double* out_bpe);

/* float64 tracers take a three-pass path: a stable LSD sort on a 24-bit RANGE key -- a monotone, piecewise-linear map of the
 * value range onto [0, 2^24 - 2] that gives densely populated parts of the range more keys (sampled histogram equalisation over
 * the plane's ROBUST range, the 9th smallest / largest of its block extrema; the few cells outside it -- a stray fill value -- get
 * 2^16 linear keys on either side instead of stretching the range) -- then a repair pass that puts every run of equal range key into exact order (stable rank inside the run, in
 * LDS) and proves the result sorted; its flag is read back -- the ONE host round trip these calls (also the _dev ones) make;
 * a stack that fails it (more than 128 distinct values inside one range key) is sorted again with the eight key passes.  The result is the same stable sort either way.  xc_last_sort_path: 0 = key passes only (float32
 * tracers, or XC_SORT_RANGE=0 in the environment at xc_create), 1 = range-key path, 2 = range-key path failed the check. */
int xc_last_sort_path(xc_ctx* ctx, int* out_path);

/* The same for a stack of nslab planes in ONE set of launches (segmented sort: every plane keeps its own
 * tile histograms, digit bases and cumulative area).  q: [nslab][ny][nx]; mask: [ny][nx] shared or
 * [nslab][ny][nx] (mask_per_slab); dA_rank NONE / ROW / PLANE (shared) or SLAB ([nslab][ny][nx]);
 * targets / tbl / coord shared.  Outputs: out_Q double[nslab][J], out_qsorted / out_acum
 * double[nslab][ny*nx], out_nvalid uint32[nslab], out_bpe double[nslab]; any may be NULL.        */
int xc_sort_profile_batch_dev(xc_ctx* ctx, const void* q, int q_dtype, const void* mask, int mask_dtype, int mask_per_slab,
                              const double* dA, int dA_rank, int64_t nslab, int64_t ny, int64_t nx, int negate,
                              const double* targets, int J, const double* tbl, const double* coord, int ntbl,
                              double* out_Q, double* out_qsorted, double* out_acum, uint32_t* out_nvalid, double* out_bpe);
int xc_sort_profile_batch(xc_ctx* ctx, const void* q, int q_dtype, const void* mask, int mask_dtype, int mask_per_slab,
                          const double* dA, int dA_rank, int64_t nslab, int64_t ny, int64_t nx, int negate,
                          const double* targets, int J, const double* tbl, const double* coord, int ntbl,
                          double* out_Q, double* out_qsorted, double* out_acum, uint32_t* out_nvalid, double* out_bpe);

/* ------------------------------------------------------------------ K9  box-counting contour crossing
 * Replaces Contour2D.cal_contour_crossing (core.py:640-693) and the numba kernel
 * _contour_crossing (core.py:1490-1566), for ALL contours of a slab in one pass.
 * The slab is padded on the X side by pad_x columns (mode pad_mode; pass 0 when the grid
 * has no 'X' dim, core.py:673-679); coarse shape Jn = round(ny/stride),
 * In = round((nx+pad_x)/stride) (round half to even, core.py:1510-1511); box (j, i),
 * j < Jn-1, covers corner rows j*s..j*s+s and corner columns i*s..i*s+s; contour c crosses
 * it iff some non-NaN corner <= c and some non-NaN corner > c (core.py:1531-1557).
 *   out_len[slab][k] = nansum over crossed boxes of sqrt(areaPad[j][i]) * stride
 *                      (area taken at the COARSE indices, core.py:1560; f32 area: f32 sqrt)
 *   out_cnt[slab][k] = number of crossed boxes (exact)
 * full_width == 0 scans box columns i < min(Jn, In) - 1 -- the reference's loop bound is
 * range(Jn-1) (core.py:1521), cut at In-1 where it would leave the array; full_width != 0
 * scans all In-1 columns.  contours: double[ncont] or double[nslab][ncont]
 * (contours_per_slab), ASCENDING, no NaN (the host entry point checks; callers with
 * other orders sort and un-permute, as xcontour_amd/core.py does).  area: [ny][nx] or
 * [nslab][ny][nx] (area_per_slab) of area_dtype.  Either output may be NULL.           */
int xc_crossing_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                    int pad_x, int pad_mode, const double* contours, int ncont, int contours_per_slab,
                    const void* area, int area_dtype, int area_per_slab, int stride, int full_width,
                    double* out_len, uint64_t* out_cnt);
int xc_crossing(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                int pad_x, int pad_mode, const double* contours, int ncont, int contours_per_slab,
                const void* area, int area_dtype, int area_per_slab, int stride, int full_width,
                double* out_len, uint64_t* out_cnt);

/* ------------------------------------------------------------------ K10 marching-squares contour lengths
 * Replaces Contour2D.cal_contour_lengths (core.py:969-1014), _contour_lengths (core.py:1437-1487) and
 * utils.contour_length / __segment_length_latlon / __segment_length_cartesian / __geodist (utils.py:565-761):
 * the total length of every contour traced by skimage's find_contours(slab, c) (defaults), for ALL contours
 * of a slab in one pass.  Rows are ycoord (ny), columns xcoord (nx); no wrap across the X seam unless the
 * _periodic entry points below are used.
 *   a cell with a NaN corner contributes nothing; case = (ul>c) + 2(ur>c) + 4(ll>c) + 8(lr>c);
 *   saddles 6 and 9 pair their points like fully_connected='low'; a segment whose two end points are
 *   equal is dropped; end points map to coordinates like np.interp(x, arange(n), coord).
 *   radius > 0: coordinates in radians, segment = haversine (__geodist), total * radius;
 *   radius == 0: Cartesian, segment = hypot(dx, dy).
 *   out_len[slab][k]  = total length, NaN where the total is 0 (utils.py:603-604): a level outside the
 *                       field's range, at its minimum or maximum;
 *   out_nseg[slab][k] = number of segments (exact; may be NULL).
 * Totals are bit-reproducible (fixed-point sums, independent of launch geometry and slabs per call).
 * contours: double[ncont] or double[nslab][ncont] (contours_per_slab), ASCENDING, no NaN (the host entry
 * point checks; callers with other orders sort and un-permute).  Coordinates must be finite (checked by
 * the host entry point).  Any ncont is accepted.                                                  */
int xc_contour_lengths_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                           const double* ycoord, const double* xcoord, double radius,
                           const double* contours, int ncont, int contours_per_slab,
                           double* out_len, uint64_t* out_nseg);
int xc_contour_lengths(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                       const double* ycoord, const double* xcoord, double radius,
                       const double* contours, int ncont, int contours_per_slab,
                       double* out_len, uint64_t* out_nseg);

/* K10 with a periodic X direction (a longitude ring).  The Y direction is never periodic.
 *   period: a float64, finite and non-zero, of the sign of xcoord[nx-1] - xcoord[0], with
 *     |period| > |xcoord[nx-1] - xcoord[0]|; the ring needs nx >= 2.  The coordinate of a node column c outside
 *     [0, nx) is xcoord[c mod nx] + period or xcoord[c mod nx] - period: one float64 addition or subtraction
 *     (only one lap either way can occur).
 *   The plane gains one cell column, index nx-1: its left corners are node column nx-1, its right corners node
 *     column 0; cL = nx-1, xL = xcoord[nx-1], xR = xcoord[0] + period.  Everything else is the rule above,
 *     unchanged: case table, frac, np.interp end points between (nx-1, xL) and (nx, xR), saddles, dropped
 *     degenerate segments, a NaN corner emits nothing, a total of 0 becomes NaN.  The window constant of the
 *     fixed-point sums takes the seam cell's width into its largest cell diagonal.
 *   By construction the result is, bit for bit, what xc_contour_lengths returns for the plane with column 0
 *     appended as column nx and xcoord[0] + period appended to the coordinates.
 * The host form checks the period conditions (XC_EBADARG); the device form checks what it can without reading
 * xcoord (finite, non-zero, nx >= 2).  xc_last_clen_geometry counts the tiles over nx cell columns.          */
int xc_contour_lengths_periodic_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                    const double* ycoord, const double* xcoord, double period, double radius,
                                    const double* contours, int ncont, int contours_per_slab,
                                    double* out_len, uint64_t* out_nseg);
int xc_contour_lengths_periodic(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                const double* ycoord, const double* xcoord, double period, double radius,
                                const double* contours, int ncont, int contours_per_slab,
                                double* out_len, uint64_t* out_nseg);

/* ------------------------------------------------------------------ K15 integrals of a field along contours
 * The line integral of `f` (the tracer's shape, float32 or float64) along every contour K10 traces, evaluated on the traced
 * segments themselves (the reference's cal_contour_mean is an area-derivative estimate; nothing there walks the contour).
 *   segments: exactly K10's -- cells, crossed levels, cases, saddles, end points, lengths `len`; with period != 0 the seam
 *     cell of xc_contour_lengths_periodic among them (period == 0.0: two free edges);
 *   F(u) at an end point u on the grid edge between two nodes: f mapped as the coordinates are -- the node's value on a
 *     node (the other node does not enter), else (F1 - F0) * (x - i0) + F0 in float64, every operation rounded once; the
 *     seam cell's right nodes are column 0;
 *   term = (0.5 * (F(u) + F(v))) * len; a segment with a NaN F(u) or F(v) is skipped in EVERY output;
 *   out_integral[slab][k] = sum of the terms, out_length[slab][k] = sum of len over the same segments, each times the radius
 *     once when radius > 0; out_nseg[slab][k] = their number (may be NULL).  Both sums are NaN where the length sum is 0
 *     (K10's rule); a level that met an infinite term has a NaN integral and keeps its length.
 * With a NaN-free f, out_length and out_nseg are xc_contour_lengths' bit for bit.  Sums are bit-reproducible (signed
 * fixed-point sums, independent of launch geometry and slabs per call).  contours, coordinates and the period: as for
 * xc_contour_lengths / xc_contour_lengths_periodic (the host form checks them; the device form checks what it can without
 * reading xcoord).  xc_last_clen_geometry reports this launch too.                                              */
int xc_contour_line_integrals_dev(xc_ctx* ctx, const void* q, int q_dtype, const void* f, int f_dtype,
                                  int64_t nslab, int64_t ny, int64_t nx,
                                  const double* ycoord, const double* xcoord, double period, double radius,
                                  const double* contours, int ncont, int contours_per_slab,
                                  double* out_integral, double* out_length, uint64_t* out_nseg);
int xc_contour_line_integrals(xc_ctx* ctx, const void* q, int q_dtype, const void* f, int f_dtype,
                              int64_t nslab, int64_t ny, int64_t nx,
                              const double* ycoord, const double* xcoord, double period, double radius,
                              const double* contours, int ncont, int contours_per_slab,
                              double* out_integral, double* out_length, uint64_t* out_nseg);

/* ------------------------------------------------------------------ K11 local (sliding-window) contour lengths
 * Replaces the loop of the reference's tests/test_localLength.py (rolling(center=True).construct(stride=), one
 * find_contours call per window): per window, the length of ONE contour traced on the window alone.
 *   windows: centres are the nodes (j, i), j = 0, sy, 2 sy, ... < ny and i = 0, sx, ... < nx, so
 *     nwy = ceil(ny / sy), nwx = ceil(nx / sx); window (j, i) owns node rows [j - wy/2, j - wy/2 + wy - 1]
 *     (integer division) and likewise columns, clipped to the plane; no wrap across the X seam unless the
 *     _periodic entry points below are used.  wy, wx >= 2;
 *   level: levels[slab][wj][wi] when `levels` is given; else (levels == NULL) the window's NaN-skipping mean in
 *     float64, in a fixed order: per window row the valid nodes left to right from 0.0 (a NaN node adds nothing
 *     and does not count), the row sums top to bottom, one IEEE division by the valid count; fewer than
 *     min_periods valid nodes give a NaN level;
 *   length: the window is a plane of its own -- cell indices count from its first row and column, coordinates are
 *     its slice of ycoord / xcoord -- under exactly the rule of K10 above (case table, frac, saddle pairing,
 *     dropped degenerate segments, np.interp end points, radius > 0 haversine x radius / radius == 0 hypot,
 *     a total of 0 -> NaN).  A NaN level gives a NaN length and 0 segments.
 *   out_len[slab][wj][wi], out_level[slab][wj][wi] (the level used; may be NULL), out_nseg[slab][wj][wi] (may be NULL).
 * Totals use K10's fixed-point sums on K10's window constant (from the whole plane's coordinates): a window's bits
 * do not depend on the launch geometry, the stride or the slabs per call.  Coordinates must be finite and sizes
 * positive (checked by the host entry point).  One launch set for all windows of all slabs.              */
int xc_local_contour_lengths_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                 const double* ycoord, const double* xcoord, double radius,
                                 int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                                 const double* levels, double* out_len, double* out_level, uint64_t* out_nseg);
int xc_local_contour_lengths(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                             const double* ycoord, const double* xcoord, double radius,
                             int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                             const double* levels, double* out_len, double* out_level, uint64_t* out_nseg);

/* K11 with a periodic X direction: `period` as for xc_contour_lengths_periodic.  Windows are no longer clipped in X:
 *   window i owns the node columns [i - wx/2, i - wx/2 + wx - 1] taken modulo nx, in that (unwrapped) order, with the
 *   unwrapped coordinates xcoord[c mod nx] +/- period.  It needs wx <= nx, else XC_EBADARG.  Y clipping, the window
 *   centres and nwx = ceil(nx / sx) are unchanged.  The mean level keeps its order: per row left to right in window
 *   order.  Length, NaN rules and the window constant are those of periodic K10.  The result is, bit for bit, what
 *   xc_local_contour_lengths returns at the matching centres of the plane with h columns of the ring copied to either
 *   side (h a multiple of sx, h >= wx).                                                                           */
int xc_local_contour_lengths_periodic_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                          const double* ycoord, const double* xcoord, double period, double radius,
                                          int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                                          const double* levels, double* out_len, double* out_level, uint64_t* out_nseg);
int xc_local_contour_lengths_periodic(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                      const double* ycoord, const double* xcoord, double period, double radius,
                                      int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                                      const double* levels, double* out_len, double* out_level, uint64_t* out_nseg);

/* ------------------------------------------------------------------ K12 marching-squares contour segments
 * No call site inside the reference's package: its scripts trace the contours themselves with skimage's find_contours
 * (tests/test_clength.py:615-630, tests/test_breaking.py, tests/test_localLength.py).  The segments K10 sums, written
 * out, for ALL contours of all slabs.  The rule is K10's (case table, frac, saddles as fully_connected='low', a cell
 * with a NaN corner emits nothing; no wrap across the X seam unless the _periodic entry points below are used) with two differences: segments are DIRECTED, start ->
 * end, in the order of skimage's _get_contour_segments
 *     1 T->L   2 R->T   3 R->L   4 L->B   5 T->B   6 R->T, L->B   7 R->B
 *     8 B->R   9 T->L, B->R   10 B->T   11 B->L   12 L->R   13 T->R   14 L->T        (T top, B bottom, L left, R right)
 * and a segment whose two end points coincide is KEPT (the join needs it).
 *   record (structure of arrays):  e_from[i], e_to[i]  the ids of the grid edges the start / end point lie on:
 *       the horizontal edge between nodes (r, c) and (r, c+1) is 2 (r nx + c), the vertical edge between (r, c) and
 *       (r+1, c) is 2 (r nx + c) + 1; cell (r0, c0) has T = H(r0, c0), B = H(r0+1, c0), L = V(r0, c0), R = V(r0, c0+1).
 *       Within one (slab, contour) every edge is the start of at most one segment and the end of at most one.
 *     pts[4 i .. 4 i + 3] = (r1, c1, r2, c2) in index space (row, column), float64, one correctly rounded
 *       subtraction, division and addition each: reproducible bit for bit.
 *   layout: segments packed by (slab, contour) in the caller's contour order; the range of (s, k) is
 *     [off[s ncont + k], off[s ncont + k + 1]) with off the exclusive scan of out_count.  The order INSIDE a range is
 *     unspecified.
 *   out_count[nslab][ncont] is always written (segments per contour, coincident-end ones included).
 *   capacity >= sum(out_count): the records are written, XC_OK.  Otherwise nothing is written to the record arrays
 *     and 1 is returned (capacity 0 with NULL record arrays = count only).
 *   q f32 / f64; contours double[ncont] or double[nslab][ncont] (contours_per_slab), ASCENDING, no NaN, as for K10
 *     (the host entry point checks).  Any ncont is accepted: contours beyond XC_CSEG_GROUP_LEVELS are processed in
 *     groups of that many.  ny < 2 or nx < 2: no cells, all counts 0, XC_OK.
 * Both forms wait for the stream once (the total decides on the host whether the records fit).               */
#define XC_CSEG_GROUP_LEVELS 2048
int xc_contour_segments_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                            const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                            uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts);
int xc_contour_segments(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                        const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                        uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts);

/* K12 with a periodic X direction (no period value: K12 works in index space).  The plane is a ring of nx cell columns:
 *   the seam cell, cell column nx-1, has its left corners on node column nx-1 and its right corners on node column 0; its
 *   columns run from nx-1 to nx exactly (a point on its right edge has column (double)nx).  Its top and bottom edges are
 *   H(r, nx-1) and H(r+1, nx-1) -- ids the plain call never uses -- and its right edge is column 0's, V(r, 0) = 2 r nx + 1;
 *   every other id and every other cell is as above, and within one (slab, contour) every edge is still the start of at
 *   most one segment and the end of at most one.  Y never wraps.
 *   By construction: for the plane with column 0 appended as column nx, the periodic call returns the records of the plain
 *   call on that (ny, nx + 1) plane, up to the order inside a range: pts are bit for bit the same, and every edge id is
 *   folded from the extended plane's numbering to the ring's: (kind, r, c) over nx + 1 columns, id 2 (r (nx+1) + c) + kind,
 *   becomes 2 (r nx + (c mod nx)) + kind.
 *   Arguments, layout, the capacity protocol and the return values are those of the plain pair.  It needs nx >= 2, else
 *   XC_EBADARG; ny < 2: no cells, all counts 0, XC_OK.                                                              */
int xc_contour_segments_periodic_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                     const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                                     uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts);
int xc_contour_segments_periodic(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                 const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                                 uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts);

/* ------------------------------------------------------------------ K13 contour pieces and their statistics
 * The reference's scripts work piece by piece (tests/test_breaking.py: the largest contour round the pole; tests/test_clength.py:
 * contour_length(seg) per piece; utils.contour_area).  Input: K12's records ON THE DEVICE, as the K12 _dev entry points wrote them --
 * count[nrange] (a range = one (slab, contour), K12's out_count), e_from, e_to, pts -- with ny, nx and `periodic` of that call.
 * A PIECE is a connected chain of segments under "next(i) is the segment of the same range whose e_from == e_to[i]": a ring, or an
 * open polyline headed by a segment without a predecessor (the polylines of the host join above).  2 ny nx < 2^31 and every range has
 * fewer than 2^31 segments, else XC_EBADARG.
 *   ycoord[ny], xcoord[nx], period, radius: the plane's coordinates with exactly the meaning they have for the K10 entry points
 *     (radians when radius > 0; period is read only when periodic != 0: column nx is xcoord[0] + period).
 *   record (structure of arrays, one per piece):
 *     first_edge int64  the smallest e_from of the piece: unique within a range, the key the host join orders polylines by
 *     nseg       int64  its segments, coincident-end ones included
 *     closed     int32  1 for a ring, 0 for an open polyline
 *     winding    int32  rings of a periodic plane: the number of links that jump from column nx to column 0 minus those that jump
 *                       back (the ring's closing link included) -- what the facade's contour_polylines computes; else 0
 *     length     f64    the sum of K10's segment lengths (np.interp end points, haversine x radius or hypot; a segment whose end
 *                       points coincide adds nothing; a piece of such segments only has length 0, not NaN)
 *     area       f64    S = 1/2 sum over the directed segments a -> b of (Ya' + Yb') (Xa - Xb); Y' = Y on a Cartesian plane; Y' = sin(Y)
 *                       when radius > 0, and S is then multiplied by radius^2 (the shoelace formula on the equal-area (lambda, sin phi)
 *                       plane).  Signed; NaN for an open piece.  Ring with winding 0: |S| is the enclosed area, S > 0 when the ring
 *                       encloses values ABOVE the level for (ycoord, xcoord) both ascending (each descending coordinate flips the
 *                       sign).  Ring with winding != 0: S is the signed area between the ring and the line Y' = 0; on the sphere
 *                       the polar cap it bounds measures 2 pi radius^2 -/+ S.
 *     row_min, row_max f64  the smallest / largest index-space row over the end points of the piece's segments
 *   length and area are exact sums of their float64 terms rounded once (fixed-point accumulators), and every other field is an
 *   integer reduction: the records do not depend on the order of the segments or of arrival.  Each sum has a window of 160 bits
 *   under 2^top, top = 12 + the frexp exponent of a bound on one term fixed from the coordinates alone (length: 1.0000001 x the
 *   largest cell diagonal, 3.2 on the sphere; area: 1.0000001 x max |Y'| x the largest cell width; the seam cell counts on a periodic
 *   plane).  Every term of K12's records lies inside.  Of other records: the bits of a term under 2^(top - 160) are cut off (toward
 *   zero; the sum is then exact in the cut terms), and a term of 2^top or more, or a non-finite one, makes THAT sum of THAT piece
 *   NaN -- length and area each by their own window; every other piece of the call is untouched.
 *   layout: pieces packed by range: the pieces of range r are [poff[r], poff[r+1]), poff the exclusive scan of piece_count.  The order
 *     INSIDE a range is unspecified (sort by first_edge for the order of the host join).
 *   piece_count[nrange] is always written.  capacity >= sum(piece_count): the records are written, XC_OK.  Otherwise nothing is
 *     written to the record arrays and 1 is returned (capacity 0 with NULL record arrays = count only).  The number of segments is an
 *     upper bound of the number of pieces.
 * The call waits for the stream twice (K12's counts size the work; the piece counts decide whether the records fit).  Edge tables of
 * 2 ny nx int32 per range are built for groups of ranges; xc_set_cpiece_workspace caps a group's tables in bytes (default 1 GiB; one
 * range is always allowed; the result does not depend on it).  With xc_set_kernel_timing on, xc_last_cpiece_profile returns the last
 * call's device times in ms -- ms[0] edge tables (clear, scatter, link), ms[1] the doubling rounds, ms[2] roots and slots, ms[3] the
 * reductions -- the number of rounds summed over the groups, and the number of groups.                                          */
int xc_contour_pieces_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                          int64_t ny, int64_t nx, int periodic, const double* ycoord, const double* xcoord, double period, double radius,
                          int64_t capacity, uint64_t* piece_count, int64_t* first_edge, int64_t* nseg, int32_t* closed, int32_t* winding,
                          double* length, double* area, double* row_min, double* row_max);
int xc_set_cpiece_workspace(xc_ctx* ctx, uint64_t bytes);
int xc_last_cpiece_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K14 contour polylines: the join on the device
 * The content of xc_join_segments (below) computed on the device from K12's records where the K12 _dev entry points left them, with
 * the records already gathered into walk order: nothing is sorted or walked on the host.  Input as for K13: count[nrange], e_from,
 * e_to, pts, with ny, nx of that call (plain or periodic: the ids alone decide the links).  2 ny nx < 2^31 and every range has fewer
 * than 2^31 segments, else XC_EBADARG.
 *   per polyline, packed by range, and inside a range in ascending first_edge order -- the order of xc_join_segments, no host sort:
 *     poly_nseg int64  its segments;  poly_closed int32  1 for a ring;  poly_first_edge int64  the smallest e_from it contains
 *   per segment, at its WALK POSITION: polylines laid out range by range in the order above (range r fills [off[r], off[r+1]), off the
 *     exclusive scan of count: the polyline offsets are the running sum of poly_nseg), inside a polyline in walk order; an open
 *     polyline starts at its segment without predecessor, a ring at its segment of smallest e_from:
 *     pts_walk[total][4], e_from_walk[total]  the records of the segment that stands there, bit for bit;
 *     order[total]  its index among the input records (xc_join_segments' `order`).  Each of the three may be NULL.
 *   poly_count[nrange] is always written.  capacity >= sum(poly_count): everything is written, XC_OK.  Otherwise nothing but poly_count
 *     is written and 1 is returned (capacity 0 with NULL arrays = count only).  The number of segments bounds the number of polylines.
 *   Records that are no join's input are XC_EBADARG, as for xc_join_segments: an edge id outside [0, 2 ny nx), or an id that repeats
 *     among the e_from or among the e_to of one range.  No input makes the call write outside the caller's arrays or loop unboundedly.
 * The call waits for the stream twice (K12's counts; the polyline counts).  It works in K13's groups of ranges under K13's cap
 * (xc_set_cpiece_workspace; the result does not depend on it).  With xc_set_kernel_timing on, xc_last_cjoin_profile returns the last
 * call's device times in ms -- ms[0] edge tables (clear, scatter, link, check), ms[1] the label rounds, ms[2] roots and the ranking
 * rounds, ms[3] placement (the scan along the tables), ms[4] the gather into walk order -- the number of rounds summed over the
 * groups (labels and ranks), and the number of groups.                                                                          */
int xc_contour_polylines_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                             int64_t ny, int64_t nx, int64_t capacity, uint64_t* poly_count, int64_t* poly_nseg, int32_t* poly_closed,
                             int64_t* poly_first_edge, double* pts_walk, int64_t* e_from_walk, int64_t* order);
int xc_last_cjoin_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K16 contour overturning: meridian crossings of selected pieces
 * The reference's tests/test_breaking.py traces a PV contour and keeps "the largest contour fully encircling the pole" (its
 * Subroutines 4-5).  The next step of a wave-breaking analysis is to find where that contour is OVERTURNED -- where one meridian meets
 * it three times or more -- and how far in latitude the fold reaches.  Build-defined; it works in index space, needs no coordinates,
 * and every output is an integer or a copy of a K12 value.
 * Input as for K13: count[nrange], e_from, e_to, pts where the K12 _dev entry points left them, with ny, nx, periodic of that call.
 * Pieces, closed, winding, nseg and first_edge are K13's.  2 ny nx < 2^31 and every range has fewer than 2^31 segments, else
 * XC_EBADARG; so is an edge id outside [0, 2 ny nx).
 *   select: 0 'all'         every piece
 *           1 'circumpolar' every ring with winding != 0
 *           2 'main'        of those, per range, the one ring with the most segments, ties broken by the smallest first_edge
 *     select != 0 with periodic == 0 is XC_EBADARG (nothing is written): no piece goes round a plain plane.
 *   A MERIDIAN CROSSING of a selected piece is the start point of any of its segments whose e_from is odd (it lies on a vertical
 *     edge V(r, c)), or the end point of a segment without successor (the tail of an open piece) whose e_to is odd.  Its column is
 *     (id >> 1) % nx, its row the stored r1 (a start point) or r2 (an end point) of that record, bit for bit.  On a ring every vertex
 *     is counted once.  On the periodic plane V(r, 0) is cell 0's left edge and the seam cell's right edge, and is column 0.  Which
 *     edge a point on a node belongs to is whatever K12 wrote: the ids are read, the field is not looked at again.
 *   per (range, column), dense [nrange][nx]:
 *     ncross int32  the crossings;  row_lo, row_hi f64  the smallest / largest crossing row, NaN where ncross == 0
 *   per range, [nrange]:
 *     nsel int32  the selected pieces;  main_first_edge int64 (-1: none), main_nseg int64 (0), main_winding int32 (0): the ring
 *     'main' would pick, filled under every select on a periodic plane.  main_first_edge is the key under which K13 and K14 list
 *     that ring.
 *   A column of the main ring with ncross >= 3 is overturned; row_hi - row_lo there is the depth of the fold.  Every output is an
 *   integer reduction (rows by their bit patterns: they are non-negative): nothing depends on the order of the segments or of arrival.
 *   On XC_OK all seven arrays are fully written, whatever the records hold; there is no capacity protocol.
 * The call waits for the stream twice (K12's counts; the word that says whether the ids were in range).  It works in K13's groups of
 * ranges under K13's cap and in K13's workspace (xc_set_cpiece_workspace; the result does not depend on it).  With xc_set_kernel_timing
 * on, xc_last_coverturn_profile returns the last call's device times in ms -- ms[0] edge tables (clear, scatter, link), ms[1] the
 * doubling rounds, ms[2] per-piece sums and the selection, ms[3] the count (with the init and finish passes over the outputs) -- the
 * number of rounds summed over the groups, and the number of groups.                                                             */
int xc_contour_overturning_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                               int64_t ny, int64_t nx, int periodic, int select, int32_t* ncross, double* row_lo, double* row_hi, int32_t* nsel,
                               int64_t* main_first_edge, int64_t* main_nseg, int32_t* main_winding);
int xc_last_coverturn_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K17 contour interior: what the selected pieces bound
 * The threshold rule of the reference's cal_integral_within_contours sums over every node with q > c: cut-off blobs and filaments
 * land in the same bucket as the vortex they left.  This call measures the region bounded by the SELECTED pieces alone -- with
 * select 2, by the one ring K16 calls main -- and can return it as a mask.  Build-defined; index space; the field is not read again.
 * Input as for K13 and K16: count[nrange], e_from, e_to, pts where the K12 _dev entry points left them, with ny, nx, periodic of that
 * call.  Pieces, rings, winding, select (0 all, 1 circumpolar, 2 main) and the tie rule of the main ring are K16's.  2 ny nx < 2^31,
 * every range has fewer than 2^31 segments, every edge id lies in [0, 2 ny nx), else XC_EBADARG; select != 0 with periodic == 0 is
 * XC_EBADARG (nothing is written).  range = s ncont + k: nrange is a multiple of ncont, and nrange / ncont (at most 65535) is the
 * number of slabs of w (with w_per_slab) and of f.
 *   CROSSING FLAG  X[r][c], 0 <= r < ny - 1, 0 <= c < nx, is 1 iff the vertical edge V(r, c) carries a meridian crossing of a selected
 *     piece under K16's definition: the start point of a segment with odd e_from, or the end point of a segment without successor
 *     with odd e_to.  Column (id >> 1) % nx, row (id >> 1) / nx.  Setting the flag is idempotent; an edge is the start of at most one
 *     segment per range in K12's records, so sum_r X[r][c] is K16's ncross[c] under the same select.
 *   NODE PARITY    P[r][c] = XOR over r' < r of X[r'][c]; P[0][c] = 0: whether the node lies on the other side of the selected pieces
 *     from row 0 of its own column.
 *   INSIDE         inside = P ^ flip, flip 0 or 1.
 *   per range, [nrange]:
 *     n_in   int64  the inside nodes
 *     sum_w  f64    the sum over the inside nodes of w[r][c]; w is double[ny][nx], or double[nslab][ny][nx] with w_per_slab != 0;
 *                   w == NULL is weight 1 (sum_w == n_in)
 *     sum_wf f64    the sum of w[r][c] f[s][r][c], each product rounded once; f is f32 (f_dtype XC_F32) or f64 [nslab][ny][nx], or
 *                   NULL, and sum_wf is NULL exactly when f is
 *     mask   uint8 [nrange][ny][nx], 1 inside; may be NULL
 *   The sums are K13's: exact sums of their float64 terms rounded once, independent of order and launch geometry.  Each has a window
 *   of 160 bits under 2^top, top = 12 + the frexp exponent of max |w| (max |w f|) over the finite values of the range's slab (all of
 *   the plane, inside or not), never below -800; the bits of a term under 2^(top - 160) are cut off toward zero.  A NaN term is
 *   skipped (as np.nansum does); a +-inf term makes THAT sum of THAT range NaN, and no other.
 *   With select 0 on the records of a NaN-free field, P[r][c] == (q[r][c] > level) ^ (q[0][c] > level).  Beside NaN cells, and for
 *   a vertex on a node, the ids are whatever K12 wrote: a crossing that no NaN-free cell saw is no crossing.
 *   On XC_OK every output is fully written, whatever the records hold; there is no capacity protocol.
 * The call waits for the stream twice (K12's counts; the word that says whether the ids were in range).  It works in K13's groups of
 * ranges under K13's cap and in K13's workspace (xc_set_cpiece_workspace; the result does not depend on it), with ny ceil(nx / 32)
 * 32-bit words of crossing flags per range of a group.  With xc_set_kernel_timing on, xc_last_cinterior_profile returns the last call's
 * device times in ms -- ms[0] edge tables (clear, scatter, link), ms[1] the doubling rounds, ms[2] per-piece sums and the selection,
 * ms[3] the marks and the scan (with the bounds of the windows and the finish pass) -- the number of rounds summed over the groups,
 * and the number of groups.                                                                                                     */
int xc_contour_interior_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                            int64_t ny, int64_t nx, int periodic, int select, int flip, int ncont, const double* w, int w_per_slab,
                            const void* f, int f_dtype, int64_t* n_in, double* sum_w, double* sum_wf, uint8_t* mask);
int xc_last_cinterior_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K18 contour piece interiors: what EVERY piece bounds
 * K17 measures one selection per range and leaves out what the vortex has shed.  A cut-off low, a shed filament, a blob of
 * stratospheric air is a closed piece with winding 0, and the questions asked of it are per piece: how many nodes, how much w, how much
 * w f does it enclose.  This call answers for every piece of every range at once; only a per-piece table is written.  Build-defined;
 * index space; the field is not read again.
 * Input as for K13, K16 and K17: count[nrange], e_from, e_to, pts where the K12 _dev entry points left them, with ny, nx, periodic of
 * that call; w with w_per_slab and f with f_dtype exactly as K17 reads them (range = s ncont + k, nrange a multiple of ncont, at most
 * 65535 slabs).  Pieces, closed, winding, nseg and first_edge are K13's.  2 ny nx < 2^31, every range has fewer than 2^31 segments,
 * every edge id lies in [0, 2 ny nx) and repeats neither among the e_from nor among the e_to of a range, else XC_EBADARG (the edge
 * tables are handed on clean first).  periodic with nx < 3 is XC_EBADARG: with two columns a cell's two vertical edges are one edge.
 * For ONE piece p of a range, K17's definitions with the selection being p alone:
 *   CROSSING FLAG  X_p[r][c] = 1 iff V(r, c), r < ny - 1, carries a meridian crossing (K16's definition) of a segment of p.
 *   NODE PARITY    P_p[r][c] = XOR over r' < r of X_p[r'][c].
 *   INSIDE         a ring with winding 0: inside = P_p (row 0 is always outside such a ring);
 *                  a ring with winding != 0: inside = P_p ^ flip, flip 0 or 1 (K17's);
 *                  an open piece bounds nothing: n_in = -1 and both sums are NaN.
 *   The interior is that of the ring ALONE: the nodes of a ring nested inside it are counted, not subtracted -- K19
 *   (xc_contour_piece_tree_dev) says which piece is nested in which and gives the net records.
 * per piece, packed by range like K13's records (the pieces of range r are [poff[r], poff[r+1]), poff the exclusive scan of
 * piece_count; the order INSIDE a range is unspecified: sort by first_edge):
 *     first_edge int64  the smallest e_from of the piece: the key that joins the row to xc_contour_pieces_dev
 *     nseg int64, closed int32, winding int32   K13's
 *     n_in   int64  the inside nodes
 *     sum_w  f64    the sum of w over them; w == NULL is weight 1
 *     sum_wf f64    the sum of w f, each product rounded once; NULL exactly when f is NULL
 *   The sums are K17's: exact sums of their float64 terms rounded once, a window of 160 bits under 2^top, top = 12 + the frexp exponent
 *   of max |w| (max |w f|) over the finite values of the range's slab; a NaN term is skipped; a +-inf term makes THAT sum of THAT piece
 *   NaN, and no other.  Nothing depends on the order of the segments or of arrival, on the cap of a group, or on the launch geometry.
 *   piece_count[nrange] is always written.  capacity >= sum(piece_count): the records are written, XC_OK.  Otherwise nothing is
 *     written to the record arrays and 1 is returned (capacity 0 with NULL record arrays = count only).  The number of segments is an
 *     upper bound of the number of pieces.
 * What the call relies on: a ring of K12's records is a simple closed curve, so down one column its crossings alternate between
 * entering and leaving, and the ids say which is which (xc_cpiece_interior.h states how).  On such records the result IS the rule above.  On
 * records that are no K12 output n_in and the sums are unspecified, but every access stays in bounds and every walk ends within ny steps.
 * The call waits for the stream once for K12's counts, once per group for its piece counts, once at the end.  It works in K13's groups
 * of ranges under K13's cap and in K13's workspaces (xc_set_cpiece_workspace; the result does not depend on it).  With
 * xc_set_kernel_timing on, xc_last_cpinside_profile returns the last call's device times in ms -- ms[0] edge tables (clear, scatter,
 * link), ms[1] the doubling rounds, ms[2] roots, slots and the per-piece signs (with the wait for the piece counts), ms[3] the walks
 * (with the bounds of the windows and the finish pass) -- the number of rounds summed over the groups, and the number of groups.    */
int xc_contour_piece_interiors_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                   const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                                   int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                                   int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf);
int xc_last_cpinside_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K19 contour piece tree: which piece is NESTED in which
 * K18 gives every ring what it bounds, nested rings' nodes included, and a flat list.  A cut-off low with a warm core, a vortex with a
 * hole, an eddy with a ring round it are rings INSIDE rings: this call adds the hierarchy -- per piece its parent, its depth, the number
 * of its children -- and what the ring bounds NET of its children.  Build-defined; index space; the field is not read again.
 * Input exactly as K18 takes it: count[nrange], e_from, e_to, pts where the K12 _dev entry points left them, with ny, nx, periodic of
 * that call, flip, ncont, w with w_per_slab and f with f_dtype; the same limits and the same XC_EBADARG cases.  Pieces, closed, winding,
 * nseg, first_edge, n_in, sum_w and sum_wf are K18's, bit for bit.
 * For a ring p let I_p be K18's inside set: P_p for winding 0, P_p ^ flip for winding != 0.
 *   ENCLOSES   for two different rings a, b of the same range, a encloses b iff every node of I_b lies in I_a.  Rings of one level do
 *              not meet: two rings are nested one way, nested the other way, or disjoint, and never have the same inside set.
 *   PARENT     parent[b] is the ring that encloses b and has the fewest inside nodes -- the innermost enclosing ring --, -1 when no
 *              ring encloses b.  Pieces of different ranges (levels, slabs) are never related.
 *   OPEN PIECES bound nothing and are transparent: they are nobody's parent; their own parent is -1, depth 0, nchild 0, n_net -1 and
 *              both net sums NaN.
 *   DEPTH      0 where parent is -1, else depth[parent] + 1.
 *   NCHILD     the number of rings whose parent is p.
 *   NET        over the nodes of I_p that lie in no child's inside set: n_net their number, net_w and net_wf the sums of w and of w f
 *              over them under K17/K18's rule (each product rounded once; the exact sum of the float64 terms rounded once, in K18's
 *              window; a NaN term is skipped).  A net sum is NaN exactly when the ring's own gross sum (sum_w / sum_wf) is NaN.  The
 *              children's inside sets are disjoint subsets of I_p: n_net = n_in - the sum of n_in over the children, and so for the
 *              exact sums.
 * per piece, packed like K18's records, beside them:
 *     parent int64  an index into this call's piece table, poff[r] + position as the rows are packed; -1 for none
 *     depth  int32, nchild int32
 *     n_net  int64, net_w f64, net_wf f64 (NULL exactly when f is NULL)
 *   Nothing depends on the order of the segments or of arrival, on the cap of a group, or on the launch geometry.
 *   piece_count and the capacity / count-only protocol are K18's: short of capacity nothing is written to any record array, 1 is returned.
 * What the call relies on is what K18 relies on (xc_cpiece_tree.h states how the parent is found: one column walk per ring from the node
 * across its outermost crossing).  On records that are no K12 output the tree fields are unspecified, but every access stays in bounds and
 * every loop ends: walks within ny steps, chases of parents within the range's piece count (one that does not end there is XC_EBADARG).
 * Stream waits, groups and workspaces are K18's.  With xc_set_kernel_timing on, xc_last_cptree_profile returns the last call's device
 * times in ms -- ms[0] to ms[3] as xc_last_cpinside_profile, ms[4] the tree stages (top crossings, parent walks, depths, net words and
 * their finish pass) -- the number of rounds summed over the groups, and the number of groups.                                      */
int xc_contour_piece_tree_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                              const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                              int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                              int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                              int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf);
int xc_last_cptree_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K20 contour piece labels: which ring HOLDS each node
 * K18 and K19 say, per ring, how many nodes, how much w and how much w f it bounds, gross and net of its children -- not WHICH nodes.
 * This call returns K19's records unchanged and, per range, a dense map [ny][nx] that names the innermost ring round every node: what
 * a centroid, an extremum, a composite of further fields over one ring, or the overlap of two days' blobs need (the label image that
 * image libraries ship beside their ring tree).  Build-defined; index space; the field is not read again.
 * Input exactly as K19 takes it, with the same limits and the same XC_EBADARG cases; the thirteen record columns are K19's, bit for bit.
 * For a ring p let I_p be K18's inside set: P_p for winding 0, P_p ^ flip for winding != 0.
 *   LABEL      label[range][r][c] is the ring p of that range with (r, c) in I_p and the fewest inside nodes, -1 where no ring holds the
 *              node.  Rings of one range are nested or disjoint and never share an inside set, so that ring is unique: the DEEPEST ring
 *              that holds the node.
 *   OPEN PIECES are transparent, as in K19: they never appear in the map.
 *   VALUE      the ring's position inside its own range as the rows are packed, p - poff[range] (int32: a range has fewer than 2^31
 *              segments, hence pieces); sort the range's rows by first_edge and map the values likewise to line them up with K13.
 *   On K12's records:
 *     the number of nodes with label == p is n_net[p];
 *     the nodes with label == p or label a descendant of p are I_p;
 *     depth[label] is the number of rings that hold the node, minus 1.
 *   label int32 [nrange][ny][nx].  On XC_OK the map is fully written, whatever the records hold; a range without segments is all -1.
 *   piece_count and the capacity / count-only protocol are K19's: short of capacity nothing is written to any record array, 1 is
 *   returned, and the contents of the map are then unspecified.  label == NULL with capacity > 0 is XC_EBADARG.
 *   Nothing depends on the order of the segments or of arrival, on the cap of a group, or on the launch geometry.
 * What the call relies on is what K19 relies on (xc_cpiece_label.h states the scan: one pass per column from the row that lies outside
 * every ring, a crossing enters its ring or leaves it for the ring's parent).  On records that are no K12 output the labels are
 * unspecified (-1, or a position inside the range's piece count), but every access stays in bounds and every loop ends within ny steps.
 * Stream waits, groups and workspaces are K18's.  With xc_set_kernel_timing on, xc_last_cplabel_profile returns the last call's device
 * times in ms -- ms[0] to ms[4] as xc_last_cptree_profile, ms[5] the label scan (carries, scan and the -1 fill of ranges without
 * segments) -- the number of rounds summed over the groups, and the number of groups.                                                */
int xc_contour_piece_labels_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                                int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                                int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                                int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf,
                                int32_t* label);
int xc_last_cplabel_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K21 contour piece props: what every ring HOLDS of further fields
 * K20's map names the ring round every node; what its consumers then compute per ring -- the centroid of a cut-off low (three moments),
 * the extremum of the tracer inside a ring, a composite of further fields over one ring -- are reductions over that map.  This call
 * returns K19's records unchanged and those reductions, per ring and in one pass over the columns: the map [nrange][ny][nx] is never
 * allocated and only per-piece tables are written.  Build-defined; index space.
 * Input exactly as K19 takes it, with the same limits and the same XC_EBADARG cases; the thirteen record columns are K19's, bit for bit.
 * Further input:
 *   nf           the number of fields, 0 <= nf <= XC_PROPS_MAXF
 *   g[nf]        HOST array of device pointers, one plane or stack per field
 *   g_dtype[nf]  HOST array: XC_F32 or XC_F64
 *   g_per_slab[nf] HOST array: 0 one plane [ny][nx] shared by all slabs, non-zero [nslab][ny][nx]
 *   x, x_dtype   the extremum field [nslab][ny][nx], XC_F32 or XC_F64, or NULL
 * For a ring p let I_p be K18's inside set and N_p its NET set: the nodes K20 would label p (I_p minus the inside sets of p's children).
 * Open pieces are transparent, as in K19 and K20.
 * per piece, packed like K19's records; column m of a per-field array starts at m * capacity:
 *     net_g f64 [nf][capacity]  the sum over N_p of w g_m, each product rounded once (float32 fields widened first; w == NULL is weight 1)
 *     sum_g f64 [nf][capacity]  the same over I_p
 *       Both are K17's sums: the exact sum of the float64 terms rounded once, a window of 160 bits under 2^top, top = 12 + the frexp
 *       exponent of max |w g_m| over the finite values of the range's slab.  A NaN term is skipped.  A +-inf term makes THAT field's sums
 *       NaN for the ring that holds the node (net and gross) and for every ring that encloses it (gross), and for no other ring and no
 *       other field.  For an open piece the sums are NaN.  Both pointers are NULL exactly when nf == 0.
 *     x_min, x_max f64, at_min, at_max int64   the extremum of x over the nodes of N_p whose x is not NaN, and the flat node r * nx + c
 *       it sits on.  Order: by value, -0.0 below +0.0 (the order of the usual monotone 64-bit key of a double); ties go to the smallest
 *       flat node.  With no such node, or for an open piece: NaN and -1.  The four pointers are NULL exactly when x is NULL.  Only the
 *       NET extremum is computed: the gross one is a min / max over the subtree of parent[], exact on the host.
 *   On K12's records sum_g[m][p] is the exact sum of the terms of net_g[m] over p and all its descendants.
 *   piece_count and the capacity / count-only protocol are K19's: short of capacity nothing is written to any record array, 1 is returned.
 *   Nothing depends on the order of the segments or of arrival, on the cap of a group, or on the launch geometry.
 * What the call relies on is what K20 relies on (xc_cpiece_props.h states the scan).  On records that are no K12 output the new fields are
 * unspecified, but every access stays in bounds and every loop ends: scans within ny steps, chases of parents within the range's piece
 * count (one that does not end there is XC_EBADARG, as in K19).
 * Stream waits, groups and workspaces are K18's; the staged words take 2 x 40 bytes per field and piece of min(capacity, segments).  With
 * xc_set_kernel_timing on, xc_last_cpprops_profile returns the last call's device times in ms -- ms[0] to ms[4] as
 * xc_last_cptree_profile, ms[5] the carries and the props scans (with the bounds of the fields' windows), ms[6] the fold up the tree and
 * the finish pass -- the number of rounds summed over the groups, and the number of groups.                                          */
#define XC_PROPS_MAXF 8
int xc_contour_piece_props_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                               const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                               int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                               int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                               int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf,
                               int nf, const void* const* g, const int* g_dtype, const int* g_per_slab, const void* x, int x_dtype,
                               double* net_g, double* sum_g, double* x_min, double* x_max, int64_t* at_min, int64_t* at_max);
int xc_last_cpprops_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K22 label overlap: which rings of two fields share nodes
 * K20's map names the ring round every node of one field.  Following a cut-off low or a shed filament from one day to the next -- the
 * reason to label rings at all -- is a contingency table between the maps of two fields: for every pair of rings (a of field A, b of
 * field B) that share a node, how many nodes, how much w and how much w f they share.  This call builds that sparse table from two maps
 * on the device; only the table is written.  Build-defined; index space.  The maps need not be K20's: any two int32 maps are taken.
 * Input (all pointers device pointers):
 *   lab_a, lab_b int32 [nrange][ny][nx]   the two maps; range r belongs to slab r / ncont (this matters for w when w_per_slab is
 *                                         set, and for f); nrange a multiple of ncont >= 1
 *   w f64 [ny][nx], or [nslab][ny][nx] with w_per_slab, or NULL: weight 1;  f [nslab][ny][nx] XC_F32 or XC_F64, or NULL
 *   LABELS     any negative label means "no ring" and is reported as -1.  Every non-negative int32 is a valid label: no bound on the
 *              label values is needed and none is checked.
 *   ROWS       for every range one row per distinct pair (a, b) that occurs on at least one node.  The pair (-1, -1) is omitted;
 *              pairs with exactly one -1 ARE rows (a node in a ring of A but in no ring of B).  Hence for every a >= 0 the sum of n
 *              over that a's rows is the number of nodes labelled a, and the same holds for b.
 *   a, b int32, n int64      the pair and the number of its nodes
 *   sum_w, sum_wf f64        K17's sums over the pair's nodes, with its rules: the exact sum of the float64 terms rounded once, a window
 *              of 160 bits under 2^top, top = 12 + the frexp exponent of max |w| resp. max |w f| over the finite values of the range's
 *              slab; w == NULL is weight 1; a float32 f is widened first and the product is rounded once; a NaN term is skipped; a
 *              +-inf term makes THAT sum of THAT pair NaN, and no other.  sum_wf is NULL exactly when f is NULL.
 *   PACKING    rows are packed by range: range r starts at the exclusive scan of pair_count.  The order inside a range is the call's
 *              own; callers sort by (a, b).
 *   CAPACITY   K19's count-only / capacity protocol: pair_count uint64 [nrange] is always written; short of capacity nothing is
 *              written to any row array and 1 is returned; with capacity == 0 the row pointers may be NULL.  A NULL row pointer (other
 *              than sum_wf) with capacity > 0 is XC_EBADARG, and so are ny, nx, nrange or ncont < 1, nrange % ncont != 0, a plane of
 *              2^31 nodes or more, and more than 65535 slabs.
 *   Nothing depends on the order of arrival, on the cap of a group, or on the launch geometry: two calls give the same rows, bit for
 *   bit, after sorting.
 * xc_cpoverlap.hip states the mapping: runs of constant pair down column chunks, handed over to a per-range open-addressing table in
 * K13's workspaces (64 bytes a slot, 104 with f; twice the range's runs rounded up to a power of two; groups of ranges under the
 * xc_set_cpiece_workspace cap, one range always allowed; the result does not depend on it).  Allocation failure is XC_ENOMEM.  The call
 * waits for the stream as K18 does.  With xc_set_kernel_timing on, xc_last_cpoverlap_profile returns the last call's device times in ms
 * -- ms[0] the run count, ms[1] the accumulate pass (with the bounds of the windows and the clearing of the tables), ms[2] the finish --
 * and the number of groups; `rounds` is 0 and is kept for symmetry with the other profile calls.                                      */
int xc_label_overlap_dev(xc_ctx* ctx, int64_t nrange, int64_t ny, int64_t nx, int ncont,
                         const int32_t* lab_a, const int32_t* lab_b,      /* device, [nrange][ny][nx] each */
                         const double* w, int w_per_slab, const void* f, int f_dtype,
                         int64_t capacity, uint64_t* pair_count,          /* [nrange] */
                         int32_t* a, int32_t* b, int64_t* n, double* sum_w, double* sum_wf);
int xc_last_cpoverlap_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K23 ring tracks: rings followed over many fields
 * K22 pairs the rings of two fields.  Following every ring of a stack of fields from birth to death, with splits and mergers, is a graph
 * problem: the rings of all steps are vertices, the accepted overlaps between the rings of consecutive steps are edges, and a TRACK is a
 * connected component.  This call takes that graph as arrays and labels it on the device.  It is generic: it knows nothing of planes, and
 * any ring / link arrays are taken.  Build-defined.
 * Input (all pointers device pointers):
 *   nring >= 1, nlink >= 0
 *   ring_step int32 [nring]               the step of every ring (only its min and max per track are taken)
 *   ring_size int64 [nring]               the size the threshold compares with; may be NULL iff min_overlap == 0
 *   link_a, link_b int64 [nlink]          ring indices, a the earlier ring; any negative index means "no ring"
 *   link_n int64 [nlink]                  the shared nodes
 *   min_overlap                           in [0, 1]
 *   ACCEPT     a link is accepted when a >= 0 && b >= 0 && n >= 1 and either min_overlap == 0 or
 *              (double)n >= min_overlap * (double)min(size[a], size[b]), the product rounded once in float64.
 *   REFUSALS   an index >= nring, a NaN min_overlap or one outside [0, 1], ring_size NULL with min_overlap != 0, nring < 1, nlink < 0,
 *              more than 2^38 rings or links, a NULL output with capacity > 0: XC_EBADARG.  The indices are checked on the device through
 *              an error word, as K22 checks its rows.  On an error nothing is written.
 * Output per ring:
 *   root int64      the smallest ring index of the ring's component over the accepted links
 *   track int64     the rank of that root among all roots, ascending: tracks are numbered in the order of their first rings
 *   nprev, nnext int32   the accepted links in which the ring is b, resp. a (duplicate links count as often as they are given)
 * Output per link:  link_ok uint8, 1 where the link was accepted.
 * Output per track, by K19's / K22's capacity protocol: ntrack uint64 [1] is always written; with ntrack > capacity nothing else is written
 * -- no per-ring and no per-link array either -- and 1 is returned; with capacity == 0 every other output pointer may be NULL.  Row t:
 *   first_ring int64          the root itself
 *   first_step, last_step int32   min and max of ring_step over the track
 *   nrings int64              its rings
 *   nsplit, nmerge int64      its rings with nnext >= 2, resp. nprev >= 2
 * All reductions are integer atomics (add, min, max), and the fixed point root = the component's minimum is unique: link order and launch
 * geometry do not show in any word.  xc_cptrack.hip states the mapping: a parent array with parent[g] <= g, rounds of hook (atomicMin of
 * the larger root under the smaller, per accepted link) and compress until the host reads an unchanged round; no thread waits for another;
 * more than nring + 1 rounds is XC_EHIP.  The dense rank is a per-block count, the host's scan and a per-block ranking.  The call waits for
 * the stream as K22 does.  xc_last_cptrack_profile returns the rounds of the last call (the last, unchanged one included; 0 without links)
 * and, with xc_set_kernel_timing on, its device times in ms: ms[0] accept and degrees, ms[1] the rounds, ms[2] ranks, rows and copies. */
int xc_ring_tracks_dev(xc_ctx* ctx, int64_t nring, int64_t nlink,
                       const int32_t* ring_step, const int64_t* ring_size,            /* [nring] */
                       const int64_t* link_a, const int64_t* link_b, const int64_t* link_n,   /* [nlink] */
                       double min_overlap,
                       int64_t* root, int64_t* track, int32_t* nprev, int32_t* nnext,   /* [nring] */
                       uint8_t* link_ok,                                               /* [nlink] */
                       int64_t capacity, uint64_t* ntrack,
                       int64_t* first_ring, int32_t* first_step, int32_t* last_step, int64_t* nrings, int64_t* nsplit, int64_t* nmerge);
int xc_last_cptrack_profile(xc_ctx* ctx, double* ms, int* rounds);

/* ------------------------------------------------------------------ K24 contour folds: wave-breaking events
 * K16 says which meridians are overturned, K17 what the selected pieces bound.  The step after both (the Barnes and Hartmann 2012 kind
 * of analysis, where the reference's Subroutines 3-5 were heading): which runs of overturned meridians form one EVENT, where it sits,
 * how much has folded over in it, and which way it leans.  Build-defined; index space; the field is not read again.
 * Input exactly as for K17: count[nrange], e_from, e_to, pts where the K12 _dev entry points left them, ny, nx, periodic, select, ncont,
 * w, w_per_slab, f, f_dtype, with K17's limits and XC_EBADARG cases (2 ny nx < 2^31, edge ids in range, select != 0 needs periodic,
 * nrange % ncont == 0, at most 65535 slabs); nrange nx < 2^38; and gap, 0 <= gap < nx, else XC_EBADARG.  There is no flip.
 *   CROSSINGS      X[r][c], 0 <= r < ny - 1, and P[r][c] are K17's, bit for bit, under the same select.  For a column c:
 *                  n[c] = sum_r X[r][c] (K16's ncross on K12's records), lo[c] / hi[c] the smallest / largest r with X[r][c] = 1.
 *   FOLDED COLUMN  n[c] >= 3.
 *   FOLD NODES     of a folded column: the nodes (r, c), lo[c] < r <= hi[c] -- those between its lowest and its highest crossed edge.
 *                  Each belongs to a tongue t = P[r][c] ^ P[lo[c] + 1][c]: t = 0 'under' (air of the side beyond the lowest crossing,
 *                  lying under air of the near side), t = 1 'over' (air of the side of row 0, lying over it).  Neither depends on K17's flip.
 *   EVENT          a maximal set of folded columns in which consecutive folded columns are separated by at most `gap` unfolded columns;
 *                  on a periodic plane column nx - 1 is followed by column 0.  c_west is its first column (the gap + 1 columns in front
 *                  of it hold no folded column), c_east its last folded column.  A periodic range without such a first column (every
 *                  cyclic gap <= `gap`) is ONE event, c_west its smallest folded column, c_east the last one reached going east.  The
 *                  events of a range are ordered by c_west ascending; one that runs across the seam has c_east < c_west.
 *                  dx(c) = (c - c_west) mod nx for a column of the event.
 *   per (range, column), dense [nrange][nx], always fully written:
 *     ncross int32            n[c]
 *     row_lo, row_hi f64      K16's: the smallest / largest stored row (r1 of a start point, r2 of a tail) over the crossings of the
 *                             column, bit for bit; NaN where ncross == 0
 *     col_event int32         the index of the column's event within its range for a folded column, else -1 (an unfolded column
 *                             bridged by `gap` too)
 *   per event, packed by range (the events of range r are [eoff[r], eoff[r+1]), eoff the exclusive scan of event_count; inside a range
 *   in the order above):
 *     c_west, c_east int32    first column, last folded column
 *     ncol int32              its folded columns;   ncross_max int32   the largest ncross over them
 *     ev_row_lo, ev_row_hi f64   the min of row_lo / the max of row_hi over them, copied bit for bit
 *     nodes int64 [.][2]      the fold nodes of tongue t: nodes[2 e + t]; the five below are laid out alike
 *     area f64 [.][2]         the sum of w over them (w == NULL: weight 1); w as K17 reads it
 *     mx f64 [.][2]           the sum of w * (double)dx(c), each product rounded once
 *     my f64 [.][2]           the sum of w * (double)r, each product rounded once
 *     integral f64 [.][2]     the sum of w * f, each product rounded once, f32 widened first; NULL exactly when f is
 *   The float sums are K13's exact sums: every term whole into fixed-point limbs, rounded once -- independent of order, chunks, groups
 *   and launch geometry.  Each has a window of 160 bits under 2^top, top = 12 + the frexp exponent of a bound on one term, never below
 *   -800: with max |w| and max |w f| over the finite values of the range's slab as K17 takes them (all of the plane), the bound is
 *   max |w| for area, max |w| * nx for mx, max |w| * ny for my (the float64 product; one that overflows counts as the largest finite
 *   double), max |w f| for integral.  The bits of a term under 2^(top - 160) are cut off toward zero.  A NaN term is skipped; a +-inf
 *   term makes THAT sum of THAT tongue of THAT event NaN, and no other.
 *   event_count[nrange] and the dense column arrays are always written.  capacity >= sum(event_count): the event arrays are written,
 *   XC_OK.  Otherwise nothing is written to the event arrays and 1 is returned (capacity 0 with NULL event arrays = count only: the
 *   sums are then not computed, and w and f not read).  A range has at most ceil(nx / 2) events.
 *   On records that are not K12's every access still stays in bounds and every loop ends, as K16 and K17 promise: n[c] counts flags
 *   (an edge named twice counts once), the rows are taken over every crossing K16 would count.
 * The call waits for the stream twice (K12's counts; the event counts, with the word that says whether the ids were in range).  It
 * works in K13's groups of ranges under K13's cap and in K13's workspace (xc_set_cpiece_workspace; the result does not depend on it),
 * with K17's bit planes, two int32 per (range, column), 112 bytes per (range, possible event) and 340 per (range of a group, possible
 * event).  With xc_set_kernel_timing on, xc_last_cfold_profile returns the last call's device times in ms -- ms[0] edge tables, ms[1]
 * the doubling rounds, ms[2] per-piece sums and the selection (as K17), ms[3] the marks and the column pass, ms[4] the run pass, ms[5]
 * the fold scan and the finish (with the bounds of the windows and the compaction) -- the rounds summed over the groups, and the groups. */
int xc_contour_folds_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                         int64_t ny, int64_t nx, int periodic, int select, int ncont, const double* w, int w_per_slab, const void* f,
                         int f_dtype, int64_t gap,
                         int32_t* ncross, double* row_lo, double* row_hi, int32_t* col_event,                     /* [nrange][nx] */
                         int64_t capacity, uint64_t* event_count,                                                 /* [nrange] */
                         int32_t* c_west, int32_t* c_east, int32_t* ncol, int32_t* ncross_max, double* ev_row_lo, double* ev_row_hi,
                         int64_t* nodes, double* area, double* mx, double* my, double* integral);
int xc_last_cfold_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups);

/* ------------------------------------------------------------------ K25 contour map: contour vectors back on the plane
 * Everything above ends in contour space.  The way back -- the equivalent latitude of every node, nkeff painted onto the plane, the
 * displacement of a node from its equivalent coordinate -- is var(contour) evaluated at the tracer value of every node: the reference's
 * _interp1d(x, xf, yf, inc) (core.py:1405-1434) with x = q(node), xf = the levels, yf = the vector.  The reference only has the forward
 * direction (interp_to_coords, core.py:1050-1100); this call is build-defined.  One streaming pass: the tracer is read once, nv planes
 * are written.
 * Input:
 *   q            XC_F32 or XC_F64 [nslab][ny][nx]
 *   xp           f64 levels, [N] for all slabs (xp_per_slab == 0) or [nslab][N]; N >= 2
 *   nv           the number of value vectors, 1 <= nv <= XC_CMAP_MAXV
 *   fp[nv]       HOST array of pointers (device pointers in the _dev form), each f64 [N] or [nslab][N]
 *   fp_per_slab[nv]  HOST array: 0 one vector [N] shared by all slabs, non-zero [nslab][N]
 *   out[nv]      HOST array of pointers to the nv output planes, out_dtype [nslab][ny][nx] each
 *   out_dtype    XC_F64, or XC_F32: the float64 result rounded to float32 once
 * RULE       per slab s, node (r, c) and vector v, everything promoted to float64:
 *                rev = !(xp[s][0] < xp[s][N-1])                                          (core.py:1426-1430)
 *                out_v[s][r][c] = np.interp(q[s][r][c], X, F),  X, F = xp[s], fp_v[s], both reversed when rev is set
 *            bit for bit numpy's compiled arr_interp: below X[0] the result is F[0], above X[N-1] it is F[N-1]; a NaN q gives NaN;
 *            with j the largest index with X[j] <= q: j == N - 1 or q == X[j] gives F[j] itself; else with
 *            slope = (F[j+1] - F[j]) / (X[j+1] - X[j]) the result is slope * (q - X[j]) + F[j]; where that is NaN,
 *            slope * (q - X[j+1]) + F[j+1]; where that is NaN too and F[j+1] == F[j], F[j].  Every operation rounds once (no FMA).
 * LEVELS     strictly monotonic (either direction) and finite in every slab.  A slab whose xp[s][0] or xp[s][N-1] is NaN (the
 *            levels of an all-NaN tracer) gets NaN on every node.  The host form checks this first: two adjacent equal levels are
 *            XC_EEDGES with the reference's text 'non monotonic bins' (core.py:1233-1251); a slab that is not finite or not
 *            monotonic in the direction of its ends is XC_EBADARG.  The _dev form cannot read the levels and trusts its caller: on
 *            other levels the result is unspecified, but every access stays in bounds.
 * LIMITS     The levels and the vectors of a slab live in LDS: (nv + 1) * N <= XC_CMAP_MAX_LDS_DOUBLES (64 KiB: N = 3000 with
 *            nv <= 1, N = 201 with nv <= 8, N <= 4096 at all); more is XC_EBADARG.  At most 65535 slabs per call, as the other
 *            entries.  A workgroup walks tiles of XC_CMAP_TILE cells.  No alignment is asked of any pointer beyond its element's.
 * REFUSALS   XC_EBADARG with nothing written: a NULL pointer (q, xp, fp, fp_per_slab, out, or one of the first nv entries of fp or
 *            out), nslab, ny or nx < 1, N < 2, nv outside [1, XC_CMAP_MAXV], a dtype code that is neither XC_F32 nor XC_F64, and the
 *            two limits above.
 * The _dev form takes device pointers and only enqueues; the host form stages through the context's arena (a tracer with a device
 * mirror is read where it is) and returns with the planes in the caller's arrays.                                                    */
#define XC_CMAP_MAXV 8
#define XC_CMAP_MAX_LDS_DOUBLES 8192
#define XC_CMAP_TILE 1024
int xc_contour_map_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                       const double* xp, int N, int xp_per_slab,
                       int nv, const double* const* fp, const int* fp_per_slab, void* const* out, int out_dtype);
int xc_contour_map(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                   const double* xp, int N, int xp_per_slab,
                   int nv, const double* const* fp, const int* fp_per_slab, void* const* out, int out_dtype);

/* ------------------------------------------------------------------ K26 contour lengths at coarsened resolutions
 * The reference's fractal-dimension script (tests/test_fractal.py:60-73) measures every contour at the ruler strides 1, 2, 4, ... twice:
 * box-counting crossings (K9, all strides on one upload) and cal_contour_lengths of the block-averaged tracer, once per ratio.  The
 * `coarsen` it calls ships with neither project; this rule is build-defined.  One call coarsens the tracer on the GPU for every ratio and
 * hands each coarse plane to K10, which is unchanged.
 * RULE       ratio r >= 1, plane (ny, nx) -> coarse plane (ny / r, nx / r) (integer division): blocks start at index 0, trailing rows
 *            and columns that fill no block are dropped (trim).  Coarse node (I, J) is the mean of the fine block
 *            [I r, I r + r) x [J r, J r + r).  Every fine value is converted to float64 first (a float32 tracer too); the coarse plane
 *            is float64 always.  The block sum is sequential: each block row is summed left to right starting FROM its first element,
 *            then the row sums are added top to bottom starting FROM the first; the mean is that sum divided once by double(r r).
 *            Additions and one division, each rounded once: no multiplication that contraction could fuse, no reassociation.
 * NaN        skipna == 0: a block with a NaN node is NaN (land stays land).  skipna != 0: NaN nodes are left out of the same order, a
 *            row without a node left adds nothing, the divisor is the number of nodes used, a block with none is NaN.  An infinite node
 *            is an ordinary value in both modes.
 * COORDS     Yc[I] = (ycoord[I r] + ... + ycoord[I r + r - 1]) / double(r), the sum sequential from the first, in float64; Xc[J] the same.
 *            These are the coordinates as K10 gets them (the caller's casts and deg2rad done); nothing is cast again.
 * RATIO 1    the plane and the coordinates themselves: K10 reads the caller's buffers, nothing is copied.
 * PERIODIC   the period passes through unchanged and nx % r == 0 is required: otherwise the seam cell would swallow the trimmed columns.
 * xc_coarsen[_dev]: the kernel alone.  out is f64 [nslab][ny / r][nx / r].  XC_EBADARG: a NULL pointer, nslab, ny or nx < 1, a dtype
 *            that is neither XC_F32 nor XC_F64, a ratio outside 1 .. XC_CSCALE_MAXRATIO or one that leaves no coarse node, more than
 *            65535 slabs.
 * xc_contour_lengths_scales[_dev]: ratios[nratio] is a HOST array in both forms, 1 <= nratio <= XC_CSCALE_MAXR, in any order, repeats
 *            allowed.  period == 0.0: two free edges (as K15 has it), else periodic X.  out_len f64 [nratio][nslab][ncont]; out_nseg
 *            the same shape, may be NULL.  For every ratio they are, bit for bit, what xc_contour_lengths (xc_contour_lengths_periodic)
 *            returns for the coarse plane and the coarse coordinates of the rule above: the sums are K10's and as reproducible.
 *            Levels, coordinates, period and radius obey K10's conditions: the host form checks them as xc_contour_lengths does
 *            (XC_EEDGES for levels that do not ascend), the device form checks what it can without reading device memory.
 * REFUSALS   XC_EBADARG, the message naming the ratio, before anything is launched or written: a ratio outside
 *            1 .. XC_CSCALE_MAXRATIO; one that leaves fewer than 2 coarse rows; on a plain plane one that leaves fewer than 2 coarse
 *            columns; on a periodic plane one that does not divide nx.  Also nratio outside 1 .. XC_CSCALE_MAXR.
 * The coarse planes live in a workspace of the context sized by the largest of them and reused ratio after ratio on the context's
 * stream.  xc_last_clen_geometry reports the K10 launch of the last ratio.                                                           */
#define XC_CSCALE_MAXR 8
#define XC_CSCALE_MAXRATIO 64
int xc_coarsen_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx, int ratio, int skipna, double* out);
int xc_coarsen(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx, int ratio, int skipna, double* out);
int xc_contour_lengths_scales_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                  const double* ycoord, const double* xcoord, double period, double radius,
                                  const int* ratios, int nratio, int skipna,
                                  const double* contours, int ncont, int contours_per_slab, double* out_len, uint64_t* out_nseg);
int xc_contour_lengths_scales(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                              const double* ycoord, const double* xcoord, double period, double radius,
                              const int* ratios, int nratio, int skipna,
                              const double* contours, int ncont, int contours_per_slab, double* out_len, uint64_t* out_nseg);
/* how the last xc_coarsen(_dev) (nratio = 1) or xc_contour_lengths_scales(_dev) call launched k_coarsen, ratio by ratio in the caller's
 * order: a tile is tile_y x tile_x COARSE nodes, one workgroup of `block` threads each, grid (tiles in x, tiles in y, slabs).  A ratio
 * of 1 inside xc_contour_lengths_scales launches nothing: its grid and tile are 0.  All zero when the last such call failed.        */
typedef struct xc_cscale_geometry {
    int32_t q_dtype;    /* XC_F32 / XC_F64 */
    int32_t nratio;
    int32_t block;      /* threads per workgroup */
    int32_t ratio[XC_CSCALE_MAXR];
    int32_t grid_x[XC_CSCALE_MAXR], grid_y[XC_CSCALE_MAXR], grid_z[XC_CSCALE_MAXR];
    int32_t tile_y[XC_CSCALE_MAXR], tile_x[XC_CSCALE_MAXR];
} xc_cscale_geometry;
int xc_last_cscale_geometry(xc_ctx* ctx, xc_cscale_geometry* out);

/* ------------------------------------------------------------------ K27 contour distance: how far every node lies from a contour
 * K25 brings contour vectors back onto the plane; this brings the contour's GEOMETRY back: per node the distance to the selected pieces
 * of a contour, and which segment and which piece is nearest -- the cross-contour coordinate of front-relative composites.  The
 * reference's scripts trace a level and query a KD-tree on the host (tests/test_breaking.py, scipy.spatial).  Build-defined.
 * Input as for K13, K16 and K17: count[nrange], e_from, e_to, pts where the K12 _dev entry points left them, with ny, nx, periodic of that
 * call; ycoord[ny], xcoord[nx], period, radius with K13's meaning; select (0 all, 1 circumpolar, 2 main), pieces, rings, winding and the
 * tie rule of the main ring are K16's.  A record end point (rho, gamma) maps to coordinates exactly as K13 maps it: np.interp on the
 * coordinates, column nx of a periodic plane at xcoord[0] + period.  Node (r, c) is (ycoord[r], xcoord[c]).
 *   refused with XC_EBADARG, nothing written: select != 0 with periodic == 0; 2 ny nx >= 2^31; a range of 2^31 segments or more; an edge
 *     id (e_from or e_to) outside [0, 2 ny nx); a periodic plane without a finite, non-zero period or with nx < 2; radius > 0 with
 *     periodic != 0 and a period that is not +-(double)(float)(2 pi) = float64(deg2rad(float32(+-360))) -- the plane is then no sphere;
 *     a NaN max_dist.
 *   PLANE (radius == 0).  Segment a -> b, node p, every operation rounded once, in this order:
 *     u = b - a;  w = p - a;  uu = uy uy + ux ux;  t = 0 if uu == 0, else (wy uy + wx ux) / uu clamped to [0, 1];  f = a + t u;
 *     d2 = (py - fy) (py - fy) + (px - fx) (px - fx).
 *     With periodic != 0, d2 is the minimum over px, px + period and px - period.  dist = sqrt(min over the selected segments of d2).
 *   SPHERE (radius > 0, coordinates in radians).  Points are unit vectors (cos y cos x, cos y sin x, sin y); a candidate is compared by
 *     its squared chord c2, from arithmetic and sqrt alone:  n = a x (b - a) (the difference first: a short arc keeps its direction), nn = n . n;
 *     nn == 0: c2 = |p - a|^2;  else if (a x p) . n >= 0 and (p x b) . n >= 0 (the foot lies on the arc): s2 = (p . n)^2 / nn,
 *     c2 = 2 s2 / (1 + sqrt(1 - min(s2, 1)));  else c2 = min(|p - a|^2, |p - b|^2).  Products first, sums from the left.
 *     dist = radius * 2 asin(min(1, sqrt(min c2) / 2)): one asin per node.  No image shifts.
 *   per range, dense [nrange][ny][nx]:
 *     dist  f64    +inf where the range has no selected segment, and where max_dist > 0 (finite) and the distance exceeds it; max_dist
 *                  is in the units of dist; <= 0 or +inf: no cap
 *     edge  int64  (may be NULL) the e_from of the nearest selected segment -- unique within a range --; among segments whose d2 / c2 are
 *                  equal as bit patterns the smallest id; -1 wherever dist is infinite.  Its cell: row (id >> 1) / nx, column
 *                  (id >> 1) % nx; K14's e_from_walk turns it into the position along the polyline
 *     piece int64  (may be NULL) K13's first_edge of the piece of that segment; -1 where edge is
 *   negate_mask uint8 [nrange][ny][nx] or NULL: where it is 1, a finite dist changes sign (K17's mask makes the distance signed).
 *   min is order-free: no output depends on the order of the segments or of arrival, on the launch geometry or on the workspace cap.
 *   On XC_OK every output is fully written, whatever the records hold; there is no capacity protocol.
 * The selected segments of a range are binned by blocks of 32 x 32 cells; a workgroup owns 16 x 16 nodes and skips every block whose
 * conservative lower bound on the distance to its nodes exceeds what its nodes already have (or max_dist): the result is that of the
 * unpruned rule, bit for bit.  xc_set_cdist_prune(ctx, 0) visits every block (default 1; same result; for tests and A/B).
 * The call waits for the stream three times (K12's counts; the word that says whether the ids were in range, before anything is
 * written; the pair counts).  It works in K13's groups of ranges under K13's cap and in K13's workspace (xc_set_cpiece_workspace; the
 * result does not depend on it).  xc_last_cdist_profile returns of the last call: with xc_set_kernel_timing on the device times in ms --
 * ms[0] edge tables, doubling rounds and the selection, ms[1] the binning (count, scan, segment table, boxes), ms[2] the distance
 * pass --, then the (node, segment) pairs it evaluated, the pairs an unpruned call evaluates, and the number of groups.            */
int xc_contour_distance_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                            int64_t ny, int64_t nx, int periodic, int select, const double* ycoord, const double* xcoord, double period,
                            double radius, double max_dist, const uint8_t* negate_mask, double* dist, int64_t* edge, int64_t* piece);
int xc_set_cdist_prune(xc_ctx* ctx, int on);
int xc_last_cdist_profile(xc_ctx* ctx, double* ms, int64_t* pairs_visited, int64_t* pairs_total, int* groups);

/* ------------------------------------------------------------------ K28 contour distance profile: composites by distance
 * K27 gives the cross-contour coordinate as planes; the composite taken of it -- the mean of a field as a function of the (signed)
 * distance from the vortex edge -- is a histogram of those planes with weights.  This call bins every node's distance where it is made
 * and returns per (range, bin) the node count, the area and up to XC_PROPS_MAXF area-weighted field sums: no plane is an output, only
 * nrange x M numbers per quantity reach the caller.  Build-defined.
 * Input: everything xc_contour_distance_dev takes up to negate_mask, with the same meaning, limits and XC_EBADARG cases.  The distance d
 * of a node is K27's, bit for bit: the same search (one device function serves both kernels), after sqrt / asin, after the cap, after
 * the sign.  Further input:
 *   nedge, edges HOST array float64[nedge]: the bin edges in the units of dist; finite, strictly ascending, 2 <= nedge <= 4097, else
 *                XC_EBADARG before anything is written.  M = nedge - 1 bins per range.
 *   ncont        ranges per slab: range = s ncont + k; nrange is a multiple of ncont, nrange / ncont (at most 65535) the slabs of w and
 *                of the fields
 *   w, w_per_slab  K17's weights: double[ny][nx], or [nslab][ny][nx] with w_per_slab != 0; NULL is weight 1
 *   nf, f[nf], f_dtype[nf], f_per_slab[nf]  K21's fields: HOST arrays of device pointers, of XC_F32 / XC_F64, and of 0 (one plane
 *                [ny][nx] for all slabs) or non-zero ([nslab][ny][nx]); 0 <= nf <= XC_PROPS_MAXF
 *   BIN RULE     a node with distance d belongs to bin b when edges[b] <= d < edges[b + 1]; d == edges[M] belongs to bin M - 1
 *                (np.histogram's rule).  A node with d = +inf (a range without selected segment; beyond max_dist) belongs nowhere, and
 *                so does one outside [edges[0], edges[M]].
 *   per (range, bin), dense:
 *     nodes int64 [nrange][M]      the nodes of the bin, whatever their weights and fields hold
 *     area  f64   [nrange][M]      the sum of w over them
 *     sums  f64   [nf][nrange][M]  the sum of w f_m, each product rounded once (float32 fields widened first); NULL exactly when nf == 0
 *     flags int32 [nrange][1 + nf] channel 0 the area, 1 + m field m: 1 where a term of that channel at a node in a bin of that range was
 *                                  +-inf (a NaN term sets nothing, nor does a node in no bin)
 *   The sums are K17's: the exact sum of the float64 terms rounded once, a window of 160 bits under 2^top, top = 12 + the frexp exponent
 *   of max |w| (max |w f_m|) over the finite values of the range's slab.  A NaN term is skipped; a +-inf term makes THAT channel of THAT
 *   bin NaN (and sets the flag of its range and channel), and no other.  No output depends on the order of the segments or of arrival,
 *   on the launch geometry, on the workspace cap, on pruning or on the path below.  Ranges without segments have zero counts and sums.
 * The tile pass is K27's with an epilogue: a workgroup's 16 x 16 nodes find their bins by binary search (the edges in LDS up to 512 of
 * them, else through the cache); where they span at most 16 bins the terms are added to a window of LDS words with LDS integer atomics
 * and every non-zero word is flushed with one global 64-bit atomic; a wider tile adds every term to the global words.  The window and
 * the edges live in the LDS the search staged its segments in.  xc_set_cdprofile_global(ctx, 1) sends every tile down the global path
 * (default 0; same result; for tests and A/B); xc_set_cdist_prune applies as in K27.
 * Stream waits, groups and workspace are K27's; the words take 40 (1 + nf) + 12 bytes per (range, bin).  xc_last_cdprofile_profile
 * returns of the last call: with xc_set_kernel_timing on the device times in ms -- ms[0] to ms[2] as xc_last_cdist_profile (the
 * distance pass with the accumulation), ms[3] the bounds of the windows, ms[4] the finish pass --, K27's pair counts, the tiles that
 * took the LDS window and the tiles that took the global path (tiles without a node in any bin count in neither), and the groups.   */
int xc_contour_distance_profile_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                    const double* pts, int64_t ny, int64_t nx, int periodic, int select, const double* ycoord,
                                    const double* xcoord, double period, double radius, double max_dist, const uint8_t* negate_mask,
                                    int nedge, const double* edges, int ncont, const double* w, int w_per_slab, int nf, const void* const* f,
                                    const int* f_dtype, const int* f_per_slab, int64_t* nodes, double* area, double* sums, int32_t* flags);
int xc_set_cdprofile_global(xc_ctx* ctx, int on);
int xc_last_cdprofile_profile(xc_ctx* ctx, double* ms, int64_t* pairs_visited, int64_t* pairs_total, int64_t* tiles_window,
                              int64_t* tiles_global, int* groups);

/* ------------------------------------------------------------------ fused, batched Keff pipeline
 * The reference's call sequence SURVEY 3.1 steps 2-10 for a batch of slabs resident
 * in HBM: min/max -> levels/edges -> one histogram pass (dA, |grad q|^2 dA or grdS dA)
 * -> CDF -> table lookup -> d/dA -> Leq2 -> Lmin -> nkeff [-> interpolation to preY].
 * Replaces core.py:205-249, 412-460, 1136-1174, 463-488, 619-637, 945-966, 1050-1100
 * and utils.py:518-534.  Three kernel launches per batch, no host round trip.
 * All pointers are DEVICE pointers.  Outputs are double[nslab][N] unless noted and any
 * of them may be NULL except ctr/area.                                               */
typedef struct xc_keff_desc {
    const void*   q;            int32_t q_dtype;  int32_t ctr_dtype;
    int64_t       nslab, ny, nx;
    int32_t       N;            int32_t increase; int32_t lt; int32_t right_edge;
    const double* dA;           int32_t dA_rank;  int32_t grad;       /* grad: 1 in-kernel, 0 use grdS */
    const void*   grdS;         int32_t grdS_dtype; int32_t prod_f32;
    const double* rdx;          const double* rdy;  int32_t periodic_x; int32_t npre;
    const double* tbl;          /* double[ny] area table A(Yeq), ascending-coordinate order */
    const double* tbl_coord;    /* double[ny] ascending coordinate values                   */
    const double* preY;         /* double[npre] prescribed equivalent coordinates (or NULL) */
    double        nkeff_mask;   /* values >= this become NaN (reference default 1e5)        */
    double        lmin_scale;   /* 2*pi*R: Lmin = lmin_scale*cos(deg2rad(latEq))            */
    double*       ctr;          double* area;   double* intgrdS; double* latEq;
    double*       dqdA;         double* dintSdA; double* Leq2;   double* Lmin;  double* nkeff;
    uint64_t*     counts;       /* uint64[nslab][N]; NULL: not wanted -- the histogram pass then skips the count adds (a third of its LDS atomics) */
    double*       interp;       /* double[nslab][9][npre]: ctr, area, intgrdS, latEq, dintSdA, dqdA, Leq2, Lmin, nkeff on preY */
    int32_t*      status;       /* int32[nslab] 0 ok, 1 degenerate levels ('non monotonic bins', core.py:1233), 2 the single-read kernel gave up
                                   waiting for its workgroups (see single_read): nothing was computed for the slab */
    const void*   q_next;       /* optional: the batch the NEXT xc_keff_dev call will process (same dtype and
                                   shape, may equal q).  Its per-slab min/max partials are accumulated inside this
                                   call's histogram pass (+8 B/cell of loads, no extra kernel) and the next call on
                                   that pointer skips its K1 pass -- provided the batch is provably unchanged: the
                                   cached partials are dropped when xc_memcpy_h2d / xc_memset / xc_synth_dev / xc_free
                                   touch the batch, and whenever `q_gen` differs from the value given with q_next (a
                                   caller that writes the batch through its own pointer bumps q_gen).  NULL: off. */
    int32_t       dA_pos_finite;/* caller verified that every dA value is finite and >= 0: the kernel then skips the
                                   fillna(0) selects on the dA channel (optional speed-up; 0 is always safe) */
    int32_t       q_gen;        /* generation of the tracer buffers (see q_next): any change invalidates chained min/max */
    int32_t       deterministic;/* != 0: order-free fixed-point sums (below); q_next rides in their second pass */
    int32_t       out_stride;   /* doubles between consecutive slabs in each of the nine vector outputs (ctr ... nkeff); 0 = N
                                   (nine dense [nslab][N] arrays).  9 * N with ctr = base, area = base + N, ... lays the
                                   results out slab-major, [nslab][9][N] -- the block a rank hands to the one gather
                                   with no repacking pass.  counts / interp / status keep their dense layout. */
    double        dA_max;       /* deterministic sums only: the largest finite |dA| value, if the caller knows it (a static metric: computed once
                                   on the host); <= 0 or NaN: the library takes it from the device array with one extra min / max pass over dA per call */
    int32_t       single_read;  /* calls of ONE slab (the reference's own pattern: one (time, level) plane per call, tests/LWA.py:40-43;
                                   core.py:224-225 then 1307 per object): XC_SINGLE_AUTO (0) takes the single-read kernel -- min / max, levels and
                                   histogram in ONE launch with the slab held in registers between them, the tracer read once, then k_finalize --
                                   when grad = 1, the sums are not `deterministic` and the slab fits the chip's register tiles (3600 x 1801 does);
                                   XC_SINGLE_NEVER (1) keeps the min/max pass + histogram pass + finalize chain; XC_SINGLE_FORCE (2) takes the
                                   kernel for calls of TWO slabs too (measured slower there than the chain, 64.7 against 59.3 us: the two slabs
                                   run one after the other; kept for tests).  That kernel waits for ALL its workgroups to be resident at once;
                                   every wait is bounded (XC_KEFF_SINGLE_TIMEOUT_US, default 50 ms): when something else holds compute units
                                   for longer, status[slab] = 2 comes back, NOTHING is written to the slab's result vectors, and the caller
                                   repeats the call with XC_SINGLE_NEVER (pipeline.KeffPlan.fetch does). */
    int32_t       reserved0;
} xc_keff_desc;
#define XC_SINGLE_AUTO  0
#define XC_SINGLE_NEVER 1
#define XC_SINGLE_FORCE 2
int xc_keff_dev(xc_ctx* ctx, const xc_keff_desc* d);
/* which path the last xc_keff_dev call took: 0 the min/max + histogram + finalize chain (two reads of the tracer), 1 the single-read kernel */
int xc_last_keff_path(xc_ctx* ctx, int* out_path);
/* diagnostics of the single-read kernel: wall-clock stamps (100 MHz) of every workgroup at its phase boundaries, [2][CUs][slots] uint64 on
 * the device (enable = 0 frees them) */
int xc_dbg_single_stamps(xc_ctx* ctx, int enable, void** out_dev, int* out_slots);

/* K5 / K6 alone -- the Keff epilogue without the cell-touching passes (SURVEY 8b `xc_keff_epilogue`): from the per-bin sums of
 * dA and |grad q|^2 dA (the PDFs xc_hist returns, ascending-VALUE bin order, bin 0 = the dummy bin) to the nine Keff vectors.
 * Replaces, per slab: cumsum + `cdf[-1] - cdf` when not lt + reversal to level order (core.py:1320-1323, 454-455),
 * Table.lookup_coordinates (1136-1174), cal_gradient_wrt_area (463-488), cal_sqared_equivalent_length (619-637),
 * latitude_lengths_at (utils.py:518-534), cal_normalized_Keff (945-966) and, with npre > 0, interp_to_dataset (1050-1100).
 *   pdf   double[nslab][2][N]   channel 0: sum of dA per bin, channel 1: sum of integrand * dA per bin
 *   ctr   double[nslab][N]      the contour levels in LEVEL order (ctr_dtype: XC_F32 when they are float32 values: d/dk then
 *                               runs in float32 like np.gradient on a float32 array)
 *   tbl / tbl_coord  double[ntbl]  A(Yeq) table, ascending-coordinate order;  preY double[npre] or NULL
 *   outputs double[nslab][N] each (any may be NULL); interp double[nslab][9][npre] or NULL.
 * The _dev form takes device pointers and only enqueues; the host form stages through the context's arena. */
int xc_keff_epilogue_dev(xc_ctx* ctx, const double* pdf, const double* ctr, int ctr_dtype, int64_t nslab, int N,
                         int increase, int lt, const double* tbl, const double* tbl_coord, int ntbl,
                         const double* preY, int npre, double nkeff_mask, double lmin_scale,
                         double* area, double* intgrdS, double* latEq, double* dqdA, double* dintSdA,
                         double* Leq2, double* Lmin, double* nkeff, double* interp);
int xc_keff_epilogue(xc_ctx* ctx, const double* pdf, const double* ctr, int ctr_dtype, int64_t nslab, int N,
                     int increase, int lt, const double* tbl, const double* tbl_coord, int ntbl,
                     const double* preY, int npre, double nkeff_mask, double lmin_scale,
                     double* area, double* intgrdS, double* latEq, double* dqdA, double* dintSdA,
                     double* Leq2, double* Lmin, double* nkeff, double* interp);

/* time of the dominant kernel (the histogram pass) of the last xc_keff_dev / xc_hist_dev
 * call, from HIP events recorded on the context's stream around that launch only.
 * Enable with xc_set_kernel_timing(ctx, 1); xc_last_hist_ms waits for the launch.     */
int xc_set_kernel_timing(xc_ctx* ctx, int enable);
int xc_last_hist_ms(xc_ctx* ctx, float* out_ms);
/* which histogram kernel the last xc_hist / xc_hist_dev / xc_keff_dev call launched: its template arguments and its launch geometry, as
 * the launcher chose them on the host.  All zero when the last such call failed.                                                        */
typedef struct xc_hist_variant {
    int32_t kernel;     /* 0 none, 1 K3 (k_hist), 2 K3 with deterministic sums (k_hist, DET = 3), 3 K3S (k_keff_single, the single-read kernel) */
    int32_t q_dtype;    /* XC_F32 / XC_F64 */
    int32_t vec, nint, grad, da2d, next, fast, e32, det, wcnt;   /* template arguments (K3S: vec 2, grad 1, wcnt = counts wanted) */
    int32_t threads, ncopy, nstrip;                              /* both kernels: threads per block, LDS histogram copies, column strips */
    int32_t bps, xcd_map, nchunk;                                /* K3: blocks per slab, XCD-aware block order, row chunks of the strip-fastest order (0: off) */
    int32_t G, cps, rpc;                                         /* K3S: workgroups, chunks per strip, rows per chunk */
} xc_hist_variant;
int xc_last_hist_variant(xc_ctx* ctx, xc_hist_variant* out);
/* how the last xc_contour_lengths / xc_contour_lengths_dev call (or its _periodic form; or xc_contour_line_integrals(_dev): K15, whose copies take 16383 cells) launched K10, as the launcher chose it on the host.  All zero
 * when the last such call failed; bps = 0 (and bps_rule 0) when the plane has no cells.                                      */
#define XC_CLEN_BPS_SHARE    1   /* bps = 2048 / nslab: the launch's share of ~2048 blocks */
#define XC_CLEN_BPS_FLOOR    2   /* bps = 8: the floor under that share */
#define XC_CLEN_BPS_CAPACITY 3   /* bps = ceil(ntile / max_tiles): no LDS copy may receive more than 32767 cells */
#define XC_CLEN_BPS_NTILE    4   /* bps = ntile: no more blocks than tiles */
typedef struct xc_clen_geometry {
    int32_t q_dtype;    /* XC_F32 / XC_F64 */
    int32_t latlon;     /* 1 haversine (radius > 0), 0 hypot */
    int32_t N;          /* levels per slab */
    int32_t ncopy;      /* LDS accumulator copies per level: 8 / 4 / 2 / 1 */
    int32_t G;          /* levels per group (gridDim.z) */
    int32_t ngroup;     /* level groups: ceil(N / G) */
    int64_t ntile;      /* 32 x 252-cell tiles per slab */
    int32_t bps;        /* blocks per slab (gridDim.x) */
    int32_t bps_rule;   /* which XC_CLEN_BPS_* rule set bps; 0 when bps = 0 */
    int64_t nslab;      /* slabs in the launch (gridDim.y) */
} xc_clen_geometry;
int xc_last_clen_geometry(xc_ctx* ctx, xc_clen_geometry* out);
/* One-shot: record the caller's events (from xc_event_create) immediately before and after
 * the NEXT histogram launch instead of the context's own pair -- lets a benchmark time every
 * launch of a timed region without synchronising inside it.                              */
int xc_set_hist_events(xc_ctx* ctx, void* start_event, void* stop_event);

/* ------------------------------------------------------------------ X1  the one collective (RCCL over xGMI)
 * No reference call site (the reference has no multi-process path).  Independent slabs are
 * partitioned over one process per GPU; at the end of a job every rank contributes its block of
 * per-slab result vectors to ONE all-gather.  Rank 0 creates the 128-byte id, the launcher
 * distributes it (bench.py: torch.distributed store), every rank calls xc_comm_init.
 * xc_comm_allgather_dev enqueues ncclAllGather on the context's stream: `send` holds
 * bytes_per_rank bytes, `recv` nranks * bytes_per_rank (device pointers).                 */
int xc_comm_unique_id(xc_ctx* ctx, void* out_id128);
int xc_comm_init(xc_ctx* ctx, int nranks, int rank, const void* id128);
/* The same in two steps, for callers that put a deadline on the first contact with RCCL: ncclCommInitRank blocks until every rank has
 * joined, so it runs in a helper thread -- xc_comm_create touches NO context (device: the HIP device of the rank; err: the failure text),
 * xc_comm_attach hands the finished communicator to a context from the thread that owns it, xc_comm_release disposes of one that was
 * never attached (its creator stopped waiting). */
int xc_comm_create(int device, int nranks, int rank, const void* id128, void** out_comm, char* err, size_t errlen);
int xc_comm_attach(xc_ctx* ctx, void* comm, int nranks, int rank);
int xc_comm_release(void* comm);
/* What RCCL itself reports about the context's communicator (ncclCommCount, ncclCommUserRank, ncclCommCuDevice, ncclGetVersion, the
 * file librccl was loaded from): the evidence that a multi-GPU job's collective really spanned N ranks on N devices.
 * comm_count = 0: no RCCL communicator on this context (the gather runs on another carrier). */
typedef struct xc_comm_info_t {
    int32_t comm_count, comm_rank, comm_device, ctx_device;
    int32_t rccl_version, reserved0;
    char    rccl_path[256];
} xc_comm_info_t;
int xc_comm_info(xc_ctx* ctx, xc_comm_info_t* out);
int xc_comm_allgather_dev(xc_ctx* ctx, const void* send, void* recv, size_t bytes_per_rank);
int xc_comm_finalize(xc_ctx* ctx);
/* Gather to ONE root (north_star: "RCCL gather"; SURVEY 8e "or gather-to-root"): every rank's `bytes` at `send` arrive at
 * recv + r * rank_stride on rank `root` (grouped ncclSend / ncclRecv; the root's own block is a device-to-device copy).  Moves
 * 1 / nranks of the all-gather's bytes.  Enqueued on the context's COMM stream (below), not on the compute stream. */
int xc_comm_gather_dev(xc_ctx* ctx, const void* send, size_t bytes, void* recv, size_t rank_stride, int root);
/* Give up on a communicator whose collective does not finish (ncclCommAbort): the first contact with RCCL on a new node runs
 * under a deadline (bench.py), and a job must be able to move on to the next carrier instead of hanging. */
int xc_comm_abort(xc_ctx* ctx);

/* The COMM stream: a third HIP stream of the context (beside compute and upload), created on first use.  A rank's result
 * block leaves on it -- an RCCL send or a device-to-device push -- while the next launch set computes.
 *   xc_comm_wait_compute  everything enqueued on the comm stream AFTER the call waits for the compute work enqueued so far
 *   xc_compute_wait_comm  later compute-stream work (and therefore xc_sync) waits for the comm work enqueued so far
 *   xc_comm_memcpy_d2d    device-to-device copy on the comm stream (dst may be another process's memory opened by xc_ipc_open)
 *   xc_streams_idle       *out_idle = 1 once both streams have drained, 0 while they have not; never blocks */
int xc_comm_wait_compute(xc_ctx* ctx);
int xc_compute_wait_comm(xc_ctx* ctx);
int xc_comm_memcpy_d2d(xc_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
int xc_streams_idle(xc_ctx* ctx, int* out_idle);

/* HIP IPC carrier of the same gather (no RCCL involved; no reference call site): the root exports the base pointer of its
 * receive buffer (an xc_malloc allocation) as a 64-byte handle, the rendezvous hands it to every rank, every rank opens it
 * and pushes its block with xc_comm_memcpy_d2d -- a peer write over xGMI between GPUs, a plain copy between ranks that share
 * one GPU.  Needs dmabuf IPC: HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment on this driver stack (see bench.py).
 *   xc_ipc_export  handle of the ALLOCATION that starts at dptr        xc_ipc_open  map it (returns its base address)
 *   xc_ipc_close   unmap (drains the comm stream first)                xc_device_can_access_peer  hipDeviceCanAccessPeer */
int xc_ipc_export(xc_ctx* ctx, const void* dptr, void* out_handle64);
int xc_ipc_open(xc_ctx* ctx, const void* handle64, void** out_dptr);
int xc_ipc_close(xc_ctx* ctx, void* dptr);
int xc_device_can_access_peer(int device, int peer, int* out_can);

/* ------------------------------------------------------------------ host-only helpers of the facade (no context, no device)
 * d(var)/d(area) along the contour index -- cal_gradient_wrt_area (core.py:463-488): np.gradient of both arguments against their
 * contour coordinate (uniform spacing, edge_order 1) and the quotient, numpy's arithmetic operation for operation and dtype for dtype
 * (float32 stays float32 until it meets a float64).  var: nlead rows of n values, var_row_stride ELEMENTS apart (a row of a larger result
 * array is fine), area: area_rows = nlead or 1 rows (one area profile for every row), area_row_stride apart; the two coordinates: [n] each;
 * out: [nlead][n], dense, in the WIDER of the two dtypes.
 * Returns XC_OK, XC_EBADARG, or 1 when a coordinate is not equally spaced (or is float64 under a float32 array): nothing was written,
 * the caller takes np.gradient's general branch. */
int xc_host_gradient_wrt_area(const void* var, int var_dtype, const void* var_coord, int var_coord_dtype,
                              const void* area, int area_dtype, const void* area_coord, int area_coord_dtype,
                              int64_t nlead, int64_t n, int64_t area_rows, int64_t var_row_stride, int64_t area_row_stride, void* out);

/* Histogram edges from contour levels, the way _histogram prepares them (core.py:1296-1305: a dummy first edge one mean step below the
 * lowest level) plus xhistogram's `last edge + 1e-8` when right_edge = XC_EDGE_XHISTOGRAM -- both evaluated in the levels' OWN dtype --
 * for a stack: levels levels_dtype[nslab][N] in level order -> out_edges double[nslab][N + 1] ascending; *out_increasing = 1 when the
 * levels ascend (the direction of slab 0; a slab running the other way is an error unless it holds a NaN).  Errors, with the
 * reference's texts in xc_last_error(NULL): XC_EEDGES 'non monotonic bins' (two adjacent levels coincide, core.py:1233-1251),
 * XC_EBADARG 'need at least two contour levels' / 'not every time or level is increasing/decreasing'. */
int xc_host_edges_from_levels(const void* levels, int levels_dtype, int64_t nslab, int64_t N, int right_edge,
                              double* out_edges, int* out_increasing);

/* The directed segments of K12 joined into polylines (host only; compiles without HIP).  nrange ranges (one per (slab,
 * contour)), range r = segments [off[r], off[r+1]) of e_from / e_to, off[0] = 0.  Per range: next(i) is the segment whose
 * e_from == e_to[i], prev(i) the one whose e_to == e_from[i] (sort + binary search on the edge ids); a segment without prev heads
 * an OPEN polyline; every remaining segment lies on a RING, which starts at its segment of smallest e_from; the polylines of a
 * range are ordered by the smallest e_from they contain.
 *   order[total]               global segment indices, polyline by polyline, in walk order (total = off[nrange])
 *   poly_off[total + 1]        polyline p = order[poly_off[p] .. poly_off[p+1])   (capacity total + 1; npoly + 1 entries written)
 *   poly_closed[total]         1 for a ring, 0 for an open polyline                (capacity total; npoly entries written)
 *   range_poly_off[nrange + 1] the polylines of range r are [range_poly_off[r], range_poly_off[r+1]); npoly = the last entry
 * XC_EBADARG: a duplicate e_from or a duplicate e_to within a range (such input is never walked), descending off, NULL arrays. */
int xc_join_segments(int64_t nrange, const int64_t* off, const int64_t* e_from, const int64_t* e_to,
                     int64_t* order, int64_t* poly_off, uint8_t* poly_closed, int64_t* range_poly_off);

/* ------------------------------------------------------------------ synthetic slabs (bench / tests)
 * PV-like tracer q = sin(phi) + 0.25 sum_k a_k cos(k lambda + theta_k) cos^2(phi) + 0.02 eps
 * generated on device from a counter-based RNG.  variant 0: PV-like,
 * 1: pure noise, 2: sin(phi) only.  out: q_dtype[nslab][ny][nx]; slab s uses seed+s. */
int xc_synth_dev(xc_ctx* ctx, void* out, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                 const double* lat_deg, const double* lon_deg, uint64_t seed, int variant);

#ifdef __cplusplus
}
#endif
#endif /* XCONTOUR_HIP_H */
