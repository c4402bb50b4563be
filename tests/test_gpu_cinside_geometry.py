"""K17's scan (k_ci_chunk, k_ci_scan of xc_cinside.hip) at the cuts of its launch geometry, against cinside_ref.interior: the cap of 64
chunks of rows, a last chunk of one row, several column blocks of 256 together with many chunks, one chunk alone (k_ci_chunk not
launched), long chunks over a partly filled bit-plane word -- and a call without any segment.  The shapes of the records suite
(test_gpu_cinside_records.py) all have one column block, or at most two chunks beside two blocks.

cinside_ref.scan_geometry restates the four lines of launch_contour_interior that fix the geometry; the tests use it ONLY to assert that
a shape lands in the regime its name claims, so that a later change of the launch constants cannot silently turn these tests into
repeats of the old ones.  Every expected value comes from cinside_ref.interior.  The records are K12's own (Context.contour_segments)
on noise with NaN cells, or a hand-built band whose crossings in the columns at the word, wave and block boundaries lie on rows of
their own."""
import numpy as np
import pytest

import cinside_ref as IR
import test_gpu_cinside_records as T17
import test_gpu_cpinside_records as T18
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

# (ny, nx, nslab, nlev) -> the regime the shape must show: nrange = nslab * nlev
SHAPES = {
    (256, 5, 1, 1): dict(ncb=1, nchunk=64, rc=4, last=4),                    # nchunk = 64 = the cap, the shortest chunks
    (320, 5, 1, 1): dict(ncb=1, nchunk=64, rc=5, last=5),                    # the cap binds: 80 chunks of 4 rows would fit
    (261, 5, 1, 1): dict(ncb=1, nchunk=53, rc=5, last=1),                    # a last chunk of one row
    (261, 257, 2, 1): dict(ncb=2, nchunk=53, rc=5, last=1),                  # two column blocks, the second of one column
    (41, 513, 1, 3): dict(ncb=3, nchunk=9, rc=5, last=1),                    # three column blocks, nx = 2 x 256 + 1
    (7, 513, 3, 1): dict(ncb=3, nchunk=1, rc=7, last=7),                     # one chunk: k_ci_chunk is not launched
    (1025, 3, 1, 1): dict(ncb=1, nchunk=61, rc=17, last=5, wpr=1),           # long chunks, one partly filled word
}
IDS = ['%dx%d-%dx%d' % k for k in SHAPES]


def regime(ny, nx, nrange):
    g = IR.scan_geometry(ny, nx, nrange)
    assert (g['nchunk'] - 1) * g['rc'] + g['last'] == ny and 1 <= g['last'] <= g['rc'] and g['nchunk'] <= IR.CI_MAX_CHUNKS
    return g


@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
@pytest.mark.parametrize('shape', list(SHAPES), ids=IDS)
def test_k12_records_on_noise_at_every_cut_of_the_scan(ctx, shape, periodic):
    """selects 0 and 2, both flips, with and without the mask, w per slab and a float32 f, one group and one range per group"""
    ny, nx, nslab, nlev = shape
    g = regime(ny, nx, nslab * nlev)
    assert {k: g[k] for k in SHAPES[shape]} == SHAPES[shape]
    q = T17.field((ny, nx), nslab, 300 + ny + nx, nan=True)
    lv = np.array([0.1]) if nlev == 1 else np.array([-0.6, 0.1, 0.9])
    rng = np.random.default_rng(301 + nx)
    w, f = T17.scaled(rng, (nslab, ny, nx)), T17.scaled(rng, (nslab, ny, nx), np.float32)
    cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=bool(periodic))
    rec = (cnt.ravel(), ef, et, pts)
    assert (cnt > 0).all()
    for select in (0, 2) if periodic else (0,):
        for flip in (0, 1):
            got, ref = T17.check(ctx, rec, ny, nx, periodic, select, flip, nlev, 'noise %r' % (shape,), w=w, f=f)
            for kw in (dict(cap=1), dict(want_mask=False), dict(cap=1, want_mask=False)):
                other = T17.run(ctx, rec, ny, nx, periodic, select, flip, nlev, w=w, f=f, **kw)
                assert T17.differences(other, got) == [], (select, flip, kw)
            assert np.array_equal(got['n_in'], got['mask'].reshape(nslab * nlev, -1).sum(axis=1))
            assert select != 0 or (0 < got['n_in'].min() and got['n_in'].max() < ny * nx)


def band_columns(nx):
    """the last bit of a bit-plane word and the first of the next; of a wave; of a block of 256 columns; the last column"""
    return tuple(dict.fromkeys((31, 32, 63, 64, 255, 256, nx - 1)))


def band(ny, nx, rc, step=False):
    """q = 1 on a band of rows [h[c], h[c] + thick) and 0 elsewhere: two crossings per column (step: on every row from h[c] on, one
    crossing per column and, on a ring of columns, ONE ring round the plane).  The upper crossing lies on row h[c] - 1; in the named
    columns every one on a row of its own, column 31's on the LAST row of chunk 0, column 32's on the FIRST row of chunk 1 (where the
    plane has more than one chunk) -> (q, the rows of the upper crossings of the named columns)"""
    thick = 2 if ny < 12 else 7
    room = ny - thick - 2
    h = np.full(nx, 1 + room // 2)
    cols = band_columns(nx)
    for k, c in enumerate(cols):
        h[c] = 1 + (rc - 1 + k) % room if rc < ny else 1 + k % room
    q = np.zeros((ny, nx))
    for c in range(nx):
        q[h[c]:(ny if step else h[c] + thick), c] = 1.0
    return q, [int(h[c]) - 1 for c in cols]


@pytest.mark.parametrize('step', [False, True], ids=['band', 'step'])
@pytest.mark.parametrize('shape', [s for s in SHAPES if s[1] >= 257], ids=[i for i, s in zip(IDS, SHAPES) if s[1] >= 257])
def test_crossings_at_the_word_wave_and_block_boundaries_on_rows_of_their_own(ctx, shape, step):
    """the prefix parity from cpar and the walk inside a chunk each have to get these columns right.  The band: select 0 on both planes
    against the reference and the threshold identity; the step: select 2 as well, its one ring round the plane being the main ring"""
    ny, nx, nslab, nlev = shape
    g = regime(ny, nx, nslab * nlev)
    q, rows = band(ny, nx, g['rc'], step)
    cols = band_columns(nx)
    if g['nchunk'] > 1:
        assert len(set(rows)) == len(rows) == len(cols)
        assert rows[0] == g['rc'] - 1 and rows[1] == g['rc']                 # the last row of chunk 0, the first of chunk 1
        assert len({r // g['rc'] for r in rows}) >= 2
    lv = np.array([0.5]) if nlev == 1 else np.array([0.25, 0.5, 0.75])
    qs = np.repeat(q[None], nslab, axis=0)
    above = q > 0.5
    for periodic in (0, 1):
        cnt, ef, et, pts = ctx.contour_segments(qs, lv, periodic=bool(periodic))
        rec = (cnt.ravel(), ef, et, pts)
        for select in (0, 2) if periodic and step else (0,):
            for flip in (0, 1):
                got, ref = T17.check(ctx, rec, ny, nx, periodic, select, flip, nlev, 'band %r' % (shape,))
                one = T17.run(ctx, rec, ny, nx, periodic, select, flip, nlev, cap=1)
                assert T17.differences(one, got) == []
                assert all(ref['X'][k, r, c] == 1 for r, c in zip(rows, cols) for k in range(nslab * nlev))
                assert ref['X'].sum() == nslab * nlev * nx * (1 if step else 2)
                for m in got['mask'].astype(bool):
                    assert np.array_equal(m, (above ^ above[:1]) ^ bool(flip))    # the threshold identity of a NaN-free field


@pytest.mark.parametrize('null_records', [False, True], ids=['records given', 'records NULL'])
def test_a_call_without_any_segment(ctx, null_records):
    """every level lies outside the field: no group, every range scanned by the trailing scan alone.  K17: XC_OK, the mask is all flip,
    n_in is 0 or ny nx, the sums are those of the reference, every output is written and every guard intact.  K18: XC_OK, piece_count all
    zero, the record arrays untouched"""
    ny, nx, nslab = 41, 513, 2
    q = T17.field((ny, nx), nslab, 310)
    lv = np.array([-50.0, 50.0])
    rng = np.random.default_rng(311)
    w, f = T17.scaled(rng, (nslab, ny, nx)), T17.scaled(rng, (nslab, ny, nx), np.float32)
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 4)))
    for periodic in (0, 1):
        cnt, ef, et, pts = ctx.contour_segments(q, lv, periodic=bool(periodic))
        assert cnt.shape == (nslab, 2) and not cnt.any() and ef.size == 0
        for flip in (0, 1):
            for select in (0, 2) if periodic else (0,):
                for kw in (dict(w=w, f=f), dict(), dict(w=w[0], f=None, want_mask=False)):
                    rc, got, untouched = T17.call(ctx, cnt.ravel(), *none, ny, nx, periodic, select, flip, 2, null_records=null_records, **kw)
                    assert rc == nat.XC_OK and not untouched
                    ref = IR.interior(cnt.ravel(), *none, ny, nx, periodic, select, flip=flip, ncont=2, w=kw.get('w'), f=kw.get('f'))
                    assert T17.differences(got, ref) == [], (periodic, select, flip, sorted(kw))
                    assert got['n_in'].tolist() == [ny * nx * flip] * 4
                    if kw.get('want_mask', True):
                        assert (got['mask'] == flip).all()
            for kw in (dict(w=w, f=f), dict()):
                rc, pc, cols, untouched = T18.call(ctx, cnt.ravel(), *none, ny, nx, periodic, flip, 2, capacity=8, null_inputs=null_records, **kw)
                assert rc == nat.XC_OK and pc.tolist() == [0] * 4 and untouched and all(c.size == 0 for c in cols)
            rc, pc, _, untouched = T18.call(ctx, cnt.ravel(), *none, ny, nx, periodic, flip, 2, capacity=0, null_records=True, null_inputs=null_records)
            assert rc == nat.XC_OK and pc.tolist() == [0] * 4 and untouched
