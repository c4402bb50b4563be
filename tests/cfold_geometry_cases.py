"""The planes behind test_gpu_cfold_geometry.py, shared with test_cfold_geometry_host.py -- a helper, no tests here.  cfold_ref.cases()
shows that K24's RULE is right; these planes sit on the boundaries of its LAUNCH GEOMETRY (xc_cfold.hip): the waves of 64 and the tiles
of 256 columns of the run pass (cf_tile, k_cf_runs), the carries `last` / `heads` across tiles, the seam renumbering with three and more
heads, the emax = ceil(nx / 2) staging slots of a range, the events of one wave of the fold scan (k_cf_scan's `todo` loop), events whose
limbs several waves and workgroups add up, the chunks of rows (one chunk: k_ci_chunk is not launched and cpar stays unused), and calls
of hundreds of ranges (k_cf_offsets' runs of ranges per thread, k_cf_compact's search).

Built with cfold_ref.plane / hook and ONE-CELL BLOBS: m[r, c] = 1 above the base ring under select 0 (all) folds exactly column c -- two
crossings of its own plus the base ring's.  Blobs in neighbouring columns form one blob, every column of which is folded.

cases(): name -> Case(masks, periodic, select, gap, ncont, tag, events, pins)
  masks    the planes of the call's ranges, one uint8 (ny, nx) each, None for a range without segments
  tag      what the case pins, in words
  events   per range the events the planes were drawn with: [(c_west, c_east, ncol)]
  pins     what test_cfold_geometry_host.py must find besides, by key:
             'apart': (a, b)        two consecutive events have the unfolded columns a .. b between them
             'bridged': (a, b)      one event has the unfolded columns a .. b inside it
             'straddles': c         one event has folded columns on both sides of c - 1 | c, without going round the seam
             'full': True           range 0 has event_count == emax
             'wave events': n       every full wave of range 0 holds n events
             'nchunk', 'rc'         cinside_ref.scan_geometry of the call
             'cut': n               the fold nodes of a folded column lie in at least n chunks of rows
             'opens': True          lo + 1 of a fold is the first row of a chunk behind the first
             'closes': True         hi of a fold is the last row of a chunk in front of the last
             'ncross': n            the folded columns have n crossings
             'chunk0': n            ... n of them in the first chunk of rows
             'wrong': (..)          the rules of cfold_ref.WRONG that must change the result
             'next': name           the case with gap + 1 on the same planes: another number of events
No expected value of a GPU test comes from here: the GPU tests take theirs from cfold_ref.folds."""
import collections
import functools

import numpy as np

import cfold_ref as FR

Case = collections.namedtuple('Case', 'masks periodic select gap ncont tag events pins')
JOINS = ('gap ignored', 'bridged columns labelled')                          # what a gap that joins two runs must tell
SEAM = ('no seam join', 'dx without mod') + JOINS                            # ... and a join round the seam


def blobs(ny, nx, cols, row=3, base=6):
    """one-cell blobs (columns next to each other: one blob) on row `row` over a base ring at `base`"""
    assert 0 < row < base - 1 < ny - 1
    m = FR.plane(ny, nx, base)
    m[row, list(cols)] = 1
    return m


def hook3(nx):
    """cfold_ref's 'hook of 3' on nx columns"""
    return FR.hook(FR.plane(9, nx, 6), (3, 4), 5, 2, 4, 6)


def singles(cols):
    return [(c, c, 1) for c in cols]


def tall():
    """61 x 8: three hooks over columns 3, 4: crossings on the rows 2, 5, 20, 33, 40, 42, 54.  The fold nodes 3 .. 54 lie in the chunks
    0 .. 10 of 5 rows; chunk 0 holds ONE crossing, so its cpar word counts in every later chunk, chunk 8 holds two (rows 40, 42), whose
    cpar bits cancel"""
    m = FR.plane(61, 8, 55)
    for top, bottom in ((3, 6), (21, 34), (41, 43)):
        FR.hook(m, (3, 4), 5, top, bottom, 55)
    return m


MANY = 300                                                                   # the ranges of the 'many ranges' case


def many_planes():
    """300 ranges of 7 x 8: every third one without segments, the others hook, seam hook, no fold in turn"""
    kinds = (FR.hook(FR.plane(7, 8, 5), (3, 4), 5, 1, 3, 5), FR.hook(FR.plane(7, 8, 5), (7, 0), 1, 1, 3, 5), FR.plane(7, 8, 4))
    drawn = ([(3, 4, 2)], [(7, 0, 2)], [])
    masks, events, k = [], [], 0
    for r in range(MANY):
        if r % 3 == 2:
            masks.append(None); events.append([])
        else:
            masks.append(kinds[k % 3]); events.append(drawn[k % 3])
            k += 1
    return masks, events


@functools.lru_cache(maxsize=None)
def cases():
    C = {}

    def add(name, masks, periodic, select, gap, tag, events, ncont=1, **pins):
        masks = list(masks) if isinstance(masks, (list, tuple)) else [masks]
        events = events if len(masks) > 1 else [events]
        assert name not in C and len(events) == len(masks)
        C[name] = Case(masks, periodic, select, gap, ncont, tag, events, pins)

    # ---- gap on an edge: the max-scan of the previous folded column across a wave (63 | 64) and across a tile (255 | 256, 511 | 512)
    for a, edge in ((62, 'wave edge 63|64'), (254, 'tile edge 255|256'), (510, 'tile edge 511|512')):
        m = blobs(9, 520, (a, a + 3))
        add('%d and %d, gap 1' % (a, a + 3), m, 1, 0, 1, 'two unfolded columns over the %s against gap + 1: two heads' % edge,
            singles((a, a + 3)), apart=(a + 1, a + 2), next='%d and %d, gap 2' % (a, a + 3))
        add('%d and %d, gap 2' % (a, a + 3), m, 1, 0, 2, 'prev comes over the %s: one head' % edge, [(a, a + 3, 2)],
            bridged=(a + 1, a + 2), straddles=a + 2, wrong=JOINS)
        add('%d next to %d' % (a + 1, a + 2), blobs(9, 520, (a + 1, a + 2)), 1, 0, 0, 'a run over the %s at gap 0: one head' % edge,
            [(a + 1, a + 2, 2)], straddles=a + 2)

    # ---- empty waves: `before` over ALL the waves in front, not the neighbouring one alone (one tile; folded columns in waves 0 and 3)
    far = blobs(9, 201, (10, 200))
    add('empty waves, gap 188', far, 0, 0, 188, '189 unfolded columns and two empty waves between two heads', singles((10, 200)),
        apart=(11, 199), next='empty waves, gap 189')
    add('empty waves, gap 189', far, 0, 0, 189, 'prev comes over two empty waves of one tile: one head', [(10, 200, 2)], bridged=(11, 199),
        wrong=JOINS)

    # ---- empty tiles: the carry `last` through tiles without folded column (four tiles, folded columns in tiles 0, 1 and 3)
    two, three = blobs(9, 1000, (10, 900)), blobs(9, 1000, (10, 500, 900))
    add('empty tiles, plain, gap 888', two, 0, 0, 888, '889 unfolded columns and two empty tiles between two heads', singles((10, 900)),
        apart=(11, 899), next='empty tiles, plain, gap 889')
    add('empty tiles, plain, gap 889', two, 0, 0, 889, '`last` carried through two empty tiles: one head; F + nx - L - 1 <= gap on a plain '
        'plane', [(10, 900, 2)], bridged=(11, 899), wrong=JOINS)
    add('empty tiles, ring, gap 108', three, 1, 0, 108, 'cyclic gap 109 against gap + 1 with K = 3: no join', singles((10, 500, 900)),
        apart=(501, 899), next='empty tiles, ring, gap 109')
    add('empty tiles, ring, gap 109', three, 1, 0, 109, 'F + nx - L - 1 == gap with K = 3: lin 0 -> K - 2', [(500, 500, 1), (900, 10, 2)],
        apart=(501, 899), wrong=SEAM)

    # ---- the seam with K >= 3: four runs, the first from column 1, the last up to nx - 2, one over the tile edge
    runs4 = blobs(9, 300, (1, 2, 100, 254, 255, 256, 257, 297, 298))
    drawn4 = [(1, 2, 2), (100, 100, 1), (254, 257, 4), (297, 298, 2)]
    add('four runs, ring, gap 1', runs4, 1, 0, 1, 'cyclic gap 2 against gap + 1 with K = 4: no join', drawn4, apart=(299, 0),
        next='four runs, ring, gap 2')
    add('four runs, ring, gap 2', runs4, 1, 0, 2, 'the seam renumbering lin == 0 ? K - 2 : lin - 1 with K = 4; the joined event last',
        drawn4[1:3] + [(297, 2, 4)], straddles=256, wrong=SEAM)
    add('four runs, plain, gap 2', runs4, 0, 0, 2, 'F + nx - L - 1 <= gap on a plain plane: wrap == 0 does not join', drawn4, straddles=256)

    # ---- full slots: emax events in range 0, a checked range behind it; 32 events in every wave of the scan
    for nx in (9, 65, 513):
        even, odd = list(range(0, nx, 2)), list(range(1, nx - 1, 2))
        pins = {'wave events': 32} if nx > 64 else {}
        add('comb, plain, nx %d' % nx, [blobs(9, nx, even), hook3(nx)], 0, 0, 0, 'event_count == emax: the last slot of the range, '
            'the next range behind it' + ('; 32 passes of the todo loop per wave' if nx > 64 else ''), [singles(even), [(3, 4, 2)]],
            full=True, **pins)
        ring = [blobs(9, nx, odd), hook3(nx)]
        add('comb, ring, nx %d' % nx, ring, 1, 0, 0, 'emax - 1 events on a ring, two unfolded columns at the '
            'seam', [singles(odd), [(3, 4, 2)]], next='comb, ring, nx %d, gap 1' % nx, **pins)
        add('comb, ring, nx %d, gap 1' % nx, ring, 1, 0, 1, 'one head in the first tile, none behind: K = 1 '
            'never joins', [[(1, nx - 2, len(odd))], [(3, 4, 2)]], wrong=JOINS)

    # ---- wide events: the limbs of one event added up by several waves and workgroups
    wide = FR.hook(FR.plane(9, 320, 6), range(40, 301), 301, 2, 4, 6)
    add('wide hook', wide, 1, 2, 0, 'one event over five waves of two blocks of the scan', [(40, 300, 261)], straddles=256)
    band = FR.plane(9, 600, 6)
    band[2:4] = 1
    add('every column folded, nx 600, ring', band, 1, 0, 0, 'one event of three tiles from c_west = 0: one head, K = 1', [(0, 599, 600)],
        straddles=512)
    add('every column folded, nx 600, plain', band, 0, 0, 0, 'one event of three tiles on a plain plane', [(0, 599, 600)], straddles=512)

    # ---- rows
    add('ny 7', FR.hook(FR.plane(7, 8, 5), (3, 4), 5, 1, 3, 5), 1, 2, 0, 'one chunk of rows: k_ci_chunk not launched, cpar unused',
        [(3, 4, 2)], nchunk=1, rc=7)
    add('ny 61', tall(), 1, 2, 0, 'seven crossings, the fold in eleven chunks: t = !P[row0] from up to ten cpar words, the first one '
        'included; two flips in one chunk', [(3, 4, 2)], nchunk=13, rc=5, cut=11, ncross=7)
    add('ny 8, lo + 1 opens chunk 1', FR.hook(FR.plane(8, 8, 6), (3, 4), 5, 4, 5, 6), 1, 2, 0, 'row0 == lo + 1: t starts at 0 without '
        'cpar', [(3, 4, 2)], nchunk=2, rc=4, opens=True)
    add('ny 8, hi closes chunk 0', FR.hook(FR.plane(8, 8, 4), (3, 4), 5, 2, 3, 4), 1, 2, 0, 'hi == row0 + rc - 1: chunk 1 has no node',
        [(3, 4, 2)], nchunk=2, rc=4, closes=True)
    add('ny 12, the fold is chunk 1', FR.hook(FR.plane(12, 8, 8), (3, 4), 5, 4, 6, 8), 1, 2, 0, 'lo + 1 and hi are the first and last '
        'row of the middle chunk', [(3, 4, 2)], nchunk=3, rc=4, opens=True, closes=True)
    add('ny 12, lo + 1 opens chunk 2', FR.hook(FR.plane(12, 8, 10), (3, 4), 5, 8, 9, 10), 1, 2, 0, 'row0 == lo + 1 in the last chunk',
        [(3, 4, 2)], nchunk=3, rc=4, opens=True)
    add('ny 12, hi closes chunk 0', FR.hook(FR.plane(12, 8, 4), (3, 4), 5, 2, 3, 4), 1, 2, 0, 'hi == row0 + rc - 1: two chunks without '
        'node', [(3, 4, 2)], nchunk=3, rc=4, closes=True)
    add('ny 12, cut twice', FR.hook(FR.plane(12, 8, 10), (3, 4), 5, 2, 7, 10), 1, 2, 0, 'a fold over all three chunks, a flip in each',
        [(3, 4, 2)], nchunk=3, rc=4, cut=3)

    # ---- many ranges
    masks, events = many_planes()
    add('many ranges', masks, 1, 2, 0, 'nrange > 256: two ranges per thread of k_cf_offsets, cp_range_of over 300 ranges with empty '
        'ones; one chunk of rows', events, ncont=3, nchunk=1, rc=7)
    return C


def shape(case):
    return next(m for m in case.masks if m is not None).shape


def stacked(case, records):
    """the records of the call: records(mask) -> (count, e_from, e_to, pts) of one plane, traced once per distinct plane"""
    seen, recs = {}, []
    for m in case.masks:
        if m is None:
            recs.append((np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 4))))
            continue
        if id(m) not in seen:
            r = records(m)
            seen[id(m)] = (np.asarray(r[0]).ravel(),) + tuple(r[1:])
        recs.append(seen[id(m)])
    return (np.concatenate([r[0] for r in recs]).astype(np.uint64), np.concatenate([r[1] for r in recs]),
            np.concatenate([r[2] for r in recs]), np.concatenate([np.asarray(r[3], dtype=np.float64).reshape(-1, 4) for r in recs]))
