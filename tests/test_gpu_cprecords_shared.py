"""K18-K21 (xc_contour_piece_{interiors,tree,labels,props}_dev) on ONE context in every order: the four entries share the context's two
workspaces, so whatever one of them leaves behind -- a larger block, staged records, a carry, the table of fields -- is what the next one
finds.  Every result of every call of all 24 orders is BITWISE the result of the same call on a context that has done nothing else, and
each entry's profile reports its own call's groups, whichever entry ran last.  The reference side is the library itself on a fresh
context: no tolerance, no CPU oracle.

The input is a stack of four 24 x 65 planes (a second row chunk, columns on both sides of a wave), periodic and plain, at three levels of
which the middle one has no segments: twelve ranges, every third one empty.  The four entries run under four caps of the edge tables --
1, 3, 4 and 6 table rows -- which cut the twelve ranges into 8, 4, 3 and 2 groups (cp_plan_groups: empty ranges in front of a group and
behind it cost no row), so that a profile that took another entry's count shows.  Inside a range the pieces come in the order their roots
were counted, which is the call's own: rows are compared sorted by first_edge, parents and labels renumbered to match."""
import itertools

import numpy as np
import pytest

import cpprops_ref as QR
import cptree_cases as CS
import test_gpu_cpinside_records as K18
import test_gpu_cplabel_records as K20
import test_gpu_cpprops_records as K21
import test_gpu_cptree_records as K19
from test_gpu_cpinside_records import DEFAULT_CAP, scaled, shuffled, trace
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

NY, NX, NSLAB = 24, 65, 4
LEVELS = (-0.4, 99.0, 0.5)
ROW = 2 * NY * NX * 4                                                        # bytes of one row of the edge tables
# entry -> (table rows under its cap, the groups that makes of the twelve ranges)
PLAN = {'inside': (1, 8), 'tree': (3, 4), 'label': (4, 3), 'props': (6, 2)}
PROFILE = {'inside': 'last_cpinside_profile', 'tree': 'last_cptree_profile', 'label': 'last_cplabel_profile', 'props': 'last_cpprops_profile'}


def canonical(pc, cols, label=None, props=None):
    """the bytes of one call's results, the rows of every range sorted by first_edge"""
    out, p0 = [np.asarray(pc, dtype=np.int64).tobytes()], 0
    for r, n in enumerate(int(v) for v in pc):
        order = np.argsort(cols[0][p0:p0 + n], kind='stable')
        where = np.empty(n, dtype=np.int64)
        where[order] = np.arange(n)
        for name, col in zip(K19.NAMES, cols):
            c = col[p0:p0 + n]
            if name == 'parent' and n:
                c = np.where(c >= 0, where[np.clip(c - p0, 0, n - 1)], -1)
            out.append(np.ascontiguousarray(c[order]).tobytes())
        if label is not None:
            m = label[r]
            assert m.min() >= -1 and m.max() < max(n, 1)
            out.append(np.where(m >= 0, where[np.clip(m, 0, max(n - 1, 0))] if n else -1, -1).astype(np.int32).tobytes())
        if props is not None:
            out += [np.ascontiguousarray(v[:, p0:p0 + n][:, order]).tobytes() for _, v in sorted(props.items())]
        p0 += n
    return out


def run(ctx, entry, rec, periodic, flip, w, f, fields, x):
    """one call of `entry` under its cap -> (the canonical bytes of everything it returned, the groups its profile reports)"""
    a = (*rec[:4], NY, NX, periodic, flip, len(LEVELS))
    ctx.set_cpiece_workspace(PLAN[entry][0] * ROW)
    try:
        if entry == 'inside':
            rc, pc, cols, _ = K18.call(ctx, *a, w=w, f=f)
            got = canonical(pc, cols)
        elif entry == 'tree':
            rc, pc, cols, _ = K19.call(ctx, *a, w=w, f=f)
            got = canonical(pc, cols)
        elif entry == 'label':
            rc, pc, cols, lab = K20.call(ctx, *a, w=w, f=f)
            got = canonical(pc, cols, label=lab)
        else:
            rc, pc, cols, pr = K21.call(ctx, *a, w=w, fields=fields, x=x)
            got = canonical(pc, cols, props=pr)
    finally:
        ctx.set_cpiece_workspace(DEFAULT_CAP)
    assert rc == 0, '%s returned %d' % (entry, rc)
    return got, getattr(ctx, PROFILE[entry])()['groups']


@pytest.mark.parametrize('periodic', [0, 1], ids=['plain', 'ring'])
def test_the_four_entries_in_all_24_orders_on_one_context(ctx, periodic):
    q = np.stack([CS.smooth_noise(NY, NX, 300 + s) for s in range(NSLAB)])
    rec = shuffled(trace(q, periodic, LEVELS), 17)
    assert (rec[0].reshape(NSLAB, 3) > 0).tolist() == [[True, False, True]] * NSLAB
    rng = np.random.default_rng(23)
    w, f = scaled(rng, (NSLAB, NY, NX)), scaled(rng, (NSLAB, NY, NX), np.float32)
    fields, x = QR.field_set(rng, 5, NSLAB, NY, NX, scaled), QR.integer_x(rng, NSLAB, NY, NX)
    ctx.set_kernel_timing(True)
    try:
        for flip in (0, 1):
            alone = {}
            for entry in PLAN:                                               # the same call on a context that has done nothing else
                fresh = nat.Context(0)
                try:
                    fresh.set_kernel_timing(True)
                    alone[entry], groups = run(fresh, entry, rec, periodic, flip, w, f, fields, x)
                finally:
                    fresh.close()
                assert groups == PLAN[entry][1], (entry, groups)
            for order in itertools.permutations(PLAN):
                for entry in order:
                    got, _ = run(ctx, entry, rec, periodic, flip, w, f, fields, x)
                    assert got == alone[entry], '%s in the order %s (flip %d) is not what it is alone' % (entry, ' '.join(order), flip)
                for entry in PLAN:                                           # after the sequence: every profile still its own call's
                    assert getattr(ctx, PROFILE[entry])()['groups'] == PLAN[entry][1], (entry, order)
    finally:
        ctx.set_kernel_timing(False)
