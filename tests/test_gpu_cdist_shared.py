"""K27 (Context.contour_distance) and K28 (Context.contour_distance_profile) taking turns on ONE context: they share the launcher, the
layout of the piece workspace (K28's words take no byte in a K27 call) and the type of the record behind last_cdist_profile /
last_cdprofile_profile.  Every result must be, bit for bit, what the same call gives on a context of its own, and each call's record must
survive the other call.  The inputs are the smallest of cdist_cases: the 37 x 45 plane and the first 70 x 100 sphere, two levels each.

Asserted elsewhere and not repeated: that an unpruned / global-path K28 call gives the bits of the plain one and that the forced global
path reports tiles_window == 0 on its own context (test_gpu_cdprof.variants); pairs_visited == pairs_total of an unpruned K27 call on
its own context (test_gpu_cdist_records.test_sphere_records).  Here both switches are set once and BOTH kernels run under them."""
import functools

import numpy as np
import pytest

import cdist_cases as CC
import cdprof_ref as PR
from xcontour_amd import _native as nat

pytestmark = pytest.mark.gpu

PLANE, SPHERE = '37x45', sorted(CC.sphere_cases())[0]
PAIRS = ('pairs_visited', 'pairs_total', 'groups')
TILES = PAIRS + ('tiles_window', 'tiles_global')
R = CC.R_EARTH
EDGES_S = np.array([-2.1e7, -1.5e6, 1.5e6, 2.1e7])          # symmetric: a node nearer than 1500 km lies in the middle bin whatever its sign
EDGES_P = np.array([0.0, 2.0, 6.0, 60.0])


@functools.lru_cache(maxsize=None)
def inputs():
    """the fields the two cases were made of (cdist_cases.plane_cases, sphere_cases) with their levels, weights and two fields"""
    p, s = CC.plane_cases()[PLANE], CC.sphere_cases()[SPHERE]
    qp, qs = CC.smooth(37, 45, 37 * 45), CC.ring_with_gradient(70, 100, 10)
    w = np.ascontiguousarray(np.broadcast_to(1.0 + 0.37 * np.sin(1.0 + np.arange(70.0))[:, None], (70, 100)))
    rng = np.random.default_rng(3)
    f1 = rng.normal(size=(70, 100)) * 10.0 ** rng.uniform(0.0, 6.0, size=(70, 100))            # mixed signs, six decades
    return dict(p=p, s=s, qp=qp[None], qs=qs[None], lvp=np.array([-0.4, 0.1]), lvs=np.array([-0.3, 0.2]), w=w, f=(f1, CC.smooth(70, 100, 4)))


def test_the_bin_edges_hold_nodes():
    """on the CPU (cdprof_ref): the edges of both K28 calls leave at least one bin with nodes"""
    for name, edges in ((PLANE, EDGES_P), (SPHERE, EDGES_S)):
        d = CC.cached_reference(name)['dist'][:2]
        b = PR.bins_of(d, edges)
        assert (b >= 0).any() and (b == 1).any(), name


def k28_sphere(c):
    i = inputs()
    return c.contour_distance_profile(i['qs'], i['lvs'], i['s']['ycoord'], i['s']['xcoord'], EDGES_S, w=i['w'], fields=i['f'], radius=R,
                                      period=i['s']['period'], signed=True)


def k28_plane(c):
    i = inputs()
    return c.contour_distance_profile(i['qp'], i['lvp'], i['p']['ycoord'], i['p']['xcoord'], EDGES_P)


def k27_plane(c):
    i = inputs()
    return c.contour_distance(i['qp'], i['lvp'], i['p']['ycoord'], i['p']['xcoord'], return_nearest=True)


def k27_sphere(c):
    i = inputs()
    return c.contour_distance(i['qs'], i['lvs'], i['s']['ycoord'], i['s']['xcoord'], radius=R, period=i['s']['period'])


def last(c, call):
    p = c.last_cdprofile_profile() if call in (k28_sphere, k28_plane) else c.last_cdist_profile()
    return {k: p[k] for k in (TILES if 'tiles_window' in p else PAIRS)}


@functools.lru_cache(maxsize=None)
def alone(call):
    """the call on a context of its own -> (its arrays, its record), computed once and left unchanged"""
    c = nat.Context(0)
    try:
        out = call(c)
        out = out if isinstance(out, tuple) else (out,)
        for a in out:
            a.setflags(write=False)
        return out, last(c, call)
    finally:
        c.close()


def same(got, call, what):
    got = got if isinstance(got, tuple) else (got,)
    ref = alone(call)[0]
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), '%s: output %d differs' % (what, k)


def test_k28_has_something_to_say():
    nodes = alone(k28_sphere)[0][0]
    assert nodes[..., 1].min() > 0 and nodes[..., 0].sum() > 0 and nodes[..., 2].sum() > 0          # both signs, both levels
    assert alone(k28_plane)[0][0].sum() > 0 and np.isfinite(alone(k27_sphere)[0][0]).all()


def test_taking_turns_on_one_context_changes_no_bit():
    c = nat.Context(0)
    try:
        for step, call in enumerate((k28_sphere, k27_plane, k28_sphere, k27_sphere, k28_plane)):
            same(call(c), call, 'step %d (%s)' % (step, call.__name__))
            assert last(c, call) == alone(call)[1], 'step %d (%s): its record' % (step, call.__name__)
    finally:
        c.close()


@pytest.mark.parametrize('first,second', [(k27_plane, k28_sphere), (k28_sphere, k27_plane)], ids=['K27 then K28', 'K28 then K27'])
def test_a_call_leaves_the_record_of_the_other_alone(first, second):
    c = nat.Context(0)
    try:
        first(c)
        mine = last(c, first)
        assert mine == alone(first)[1] and mine['pairs_total'] > 0
        second(c)
        assert last(c, first) == mine and last(c, second) == alone(second)[1]
    finally:
        c.close()


def test_both_switches_reach_both_kernels(ctx):
    try:
        ctx.set_cdist_prune(False)
        for call in (k28_sphere, k27_sphere, k27_plane):
            same(call(ctx), call, 'unpruned ' + call.__name__)
            p = last(ctx, call)
            assert p['pairs_visited'] == p['pairs_total'] == alone(call)[1]['pairs_total'] > 0, call.__name__
        ctx.set_cdist_prune(True)
        ctx.set_cdprofile_global(True)
        for call in (k28_sphere, k27_sphere, k28_plane):
            same(call(ctx), call, 'global path ' + call.__name__)
        p, q = last(ctx, k28_plane), alone(k28_plane)[1]
        assert p['tiles_window'] == 0 and p['tiles_global'] == q['tiles_window'] + q['tiles_global'] > 0
        assert last(ctx, k27_sphere) == alone(k27_sphere)[1]
    finally:
        ctx.set_cdist_prune(True)
        ctx.set_cdprofile_global(False)
