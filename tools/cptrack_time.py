"""Times Contour2D.cal_contour_piece_tracks (K23) on one PV-like stack and, beside it, in the same process, the loop of
cal_contour_piece_overlap calls it replaces (every step traced and labelled twice, the union-find over the rows NOT included: the loop is
charged less than it costs).  Prints one JSON line: wall times (the median of record_timing.wall_times over --repeat runs after one
warm-up; sync=False: every call ends in its own downloads), the K23 stage times and the rounds (stage_times of ONE call, warm=False).

    python tools/cptrack_time.py [--ny 181 --nx 360 --steps 24 --levels 5 --repeat 3]
"""
import argparse
import json
import sys

import numpy as np

import record_timing as rt

sys.path.insert(0, rt.ROOT)
import xcontour_amd as xa  # noqa: E402


def pv_like(nstep, ny, nx, seed=23):
    """a polar vortex with drifting waves and a few drifting cut-off blobs; rows 0 and ny - 1 are uniform"""
    rng = np.random.default_rng(seed)
    lat, lon = np.linspace(-90.0, 90.0, ny), np.arange(nx) * (360.0 / nx)
    y, x = np.deg2rad(lat)[:, None], np.deg2rad(lon)[None, :]
    blobs = [(rng.uniform(-60, 60), rng.uniform(0, 360), rng.uniform(-6, 6), rng.uniform(4, 9), rng.uniform(0.3, 0.8) * rng.choice([-1, 1]))
             for _ in range(24)]
    q = np.empty((nstep, ny, nx))
    for t in range(nstep):
        f = np.sin(y) + 0.25 * np.cos(y) ** 2 * (np.sin(3 * x - 0.2 * t) + 0.6 * np.sin(5 * x + 0.13 * t))
        for cy, cx, u, sig, amp in blobs:
            dx = (lon[None, :] - cx - u * t + 180.0) % 360.0 - 180.0
            f = f + amp * np.exp(-((lat[:, None] - cy) ** 2 + (dx * np.cos(y)) ** 2) / (2 * sig * sig))
        q[t] = f
    return q, lat, lon


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ny', type=int, default=181)
    ap.add_argument('--nx', type=int, default=360)
    ap.add_argument('--steps', type=int, default=24)
    ap.add_argument('--levels', type=int, default=5)
    ap.add_argument('--repeat', type=int, default=3)
    a = ap.parse_args()
    q, lat, lon = pv_like(a.steps, a.ny, a.nx)
    dA = np.cos(np.deg2rad(lat))[:, None] * np.ones(a.nx) + 1e-3
    lv = np.quantile(q, np.linspace(0.15, 0.85, a.levels))
    c = {'time': np.arange(a.steps), 'latitude': lat, 'longitude': lon}
    dims = {'X': 'longitude', 'Y': 'latitude'}
    cm = xa.Contour2D(xa.DataArray(q, ('time', 'latitude', 'longitude'), c, 'q'), xa.DataArray(dA, ('latitude', 'longitude'), c, 'dA'),
                      dims, {'Y': 'latitude'}, dtype=np.float64)
    c2 = {'latitude': lat, 'longitude': lon}
    steps = [xa.DataArray(q[t], ('latitude', 'longitude'), c2, 'q') for t in range(a.steps)]
    singles = [xa.Contour2D(s, xa.DataArray(dA, ('latitude', 'longitude'), c2, 'dA'), dims, {'Y': 'latitude'}, dtype=np.float64) for s in steps]

    def tracks():
        return cm.cal_contour_piece_tracks(lv, 'time', periodic=True)

    def loop():
        return [singles[t].cal_contour_piece_overlap(lv, steps[t + 1], periodic=True)[2] for t in range(a.steps - 1)]

    t_tracks, t_loop = (float(np.median(rt.wall_times(cm.ctx, fn, a.repeat, sync=False))) for fn in (tracks, loop))
    got = []
    _, prof = rt.stage_times(cm.ctx, lambda: got.append(tracks()), cm.ctx.last_cptrack_profile, (), 1, sync_each=False, warm=False)
    tree, links, tr = got[0]
    pairs = loop()
    same = all(np.array_equal(links[k][links[k]['step'] == t][f], pairs[t][k][f]) for t in range(a.steps - 1) for k in range(a.levels)
               for f in ('a', 'b', 'nodes', 'area'))
    print(json.dumps(dict(device=cm.ctx.device_name(), ny=a.ny, nx=a.nx, steps=a.steps, levels=a.levels, rings=int(sum(t.size for s in tree for t in s)),
                          links=int(sum(l.size for l in links)), tracks=int(sum(t.size for t in tr)), tracks_call_s=t_tracks, overlap_loop_s=t_loop,
                          links_equal_the_loops_rows=bool(same), k23=prof)))


if __name__ == '__main__':
    main()
