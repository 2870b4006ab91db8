"""Seen maps (`ms_nav_seen`, `cuda.seen_maps`, `SeenMaps.mark`, `modules.Coverage`, `demo.FloorCoverage`) on the CPU: the
contract of include/megastep_hip.h (MsNavSeen) restated in binary32 numpy (`seen_rule`, which tests/test_gpu_navseen.py holds
the kernel to, bit for bit); the host instantiation of the kernel's own device functions against the rule; a known answer;
the promise that no wall is seen through; idempotence; and the C-ABI's declarations, layouts and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, RADIUS, F, _world, nav_rule, plans, spawn_points

INF, NAN = F(np.inf), F(np.nan)


class seen_rule:
    """The contract in numpy: float32 scalars and arrays only, one operation per statement, in the order the header gives."""

    @staticmethod
    def rays(cell, origins, dirs, distances, max_range):
        """Of viewers at `origins` (P, 2) with rays `dirs` (P, R, 2) that got `distances` (P, R): (keep (P, R) bool, ox, oy,
        ex, ey (P, R) float32, K (P, R) int64) - the rays as their samples read them."""
        c, m = F(cell), F(max_range)
        dirs, dist = np.asarray(dirs, F), np.asarray(distances, F)
        ox = np.broadcast_to(np.asarray(origins, F)[:, None, 0], dist.shape)
        oy = np.broadcast_to(np.asarray(origins, F)[:, None, 1], dist.shape)
        dx, dy = dirs[..., 0], dirs[..., 1]
        with np.errstate(all='ignore'):
            xx = dx*dx
            yy = dy*dy
            ss = xx + yy
            rlen = np.sqrt(ss)
            keep = np.isfinite(ox) & np.isfinite(oy) & np.isfinite(dx) & np.isfinite(dy) & np.isfinite(rlen) & (rlen > F(0)) & (dist > F(0))
            reach = np.where(dist < m, dist, m)
            ux = dx/rlen
            uy = dy/rlen
            ex = ux*reach
            ey = uy*reach
            exx = ex*ex
            eyy = ey*ey
            ess = exx + eyy
            elen = np.sqrt(ess)
            half = F(.5)*c
            per = elen/half
            k = np.ceil(per)
            keep = keep & (k < F(1048576.))
        K = np.maximum(np.where(keep, k, F(1)).astype(np.int64), 1)
        return keep, ox, oy, ex, ey, K

    @staticmethod
    def samples(geom, cell, ox, oy, ex, ey, K):
        """Every sample of the rays given as 1-D arrays: (which ray, x, y, flat cell or -1)."""
        jx0, iy0, nx, ny = geom
        c = F(cell)
        n = K + 1
        which = np.repeat(np.arange(len(K)), n)
        s = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
        with np.errstate(all='ignore'):
            sf = s.astype(F)
            Kf = K[which].astype(F)
            t = sf/Kf
            sx = ex[which]*t
            sy = ey[which]*t
            x = ox[which] + sx
            y = oy[which] + sy
            qx = x/c
            qy = y/c
            fx = np.floor(qx)
            fy = np.floor(qy)
            near = (np.abs(fx) < F(2.**30)) & (np.abs(fy) < F(2.**30))
        j = np.where(near, fx, F(0)).astype(np.int64) - jx0
        i = np.where(near, fy, F(0)).astype(np.int64) - iy0
        inside = near & (i >= 0) & (i < ny) & (j >= 0) & (j < nx)
        return which, x, y, np.where(inside, i*nx + j, -1)

    @staticmethod
    def marks(geom, cell, origins, dirs, distances, max_range):
        """(which viewer, x, y, flat cell) of every sample that marks a cell."""
        keep, ox, oy, ex, ey, K = seen_rule.rays(cell, origins, dirs, distances, max_range)
        viewer = np.broadcast_to(np.arange(keep.shape[0])[:, None], keep.shape)[keep]
        which, x, y, cells = seen_rule.samples(geom, cell, ox[keep], oy[keep], ex[keep], ey[keep], K[keep])
        hit = cells >= 0
        return viewer[which[hit]], x[hit], y[hit], cells[hit]

    @staticmethod
    def call(geom, cell, countable, maps, totals, origins, dirs, distances, slot=None, max_range=10., reset=None):
        """One call for one env: maps (S, ny, nx) uint8 and totals (S,) as they were -> (maps, gained, totals) as it leaves them."""
        jx0, iy0, nx, ny = geom
        S = len(maps)
        shape = np.shape(maps)
        maps, totals = np.array(maps, np.uint8).reshape(S, -1), np.array(totals, np.int32)
        gained = np.zeros(S, np.int32)
        clear = np.zeros(S, bool) if reset is None else np.asarray(reset).astype(bool)
        maps[clear] = 0
        totals[clear] = 0
        if nx*ny > 0:
            viewer, _, _, cells = seen_rule.marks(geom, cell, origins, dirs, distances, max_range)
            slot = np.arange(len(origins)) if slot is None else np.asarray(slot)
            counts = (np.asarray(countable).reshape(-1).astype(np.uint8) & 1).astype(bool)
            for s in range(S):
                after = maps[s].copy()
                after[cells[slot[viewer] == s]] = 1
                gained[s] = int(((maps[s] == 0) & (after == 1) & counts).sum())
                maps[s] = after
        return maps.reshape(shape), gained, totals + gained


_SPARE = np.zeros(8, np.uint8)         # (somewhere to point for an env without cells)


def _host(geom, cell, countable, maps, totals, origins, dirs, distances, slot=None, max_range=10., reset=None, outputs=True):
    """ms_host_nav_seen on copies: (maps, gained, totals)."""
    from megastep_amd import _lib
    h = _lib.lib()
    S = len(maps)
    geom = np.array(geom, np.int32)
    countable = np.ascontiguousarray(countable, np.uint8)
    maps, totals, gained = np.array(maps, np.uint8), np.array(totals, np.int32), np.full(S, -7, np.int32)
    origins, dirs, distances = (np.ascontiguousarray(a, F) for a in (origins, dirs, distances))
    slot = None if slot is None else np.ascontiguousarray(slot, np.int32)
    reset = None if reset is None else np.ascontiguousarray(reset, np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data
    P, R = distances.shape
    code = h.ms_host_nav_seen(ptr(geom), cell, ptr(countable) or ptr(_SPARE), S, P, R, ptr(origins), ptr(dirs), ptr(distances),
                              ptr(slot), max_range, ptr(reset), ptr(maps) or ptr(_SPARE), ptr(gained) if outputs else None,
                              ptr(totals) if outputs else None)
    assert code == 0
    return maps, gained, totals


def _same(geom, countable, maps, totals, origins, dirs, distances, cell=CELL, **kw):
    want = seen_rule.call(geom, cell, countable, maps, totals, origins, dirs, distances, **kw)
    got = _host(geom, cell, countable, maps, totals, origins, dirs, distances, **kw)
    assert np.array_equal(got[0], want[0]), int((got[0] != want[0]).sum())
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist(), (got[1:], want[1:])
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the inputs: three plain and three oblique plans, two viewers each at spawn-table points, 64 camera rays each, with the
# distances of the oracle's render
# ---------------------------------------------------------------------------------------------------------------------
class _Case:
    pass


_CASES = {}


def cases(cell=CELL, r=RADIUS):
    """The cases gridded at `cell` with clearance `r`: the viewers, rays and distances are the same whatever the grid."""
    if (cell, r) not in _CASES:
        found = _CASES[cell, r] = []
        for base, g in zip(_rendered(), plans(3) + plans(3, oblique=True)):
            case = _Case()
            case.walls, case.geom, case.free = _world(g, cell, r)
            case.origins, case.dirs, case.distances = base
            case.blank = np.zeros((2,) + case.free.shape, np.uint8)
            found.append(case)
    return _CASES[cell, r]


_RENDERED = []


def _rendered():
    """[(origins, dirs, distances)] per plan: the oracle's render from two spawn-table points."""
    if not _RENDERED:
        from megastep_amd import core, scene
        from tests import util
        from tests.test_raycast_host import camera_rays_np
        geoms = plans(3) + plans(3, oblique=True)
        rng = np.random.RandomState(31)
        sc = scene.scenery(geoms, 2, device='cpu', random=np.random.RandomState(0), bake=False)
        c = core.Core(sc, res=64, fov=130)
        pos = np.stack([(spawn_points(g)[rng.choice(len(spawn_points(g)), 2)] + rng.uniform(-.05, .05, (2, 2))).astype(F) for g in geoms])
        c.agents.positions[:] = torch.as_tensor(pos)
        c.agents.angles[:] = torch.as_tensor(rng.uniform(-180, 180, (len(geoms), 2)).astype(F))
        ref = util.OracleWorld(c)
        distances = ref.render()['distances']
        dirs = camera_rays_np(ref.agents['angles'], 64, 130)
        _RENDERED.extend((pos[e], dirs[e], np.asarray(distances[e], F)) for e in range(len(geoms)))
    return _RENDERED


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_host_instantiation_is_the_rule_at_other_cell_widths(cell, r):
    """The same viewers and rays over grids whose cell is no power of two: a ray's sample count len/(.5f*c) and a sample's cell
    are rounded there."""
    seen = 0
    for case in cases(cell, r):
        a = (case.geom, case.free, case.blank, [0, 0], case.origins, case.dirs, case.distances)
        maps, gained, totals = _same(*a, cell=cell)
        assert (gained > 0).all() and gained.tolist() == totals.tolist() == [int((m.astype(bool) & case.free).sum()) for m in maps]
        seen += int(gained.sum())
        short = _same(*a, cell=cell, max_range=1.)
        assert (short[1] <= gained).all() and 0 < short[1].sum() < gained.sum()
        _same(*a, cell=cell, max_range=1000.)
        one = (case.geom, case.free, case.blank[:1], [0], case.origins, case.dirs, case.distances)
        shared = _same(*one, cell=cell, slot=[0, 0])
        assert np.array_equal(shared[0][0], maps[0] | maps[1])
        _same(case.geom, case.free, short[0], short[2], case.origins, case.dirs, case.distances, cell=cell, reset=[1, 0])
    assert seen > 2000*(CELL/cell)**2                                    # (the same floor, in cells)


def test_the_host_instantiation_is_the_rule_bit_for_bit():
    seen = 0
    for case in cases():
        a = (case.geom, case.free, case.blank, [0, 0], case.origins, case.dirs, case.distances)
        maps, gained, totals = _same(*a)
        assert (gained > 0).all() and gained.sum() > 100 and gained.tolist() == totals.tolist() == [int((m.astype(bool) & case.free).sum()) for m in maps]
        assert np.isfinite(case.distances).any() and (case.distances[np.isfinite(case.distances)] < 10).any()
        seen += int(gained.sum())
        # max_range below most distances, and above all of them
        short = _same(*a, max_range=1.)
        assert (short[1] <= gained).all() and 0 < short[1].sum() < gained.sum()
        far = _same(*a, max_range=1000.)
        assert (far[1] >= gained).all()
        # two viewers sharing one map: a cell both see counts once
        one = (case.geom, case.free, case.blank[:1], [0], case.origins, case.dirs, case.distances)
        shared = _same(*one, slot=[0, 0])
        assert np.array_equal(shared[0][0], maps[0] | maps[1]) and max(gained) <= shared[1][0] <= gained.sum()
        # a viewer that marks no map, and one that marks the other's
        skipped = _same(*a, slot=[-1, 0])
        assert skipped[1][1] == 0 and not skipped[0][1].any() and np.array_equal(skipped[0][0], maps[1])
        _same(*a, slot=[2, 1])
        # reset set and clear on maps that already hold marks; totals carry on or start over
        held = (case.geom, case.free, short[0], short[2], case.origins, case.dirs, case.distances)
        again = _same(*held)
        assert (again[2] == short[2] + again[1]).all() and (again[2] >= totals).all() and (again[1] < gained).all()   # (other samples: a few cells more)
        mixed = _same(*held, reset=[1, 0])
        assert mixed[1][0] == gained[0] and mixed[2][0] == gained[0] and mixed[1][1] == again[1][1]
        _same(*held, reset=[0, 0])
        swapped = _same(case.geom, case.free, maps[::-1], totals[::-1], case.origins, case.dirs, case.distances, reset=[1, 1], max_range=1.)
        assert np.array_equal(swapped[0], short[0])
        # R = 1
        _same(case.geom, case.free, case.blank, [3, 4], case.origins, case.dirs[:, 5:6], case.distances[:, 5:6])
        # without outputs the maps are marked all the same
        assert np.array_equal(_host(a[0], CELL, *a[1:], outputs=False)[0], maps)
    assert seen > 2000


def test_odd_rays_are_skipped_or_cut_as_the_rule_says():
    case = cases()[3]
    rng = np.random.RandomState(5)
    origins, dirs, distances = case.origins.copy(), case.dirs.copy(), case.distances.copy()
    distances[0, :8] = [INF, 0., -1., NAN, -INF, F(1e-30), F(3e38), F(2.5)]
    dirs[0, 8:14] = [[NAN, 1.], [1., INF], [0., 0.], [-INF, NAN], [3e38, 3e38], [1e-30, 1e-30]]
    dirs[1, :16] *= rng.uniform(.01, 100., (16, 1)).astype(F)           # (any length)
    a = (case.geom, case.free, case.blank, [0, 0])
    got = _same(*a, origins, dirs, distances)
    assert (got[1] > 20).all()
    keep = seen_rule.rays(CELL, origins, dirs, distances, 10.)[0]
    assert keep[0, :8].tolist() == [True, False, False, False, False, True, True, True] and not keep[0, 8:13].any() and keep[1].all()
    for bad in ([NAN, 1.], [1., INF], [-INF, -INF]):
        origins2 = origins.copy()
        origins2[1] = bad
        assert _same(*a, origins2, dirs, distances)[1][1] == 0
    # rays that leave the grid: a viewer near the edge looking out with nothing hit, one far outside looking in, one further
    # than any grid
    lo = case.walls.reshape(-1, 2).min(0)
    origins3 = np.array([lo + .05, lo - 3.], F)
    out = np.full_like(distances, INF)
    left = _same(*a, origins3, dirs, out, max_range=30.)
    assert left[1].sum() > 0
    origins3[1] = [3e9, -3e9]
    _same(*a, origins3, dirs, out, max_range=1000.)
    origins3[1] = [3e38, 3e38]
    _same(*a, origins3, dirs, out, max_range=3e38)
    # a reach of more than 2^20 samples: skipped
    assert _same(*a, case.origins, case.dirs, out, max_range=1e6)[1].sum() == 0


def test_an_env_without_cells_marks_nothing_and_gains_nothing():
    case = cases()[0]
    none = np.zeros((2, 0, 0), np.uint8)
    for geom in ((0, 0, 0, 0), (3, 4, 0, 7)):
        got = _same(geom, np.zeros(0, np.uint8), none, [5, 6], case.origins, case.dirs, case.distances, reset=[0, 1])
        assert got[1].tolist() == [0, 0] and got[2].tolist() == [5, 0]


def test_marking_twice_with_the_same_rays_gains_nothing_the_second_time():
    for case in cases():
        a = (case.origins, case.dirs, case.distances)
        first = _same(case.geom, case.free, case.blank, [0, 0], *a)
        second = _same(case.geom, case.free, first[0], first[2], *a)
        assert second[1].tolist() == [0, 0] and second[2].tolist() == first[2].tolist() and np.array_equal(second[0], first[0])


def _ring(centre, walls_lo, walls_hi, n=720):
    """n rays round `centre` inside the axis-aligned room [lo, hi]^2 and their exact (float64, then rounded) distances to its walls."""
    angle = 2*np.pi*(np.arange(n) + .5)/n
    d = np.stack([np.cos(angle), np.sin(angle)], -1)
    with np.errstate(divide='ignore'):
        tx = np.where(d[:, 0] > 0, (walls_hi - centre[0])/d[:, 0], (walls_lo - centre[0])/d[:, 0])
        ty = np.where(d[:, 1] > 0, (walls_hi - centre[1])/d[:, 1], (walls_lo - centre[1])/d[:, 1])
    return d.astype(F)[None], np.minimum(np.abs(tx), np.abs(ty)).astype(F)[None]


def test_a_ring_of_rays_from_the_middle_of_the_box_sees_the_room_and_nothing_else():
    """toys.box(): a 5 m room. Its far corner is 2.5 sqrt(2) = 3.54 m from the centre; with max_range = 4 m neighbouring rays of
    a 720-ray ring are at most 4 x 2 pi/720 = 0.035 m apart, under half a cell (0.0625 m), everywhere a ray goes - so the whole
    room is the checked set: the ray that passes nearest a cell centre (within 0.018 m) has more than a sample spacing of its
    length inside that cell."""
    from megastep_amd import geometry, toys
    walls, geom, free = _world(toys.box())
    lo, hi = geometry.MARGIN, geometry.MARGIN + 5
    assert np.allclose(walls.reshape(-1, 2).min(0), lo) and np.allclose(walls.reshape(-1, 2).max(0), hi)
    centre = np.array([[(lo + hi)/2 + .013, (lo + hi)/2 - .021]], F)
    dirs, distances = _ring(centre[0].astype(np.float64), lo, hi)
    assert 4.*2*np.pi/720 < .5*CELL and distances.max() < 4.
    maps, gained, totals = _same(geom, free, np.zeros((1,) + free.shape, np.uint8), [0], centre, dirs, distances, max_range=4.)
    x, y = nav_rule.centres(geom, CELL)
    inside = ((x > lo) & (x < hi))[None, :] & ((y > lo) & (y < hi))[:, None]
    seen = maps[0].astype(bool)
    assert (free & inside).sum() > 1000
    assert seen[free & inside].all()
    assert not seen[free & ~inside].any()
    assert gained[0] == totals[0] == (free & inside).sum()


def _meets(a, b, walls):
    """Does the float64 segment a[k] -> b[k] meet any wall: (n,) bool. (The orientation test, touching included, restated here.)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    hit = np.zeros(len(a), bool)
    for p, q in np.asarray(walls, np.float64).reshape(-1, 2, 2):
        w = q - p
        s1 = w[0]*(a[:, 1] - p[1]) - w[1]*(a[:, 0] - p[0])
        s2 = w[0]*(b[:, 1] - p[1]) - w[1]*(b[:, 0] - p[0])
        r = b - a
        s3 = r[:, 0]*(p[1] - a[:, 1]) - r[:, 1]*(p[0] - a[:, 0])
        s4 = r[:, 0]*(q[1] - a[:, 1]) - r[:, 1]*(q[0] - a[:, 0])
        hit |= (s1*s2 <= 0) & (s3*s4 <= 0) & ((s1 != s2) | (s3 != s4))
    return hit


def test_no_wall_is_seen_through():
    """Every countable cell a map holds has a sample of some ray inside it, and the straight line from that sample - a point
    the ray reached - to the cell's centre meets no static wall."""
    checked = 0
    for case in cases():
        maps, gained, _ = seen_rule.call(case.geom, CELL, case.free, case.blank, [0, 0], case.origins, case.dirs, case.distances)
        viewer, sx, sy, cells = seen_rule.marks(case.geom, CELL, case.origins, case.dirs, case.distances, 10.)
        x, y = nav_rule.centres(case.geom, CELL)
        nx = case.free.shape[1]
        for s in range(2):
            mine = viewer == s
            first = dict(zip(cells[mine][::-1].tolist(), np.nonzero(mine)[0][::-1].tolist()))     # a sample in each marked cell
            counted = np.nonzero(maps[s].reshape(-1).astype(bool) & case.free.reshape(-1))[0]
            assert len(counted) == gained[s] and set(counted.tolist()) <= set(first)
            k = np.array([first[cell] for cell in counted.tolist()])
            samples = np.stack([sx[k], sy[k]], 1)
            centres = np.stack([x[counted % nx], y[counted // nx]], 1)
            assert (np.abs(samples - centres) <= .5*CELL + 1e-5).all()                             # (the sample is inside the cell)
            assert not _meets(samples, centres, case.walls).any()
            checked += len(counted)
        # ... whereas marked cells that do not count include the ones the hit points fell in
        assert (maps.astype(bool) & ~case.free).any()
    assert checked > 2000


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_call_and_the_loader_binds_it():
    from megastep_amd import _lib
    assert 'ms_nav_seen' in declared_symbols(('megastep_hip.h',)) and 'ms_host_nav_seen' in declared_symbols(('megastep_hip_test.h',))
    assert {'ms_nav_seen', 'ms_host_nav_seen'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert hasattr(handle, 'ms_nav_seen') and hasattr(handle, 'ms_host_nav_seen') and handle.ms_abi_version() == 17


def test_the_mirror_has_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    fields = ('n_maps', 'n_viewers', 'n_rays', 'origins', 'dirs', 'distances', 'slot', 'max_range', 'reset', 'countable', 'maps', 'gained',
              'total', 'max_cells')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(MsNavSeen));' +
           ''.join(f'printf(" %zu", offsetof(MsNavSeen, {f}));' for f in fields) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    assert [f for f, _ in _lib.MsNavSeen._fields_] == list(fields)
    assert got == [ctypes.sizeof(_lib.MsNavSeen)] + [getattr(_lib.MsNavSeen, f).offset for f in fields]


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = dict(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    seen = dict(n_maps=2, n_viewers=2, n_rays=8, origins=fake, dirs=fake, distances=fake, slot=None, max_range=10., reset=None,
                countable=None, maps=fake, gained=fake, total=fake, max_cells=64)
    G, V = _lib.MsNavGrid, _lib.MsNavSeen
    ref = ctypes.byref
    assert h.ms_nav_seen(None, ref(V(**seen)), None) == -1 and h.ms_nav_seen(ref(G(**grid)), None, None) == -1
    for bad in (dict(n_envs=0), dict(cell=0.), dict(cell=.15), dict(geom=None), dict(starts=None), dict(free_cells=None), dict(geom=68)):
        assert h.ms_nav_seen(ref(G(**{**grid, **bad})), ref(V(**seen)), None) == -1, bad
    for bad in (dict(n_maps=0), dict(n_viewers=0), dict(n_rays=0), dict(n_rays=-2), dict(origins=None), dict(dirs=None), dict(distances=None),
                dict(maps=None), dict(n_viewers=3), dict(origins=68), dict(dirs=68), dict(distances=66), dict(slot=66), dict(gained=66),
                dict(total=66), dict(max_range=0.), dict(max_range=-1.), dict(max_range=float('inf')), dict(max_range=float('nan')),
                dict(max_cells=-1)):
        assert h.ms_nav_seen(ref(G(**grid)), ref(V(**{**seen, **bad})), None) == -1, bad
    # an env of more than 2^20 cells: unsupported, and nothing is enqueued
    assert h.ms_nav_seen(ref(G(**grid)), ref(V(**{**seen, 'max_cells': 2**20 + 1})), None) == -3
    # the host instantiation
    case = cases()[0]
    ptr = lambda a: a.ctypes.data
    geom, maps = np.array(case.geom, np.int32), case.blank.copy()
    free = np.ascontiguousarray(case.free, np.uint8)
    args = lambda **kw: [kw.get('geom', ptr(geom)), kw.get('cell', CELL), ptr(free), kw.get('S', 2), kw.get('P', 2), kw.get('R', 64),
                         ptr(case.origins), ptr(case.dirs), ptr(case.distances), None, kw.get('max_range', 10.), None, ptr(maps), None, None]
    assert h.ms_host_nav_seen(*args()) == 0
    for bad in (dict(geom=None), dict(cell=0.), dict(S=0), dict(S=1), dict(P=0), dict(R=0), dict(max_range=0.), dict(max_range=float('inf'))):
        assert h.ms_host_nav_seen(*args(**bad)) == -1, bad


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    maps = cuda.seen_maps(grid, 2)
    assert maps.values.shape == (256,) and maps.totals.shape == (2, 2) and maps.n_countable.tolist() == [64, 64]
    assert maps.image(1, 1).shape == (8, 8) and maps.image(1, 1).dtype == torch.bool and maps.fraction().tolist() == [[0., 0.], [0., 0.]]
    half = torch.ones(128, dtype=torch.bool)
    half[:32] = False
    assert cuda.seen_maps(grid, 1, countable=half).n_countable.tolist() == [32, 64]
    for bad in (0, 2.5):
        with pytest.raises(RuntimeError, match='n_maps'):
            cuda.seen_maps(grid, bad)
    with pytest.raises(RuntimeError, match='countable'):
        cuda.seen_maps(grid, 1, countable=torch.ones(64, dtype=torch.uint8))
    o, d, t = torch.zeros(2, 2, 2), torch.ones(2, 2, 8, 2), torch.ones(2, 2, 8)
    with pytest.raises(RuntimeError, match='GPU'):
        maps.mark(o, d, t)
    with pytest.raises(RuntimeError, match=r'\(N, P, R, 2\)'):
        maps.mark(torch.zeros(3, 2, 2), d, t)
    with pytest.raises(RuntimeError, match=r'\(N, P, R, 2\)'):
        maps.mark(o, d, torch.ones(2, 2, 7))
    with pytest.raises(RuntimeError, match='dtype'):
        maps.mark(o.double(), d, t)
    with pytest.raises(RuntimeError, match='4-dimensional'):
        maps.mark(o, t, t)
    with pytest.raises(RuntimeError, match='one per map'):
        maps.mark(torch.zeros(2, 3, 2), torch.ones(2, 3, 8, 2), torch.ones(2, 3, 8))
    with pytest.raises(RuntimeError, match='integer'):
        maps.mark(o, d, t, slot=torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match='bool'):
        maps.mark(o, d, t, reset=torch.zeros(2, 2))
    for bad in (0., -1., float('inf'), float('nan')):
        with pytest.raises(RuntimeError, match='max_range'):
            maps.mark(o, d, t, max_range=bad)
    big = np.array([[0, 0, 1025, 1024]], np.int32)
    huge = cuda.NavGrid(torch.as_tensor(big), torch.tensor([0, 1025*1024]), torch.ones(1, dtype=torch.uint8), CELL, RADIUS, big,
                        np.array([0, 1025*1024], np.int64))
    with pytest.raises(RuntimeError, match='cells'):
        cuda.seen_maps(huge, 1)
